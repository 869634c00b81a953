"""Inputs that put ONE candidate on a decision threshold of zlib's match search and lazy parse (qcsrc/deflate.c: longest_match :1027-1168,
deflate_fast :1448-1546, deflate_slow :1554-1674).  TEST INFRASTRUCTURE, pure Python + numpy, deterministic.

Shared by oracle/gen_golden_parse.py and the tests.  catalogue() returns Case rows:

  name      unique
  family    chain | quarter | nice | clip | tie | stairs | lazy | short | reach | fast | hand | placed
  data      the bytes (one chunk of at most 64 KiB; placed continuous cases are one stream of up to 96 KiB)
  cfgs      the configurations (keys of CONFIGS) the case is meant for
  claims    {cfg: [(position, token), ...]}: the token the reference must START at that position, (dist, len) or LIT
  buckets   the hash buckets of the scenario (the trigrams at every probe and at the three positions behind it)
  fill      numpy mask of the positions that hold filler
  pair      (group, side) or None: the two sides of a group sit on either side of ONE threshold and must get different tokens
  cont      True: one continuous stream (the candidates lie in the tile in front of the probe's); False: an independent chunk

How an input is put together (class Build).  Three disjoint alphabets:
  0..131    filler: a stream in which no trigram occurs twice in 102000 bytes (three digit classes, see _stream), so nothing in it ever matches;
  132..191  patch bytes: where a trigram that holds a filler byte falls into a bucket of the scenario, or occurs twice (a seam between filler and
            scenario), one of its filler bytes is replaced by a patch byte until neither is the case -- the hash collision that once made a MAX_DIST
            prize the second candidate of its chain cannot happen unnoticed;
  192..255  the scenario: words cut from a second no-trigram-twice stream, decoys, the byte 255.
A copy of a word's prefix always ends in front of a filler byte, which no scenario byte equals: the match ends where the builder says.

Decoys share with the prize its first trigram ("tri": a three-byte match and no more) or only its BUCKET ("bkt": (b0, b1 ^ 1, b2 ^ 32) has the
same hash and matches one byte).  Every family that counts candidates asserts the count on the finished bytes (chain_of): the prize IS candidate
number d of the probe's chain.

What is left out, and why:
  * level 4 has good_length == max_lazy (4): a search with a match of good_length bytes in hand never happens (deflate.c:1590), so the
    quarter-budget family has no level 4 rows;
  * max_lazy of level 9 is 258: a match of max_lazy bytes in hand cannot be beaten, the lazy family has only the 257-byte row there;
  * nice_length of levels 8 and 9 is 258 = MAX_MATCH: there is no "nice + 1" and "nice - 1 in front of 258" is no threshold, no nice rows there;
  * the 255-step staircase of disjoint strings would span 33150 bytes, more than MAX_DIST: it is built from a run (every position of a run of
    257 equal bytes is a candidate one byte shorter than the one behind it); the 70-step one exists in both forms;
  * the level-like deflateTune rows (T13, T100, T33) and every tuned deflate_fast row are chunk cases only (the engine serves a tuned level 1-3 stream in
    chunks); the continuous cases (tile edges, and the block / window edge cases a second time) use the rows of levels 1-9 and the rows of CONT_EDGE;
  * other memLevel / windowBits change the hash: this catalogue is for the default geometry only;
  * negative arguments of deflateTune (the restatement takes unsigned values).

The rows no level's row resembles (EDGE_SLOW, EDGE_FAST; edge_catalogue).  The reference takes any four integers, and the device code rests on relations
that hold in all nine rows of the level table; each of these rows breaks one:
  * max_chain 1..3: the quarter budget is 0, which never runs out -- with good_length bytes in hand the prize is found behind max_chain + 1, 8, 40 and
    DEEP decoys, with one byte fewer in hand behind max_chain - 1 and not behind max_chain; max_chain 0 and 70000: the full budget never runs out either;
  * good_length 0 and 2 (quartered with nothing in hand: found at depth 32, not at 33, of 128), 3 (quartered behind any match), 300 (never);
  * max_lazy 0 and 2 (no search at all: repeats are literals), 3 (a search only with nothing in hand: the longer match one position on is not taken);
  * max_lazy > nice_length (hand_case): with nice_length..max_lazy - 1 bytes in hand a candidate no longer than that is passed over and a farther, longer
    one taken; the first one that IS longer ends the walk.  The "hole" cases have a near candidate that shares nice_length bytes or more with the probe,
    differs in one byte and agrees again in the two bytes a search with h bytes in hand checks first;
  * nice_length 0, 2, 3 (the first candidate that improves ends the walk) and 1000 (no walk ends on a length);
  * deflate_fast: max_insert_length 0, 3, nice - 1, nice and 258 (inside_case: a probe whose only candidate lies inside a match of exactly m bytes), and
    good_length 2 (every search quartered: budgets 1 and, for max_chain 3, none).
A ladder has at most 40 decoys but for the DEEP one per unbounded search (300: deeper than any budget of these rows, cheap for a one-lane kernel)."""
from collections import namedtuple

import numpy as np

LIT = "literal"
MAX_DIST, MAXM, TOO_FAR = 32506, 258, 4096
BLOCK, WINDOW = 64, 8192                     # walk_kernel: positions per walker block, positions per game log
TILE_EDGES = (65024, 97536)                  # continuous stream: the first tile holds 65024 positions, every other 32512

# (good_length, max_lazy, nice_length, max_chain), deflate.c:137-149
ROWS = {1: (4, 4, 8, 4), 2: (4, 5, 16, 8), 3: (4, 6, 32, 32), 4: (4, 4, 16, 16), 5: (8, 16, 32, 32), 6: (8, 16, 128, 128), 7: (8, 32, 128, 256),
        8: (32, 128, 258, 1024), 9: (32, 258, 258, 4096)}
Z_FILTERED, Z_RLE = 1, 3
Config = namedtuple("Config", "level strategy tune p0")
CONFIGS = {"L%d" % k: Config(k, 0, None, 0) for k in range(1, 10)}
CONFIGS.update({
    "T13": Config(6, 0, (5, 9, 37, 13), 0),      # deflateTune rows on a level 6 stream: budgets 13 / 3,
    "T100": Config(6, 0, (8, 16, 128, 100), 0),  # 100 / 25
    "T33": Config(6, 0, (8, 16, 32, 33), 0),     # and 33 / 8 -- no multiple of eight among the full budgets
    "L4-filtered": Config(4, Z_FILTERED, None, 0), "L6-filtered": Config(6, Z_FILTERED, None, 0),
    "L1-rle": Config(1, Z_RLE, None, 0), "L6-rle": Config(6, Z_RLE, None, 0),
    "L1-p0": Config(1, 0, None, 1), "L6-p0": Config(6, 0, None, 1),
})
SLOW = ["L4", "L5", "L6", "L7", "L8", "L9", "T13", "T100", "T33"]
FAST = ["L1", "L2", "L3"]
CONT_CFGS = ["L%d" % k for k in range(1, 10)]  # (one continuous stream: the levels' own rows)

# deflateTune rows NO level's row resembles (the reference takes any four integers): each breaks a relation that holds in all nine rows.
# They have families of their own (edge_catalogue) and stay out of SLOW / FAST, whose families assume a level-like row.
EDGE_SLOW = {
    "Q3": (6, (4, 16, 32, 3)), "Q2": (6, (4, 16, 32, 2)), "Q1": (6, (4, 16, 32, 1)),  # max_chain < 4: the quarter budget is 0, a search that never runs out
    "Q3-L4": (4, (4, 16, 32, 3)), "Q3-L9": (9, (4, 16, 32, 3)),                       # (both ends of the levels that run deflate_slow)
    "U0": (6, (8, 16, 128, 0)), "U70000": (6, (8, 16, 128, 70000)),                    # the full budget never runs out either
    "G0": (6, (0, 16, 128, 128)), "G2": (6, (2, 16, 128, 128)),                        # good_length <= 2: quartered with nothing in hand (prev_length = 2)
    "G3": (6, (3, 16, 128, 32)), "G300": (6, (300, 16, 128, 32)),                      # quartered behind ANY match; never quartered
    "Z0": (6, (8, 0, 128, 128)), "Z2": (6, (8, 2, 128, 128)), "Z3": (6, (8, 3, 128, 128)),  # max_lazy <= 2: no search at all; 3: only with nothing in hand
    "LN258": (6, (8, 258, 32, 128)), "LN64": (6, (4, 64, 8, 32)),                      # max_lazy > nice_length: a search with nice_length bytes or more in hand
    "N0": (6, (8, 4, 0, 128)), "N2": (6, (8, 4, 2, 128)), "N3": (6, (8, 4, 3, 128)),   # nice_length <= 3: the first candidate that improves ends the walk
    "N1000": (6, (8, 4, 1000, 128)),                                                   # nice_length > MAX_MATCH: no walk ends on a length
}
EDGE_FAST = {
    "I0": (1, (4, 0, 8, 4)), "I3": (1, (4, 3, 8, 4)), "I7": (1, (4, 7, 8, 4)), "I8": (1, (4, 8, 8, 4)), "I258": (1, (4, 258, 8, 4)),  # max_insert_length against nice_length
    "I0-L3": (3, (4, 0, 32, 32)), "I31-L3": (3, (4, 31, 32, 32)), "I32-L3": (3, (4, 32, 32, 32)), "I258-L3": (3, (4, 258, 32, 32)),
    "FG2": (1, (2, 4, 8, 4)), "FG2U": (1, (2, 4, 8, 3)),                               # good_length <= 2 on deflate_fast: every search quartered -- 1, and 0 = unbounded
}
CONFIGS.update({k: Config(lv, 0, t, 0) for k, (lv, t) in list(EDGE_SLOW.items()) + list(EDGE_FAST.items())})
CONT_EDGE = ["Q3", "LN258", "G2"]  # the tuned rows that go through ONE continuous stream as well (deflate_slow only: tuned deflate_fast is served in chunks)
DEEP = 300                         # the deep ladder of an unbounded search: deeper than any max_chain of these rows, cheap for a one-lane kernel
INF = 1 << 32

Case = namedtuple("Case", "name family data cfgs claims buckets fill pair cont")


def row(cfg):
    c = CONFIGS[cfg]
    return c.tune or ROWS[c.level]


def is_fast(cfg):
    return CONFIGS[cfg].level <= 3


def budget(cfg, held=2):
    """Candidates longest_match looks at with a match of `held` bytes in hand (2: none): max_chain, a quarter of it from good_length on; a
    budget of 0 never runs out (the count-down `--chain_length != 0` passes zero, deflate.c:1163)."""
    good, lazy, nice, chain = row(cfg)
    return (chain >> 2 if held >= good else chain) or INF


def bucket(t):
    """The reference's hash of three bytes for memLevel 8 (hash_bits 15, hash_shift 5; deflate.c:170)."""
    return ((t[0] << 10) ^ (t[1] << 5) ^ t[2]) & 0x7FFF


def buckets_at(data):
    """The bucket of every position that still has three bytes."""
    a = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.int64)
    return ((a[:-2] << 10) ^ (a[1:-1] << 5) ^ a[2:]) & 0x7FFF


def chain_of(data, p, pos0=False):
    """The positions deflate_slow's chain holds for position p, nearest first, as far as the search may reach them (deflate.c:1592 for the
    first, :1160 for the others)."""
    h = buckets_at(data[: p + 3])
    q = np.nonzero(h[:p] == h[p])[0][::-1]
    out = []
    for k, c in enumerate(q.tolist()):
        if p - c > MAX_DIST or (k > 0 and p - c >= MAX_DIST) or (c == 0 and not pos0):
            break
        out.append(c)
    return out


def _stream(lo, radix, units):
    """units * 3 bytes (x, y, z) = the three digits of i = 0, 1, 2, ... in `radix`, each digit in a byte class of its own (lo.., lo + radix..,
    lo + 2 radix..).  The classes say where in a unit a trigram starts, and each of the three kinds names i: no trigram occurs twice."""
    i = np.arange(units, dtype=np.int64)
    return np.stack([lo + i % radix, lo + radix + (i // radix) % radix, lo + 2 * radix + (i // (radix * radix)) % radix], 1).astype(np.uint8).ravel()


FILLER = _stream(0, 44, 34000)     # 102000 bytes of 0..131
WORDS = _stream(192, 21, 9261)     # 27783 bytes of 192..254
PATCH = list(range(132, 192)) + list(range(132))  # (the filler's own values last: many seams in one input, a staircase, use up the 60)
X0 = 255


def filler(n, forbidden=(), start=0):
    """n bytes in which no trigram occurs twice and none falls into a forbidden bucket."""
    b = Build()
    b.forbid |= set(forbidden)
    b.cur = start
    b.fill(n)
    return b.done()


def decoy(prize, j, flavour):
    """Six bytes: the prize's first trigram ("tri") or another trigram of its bucket ("bkt"), then three bytes that name j and begin with
    another byte than the prize goes on with.  The last byte is different for every j < 42, so short ladders (levels 1-3) have no match but the
    trigram's among their decoys."""
    t = bytes(prize[:3]) if flavour == "tri" else bytes([prize[0], prize[1] ^ 1, prize[2] ^ 32])
    return t + bytes([234 + j % 21, 213 + (j // 21) % 21, 192 + j if j < 42 else 234 + (j // 441) % 21])


class Build:
    def __init__(self, skew=0):
        self.buf, self.isfill, self.forbid = bytearray(), bytearray(), set()
        self.cur, self.wcur = skew, 3 * (skew % 50)

    def word(self, n):
        """n scenario bytes with no trigram twice, sharing none with any other word of this input."""
        units = (n + 2) // 3 + 1
        assert self.wcur + 3 * units <= len(WORDS)
        w = WORDS[self.wcur: self.wcur + n].tobytes()
        self.wcur += 3 * units
        return w

    def key(self, s):
        """s is searched for: filler stays out of the buckets of its first four trigrams (the probe and the lazy steps behind it)."""
        for o in range(min(4, len(s) - 2)):
            self.forbid.add(bucket(s[o: o + 3]))

    def put(self, s):
        pos = len(self.buf)
        self.buf += s
        self.isfill += bytes(len(s))
        return pos

    def fill(self, n):
        assert n >= 0 and self.cur + n <= len(FILLER)
        pos = len(self.buf)
        self.buf += FILLER[self.cur: self.cur + n].tobytes()
        self.isfill += b"\1" * n
        self.cur += n
        return pos

    def done(self):
        forbid = np.array(sorted(self.forbid), dtype=np.int64)
        for _ in range(8):
            a = np.frombuffer(bytes(self.buf), dtype=np.uint8).astype(np.int64)
            f = np.frombuffer(bytes(self.isfill), dtype=np.uint8)
            if len(a) < 3:
                break
            code = (a[:-2] << 16) | (a[1:-1] << 8) | a[2:]
            h = ((a[:-2] << 10) ^ (a[1:-1] << 5) ^ a[2:]) & 0x7FFF
            _, inv, cnt = np.unique(code, return_inverse=True, return_counts=True)
            bad = np.nonzero((f[:-2] | f[1:-1] | f[2:]).astype(bool) & ((cnt[inv] > 1) | np.isin(h, forbid)))[0]
            if len(bad) == 0:
                break
            seen = set(code.tolist())
            for i in bad.tolist():
                j = next(k for k in (i + 1, i, i + 2) if self.isfill[k])
                for v in PATCH:
                    self.buf[j] = v
                    new = [bytes(self.buf[k: k + 3]) for k in range(max(0, j - 2), min(j, len(self.buf) - 3) + 1)]
                    codes = [(t[0] << 16) | (t[1] << 8) | t[2] for t in new]
                    if len(set(codes)) == len(codes) and not any(c in seen for c in codes) and not any(bucket(t) in self.forbid for t in new):
                        seen.update(codes)
                        break
                else:
                    raise AssertionError("no patch byte fits at %d" % j)
        else:
            raise AssertionError("filler could not be patched")
        return bytes(self.buf)

    def case(self, name, family, cfgs, claims, probes, pair=None, cont=False):
        data = self.done()
        if not isinstance(claims, dict):
            claims = {c: claims for c in cfgs}
        h = buckets_at(data)
        bk = set()
        for p in probes:
            bk |= {int(h[k]) for k in range(p, min(p + 4, len(h))) if not any(self.isfill[k: k + 3])}
        assert bk <= self.forbid, (name, "a probe's bucket the filler was not told of")
        assert cont or len(data) <= 65536, (name, len(data))
        return Case(name, family, data, list(cfgs), claims, bk, np.frombuffer(bytes(self.isfill), dtype=np.uint8).astype(bool), pair, cont)


# ---- where a probe is put ----
def placements(natural):
    """[(tag, probe position)]: the first walker block edge behind `natural` that is no window edge, and the first window edge, each -1, 0, +1."""
    blk = (natural + BLOCK) // BLOCK * BLOCK + BLOCK
    if blk % WINDOW == 0:
        blk += BLOCK
    win = (natural + 1 + WINDOW) // WINDOW * WINDOW
    return [("b%+d" % e, blk + e) for e in (-1, 0, 1)] + [("w%+d" % e, win + e) for e in (-1, 0, 1)]


def tile_placements():
    return [("t%d" % (t + e), t + e) for t in TILE_EDGES for e in (-1, 0, 1)]


LEAD = 7  # filler in front of the first scenario byte where nothing asks for more: the prize is not at position 0, which no search reaches


# ---- chain depth ----
def ladder(cfg, d, flavour, at=None, tag="", cont=False, pair=None):
    """prize, d - 1 decoys, the prize again: the prize is candidate number d of the probe."""
    good, lazy, nice, chain = row(cfg)
    b = Build(skew=d)
    prize = b.word(20)
    b.key(prize)
    body = 20 + 2 + 6 * (d - 1) + 2
    b.fill(LEAD if at is None else at - body)
    ppos = b.put(prize)
    b.fill(2)
    last = None
    for j in range(d - 1):
        last = b.put(decoy(prize, j, flavour))
    b.fill(2)
    probe = b.put(prize)
    b.fill(9)
    assert at is None or probe == at
    assert flavour == "bkt" or (nice > 3 and (is_fast(cfg) or lazy > 3))  # (a decoy's trigram neither ends the walk nor ends the lazy evaluation)
    assert is_fast(cfg) or lazy > 2
    if d <= budget(cfg):
        claim = [(probe, (probe - ppos, 20))]
    elif is_fast(cfg) and flavour == "tri":
        claim = [(probe, (probe - last, 3))]
    else:
        claim = [(probe, LIT)]  # (deflate_slow: at most the trigram in hand, and the prize's second byte on is found one position on)
    c = b.case("chain-%s-%s-d%d%s" % (cfg, flavour, d, tag), "placed" if tag else "chain", [cfg], claim, [probe], pair, cont)
    ch = chain_of(c.data, probe)
    assert len(ch) == d and ch[d - 1] == ppos, (c.name, len(ch))
    return c


def depths(chain):
    return sorted({d for d in (1, 8, 9, 31, 32, 33, 64, 65, chain - 1, chain, chain + 1) if 1 <= d <= chain + 1})


def quarter(cfg, d, g, at=None, tag="", cont=False):
    """The same ladder searched with a match of g bytes in hand (g = good_length - 1: the whole budget, g = good_length: a quarter of it)."""
    good, lazy, nice, chain = row(cfg)
    assert 3 <= g < lazy
    qbudget = budget(cfg, g)
    b = Build(skew=d + g)
    prize = b.word(max(20, g + 8))
    held = bytes([X0]) + prize[: g - 1]
    b.key(prize)
    b.key(bytes([X0]) + prize)
    b.fill(LEAD if at is None else at - (g + 2 + len(prize) + 2 + 6 * (d - 1) + 2))
    hpos = b.put(held)
    b.fill(2)
    ppos = b.put(prize)
    b.fill(2)
    # (decoy 31 ends in a byte that shares its low five bits with 255: the trigram across its end falls into the bucket of the held match's.  A budget
    #  of one or two candidates with nothing in hand would never reach the held copy behind it: those rows leave it out)
    for j in (range(d - 1) if budget(cfg) > 2 else [j for j in range(d) if j != 31][: d - 1]):
        b.put(decoy(prize, j, "tri"))
    b.fill(2)
    q = b.put(bytes([X0]) + prize)
    b.fill(9)
    claim = [(q, LIT), (q + 1, (q + 1 - ppos, len(prize)))] if d <= qbudget else [(q, (q - hpos, g))]
    assert at is None or q == at
    side = None if d not in (qbudget, qbudget + 1) else ("quarter-%s-g%d%s" % (cfg, g, tag), int(d > qbudget))
    c = b.case("quarter-%s-g%d-d%d%s" % (cfg, g, d, tag), "placed" if tag else "quarter", [cfg], claim, [q, q + 1], side, cont)
    ch = chain_of(c.data, q + 1)
    cq = chain_of(c.data, q)  # (a decoy's last byte may share its low five bits with 255: one more candidate of that bucket, no match)
    assert len(cq) <= budget(cfg), c.name
    assert ch[d - 1] == ppos and (ch[-1] == hpos + 1 or g == 3) and cq[-1] == hpos and len(cq) <= 3, c.name  # (g == 3: the held copy's second trigram ends in filler)
    return c


# ---- nice length ----
def nice_case(cfg, m, far=MAXM, at=None, tag="", cont=False, pair=None, name=None):
    """A copy of `far` bytes of the probe, a nearer copy of m bytes, the probe (258 bytes)."""
    good, lazy, nice, chain = row(cfg)
    b = Build(skew=m)
    w = b.word(MAXM)
    b.key(w)
    body = far + 2 + m + 2
    b.fill(LEAD if at is None else at - body)
    fpos = b.put(w[:far])
    b.fill(2)
    npos = b.put(w[:m])
    b.fill(2)
    probe = b.put(w)
    b.fill(9)
    assert at is None or probe == at
    assert m >= lazy or is_fast(cfg)  # (no lazy step behind the nearer copy; a row whose max_lazy exceeds nice_length - 1 has hand_case instead)
    claim = [(probe, (probe - npos, m) if m >= nice or m >= far else (probe - fpos, far))]
    c = b.case(name or "nice-%s-m%d%s" % (cfg, m, tag), "placed" if tag else "nice", [cfg], claim, [probe], pair, cont)
    assert chain_of(c.data, probe) == [npos, fpos], c.name
    return c


def clip_case(cfg, look, short):
    """The probe `look` bytes in front of the chunk's end (nice_length is clipped to the lookahead, deflate.c:1060), behind two copies: the
    nearer one whole (it wins at min(look, 258) bytes) or, `short`, one byte shorter than the lookahead (the farther one wins)."""
    good, lazy, nice, chain = row(cfg)
    b = Build(skew=look)
    w = b.word(MAXM)
    b.key(w)
    m = look - 1 if short else MAXM
    b.fill(LEAD)
    fpos = b.put(w)
    b.fill(2)
    npos = b.put(w[:m])
    b.fill(2)
    probe = b.put(w[:look] if look <= MAXM else w + bytes([X0]) * (look - MAXM))
    n = min(look, MAXM)
    claim = [(probe, (probe - fpos, n) if short else (probe - npos, n))]
    return b.case("clip-%s-look%d%s" % (cfg, look, "-short" if short else ""), "clip", [cfg], claim, [probe])


# ---- ties and staircases ----
def walk(lens, prev, nice, budget):
    """longest_match over candidates of these lengths, nearest first: (index of the winner or None, its length)."""
    best, who = prev, None
    for i, l in enumerate(lens[:budget]):
        if l > best:
            best, who = l, i
            if l >= nice:
                break
    return who, best


def tie_case(cfgs):
    b = Build()
    s = b.word(10)
    b.key(s)
    b.fill(LEAD)
    b.put(s)
    b.fill(2)
    near = b.put(s)
    b.fill(2)
    probe = b.put(s)
    b.fill(9)
    return b.case("tie-two-distances", "tie", cfgs, [(probe, (probe - near, 10))], [probe])


def stairs_case(cfg, n, reverse):
    """n disjoint copies of the probe's prefix, each one byte longer than the one in front of it (3 ... n + 2 bytes): nearest shortest, or, `reverse`,
    nearest longest."""
    good, lazy, nice, chain = row(cfg)
    b = Build(skew=n)
    w = b.word(n + 3)
    b.key(w)
    lens = [n + 2 - i for i in range(n)] if reverse else [3 + i for i in range(n)]  # nearest first
    b.fill(LEAD)
    pos = []
    for l in reversed(lens):
        pos.append(b.put(w[:l]))
        b.fill(2)
    pos.reverse()
    probe = b.put(w)
    b.fill(9)
    who, best = walk(lens, 2, nice, chain)
    claim = [(probe, (probe - pos[who], best))]
    if not is_fast(cfg) and best < lazy:  # the lazy step: the same candidates one position on, each one byte shorter
        if walk([l - 1 for l in lens], best, nice, chain >> 2 if best >= good else chain)[1] > best:
            claim = [(probe, LIT)]
    c = b.case("stairs-%s-%d%s" % (cfg, n, "-reverse" if reverse else ""), "stairs", [cfg], claim, [probe])
    assert chain_of(c.data, probe) == pos, c.name
    return c


def run_stairs_case(cfg, n):
    """A run of n + 2 equal bytes in front of a run of 258: position j of the first run is a candidate of n + 2 - j bytes, n candidates, nearest shortest."""
    good, lazy, nice, chain = row(cfg)
    b = Build(skew=n)
    b.key(bytes([X0]) * 6)
    b.fill(LEAD)
    r0 = b.put(bytes([X0]) * (n + 2))
    b.fill(2)
    probe = b.put(bytes([X0]) * MAXM)
    b.fill(9)
    lens = [3 + i for i in range(n)]
    who, best = walk(lens, 2, nice, chain)
    claim = [(probe, (probe - (r0 + n - 1 - who), best))]
    if best < lazy and best < MAXM - 1:  # one position on, the probe's own first byte is a candidate of 257 bytes
        claim = [(probe, LIT)]
    c = b.case("stairs-%s-run%d" % (cfg, n), "stairs", [cfg], claim, [probe])
    assert chain_of(c.data, probe) == [r0 + n - 1 - i for i in range(n)], c.name
    return c


# ---- lazy evaluation ----
def lazy_case(cfg, h, longer):
    """A match of h bytes in hand and, one position on, one of h + 10 (`longer`; 258 at the most) or of h bytes."""
    good, lazy, nice, chain = row(cfg)
    b = Build(skew=h)
    qlen = min(MAXM, h + 10) if longer else h
    q_ = b.word(qlen)
    held = bytes([X0]) + q_[: h - 1]
    b.key(bytes([X0]) + q_)
    b.key(q_)
    b.fill(LEAD)
    hpos = b.put(held)
    b.fill(2)
    qpos = b.put(q_)
    b.fill(2)
    p = b.put(bytes([X0]) + q_)
    b.fill(9)
    switch = h < lazy and qlen > h
    claim = [(p, LIT), (p + 1, (p + 1 - qpos, qlen))] if switch else [(p, (p - hpos, h))]
    side = ("lazy-%s" % cfg, int(not switch)) if longer and h in (lazy - 1, lazy) and 3 < lazy < MAXM else None
    return b.case("lazy-%s-h%d-%s" % (cfg, h, "longer" if longer else "equal"), "lazy", [cfg], claim, [p, p + 1], side)


def lazy3_case(cfgs):
    """Matches of 4, 6 and 8 bytes at three positions in a row: two literals, then the third."""
    b = Build()
    z = b.word(12)
    b.key(z)
    b.key(z[2:])
    b.fill(LEAD)
    b.put(z[0:4])
    b.fill(2)
    b.put(z[1:7])
    b.fill(2)
    a2 = b.put(z[2:10])
    b.fill(2)
    p = b.put(z)
    b.fill(9)
    return b.case("lazy-three-steps", "lazy", cfgs, [(p, LIT), (p + 1, LIT), (p + 2, (p + 2 - a2, 8))], [p, p + 1, p + 2])


# ---- short-match rules ----
def too_far_case(dist, cfgs):
    b = Build(skew=dist)
    t = b.word(3)
    b.key(t)
    b.fill(LEAD)
    b.put(t)
    b.fill(dist - 3)
    p = b.put(t)
    b.fill(9)
    claims = {c: [(p, (dist, 3) if is_fast(c) or dist <= TOO_FAR else LIT)] for c in cfgs}
    return b.case("short-trigram-at-%d" % dist, "short", cfgs, claims, [p], ("too-far", int(dist > TOO_FAR)))


def filtered_case(n, cfgs):
    b = Build(skew=n)
    s = b.word(n)
    b.key(s)
    b.fill(LEAD)
    spos = b.put(s)
    b.fill(2)
    p = b.put(s)
    b.fill(9)
    claims = {c: [(p, LIT if CONFIGS[c].strategy == Z_FILTERED and n <= 5 else (p - spos, n))] for c in cfgs}
    return b.case("short-filtered-%d" % n, "short", cfgs, claims, [p], ("filtered", int(n > 5)))


def rle_case(n):
    """Three equal bytes, filler, a run of n of them: under Z_RLE the run's first byte has only the far candidate and stays a literal."""
    b = Build(skew=n)
    b.key(bytes([X0]) * 6)
    b.fill(LEAD)
    b.put(bytes([X0]) * 3)
    b.fill(4)
    p = b.put(bytes([X0]) * n)
    b.fill(9)
    first = min(MAXM, n - 1)
    slow = [(p, LIT), (p + 1, (1, first))] + ([(p + 1 + MAXM, (1, n - 1 - MAXM))] if n - 1 - MAXM >= 3 else [])
    return b.case("short-rle-run%d" % n, "short", ["L6-rle", "L1-rle"], {"L6-rle": slow, "L1-rle": slow[:2]}, [p])


# ---- reach ----
def reach_case(dist, second, cfgs):
    """The prize `dist` bytes in front of the probe, the first candidate of its chain or, behind one decoy of the bucket, the second."""
    b = Build(skew=dist + second)
    prize = b.word(20)
    b.key(prize)
    b.fill(LEAD)
    ppos = b.put(prize)
    if second:
        b.fill(dist - 20 - 8)
        dpos = b.put(decoy(prize, 0, "bkt"))
        b.fill(2)
    else:
        b.fill(dist - 20)
    p = b.put(prize)
    b.fill(9)
    assert p - ppos == dist
    ok = dist <= MAX_DIST - second
    c = b.case("reach-%d-%s" % (dist, "second" if second else "first"), "reach", cfgs, [(p, (dist, 20) if ok else LIT)], [p],
               ("reach-%s" % ("second" if second else "first"), int(not ok)) if dist in (MAX_DIST - second, MAX_DIST - second + 1) else None)
    assert chain_of(c.data, p) == ([dpos] if second else []) + ([ppos] if ok else []), c.name
    return c


def pos0_case():
    b = Build()
    prize = b.word(20)
    b.key(prize)
    b.put(prize)
    b.fill(5)
    p = b.put(prize)
    b.fill(9)
    cfgs = ["L1", "L6", "L1-p0", "L6-p0"]
    return b.case("reach-position-0", "reach", cfgs, {c: [(p, (p, 20) if CONFIGS[c].p0 else LIT)] for c in cfgs}, [p])


# ---- deflate_fast ----
def insert_case(cfg, extra):
    """deflate_fast puts the inside of a match into the chains only up to max_insert_length bytes (deflate.c:1508): a match of that length
    (+ `extra`), then a probe whose nearest copy starts at the match's second byte."""
    m = row(cfg)[1] + extra
    b = Build(skew=m)
    s, e = b.word(m), b.word(5)
    r = s[1:] + e
    b.key(s + e)
    b.key(r)
    b.fill(LEAD)
    s0 = b.put(s)
    b.fill(3)
    s1 = b.put(s + e)
    b.fill(3)
    p = b.put(r)
    b.fill(9)
    claim = [(s1, (s1 - s0, m)), (p, (p - (s0 + 1), m - 1) if extra else (p - (s1 + 1), m + 4))]
    return b.case("fast-insert-%s-%d" % (cfg, m), "fast", [cfg], claim, [s1, p], ("fast-insert-%s" % cfg, extra))


# ---- deflateTune rows no level's row resembles ----
def hand_case(cfg, h, near, far, hole=None, at=None, tag="", cont=False, pair=None):
    """max_lazy > nice_length: a match of h bytes in hand with nice_length <= h < max_lazy, and one position on two copies of the probe, the
    nearer of `near` bytes, the farther of `far`.  longest_match starts with best_len = h: a candidate of nice_length..h bytes neither updates nor
    ends the walk (deflate.c:1126-1163), the first one LONGER than h does both.  `hole`: the nearer copy differs from the probe in byte `hole`
    alone among its first h + 2 -- nice_length bytes or more in common, and the two bytes a search with h in hand checks first (h - 1 and h) equal."""
    good, lazy, nice, chain = row(cfg)
    assert nice <= h < lazy and 3 <= h and near < far <= MAXM and budget(cfg, h) >= 3
    b = Build(skew=h + near)
    w = b.word(MAXM)
    held = bytes([X0]) + w[: h - 1]
    ncopy = w[:near] if hole is None else w[:hole] + bytes([X0]) + w[hole + 1: h + 2]
    assert hole is None or (nice <= hole <= h - 2 and near == hole)
    b.key(w)
    b.key(w[1:])
    b.key(bytes([X0]) + w)
    b.fill(LEAD if at is None else at - (h + 2 + far + 2 + len(ncopy) + 2))
    hpos = b.put(held)
    b.fill(2)
    fpos = b.put(w[:far])
    b.fill(2)
    npos = b.put(ncopy)
    b.fill(2)
    p = b.put(bytes([X0]) + w)
    b.fill(9)
    assert at is None or p == at
    if near > h and near < lazy and far - 1 > near:  # ... and given up one position on, where the farther copy is the longer one (max_lazy is still above)
        claim = [(p + 1, LIT), (p + 2, (p + 1 - fpos, far - 1)), (p, LIT)]
    elif near > h:  # the first candidate that is longer than the match in hand: taken, and the walk ends (it is nice_length bytes or more)
        claim = [(p + 1, (p + 1 - npos, near)), (p, LIT)]
    elif far > h:   # the nearer copy is passed over, the walk goes on
        claim = [(p + 1, (p + 1 - fpos, far)), (p, LIT)]
    else:
        claim = [(p, (p - hpos, h))]
    name = "hand-%s-h%d-n%d-f%d%s%s" % (cfg, h, near, far, "-hole" if hole is not None else "", tag)
    c = b.case(name, "placed" if tag else "hand", [cfg], claim, [p, p + 1, p + 2], pair, cont)
    assert chain_of(c.data, p + 1) == [npos, fpos, hpos + 1], c.name
    return c


def repeats_case(cfgs):
    """max_lazy <= 2: deflate_slow never searches (prev_length = 2 is not below max_lazy, deflate.c:1588) -- three copies of a word, all literals."""
    b = Build()
    s_ = b.word(12)
    b.key(s_)
    b.fill(LEAD)
    b.put(s_)
    b.fill(2)
    p1 = b.put(s_)
    b.fill(2)
    p2 = b.put(s_)
    b.fill(9)
    return b.case("lazy-none-repeats", "lazy", cfgs, [(q, LIT) for p in (p1, p2) for q in range(p, p + 12)], [p1, p2])


def first_improver_case(cfgs):
    """A copy of 258 bytes of the probe and a nearer one of 4: with nice_length <= 4 the nearer one ends the walk; every cfg here has max_lazy 4,
    so nothing is looked for behind it."""
    b = Build()
    w = b.word(MAXM)
    b.key(w)
    b.fill(LEAD)
    fpos = b.put(w)
    b.fill(2)
    npos = b.put(w[:4])
    b.fill(2)
    probe = b.put(w)
    b.fill(9)
    assert all(row(c)[1] == 4 and not is_fast(c) for c in cfgs)
    claims = {c: [(probe, (probe - npos, 4) if row(c)[2] <= 4 else (probe - fpos, MAXM))] for c in cfgs}
    c = b.case("nice-first-improver", "nice", cfgs, claims, [probe])
    assert chain_of(c.data, probe) == [npos, fpos], c.name
    return c


def inside_case(cfg, m):
    """deflate_fast, max_insert_length from the other side: a match of exactly m bytes in front of five new bytes, then a probe that begins with the
    match's last two bytes and those five -- its only candidate lies INSIDE the match (at m - 2), and so do the next position's; the third
    position's is the first of the five bytes, which every row inserts."""
    good, max_insert, nice, chain = row(cfg)
    assert is_fast(cfg) and 3 <= m <= MAXM
    b = Build(skew=m)
    s_, e = b.word(m), b.word(5)
    r = s_[m - 2:] + e
    b.key(s_ + e)
    b.key(r)
    b.fill(LEAD)
    s0 = b.put(s_)
    b.fill(3)
    s1 = b.put(s_ + e)
    b.fill(3)
    p = b.put(r)
    b.fill(9)
    if m <= max_insert:
        claim = [(p, (p - (s1 + m - 2), 7)), (s1, (s1 - s0, m))]
    else:
        claim = [(p, LIT), (p + 1, LIT), (p + 2, (p - s1 - m + 2, 5)), (s1, (s1 - s0, m))]
    side = ("fast-inside-%s" % cfg, int(m > max_insert)) if m in (max_insert, max_insert + 1) and 3 <= max_insert < MAXM else None
    return b.case("fast-inside-%s-%d" % (cfg, m), "fast", [cfg], claim, [s1, p], side)


def edge_catalogue():
    out = []

    def rungs(cfg, fl="bkt"):  # the two sides of the budget that holds with nothing in hand
        bd = budget(cfg)
        for d in (bd, bd + 1):
            out.append(ladder(cfg, d, fl, pair=("chain-%s-%s" % (cfg, fl), int(d > bd))))

    # quarter 0: with good_length bytes in hand the prize is found however deep, with one fewer the budget is max_chain
    for cfg in ("Q3", "Q2", "Q1", "Q3-L4", "Q3-L9"):
        good, lazy, nice, chain = row(cfg)
        for d in sorted({chain + 1, 8, 40, DEEP}):
            out.append(quarter(cfg, d, good))
        for d in (chain, chain + 1):
            out.append(quarter(cfg, d, good - 1))
        rungs(cfg, "tri")
    # an unbounded full budget
    for cfg in ("U0", "U70000"):
        good = row(cfg)[0]
        for fl in ("tri", "bkt"):
            out.append(ladder(cfg, DEEP, fl))
        out.append(ladder(cfg, 40, "tri"))
        out.append(quarter(cfg, DEEP, good))
        out.append(quarter(cfg, DEEP, good - 1))
    # good_length 0, 2, 3, 300
    for cfg in ("G0", "G2"):
        rungs(cfg, "tri")       # 32 | 33 with nothing in hand
        rungs(cfg, "bkt")
        for d in (32, 33):
            out.append(quarter(cfg, d, 5))
    rungs("G3", "tri")          # 32 | 33: the full budget
    for d in (8, 9):
        out.append(quarter("G3", d, 3))
    rungs("G300", "tri")
    for d in (32, 33):
        out.append(quarter("G300", d, 15))
    # max_lazy 0, 2, 3
    out.append(repeats_case(["Z0", "Z2", "L6"]))
    out[-1].claims["L6"][:] = []  # (level 6 is there for the contrast: its stream must differ, see the tests; no claim)
    out.append(lazy_case("Z3", 3, True))
    rungs("Z3", "bkt")
    # max_lazy > nice_length
    for cfg in ("LN258", "LN64"):
        good, lazy, nice, chain = row(cfg)
        for h in sorted({nice, nice + 5, min(lazy, MAXM) - 1}):
            far = min(MAXM, h + 20)
            if h + 1 < far:
                out.append(hand_case(cfg, h, nice, far, pair=("hand-%s-h%d" % (cfg, h), 0)))
                out.append(hand_case(cfg, h, h + 1, far, pair=("hand-%s-h%d" % (cfg, h), 1)))
                if h > nice:
                    out.append(hand_case(cfg, h, h, far))
            if h - 2 >= nice:
                hole = h - 2 if h + 2 < MAXM else nice  # (h = 257: the copy runs to the probe's last byte, the differing byte lies as far in front as it may)
                out.append(hand_case(cfg, h, hole, max(far, h + 1), hole=hole))
        rungs(cfg, "tri")
    # nice_length 0, 2, 3, 1000
    out.append(first_improver_case(["N0", "N2", "N3", "N1000"]))
    out.append(nice_case("N1000", 200))
    out.append(nice_case("N1000", MAXM - 1))
    for cfg in ("N0", "N2", "N3", "N1000"):
        rungs(cfg, "bkt")
    # deflate_fast: max_insert_length on either side of nice_length
    for cfg in EDGE_FAST:
        if cfg.startswith("I"):
            mi, nice = row(cfg)[1], row(cfg)[2]
            for m in sorted({3, nice - 1, nice, nice + 1} | {x for x in (mi, mi + 1) if 3 <= x <= MAXM}):
                out.append(inside_case(cfg, m))
            rungs(cfg, "tri")
    for cfg in FAST:            # (the levels' own rows through the same construction)
        for m in (row(cfg)[1], row(cfg)[1] + 1):
            out.append(inside_case(cfg, m))
    # good_length <= 2 on deflate_fast: every search is quartered
    rungs("FG2", "bkt")         # 1 | 2
    rungs("FG2", "tri")
    for d in (5, 40, DEEP):
        out.append(ladder("FG2U", d, "bkt"))
    out.append(ladder("FG2U", 40, "tri"))
    # placement: walker block and log window edges (chunks, and a second time as one continuous stream), tile edges (one continuous stream)
    for cfg in CONT_EDGE:
        good, lazy, nice, chain = row(cfg)
        spots = [(t, a, False) for t, a in placements(LEAD + 400)] + [(t, a, True) for t, a in tile_placements()]
        for tag, at, cont in spots:
            if cfg == "Q3":
                for d in (chain + 1, 8):
                    out.append(quarter(cfg, d, good, at=at, tag="-" + tag, cont=cont))
                for d in (chain, chain + 1):
                    out.append(quarter(cfg, d, good - 1, at=at, tag="-" + tag, cont=cont))
            elif cfg == "G2":
                for d in (32, 33):
                    out.append(ladder(cfg, d, "tri", at=at, tag="-" + tag, cont=cont, pair=("chain-%s-%s" % (cfg, tag), int(d > 32))))
            else:
                h = nice + 5
                out.append(hand_case(cfg, h, nice, h + 20, at=at, tag="-" + tag, cont=cont, pair=("hand-%s-%s" % (cfg, tag), 0)))
                out.append(hand_case(cfg, h, h + 1, h + 20, at=at, tag="-" + tag, cont=cont, pair=("hand-%s-%s" % (cfg, tag), 1)))
                out.append(hand_case(cfg, h, h - 2, h + 20, hole=h - 2, at=at, tag="-" + tag, cont=cont))
    return out


_catalogue = None


def catalogue():
    global _catalogue
    if _catalogue is None:
        _catalogue = build_catalogue()
    return _catalogue


def build_catalogue():
    out = []
    every = FAST + SLOW
    # chain depth: levels 4-9 and the tuned rows; deflate_fast's ladders (budgets 4, 8, 32) are the same family
    for cfg in every:
        chain = row(cfg)[3]
        for d in depths(chain):
            for fl in ("tri", "bkt"):
                side = ("chain-%s-%s" % (cfg, fl), int(d > chain)) if d in (chain, chain + 1) else None
                out.append(ladder(cfg, d, fl, pair=side))
    # quarter budget (not level 4, see the module's text)
    for cfg in SLOW:
        good, lazy, nice, chain = row(cfg)
        if good >= lazy:
            continue
        qb = chain >> 2
        for d in sorted({max(1, qb - 1), qb, qb + 1}):
            out.append(quarter(cfg, d, good))
        for d in sorted({qb + 1, chain, chain + 1}):
            out.append(quarter(cfg, d, good - 1))
    # nice length
    for cfg in every:
        good, lazy, nice, chain = row(cfg)
        if nice >= MAXM - 1:
            continue
        for m in (nice - 1, nice, nice + 1):
            out.append(nice_case(cfg, m, pair=("nice-%s" % cfg, int(m >= nice)) if m < nice + 1 else None))
        out.append(nice_case(cfg, nice, far=nice + 10, name="nice-%s-two-nice" % cfg))
        for look in sorted({3, 4, nice - 1, nice, nice + 1, 257, 258, 259, 260}):
            out.append(clip_case(cfg, look, False))
        for look in (nice - 1, nice):
            if look - 1 >= lazy or is_fast(cfg):
                out.append(clip_case(cfg, look, True))
    # ties and staircases
    out.append(tie_case(every))
    for cfg in every:
        out.append(stairs_case(cfg, 70, False))
        out.append(stairs_case(cfg, 70, True))
    for cfg in SLOW:
        out.append(run_stairs_case(cfg, 70))
        out.append(run_stairs_case(cfg, 255))
    # lazy evaluation
    for cfg in SLOW:
        lazy = row(cfg)[1]
        for h in (lazy - 1, lazy):
            if 3 <= h < MAXM:
                out.append(lazy_case(cfg, h, True))
        out.append(lazy_case(cfg, lazy - 1, False))
    out.append(lazy3_case([c for c in SLOW if row(c)[1] >= 9]))
    # short-match rules
    for dist in (TOO_FAR, TOO_FAR + 1):
        out.append(too_far_case(dist, every))
    for n in (5, 6):
        out.append(filtered_case(n, ["L4-filtered", "L6-filtered", "L4", "L6"]))
    for n in (257, 258, 259, 516):
        out.append(rle_case(n))
    # reach
    for dist in (MAX_DIST - 1, MAX_DIST, MAX_DIST + 1):
        for second in (0, 1):
            out.append(reach_case(dist, second, ["L1", "L3", "L4", "L6", "L9", "T13"]))
    out.append(pos0_case())
    # deflate_fast: max_insert_length
    for cfg in FAST:
        for extra in (0, 1):
            out.append(insert_case(cfg, extra))
    # placement: the deciding rungs on a walker block edge, a log window edge and, as one continuous stream, a tile edge
    for cfg in every:
        good, lazy, nice, chain = row(cfg)
        natural = LEAD + 24 + 6 * chain
        for tag, at in placements(natural):
            for d in (chain, chain + 1):
                out.append(ladder(cfg, d, "tri", at=at, tag="-" + tag, pair=("chain-%s-%s" % (cfg, tag), int(d > chain))))
        if nice < MAXM - 1:
            for tag, at in placements(LEAD + MAXM + nice + 4):
                for m in (nice - 1, nice):
                    out.append(nice_case(cfg, m, at=at, tag="-" + tag, pair=("nice-%s-%s" % (cfg, tag), int(m >= nice))))
    for cfg in CONT_CFGS:
        good, lazy, nice, chain = row(cfg)
        for tag, at in tile_placements():
            for d in (chain, chain + 1):
                out.append(ladder(cfg, d, "tri", at=at, tag="-" + tag, cont=True, pair=("chain-%s-%s" % (cfg, tag), int(d > chain))))
            if nice < MAXM - 1:
                for m in (nice - 1, nice):
                    out.append(nice_case(cfg, m, at=at, tag="-" + tag, cont=True, pair=("nice-%s-%s" % (cfg, tag), int(m >= nice))))
    out += edge_catalogue()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
