"""Inputs that put ONE candidate on a decision threshold of zlib's match search and lazy parse (qcsrc/deflate.c: longest_match :1027-1168,
deflate_fast :1448-1546, deflate_slow :1554-1674).  TEST INFRASTRUCTURE, pure Python + numpy, deterministic.

Shared by oracle/gen_golden_parse.py and the tests.  catalogue() returns Case rows:

  name      unique
  family    chain | quarter | nice | clip | tie | stairs | lazy | short | reach | fast | placed
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
  * deflateTune rows are chunk cases only: the continuous cases (tile edges, and the block / window edge cases a second time) use the rows of levels 1-9;
  * a max_chain below 4 (a quarter budget of 0, which the reference treats as unbounded) has no row yet;
  * other memLevel / windowBits change the hash: this catalogue is for the default geometry only."""
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
CONT_CFGS = ["L%d" % k for k in range(1, 10)]  # (one continuous stream: the levels' own rows; deflateTune rows go through chunks only)

Case = namedtuple("Case", "name family data cfgs claims buckets fill pair cont")


def row(cfg):
    c = CONFIGS[cfg]
    return c.tune or ROWS[c.level]


def is_fast(cfg):
    return CONFIGS[cfg].level <= 3


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
    if d <= chain:
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


def quarter(cfg, d, g):
    """The same ladder searched with a match of g bytes in hand (g = good_length - 1: the whole budget, g = good_length: a quarter of it)."""
    good, lazy, nice, chain = row(cfg)
    assert 3 <= g < lazy
    budget = chain >> 2 if g >= good else chain
    b = Build(skew=d + g)
    prize = b.word(max(20, g + 8))
    held = bytes([X0]) + prize[: g - 1]
    b.key(prize)
    b.key(bytes([X0]) + prize)
    b.fill(LEAD)
    hpos = b.put(held)
    b.fill(2)
    ppos = b.put(prize)
    b.fill(2)
    for j in range(d - 1):
        b.put(decoy(prize, j, "tri"))
    b.fill(2)
    q = b.put(bytes([X0]) + prize)
    b.fill(9)
    claim = [(q, LIT), (q + 1, (q + 1 - ppos, len(prize)))] if d <= budget else [(q, (q - hpos, g))]
    side = None if d not in (budget, budget + 1) else ("quarter-%s-g%d" % (cfg, g), int(d > budget))
    c = b.case("quarter-%s-g%d-d%d" % (cfg, g, d), "quarter", [cfg], claim, [q, q + 1], side)
    ch = chain_of(c.data, q + 1)
    cq = chain_of(c.data, q)  # (a decoy's last byte may share its low five bits with 255: one more candidate of that bucket, no match)
    assert ch[d - 1] == ppos and ch[-1] == hpos + 1 and cq[-1] == hpos and len(cq) <= 3, c.name
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
    assert m >= lazy or is_fast(cfg)  # (no lazy step behind the nearer copy: max_lazy <= nice_length - 1 in every row used)
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
    side = ("lazy-%s" % cfg, int(not switch)) if longer and h in (lazy - 1, lazy) and lazy < MAXM else None
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
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
