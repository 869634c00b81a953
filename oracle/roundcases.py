"""Continuous streams built to mislead the GUESSES of the level 1-3 tile rounds (zlib_amd/csrc/zgpu_lz_fastwin.hip fastwin_tile_kernel,
zgpu_deflate_cont.hip lz_tiles_fast).  TEST INFRASTRUCTURE, pure Python + numpy, deterministic; Build, the filler, the patch alphabet and the words are
oracle/parsecases.py's.

deflate_fast's state at a token start is the position AND which of the 32506 positions in front of it are in the hash chains (the strings inside a match
longer than max_insert_length never enter them).  The engine parses every tile c >= 1 of a batch from nothing over its own history first (the warm-up:
empty chains in front of h(c) = 32512 c, the tile's local position 0) and repairs that in rounds; a tile that enters where it entered last time stops
once its parse is past (highest changed history bit) + MAX_DIST having reproduced its old tokens.  Each case here makes one of those steps matter.

catalogue() returns RCase rows:

  name      unique
  family    guess | reach | entry | chain
  data      one continuous stream of at most 8 tiles (tile 0 holds 65024 positions, every other 32512)
  cfgs      "L1", "L2", "L3" (rows (4,4,8,4), (4,5,16,8), (4,6,32,32): max_insert_length 4, 5, 6) -- every family exists at all three levels
  claims    {cfg: [(position, token), ...]}: the token the reference must START at that position, (dist, len) or LIT
  pair      (group, side) or None: the two sides of a group must get different tokens at their probes (the token at the probe or the one behind a literal there)
  tile      the probe's tile c
  probe     the probe's position t (chain: the first claim's)
  chain     what chain_of(data, probe) must be (the candidate count is as built)
  guess     what the warm-up of tile `tile` makes of it, derived on the CPU by warm_account(): a parse of the stream's suffix from h(c) on is a parse from
            nothing.  Keys: q (the probe's candidate), stream / warm (is q in the chains by the stream's account / by the warm-up's), k (the highest
            history position on which the two accounts differ; everything above agrees), token (what the warm-up starts at the probe); entry cases
            also exits = (the predecessor's exit by its warm-up, by the stream), or exits3 = (tile exit_tile's exit by its own warm-up, by the parse that
            follows the warm-up of the tile in front, by the stream); chain cases travel (tiles the error travels over).

Families.
  guess   `ins`: a copy of a 40-byte word W ends `end` positions behind h(c), its source lies in front of h(c): the stream has ONE match (40 > every
          max_insert_length: its inside stays out of the chains), the warm-up, which cannot see the source, literals that it inserts.  The probe, among
          the tile's first own positions, repeats the 20 bytes at q; q is the match's last position (j = 1: the guess has q, the stream has not -- the
          reference starts a literal) or the first position behind it (j = 0: both have it).  q lies 32505 and 32506 in front of the probe, and 32507
          (out of reach for both parses).  end = 8 puts q = h + 7 and the probe of distance 32505 on the tile's first own position.
          `rev`: the reverse.  A match of the stream from a source in front of h(c) straddles the start of a copy of V, so the stream starts its next
          token at V's seventh byte (q, in the chains) while the warm-up takes the copy whole from its start (q inside a 40-byte match, not in the
          chains): the guess makes a literal of the probe, the reference a match.  The partner's q is the first position behind both matches.
          Both parses fall back into step at the first filler byte behind the scenario: filler never matches.
          A few rows put the probe's tile at c = 2 and c = 3 (run heads and followers of ZGPU_FAST_RUN = 2, 3).
  reach   the `ins` scenario with j = 1 in a stream of three tiles (c = 2): in round 1 the tile enters where its warm-up did, k = q is the highest
          changed bit, the probe at t = k + 32506 has k as its sole candidate (the parse must not stop AT t), its partner at k + 32507 nothing (the parse
          must stop early and be right).  t at window offsets 0, 1, 63 (end = 7, 8, 70), and in the tile's LAST window (end = 32490: the source of
          W lies just in front of h(c), 32500 in front of the copy -- the warm-up's account is wrong 32489 positions deep).
  entry   the `ins` probe (q at 32505; W's source just in front of h(1), the copy deep in tile 1's history) is the first position of a periodic run:
          from t, 1032 positions in front of tile 1's end, every byte repeats the one 32505 in front of it, to the stream's end 300 positions into
          tile 2.  Every candidate of the run lies in the filler in front of t, which is all literals: every token of the run is a 258-byte match, so
          the j literals the reference makes and the guess does not shift every token behind them, tile 1's exit included.  (end, j) = (31487, 1): the
          stream's token ends ON the tile edge, the guess's straddles it by 257; (31488, 1) and (31489, 2): the guess's ends on the edge, the
          stream's 1 and 2 behind it.  Tile 2 is parsed from one entry in round 1 and from another in round 2.  entry-back-19 (back_case) has an exit that
          moves and moves BACK: tile 2's is 0 by its warm-up, 19 in round 1 (parsed with tile 1's guessed bits) and 0 again in round 2.  (A run is short because it
          cannot be carried on by its own matches, whose insides are not in the chains, and because every bucket collision of the filler between a
          candidate and its string uses up level 1's budget of four.)
  chain   the `ins` probe in tile 1 and one probe in each of the tiles 2, 3, 4, 32507 apart (no divisor of 32512): each repeats the 20 bytes at the
          SECOND position of the probe in front of it, at distance 32506.  That position is in the chains when the probe in front came out as literals
          and is not when it came out as a match, so the reference alternates literal+match | match | literals | match, every tile's warm-up (which
          makes literals of the probe in front) says match, and a tile's answer flips each time the tile in front is repaired: tile c is exact
          after round c and not before, one round per tile.
feed_rows(case) lists the calls that put a feed's end 0, 1, 31, 32, 33 positions in front of the probe's tile, and a Z_SYNC_FLUSH (the claim stands) and a
Z_FULL_FLUSH (the window is forgotten: the candidate is NOT taken) at the tile's first position.

What is left out, and why:
  * "only the exit differs while every token the tile made is the same": a tile's exit is the end of its last token -- with the same entry and the
    same tokens it is the same exit; no input reaches that state (tests/test_round_cases_cpu.py recomputes the exits from the tokens);
  * tuned deflate_fast rows (the engine serves them in chunks), other memLevel / windowBits, batches beyond eight tiles (ZGPU_FAST_RUN stands in for
    the phases a large batch would take)."""
from collections import namedtuple

import numpy as np

from oracle.parsecases import FAST, LIT, MAX_DIST, MAXM, ROWS, Build, _stream, chain_of  # noqa: F401

TILE0, TILE = 65024, 32512
Z_NO_FLUSH, Z_SYNC_FLUSH, Z_FULL_FLUSH = 0, 2, 3
FEED_GAPS = (0, 1, 31, 32, 33)

LONG_FILLER = _stream(0, 44, 80000)  # parsecases' filler (its first 102000 bytes) carried on: 240000 bytes, still no trigram twice

RCase = namedtuple("RCase", "name family data cfgs claims pair tile probe chain guess")


def hist(c):
    """h(c): where tile c's history begins (its local position 0)."""
    assert c >= 1
    return TILE * c


def own(c):
    """tile c's first own position"""
    return 0 if c == 0 else TILE * (c + 1)


def ntiles(n):
    return 1 if n <= TILE0 else 1 + (n - TILE0 + TILE - 1) // TILE


def level_of(cfg):
    return int(cfg[1:])


# ---- the two accounts of a tile's history ----
def starts_of(toks):
    """(start position, length, dist) of every token of oracle_py.deflate_cont_tokens' record array"""
    ln = np.where(toks["dist"] != 0, toks["lc"].astype(np.int64) + 3, 1)
    st = np.zeros(len(ln), dtype=np.int64)
    st[1:] = np.cumsum(ln)[:-1]
    return st, ln, toks["dist"].astype(np.int64)


def inserted(n, st, ln, max_insert):
    """deflate_fast's chains from its tokens (deflate.c:1508-1530): every token start, and the inside of a match no longer than max_insert_length that
    leaves MIN_MATCH bytes behind it."""
    ins = np.zeros(n, dtype=bool)
    ins[st] = True
    for p, l in zip(st[(ln > 1) & (ln <= max_insert)].tolist(), ln[(ln > 1) & (ln <= max_insert)].tolist()):
        if n - p - l >= 3:
            ins[p + 1: p + l] = True
    return ins


def token_at(st, ln, dist, p):
    i = int(np.searchsorted(st, p))
    if i >= len(st) or st[i] != p:
        return None
    return (int(dist[i]), int(ln[i])) if dist[i] else LIT


def exit_at(st, ln, edge):
    """how far the token that reaches `edge` ends behind it"""
    i = int(np.searchsorted(st, edge, side="left"))
    if i < len(st) and st[i] == edge:
        return 0
    return int(st[i - 1] + ln[i - 1] - edge)


def warm_account(data, c, level, tokens):
    """tokens(bytes, level) -> record array.  Returns (stream's parse, the warm-up's parse in stream positions, stream's chains, warm-up's chains): the
    chains as bool arrays over stream positions (the warm-up's False in front of h(c))."""
    mi = ROWS[level][1]
    h = hist(c)
    s = starts_of(tokens(data, level))
    w = starts_of(tokens(data[h:], level))
    w = (w[0] + h, w[1], w[2])
    si = inserted(len(data), s[0], s[1], mi)
    wi = np.zeros(len(data), dtype=bool)
    wi[h:] = inserted(len(data) - h, w[0] - h, w[1], mi)
    return s, w, si, wi


def highest_difference(si, wi, c):
    """the highest position of tile c's history (local positions 6 .. 32511: what the tile proper can reach) on which the accounts differ, or None"""
    h = hist(c)
    d = np.nonzero(si[h + 6: h + TILE] != wi[h + 6: h + TILE])[0]
    return None if len(d) == 0 else int(h + 6 + d[-1])


# ---- builders ----
class RBuild(Build):
    """parsecases' Build over the longer filler (a stream of four tiles needs more than 102000 bytes of it)"""

    def fill(self, n):
        assert n >= 0 and self.cur + n <= len(LONG_FILLER)
        pos = len(self.buf)
        self.buf += LONG_FILLER[self.cur: self.cur + n].tobytes()
        self.isfill += b"\1" * n
        self.cur += n
        return pos


def _finish(b, name, family, claim, pair, c, probe, chain, guess, tail=None):
    data = b.done()
    if tail is not None:  # a periodic run behind what Build made (Build would patch its repeats away)
        q, period, n = tail
        x = data[q: q + period]
        data += (x * ((n - len(data)) // period + 1))[: n - len(data)]
    assert ntiles(len(data)) <= 8 and len(data) <= 300032, (name, len(data))
    assert chain_of(data, probe) == chain, (name, chain_of(data, probe), chain)
    return RCase(name, family, data, list(FAST), {cfg: list(claim) for cfg in FAST}, pair, c, probe, chain, guess)


def misled_ins(family, c, end, j, d, tag, run=False):
    """The `ins` scenario (module text).  run: the probe is the start of a periodic run (the entry family)."""
    h = hist(c)
    wl = max(40, end + 10) if end < 1000 else 40
    b = RBuild(skew=(7 * c + end + 3 * j + d) % 97)
    w, e = b.word(wl), b.word(24)
    text = w[wl - j:] + e[: 20 - j]
    for s in (w, e, text, text[1:], text[2:]):
        b.key(s)
    copy_at = h + end - wl
    gap = 32500 if end >= 1000 else min(32400, copy_at - 7)  # (32400: the source lies behind h(c - 1) as a whole, the warm-up of the tile in front sees all of it)
    assert copy_at - gap + wl <= h and (c == 1 or copy_at - gap >= hist(c - 1)), "the source must lie in front of h(c)"
    b.fill(copy_at - gap)
    b.put(w)
    b.fill(copy_at - len(b.buf))
    b.put(w + e)
    q = h + end - j
    t = q + d
    assert own(c) <= t < own(c) + TILE
    b.fill(t - len(b.buf))
    guess = {"q": q, "stream": int(j == 0), "warm": 1, "k": h + end - 1, "token": (d, 20) if d <= MAX_DIST else LIT}
    if run:
        assert j >= 1 and c == 1
        edge = own(c) + TILE
        n = edge + 300                      # (every candidate of the run lies in the part Build made, which is all literals)
        first = t + j                       # the stream's first 258-byte match; the guess's starts at t
        claim = [(t + i, LIT) for i in range(j)] + [(first, (d, MAXM))]
        sx, gx = (first - edge) % MAXM, (t - edge) % MAXM   # how far the token that reaches the edge ends behind it
        assert n <= t + d and max(sx, gx) < n - edge and edge - first <= 5 * MAXM
        claim.append((edge + sx, (d, MAXM)))
        guess["exits"] = (gx, sx)
        guess["token"] = (d, MAXM)
        return _finish(b, "%s-c%d-end%d-j%d%s" % (family, c, end, j, tag), family, claim, None, c, t, [q], guess, tail=(q, d, n))
    b.put(text)
    b.fill(300)  # (windows of the tile behind the probe's: a parse that may stop early has a window's top to do it at)
    if d > MAX_DIST:
        claim, chain = [(t + i, LIT) for i in range(3)], []
    elif j == 0:
        claim, chain = [(t, (d, 20))], [q]
    else:
        claim, chain = [(t + i, LIT) for i in range(j)] + [(t + j, (d, 20 - j))], [q]
    return b, claim, chain, guess, t, q


def ins_case(family, c, end, j, d, pair):
    b, claim, chain, guess, t, q = misled_ins(family, c, end, j, d, "")
    return _finish(b, "%s-ins-c%d-end%d-j%d-d%d" % (family, c, end, j, d), family, claim, pair, c, t, chain, guess)


def rev_case(c, j, d, pair):
    """The `rev` scenario (module text): S0 + V[:6] at h - 300, V at h + 50, S0 + V + F at h + 190."""
    h = hist(c)
    b = RBuild(skew=(11 * c + 5 * j + d) % 97)
    s0, v, f = b.word(10), b.word(40), b.word(24)
    text = v[6:26] if j else f[:20]
    for s in (s0, v, f, text, text[1:], v[6:]):
        b.key(s)
    b.fill(h - 300)
    b.put(s0 + v[:6])
    b.fill(h + 50 - len(b.buf))
    b.put(v)
    b.fill(h + 190 - len(b.buf))
    b.put(s0 + v + f)
    q = h + 206 if j else h + 240
    t = q + d
    assert own(c) <= t < own(c) + TILE
    b.fill(t - len(b.buf))
    b.put(text)
    b.fill(300)
    claim, chain = ([(t, (d, 20))], [q]) if d <= MAX_DIST else ([(t + i, LIT) for i in range(3)], [])
    guess = {"q": q, "stream": 1, "warm": int(j == 0), "k": h + 206, "token": (d, 20) if d <= MAX_DIST and j == 0 else LIT}
    return _finish(b, "guess-rev-c%d-j%d-d%d" % (c, j, d), "guess", claim, pair, c, t, chain, guess)


def chain_case(end=30, tiles=4):
    """The `ins` probe of tile 1 (t1, q at 32506), and in every tile behind it a probe 32507 behind the last one that repeats the 20 bytes at the last
    probe's SECOND position: its sole candidate, at 32506, is in the chains or not by what the tile in front made of ITS probe."""
    h = hist(1)
    b = RBuild(skew=53)
    w, e = b.word(40), b.word(24)
    g = [b.word(8) for _ in range(tiles)]
    texts = [w[39:] + e[:19]]
    for c in range(1, tiles):
        texts.append((texts[-1] + g[c - 1])[1:21])
    for s in [w, e] + texts + [t[1:] for t in texts]:
        b.key(s)
    copy_at = h + end - 40
    b.fill(copy_at - min(32500, copy_at - 7))
    b.put(w)
    b.fill(copy_at - len(b.buf))
    b.put(w + e)
    q = h + end - 1
    ts = [q + MAX_DIST + (MAX_DIST + 1) * c for c in range(tiles)]
    for c, t in enumerate(ts):
        assert own(c + 1) <= t < own(c + 1) + TILE and (c + 1 == tiles or t + 1 >= hist(c + 2) + 6)
        b.fill(t - len(b.buf))
        b.put(texts[c] + g[c])
    b.fill(40)
    claim, probes = [], []
    for c, t in enumerate(ts):  # the reference: literal + 19 | 20 | literals | 20 ...
        if c == 0:
            claim += [(t, LIT), (t + 1, (MAX_DIST, 19))]
        elif c % 2:
            claim += [(t, (MAX_DIST, 20))]
        else:
            claim += [(t + i, LIT) for i in range(3)]
        probes.append((c + 1, t, q if c == 0 else ts[c - 1] + 1))
    guess = {"q": q, "stream": 0, "warm": 1, "k": q, "travel": tiles, "probes": probes, "token": (MAX_DIST, 20)}  # (every tile's warm-up takes its probe's candidate: it made literals of the probe in front)
    return _finish(b, "chain-flip-%dtiles" % tiles, "chain", claim, None, 1, ts[0], [q], guess)


def back_case():
    """The entry family's exit that moves and moves BACK.  The `ins` probe t1 deep in tile 1 (the guess a 20-byte match, the reference a literal and 19 bytes:
    its second position t1 + 1 is in the chains only by the reference), and 32505 behind t1 + 1 the start t2 of a run that repeats the bytes from t1 + 1 on,
    four 258-byte matches in front of tile 2's end and 300 positions into tile 3.  Tile 2's warm-up makes literals of the probe at t1, as good as the reference
    for t1 + 1: its first exit E is the stream's.  In round 1 it has tile 1's GUESSED bits -- t1 + 1 .. t1 + 19 inside a match -- and its run starts 19 literals
    late: E' = E + 19.  In round 2 tile 1 is repaired and the exit is E again.  Tile 3 is entered at E, at E' and at E."""
    h = hist(1)
    d2 = MAX_DIST - 1
    edge = own(2) + TILE
    t2 = edge - 4 * MAXM
    t1 = t2 - d2 - 1
    q = t1 - MAX_DIST
    end = q + 1 - h
    b = RBuild(skew=57)  # (a stretch of the filler whose buckets leave level 1's four candidates to the run up to tile 2's end)
    w, e, g = b.word(40), b.word(24), b.word(8)
    text = w[39:] + e[:19]
    for s in (w, e, text, text[1:], text[2:], e[:19] + g):
        b.key(s)
    copy_at = h + end - 40
    assert copy_at - 32500 + 40 <= h and own(1) <= t1 and t1 + 1 >= hist(2) + 6
    b.fill(copy_at - 32500)
    b.put(w)
    b.fill(copy_at - len(b.buf))
    b.put(w + e)
    b.fill(t1 - len(b.buf))
    b.put(text + g)
    b.fill(t2 - len(b.buf))
    n = edge + 300
    claim = [(t1, LIT), (t1 + 1, (MAX_DIST, 19))] + [(t2 + i * MAXM, (d2, MAXM)) for i in range(4)]  # (the fourth match ends on tile 2's edge)
    guess = {"q": q, "stream": 0, "warm": 1, "k": q, "token": (MAX_DIST, 20), "exit_tile": 2, "exits3": (0, 19, 0), "run": (t2, t1 + 1)}
    return _finish(b, "entry-back-19", "entry", claim, None, 1, t1, [q], guess, tail=(t1 + 1, d2, n))


def feed_rows(case):
    """[(tag, calls, claims)] for a guess or reach case: calls = [(upto, flush)] as oracle_py.cont_stream takes them (Z_FINISH implied).  A feed that ends `gap`
    positions in front of the probe's tile; a sync flush and a full flush at the tile's first position -- behind the full flush nothing in front of it is a
    candidate any more."""
    at = own(case.tile)
    rows = [("more-%d" % g, [(at - g, Z_NO_FLUSH)], None) for g in FEED_GAPS]
    rows.append(("sync", [(at, Z_SYNC_FLUSH)], None))
    rows.append(("full", [(at, Z_FULL_FLUSH)], [(case.probe, LIT)]))
    return rows


def feed_cases():
    """the cases that go through feed_rows: the guess and reach probes nearest to the tile's first position, both sides"""
    pick = ("guess-ins-c1-end8-j1-d32505", "guess-ins-c1-end8-j1-d32506", "guess-ins-c1-end8-j0-d32506", "guess-rev-c1-j1-d32506",
            "reach-ins-c2-end7-j1-d32506", "reach-ins-c2-end7-j1-d32507")
    by = {c.name: c for c in catalogue()}
    return [by[n] for n in pick]


_catalogue = None


def catalogue():
    global _catalogue
    if _catalogue is None:
        _catalogue = build_catalogue()
    return _catalogue


def build_catalogue():
    out = []
    # guess: tile 1, both polarities, q at 32505 / 32506 / 32507; the inside and the outside of the long match are a pair, and so are 32506 | 32507
    for end in (8, 30):
        for d in (MAX_DIST - 1, MAX_DIST, MAX_DIST + 1):
            for j in (1, 0):
                out.append(ins_case("guess", 1, end, j, d, ("guess-ins-end%d-d%d" % (end, d), 1 - j) if d <= MAX_DIST else None))
    for j in (1, 0):
        for d in (MAX_DIST - 1, MAX_DIST, MAX_DIST + 1):
            out.append(rev_case(1, j, d, ("guess-rev-j%d" % j, int(d > MAX_DIST)) if d >= MAX_DIST else None))
    for c in (2, 3):
        out.append(ins_case("guess", c, 30, 1, MAX_DIST, None))
        out.append(rev_case(c, 1, MAX_DIST, None))
    # reach: three tiles, the probe ON the boundary and one position out of reach
    for end in (7, 8, 70, 32490):
        for d in (MAX_DIST, MAX_DIST + 1):
            out.append(ins_case("reach", 2, end, 1, d, ("reach-end%d" % end, int(d > MAX_DIST))))
    # entry: the predecessor's exit moves by 257, 1 and 2
    d = MAX_DIST - 1  # (a run's later candidates are never the first of their chains: 32506 is out of their reach, deflate.c:1163)
    end0 = (own(1) + TILE - hist(1) - d) % MAXM + 122 * MAXM  # the stream's first match of the run starts four whole matches in front of the tile edge
    for end, j in ((end0, 1), (end0 + 1, 1), (end0 + 2, 2)):
        out.append(misled_ins("entry", 1, end, j, d, "", run=True))
    out.append(back_case())
    out.append(chain_case())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
