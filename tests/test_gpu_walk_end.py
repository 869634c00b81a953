"""The end of a chunk in walk_kernel<1> (zgpu_lz_walk.hip): the last positions of a chunk of more than 32768 are handed to the walkers in blocks
of 32 and then of 16 positions instead of 64 (WalkTaper), and the fused tail behind the walkers reads the windows' logs.  These inputs sit where
that geometry changes -- chunk lengths around the threshold and around the two boundaries, a partial last block, chunks of a few bytes; long
matches laid across a boundary and across several short blocks -- and where the tail goes from one window to the next: logs that alternate between
empty and full, logs of exactly 0, 1, 1 023, 1 024 and 1 025 games (the cut-offs of the tail's rounds), a last window of one position, a match
token deferred from one window to the next.

Every input goes through the default path in independent chunks of at most 64 KiB, with `last` 0 and 1, in groups of at most 16 chunks a launch,
and is compared byte for byte with the compiled reference where oracle/_ref is there (the CPU restatement otherwise) and with LZ_SORTED, which
shares none of this code.  The boundaries come from the engine itself (zgpu_walk_block_map), so the inputs follow the shipped values.  The plain
tests at the end check on the CPU that the inputs are what they claim."""
import ctypes as C
import functools

import pytest

from oracle import cases, oracle_py as O, refzlib as R

gpu_test = pytest.mark.gpu

WIN, CHUNK, WALKERS, BLK = 8192, 65536, 512, 64
Z_FILTERED = 1
# name -> (level, strategy).  Level 4's budgets (chain 16, a quarter of it 4) are no multiples of eight: the kernel's `vexact` form.
CONFIGS = {"L4": (4, 0), "L6": (6, 0), "L9": (9, 0), "L6-filtered": (6, Z_FILTERED)}
KINDS = ["text", "mix", "runs", "zeros", "period", "rand"]
TINY = [1, 2, 3, 63, 64, 65]


@functools.lru_cache(maxsize=None)
def block_map(n):
    """(b32, b16, blocks) of a chunk of n positions: blocks of 64 below b32, of 32 in [b32, b16), of 16 from b16 on."""
    import zlib_amd
    L = zlib_amd.load_library()
    out = (C.c_uint32 * 3)()
    L.zgpu_walk_block_map(C.c_uint32(n), out)
    return int(out[0]), int(out[1]), int(out[2])


def block_starts(n):
    b32, b16, nblk = block_map(n)
    s = list(range(0, b32, BLK)) + list(range(b32, b16, 32)) + list(range(b16, n, 16))
    assert len(s) == nblk
    return s


def taper_lengths():
    """Chunk lengths on both sides of every place the geometry changes."""
    b32, b16, _ = block_map(CHUNK)
    ns = [WALKERS * BLK, WALKERS * BLK + 1]                                     # no more blocks than walkers: uniform; one more position: tapered
    ns += [b + d for b in (b32, b16) for d in (-64, -1, 1, 64)]                 # a chunk that ends next to a full chunk's boundary
    ns += [CHUNK - 1, CHUNK - 17, CHUNK]                                        # the last block of 16 partial; a full chunk
    return sorted(set(n for n in ns if 0 < n <= CHUNK)) + TINY


class Filler:
    """Bytes in which no three-byte string occurs twice (cases.nomatch), handed out piece by piece."""

    def __init__(self):
        self.src, self.at = cases.nomatch(32768), 0

    def take(self, n):
        assert self.at + n <= len(self.src)
        self.at += n
        return self.src[self.at - n: self.at]


def planted(n, seed):
    """n bytes to plant: pairs of bytes below and above 128, which neither cases.nomatch() (they alternate there) nor the text (all below) contains."""
    r = cases.make("rand", n, seed)
    return bytes((b & 0x7F) | (0x80 if (k >> 1) & 1 else 0) for k, b in enumerate(r))


def across_boundaries():
    """A full chunk of text with 258-byte repeats of one string (first copy 20000 in front of the first boundary): one that starts 3 bytes in front of each boundary of the taper,
    and one laid over the blocks of 16 from 5 bytes behind a block's start -- a walker that stands on none of the starts of the blocks it crosses.
    The byte in front of each copy occurs nowhere else, so each is reached with nothing in hand.  Returns (data, [(position, distance)])."""
    b32, b16, _ = block_map(CHUNK)
    d = bytearray(cases.make("text", CHUNK, 91))
    rep = planted(258, 7)
    q = b32 - 20000
    d[q - 1] = 0xF0
    d[q: q + 258] = rep
    d[q + 258] = 0xF1
    at = [b32 - 3, b16 - 3, b16 + 1024 + 5]
    for k, p in enumerate(at):
        d[p - 1] = 0xF2 + k
        d[p: p + 258] = rep
        d[p + 258] = 0xF8 + k
    return bytes(d), [(p, p - q if k == 0 else p - at[k - 1]) for k, p in enumerate(at)]


def plant_repeats(d, lo, hi, count, seed):
    """`count` 12-byte repeats inside [lo, hi) of the bytearray d: the first copy 40 bytes in front of the second.  Returns [(position, distance, length)]."""
    out, step = [], (hi - lo - 200) // count
    for k in range(count):
        q = lo + 64 + k * step
        r = planted(12, seed + k)
        d[q - 1], d[q + 12] = 0xF0, 0xF1
        d[q: q + 12] = r
        d[q + 39], d[q + 52] = 0xF2, 0xF3
        d[q + 40: q + 52] = r
        out.append((q + 40, 40, 12))
    return out


def nomatch_windows(k):
    """k windows in which no three-byte string has an earlier copy within reach: cases.nomatch() repeats after 32768 bytes, beyond MAX_DIST."""
    return (cases.nomatch(32768) * 2)[: k * WIN]


def ends_only():
    """Random bytes with planted repeats in windows 0 and 7, windows 1 to 6 of bytes without a match: six empty logs between two that are not."""
    # (seed 47: no three bytes of the first window recur, by chance, in the windows behind it -- test_window_inputs_are_what_they_claim)
    d = bytearray(cases.make("rand", WIN, 47) + nomatch_windows(6) + cases.make("rand", WIN, 42))
    plants = plant_repeats(d, 0, WIN, 40, 100) + plant_repeats(d, 7 * WIN, CHUNK, 40, 200)
    return bytes(d), plants


def zeros_between():
    """A window of zeros (a game at every other position: the fullest log a run makes) between two of random bytes, then text."""
    return cases.make("rand", WIN, 43) + bytes(WIN) + cases.make("rand", WIN, 44) + cases.make("text", WIN + 77, 45)


def debruijn(k, n):
    """The lexicographically least de Bruijn sequence B(k, n) (Lyndon words): every n-gram once, every (n-1)-gram k times."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1: p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def debruijn_then_empty():
    """Five windows of B(6, 6) -- a five-byte match at every position, walkers that do not meet: logs that are full at level 9 -- and an empty one behind."""
    return bytes(97 + v for v in debruijn(6, 6))[: 5 * WIN] + nomatch_windows(1)


def deferred(seed, first_k):
    """Text in which, at every window edge e = 8192 w, a game starts k = 1, 2 or 3 positions in front of e (k cycling from first_k) and ends with a long
    match that starts AT e: at e - k + j (j < k) the longest match has 4 + j bytes, which the lazy evaluation gives up for the longer one a position
    further, and at e it has 203.  The match token belongs to the next window than its game: the tail's deferred token.
    Returns (data, [(edge, k, distance of the match at the edge)])."""
    d = bytearray(cases.make("text", CHUNK, seed))
    claims = []
    for w in range(1, CHUNK // WIN):
        e, k = w * WIN, (first_k + w - 1) % 3 + 1
        T = planted(k + 3, seed * 100 + w) + planted(200, seed * 100 + 50 + w)   # the string at e - k; T[k:] is the long match at e
        at = e - 4000
        for j in range(k):                                                        # a copy of T[j: j + 4 + j], then a byte that differs
            d[at - 1] = 0xF0 + j
            d[at: at + 4 + j] = T[j: j + 4 + j]
            d[at + 4 + j] = T[j + 4 + j] ^ 0x3C
            at += 16
        d[at - 1] = 0xF8
        d[at: at + len(T) - k] = T[k:]
        d[at + len(T) - k] = 0xF9
        d[e - k - 1] = 0xFA
        d[e - k: e - k + len(T)] = T
        d[e - k + len(T)] = 0xFB
        claims.append((e, k, e - at))
    return bytes(d), claims


def counted(k_a, k_b):
    """Four windows (n = 32768: uniform blocks of 64): bytes without a match, window 1 with exactly k_a and window 3 with exactly k_b planted six-byte
    repeats, each a copy of six bytes of the (empty) window in front of it.  Eight repeats fill a block of 64 positions from its second position on,
    eight positions apart; the 1 025th comes from one block that holds nine, seven apart.  No block start lies inside a planted match, and where no
    byte has a match a walker goes from neutral position to neutral position until it stands on one that is claimed: every position is visited
    once, by the walker of its block, and every planted match is ONE game in its window's log.  So the count of window w + 1 that the tail's prefetch
    and stage 1's rounds cut off at (512 entries a round of A1, 1 024 positions a round of stage 1) is exactly k: 0, 1, 1 023, 1 024, 1 025.
    The CPU side can pin the match tokens (= the games on the path) and that no walker starts inside a match; that the log holds nothing else follows
    from the argument above, not from a count the CPU could read.  Returns (data, {window: [(position, distance)]})."""
    nm = cases.nomatch(32768)
    d, plants = bytearray(nm), {}
    for k, wsrc, wdst in ((k_a, 0, 1), (k_b, 2, 3)):
        base, cells = wdst * WIN, []
        if k > 1024:
            cells += [base + 64 + 1 + 7 * j for j in range(9)]
        for b in range(WIN // 64):
            if not (k > 1024 and b == 1):
                cells += [base + 64 * b + 2 + 8 * j for j in range(8)]
        cells = sorted(cells)[:k]
        assert len(cells) == k
        out = []
        for j, p in enumerate(cells):
            s = wsrc * WIN + 3 + 6 * j
            d[p: p + 6] = nm[s: s + 6]
            if p + 6 < len(d) and d[p + 6] == nm[s + 6]:   # (six bytes and no more, in front and behind)
                d[p + 6] ^= 1
            if d[p - 1] == nm[s - 1]:
                d[p - 1] ^= 1
            out.append((p, p - s))
        plants[wdst] = out
    return bytes(d), plants


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> bytes, claims (name -> what the CPU tests check), groups (name -> names, at most 16 chunks a launch)."""
    ins, claims, groups = {}, {}, {}
    for kind in KINDS:
        for n in taper_lengths():
            ins["%s-%d" % (kind, n)] = cases.make(kind, n, 5)
    geo = list(ins)
    for i in range(0, len(geo), 16):
        groups["geometry-%d" % (i // 16)] = geo[i: i + 16]
    ins["across"], claims["across"] = across_boundaries()
    ins["ends-only"], claims["ends-only"] = ends_only()
    ins["zeros-between"] = zeros_between()
    ins["debruijn-empty"] = debruijn_then_empty()
    for k in (1, 7):
        ins["text-%d" % (WIN * k + 1)] = cases.make("text", WIN * k + 1, 6)
    # (which lane owns a deferred token is the index of its game in its window's log modulo 512, and that index is the order in which the walkers
    # finished their games: no input controls it.  Six texts with some 1 250 logged games a window in front of each of their seven deferred games
    # spread the owner over the lanes by chance, not by construction.)
    for s, fk in ((61, 0), (62, 1), (63, 2), (64, 0), (65, 1), (66, 2)):
        ins["deferred-%d" % (s - 61)], claims["deferred-%d" % (s - 61)] = deferred(s, fk)
    for ka, kb in ((1, 1023), (1024, 1025)):
        ins["count-%d-%d" % (ka, kb)], claims["count-%d-%d" % (ka, kb)] = counted(ka, kb)
    groups["across"] = ["across"]
    groups["windows"] = ["ends-only", "zeros-between", "debruijn-empty", "text-%d" % (WIN + 1), "text-%d" % (7 * WIN + 1)]
    groups["deferred"] = ["deferred-%d" % i for i in range(6)]
    # counts of window w + 1 of 0, 1, 1 023, 1 024, 1 025 behind an empty window, and behind a full one (the run of zeros) in a chunk of their own
    ins["count-behind-full"] = ins["count-1024-1025"][:WIN] + bytes(WIN) + ins["count-1024-1025"][WIN: 2 * WIN]   # (the copies now from two windows back)
    groups["counts"] = ["count-1-1023", "count-1024-1025", "count-behind-full"]
    # neighbouring workgroups at different stages: full and empty logs, short and full chunks, side by side in one launch
    groups["sixteen"] = ["zeros-between", "ends-only", "debruijn-empty", "deferred-0", "zeros-%d" % CHUNK, "across", "text-%d" % (WIN + 1), "rand-%d" % CHUNK,
                         "deferred-1", "ends-only", "runs-%d" % (CHUNK - 17), "debruijn-empty", "text-%d" % (7 * WIN + 1), "deferred-2", "mix-%d" % CHUNK, "text-3"]
    assert all(1 <= len(g) <= 16 and all(n in ins and len(ins[n]) <= CHUNK for n in g) for g in groups.values())
    return ins, claims, groups


N_GEOMETRY = (len(KINDS) * (13 + len(TINY)) + 15) // 16   # (13 lengths at most besides the tiny ones; test_groups_are_complete checks that none is left out)
GROUPS = ["geometry-%d" % i for i in range(N_GEOMETRY)] + ["across", "windows", "deferred", "counts", "sixteen"]
_ref_cache = {}


def reference(cfg, name, last):
    """The reference's raw chunk for one input (computed once per configuration and ending)."""
    key = (cfg, name, last)
    if key not in _ref_cache:
        level, strategy = CONFIGS[cfg]
        data = inputs()[0][name]
        _ref_cache[key] = R.deflate_chunk_raw(data, level, last, strategy=strategy) if R.available() else O.deflate_chunk(data, level, last, strategy=strategy)
    return _ref_cache[key]


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


@gpu_test
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_chunks(eng, cfg, group):
    from zlib_amd import gpu
    ins, _, groups = inputs()
    names = groups.get(group, [])   # (a geometry group past the last one is empty)
    level, strategy = CONFIGS[cfg]
    for last in (0, 1):
        if not names:
            break
        want = [reference(cfg, n, bool(last)) for n in names]
        got, sorted_ = [eng.deflate_segments_host([ins[n] for n in names], level, flags=gpu.F_FINAL if last else 0, lz_impl=impl, strategy=strategy)
                        for impl in (gpu.LZ_AUTO, gpu.LZ_SORTED)]
        for n, w, g, s in zip(names, want, got, sorted_):
            assert g == w, (cfg, n, last, "default path differs from the reference", len(g), len(w))
            assert s == g, (cfg, n, last, "default path differs from LZ_SORTED")


# ------------------------------------------------------------------ the inputs are what they claim (CPU restatement, level 6; no GPU)
def tokens_at(data, level=6):
    _, _, toks = O.deflate_chunk(data, level, True, want_tokens=True)
    pos, at = 0, {}
    for dist, lc in toks:
        at[pos] = (dist, lc)
        pos += lc + 3 if dist else 1
    return at


def matches_by_window(at):
    """Match tokens of the parse by the window they start in: each is the end of one game on the path (the logs hold these and the games off it)."""
    c = [0] * (CHUNK // WIN)
    for p, (dist, _) in at.items():
        if dist:
            c[p // WIN] += 1
    return c


def test_groups_are_complete():
    ins, _, groups = inputs()
    assert set(groups) == set(GROUPS)
    assert {n for g in groups.values() for n in g} == set(ins)


def test_taper_geometry_is_what_it_claims():
    """The block map the engine reports: uniform blocks up to 512 of them, then blocks of 64, 32 and 16 that tile the chunk, and the lengths of this
    file on both sides of every change."""
    for n in (1, 63, 64, 65, WALKERS * BLK - 1, WALKERS * BLK):
        assert block_map(n) == (n, n, (n + BLK - 1) // BLK), n
    ns = taper_lengths()
    assert WALKERS * BLK in ns and WALKERS * BLK + 1 in ns and CHUNK - 1 in ns and CHUNK - 17 in ns and len(ns) == 13 + len(TINY)
    b32, b16, nblk = block_map(CHUNK)
    assert 0 < b32 < b16 < CHUNK and b32 % 64 == 0 and b16 % 32 == 0
    assert {b + d for b in (b32, b16) for d in (-64, -1, 1, 64)} <= set(ns)
    for n in ns:
        a32, a16, blocks = block_map(n)
        s = block_starts(n)
        assert s[0] == 0 and all(0 < y - x <= BLK for x, y in zip(s, s[1:])) and 0 < n - s[-1] <= BLK, n
        if n > WALKERS * BLK:
            assert blocks > WALKERS and a32 % 64 == 0 and a16 % 32 == 0 and a32 <= a16 <= n, n
            assert CHUNK - b32 <= n - a32 <= CHUNK - b32 + 63 and CHUNK - b16 <= n - a16 <= CHUNK - b16 + 31, n
    assert (CHUNK - 1 - block_starts(CHUNK - 1)[-1], CHUNK - 17 - block_starts(CHUNK - 17)[-1]) == (15, 15)


def test_matches_across_boundaries_are_what_they_claim():
    d, plants = inputs()[0]["across"], inputs()[1]["across"]
    at = tokens_at(d)
    b32, b16, _ = block_map(CHUNK)
    starts = set(block_starts(CHUNK))
    assert [p for p, _ in plants] == [b32 - 3, b16 - 3, b16 + 1024 + 5]
    for p, dist in plants:
        assert at[p] == (dist, 258 - 3), (p, at.get(p))
    p = plants[2][0]
    inside = [s for s in starts if p < s < p + 258]
    assert p not in starts and len(inside) >= 4 and all(y - x == 16 for x, y in zip(sorted(inside), sorted(inside)[1:]))
    assert all(s not in at for s in inside)   # the parse stands on none of them


def test_window_inputs_are_what_they_claim():
    ins, claims, _ = inputs()
    at = tokens_at(ins["ends-only"])
    for p, dist, n in claims["ends-only"]:
        assert at[p] == (dist, n - 3), (p, at.get(p))
    c = matches_by_window(at)
    assert c[0] >= 40 and c[7] >= 40 and c[1:7] == [0] * 6, c
    # (matches_by_window counts the games ON THE PATH; the logs also hold the games off it -- 4 096 for a window of zeros, all 8 192 positions of a de Bruijn
    # window at level 9: scripts/walk_log_stats.py on the GPU -- which no CPU restatement plays.  Exact log counts: test_counted_windows_are_what_they_claim.)
    c = matches_by_window(tokens_at(ins["zeros-between"]))
    assert c[1] == (WIN - 1 + 257) // 258 and c[0] < 20 and c[2] < 20, c   # the run's path: a match of 258 after the first literal; its walkers play 4096 games
    d = ins["debruijn-empty"]
    at = tokens_at(d)
    c = matches_by_window(at)
    assert len(d) == 6 * WIN and c[5] == 0 and all(x > 1000 for x in c[1:5]), c
    assert all(at[p][0] == 0 for p in at if p >= 5 * WIN + 8)
    assert [len(ins["text-%d" % (WIN * k + 1)]) % WIN for k in (1, 7)] == [1, 1]


def test_counted_windows_are_what_they_claim():
    """Exactly k match tokens -- the planted ones, six bytes each -- in the counted windows, none in the windows in front of them, and no block start
    inside a planted match (a walker that started there would log a game of its own)."""
    ins, claims, _ = inputs()
    for name, ks in (("count-1-1023", (1, 1023)), ("count-1024-1025", (1024, 1025))):
        d, plants = ins[name], claims[name]
        assert len(d) == 4 * WIN and block_map(len(d))[2] == WALKERS
        starts = block_starts(len(d))
        for level in (4, 6, 9):
            at = tokens_at(d, level)
            assert matches_by_window(at)[:4] == [0, ks[0], 0, ks[1]], (name, level)
            for w in (1, 3):
                assert len(plants[w]) == ks[(w - 1) // 2]
                for p, dist in plants[w]:
                    assert at[p] == (dist, 6 - 3) and p // WIN == w, (name, level, p, at.get(p))
        for w in (1, 3):
            for p, _ in plants[w]:
                assert not any(p < s < p + 6 for s in starts[p // 64: p // 64 + 2]), (name, p)
    # behind a full window: the run's path is a match of 258 after the first literal (its walkers play a game at every other position)
    at = tokens_at(ins["count-behind-full"])
    c = matches_by_window(at)
    assert c[:3] == [0, (WIN - 1 + 257) // 258, 1024] and block_map(3 * WIN)[2] == 3 * WIN // BLK, c
    assert all(at[p + WIN] == (dist + WIN, 6 - 3) for p, dist in claims["count-1024-1025"][1])


def test_deferred_inputs_are_what_they_claim():
    ins, claims, _ = inputs()
    seen = set()
    for fk in range(6):
        d, cl = ins["deferred-%d" % fk], claims["deferred-%d" % fk]
        at = tokens_at(d)
        assert [e for e, _, _ in cl] == [w * WIN for w in range(1, 8)]
        for e, k, dist in cl:
            seen.add((e, k))
            for j in range(k):   # literals in front of the edge: the game that starts at e - k gives its matches up one by one
                assert at[e - k + j] == (0, d[e - k + j]), (fk, e, k, j, at.get(e - k + j))
            assert at[e] == (dist, 203 - 3), (fk, e, k, at.get(e))
    assert seen == {(w * WIN, k) for w in range(1, 8) for k in (1, 2, 3)}
