"""walk_kernel's fold and pass (zgpu_lz_walk.hip): a parked candidate is compared with its owner's scan string, whose position and first eight
bytes come out of the owner's registers; the scan string's two quick-check bytes are read with the candidates'; a pass issues its two LDS
atomics together.  These inputs put matches on the seams of that code: lengths around the eight bytes held in registers, at every alignment of
owner and candidate; matches cut by the end of the chunk; owners in the last lanes of a wave while a fold has one to three entries; a best
length that moves from body to body of one search; searches that start with a match in hand; passes in which every lane emits, or none.

Every input goes through the default path in independent chunks of at most 64 KiB, with `last` 0 and 1, and is compared byte for byte with the
compiled reference where oracle/_ref is there (the CPU restatement otherwise) and with LZ_SORTED, which shares none of this code.  The inputs that
reach walk_kernel<2> go through F_CONTINUOUS as one stream.  The plain tests at the end check on the CPU that the inputs are what they claim."""
import ctypes as C

import pytest

from oracle import cases, oracle_py as O, refzlib as R

gpu_test = pytest.mark.gpu

CHUNK, MAX_DIST = 65536, 32506
Z_FILTERED = 1
# name -> (level, strategy, deflateTune's good_length, max_lazy, nice_length, max_chain).  Level 4 (chain 16, a quarter of it 4) and the tuned row
# (chain 30, a quarter 7) have budgets that are no multiples of eight: the kernel's `vexact` form.  The tuned row's nice_length of 32 lies inside
# the ladder's lengths, level 6's 128 outside.
CONFIGS = {"L4": (4, 0, None), "L6": (6, 0, None), "L9": (9, 0, None), "L6-filtered": (6, Z_FILTERED, None), "L6-tuned": (6, 0, (8, 16, 32, 30))}
REPEATS = [3, 7, 8, 9, 15, 16, 17, 257, 258]


class Filler:
    """Bytes in which no three-byte string occurs twice (cases.nomatch), handed out piece by piece."""

    def __init__(self):
        self.src, self.at = cases.nomatch(32768), 0

    def take(self, n):
        assert self.at + n <= len(self.src)
        self.at += n
        return self.src[self.at - n: self.at]


def planted(n, seed):
    """n bytes to plant: in cases.nomatch() bytes below and above 128 alternate, here they come in pairs -- no three of these occur in the filler."""
    r = cases.make("rand", n, seed)
    return bytes((b & 0x7F) | (0x80 if (k >> 1) & 1 else 0) for k, b in enumerate(r))


def lcp(d, a, b, limit=None):
    """Bytes that d[a:] and d[b:] have in common (b > a), up to the end of d and to `limit`."""
    n = 0
    while b + n < len(d) and d[a + n] == d[b + n] and (limit is None or n < limit):
        n += 1
    return n


def seam():
    """1. A repeat of every length in REPEATS, at every owner position mod 4, after a candidate at an even and at an odd position (over the lengths:
    every pair of alignments).  The bytes in front of and behind the two copies differ.  Returns (data, [(owner position, candidate position, length)])."""
    f, d, plants, seed = Filler(), bytearray(), [], 1000
    d += f.take(16)
    for li, n in enumerate(REPEATS):
        for pm in range(4):
            for par in (0, 1):
                r = planted(n, seed)
                seed += 1
                d += f.take(12)
                while (len(d) + 1) % 4 != (2 * pm + par + li) % 4:
                    d += f.take(1)
                d += b"\xF2"
                q = len(d)
                d += r + b"\xF1" + f.take(12)
                while (len(d) + 1) % 4 != pm:
                    d += f.take(1)
                d += b"\x0D"
                p = len(d)
                d += r + b"\x0E"
                plants.append((p, q, n))
    d += f.take(16)
    return bytes(d), plants


def cut_by_the_end(k):
    """2. A 17-byte string whose second copy is cut by the end of the chunk after k bytes: the scan position is k bytes in front of the end."""
    f = Filler()
    r = planted(17, 2000 + k)
    d = f.take(119 + k) + b"\xF2" + r + b"\xF1" + f.take(60) + b"\x0D" + r[:k]
    return d, len(d) - k, 120 + k


def last_lanes(blocks):
    """3. Random bytes with a 12-byte repeat at the first position of each of `blocks` (blocks of 64 positions).  Block b of a wave's first hand-out
    goes to lane b mod 64: the lanes of a wave that has no block yet ask for 64 at once (one atomic on ctrl[0] by the first lane, the kernel's
    hand-out code) and lane L takes the L-th of them; the wave whose atomic comes first gets blocks 0..63.  The walker of block b searches at 64 * b
    straight away, so these searches are owned by the lanes 61, 62 and 63 while nearly nothing else in the wave parks a candidate."""
    d = bytearray(cases.make("rand", 8192, 31))
    plants = []
    for b in blocks:
        q = 1000 + 40 * (b - 60)
        d[64 * b: 64 * b + 12] = d[q: q + 12]
        d[64 * b - 1], d[64 * b + 12] = d[q - 1] ^ 0xFF, d[q + 12] ^ 0xFF
        plants.append((64 * b, q, 12))
    return bytes(d), plants


def ladder(descending):
    """4. One scan string T at P whose chain holds 76 candidates that match its first 3, 3, 4, 4, ... 40, 40 bytes, the nearest first (or 40 ... 3 with
    `descending`): several bodies of eight, and the best length moves in between.  Returns (data, P, [(candidate position, bytes in common)] nearest first)."""
    f = Filler()
    T = planted(48, 3000)
    lens = [n for n in range(3, 41) for _ in (0, 1)]
    if descending:
        lens.reverse()
    d, cands = bytearray(f.take(64)), []
    for i, n in enumerate(reversed(lens)):  # laid out farthest first
        cands.append((len(d), n))
        d += T[:n] + bytes([T[n] ^ 0x55]) + f.take(6 + i % 4) + b"\xF2"
    d += f.take(300) + b"\x0D"
    P = len(d)
    d += T + f.take(40)
    cands.reverse()
    return bytes(d), P, cands


def lazy_near():
    """5a. A four-byte match at p that the lazy evaluation gives up for a 203-byte match at p + 1: the search at p + 1 starts with four bytes in hand."""
    f = Filler()
    u, s = planted(4, 4000), planted(200, 4001)
    d = bytearray(f.take(100))
    d += u + b"\xF1" + f.take(50) + b"\xF4"
    b = len(d)
    d += u[1:] + s + b"\xF2" + f.take(50) + b"\x0D"
    p = len(d)
    d += u + s + b"\xF3" + f.take(20)
    return bytes(d), p, b


def at_max_dist(D, seeded):
    """5b, 5c. 64 KiB of random bytes in which the FIRST candidate of a search lies exactly D back.
    not seeded: a 40-byte repeat at distance D, searched with nothing in hand.
    seeded: a four-byte repeat at p at distance D; the search at p + 1 then starts with those four bytes in hand, and its first candidate is the position
    behind the first one's, again D back (three bytes in common: it cannot improve).
    A search with a match in hand whose first candidate is the LONGER one cannot be built: the four bytes at p come from some a >= p - MAX_DIST, and a + 1
    is in the chain of p + 1 in front of anything further back.  So the longer match at p + 1 comes second in its chain (lazy_far)."""
    d = bytearray(cases.make("rand", CHUNK, 50 + D % 7 + 10 * seeded))
    p = 40000
    q = p - D
    r = planted(4 if seeded else 40, 5000 + seeded)
    d[q - 1], d[p - 1] = 0x11, 0x22
    d[q: q + len(r)] = r
    d[p: p + len(r)] = r
    d[q + len(r)], d[p + len(r)] = 0x33, 0x44
    return bytes(d), p, q


def lazy_far(D):
    """5d. A four-byte match at p from 100 back, and a 60-byte match at p + 1 whose candidate lies D back, SECOND in its chain: within reach only if
    D < MAX_DIST (deflate.c:1163), where a first candidate is within reach at MAX_DIST as well."""
    d = bytearray(cases.make("rand", CHUNK, 70 + D % 7))
    p = 40000
    u, s = planted(4, 6000), planted(60, 6001)
    d[p - 100: p - 95] = u + b"\xF1"
    b = p + 1 - D
    d[b - 1] = 0x11
    d[b: b + 63] = u[1:] + s
    d[b + 63] = 0x33
    d[p - 1] = 0x22
    d[p: p + 64] = u + s
    d[p + 64] = 0x44
    return bytes(d), p, b


INPUTS, CLAIMS = {}, {}
INPUTS["seam"], CLAIMS["seam"] = seam()
for _k in range(1, 10):
    INPUTS["cut-%d" % _k], CLAIMS["cut-%d" % _k] = (lambda t: (t[0], t[1:]))(cut_by_the_end(_k))
_r3, _r4 = planted(3, 2100), planted(4, 2101)
INPUTS["tiny-3"], INPUTS["tiny-8"], INPUTS["tiny-9"] = _r3, b"\x0D" + _r3 + _r3 + _r3[:1], b"\x0D" + _r4 + _r4  # (position 0 is no candidate)
INPUTS["lanes-3"], CLAIMS["lanes-3"] = last_lanes((61, 62, 63))
INPUTS["lanes-1"], CLAIMS["lanes-1"] = last_lanes((63,))
for _n, _desc in (("ladder-up", False), ("ladder-down", True)):
    INPUTS[_n], CLAIMS[_n] = (lambda t: (t[0], t[1:]))(ladder(_desc))
INPUTS["lazy-near"], CLAIMS["lazy-near"] = (lambda t: (t[0], t[1:]))(lazy_near())
for _D in (MAX_DIST, MAX_DIST + 1):
    for _s in (0, 1):
        _n = "first-%d-%s" % (_D, "seeded" if _s else "plain")
        INPUTS[_n], CLAIMS[_n] = (lambda t: (t[0], t[1:]))(at_max_dist(_D, _s))
for _D in (MAX_DIST - 1, MAX_DIST):
    INPUTS["lazy-far-%d" % _D], CLAIMS["lazy-far-%d" % _D] = (lambda t: (t[0], t[1:]))(lazy_far(_D))
INPUTS["zeros"] = bytes(CHUNK)
INPUTS["period2"] = (b"xy" * (CHUNK // 2 + 1))[:CHUNK]
INPUTS["period5"] = (b"abcde" * (CHUNK // 5 + 1))[:CHUNK]
INPUTS["rand"] = cases.make("rand", CHUNK, 4)
CONTINUOUS = (INPUTS["seam"] + INPUTS["ladder-up"] + INPUTS["ladder-down"] + INPUTS["zeros"] + INPUTS["period2"] + INPUTS["period5"] + INPUTS["rand"])[: 4 * CHUNK]

GROUPS = {
    "seam": ["seam"],
    "cut": ["cut-%d" % k for k in range(1, 10)] + ["tiny-3", "tiny-8", "tiny-9"],
    "lanes": ["lanes-3", "lanes-1"],
    "ladder": ["ladder-up", "ladder-down"],
    "lazy": ["lazy-near"] + [n for n in INPUTS if n.startswith("first-") or n.startswith("lazy-far-")],
    "games": ["zeros", "period2", "period5", "rand"],
}
assert all(1 <= len(g) <= 16 and all(len(INPUTS[n]) <= CHUNK for n in g) for g in GROUPS.values())
_ref_cache = {}


def ref_tuned_chunk(data, level, tune, last):
    L = R.lib()
    L.deflateTune.argtypes = [C.POINTER(R.ZStream), C.c_int, C.c_int, C.c_int, C.c_int]
    s = R.ZStream()
    assert L.deflateInit2_(C.byref(s), level, 8, -15, 8, 0, b"1.2.3", C.sizeof(R.ZStream)) == 0
    assert L.deflateTune(C.byref(s), *tune) == 0
    cap = len(data) + (len(data) >> 8) + 256
    out = C.create_string_buffer(cap)
    inb = C.create_string_buffer(data, max(len(data), 1))
    s.next_in = C.addressof(inb); s.avail_in = len(data); s.next_out = C.addressof(out); s.avail_out = cap
    rc = L.deflate(C.byref(s), R.Z_FINISH if last else R.Z_FULL_FLUSH)
    assert rc == (1 if last else 0) and s.avail_in == 0
    z = out.raw[: s.total_out]
    L.deflateEnd(C.byref(s))
    return z


def reference(cfg, name, last):
    """The reference's raw chunk for one input (computed once per configuration and ending)."""
    key = (cfg, name, last)
    if key not in _ref_cache:
        level, strategy, tune = CONFIGS[cfg]
        data = INPUTS[name]
        if R.available():
            z = ref_tuned_chunk(data, level, tune, last) if tune else R.deflate_chunk_raw(data, level, last, strategy=strategy)
        else:
            z = O.deflate_chunk(data, level, last, strategy=strategy, tune=tune)
        _ref_cache[key] = z
    return _ref_cache[key]


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.set_tuning(None)
    e.close()


def run_segments(eng, cfg, names, last, impl):
    from zlib_amd import gpu
    level, strategy, tune = CONFIGS[cfg]
    eng.set_tuning(tune)
    try:
        return eng.deflate_segments_host([INPUTS[n] for n in names], level, flags=gpu.F_FINAL if last else 0, lz_impl=impl, strategy=strategy)
    finally:
        eng.set_tuning(None)


@gpu_test
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_chunks(eng, cfg, group):
    from zlib_amd import gpu
    names = GROUPS[group]
    for last in (0, 1):
        want = [reference(cfg, n, bool(last)) for n in names]
        got = run_segments(eng, cfg, names, last, gpu.LZ_AUTO)
        sorted_ = run_segments(eng, cfg, names, last, gpu.LZ_SORTED)
        for n, w, g, s in zip(names, want, got, sorted_):
            assert g == w, (cfg, n, last, "default path differs from the reference", len(g), len(w))
            assert s == g, (cfg, n, last, "default path differs from LZ_SORTED")


@gpu_test
@pytest.mark.parametrize("level", [4, 6, 9])
def test_continuous_stream(eng, level):
    """Inputs 1, 4 and 6 as one stream of 256 KiB: the tiles' walkers (walk_kernel<2>) against compress2()."""
    from zlib_amd import gpu
    one = eng.deflate_host(CONTINUOUS, level, flags=gpu.F_FINAL | gpu.F_ZLIB_WRAP | gpu.F_CONTINUOUS)
    want = R.compress2(CONTINUOUS, level) if R.available() else O.cont_stream(CONTINUOUS, level)
    assert one == want, (level, len(one), len(want))


# ------------------------------------------------------------------ the inputs are what they claim (CPU restatement, level 6; no GPU)
def tokens_at(data, level=6, tune=None):
    _, _, toks = O.deflate_chunk(data, level, True, want_tokens=True, tune=tune)
    pos, at = 0, {}
    for dist, lc in toks:
        at[pos] = (dist, lc)
        pos += lc + 3 if dist else 1
    return at


def test_seam_repeats_are_what_they_claim():
    d, plants = INPUTS["seam"], CLAIMS["seam"]
    at = tokens_at(d)
    assert sorted({n for _, _, n in plants}) == REPEATS
    for n in REPEATS:
        assert {(p % 4, q % 2) for p, q, m in plants if m == n} == {(a, b) for a in range(4) for b in (0, 1)}
    assert {(p % 4, q % 4) for p, q, _ in plants} == {(a, b) for a in range(4) for b in range(4)}
    for p, q, n in plants:
        assert lcp(d, q, p) == n and d[p - 1] != d[q - 1], (p, q, n)
        assert at[p] == (p - q, n - 3), (p, q, n, at.get(p))


def test_cut_inputs_are_what_they_claim():
    for k in range(1, 10):
        d, (p, q) = INPUTS["cut-%d" % k], CLAIMS["cut-%d" % k]
        assert p == len(d) - k and lcp(d, q, p) == k and d[p - 1] != d[q - 1]
        at = tokens_at(d)
        assert at[p] == ((p - q, k - 3) if k >= 3 else (0, d[p])), (k, at.get(p))
    assert [len(INPUTS[n]) for n in ("tiny-3", "tiny-8", "tiny-9")] == [3, 8, 9]
    assert tokens_at(INPUTS["tiny-8"])[4] == (3, 1) and tokens_at(INPUTS["tiny-9"])[5] == (4, 1)


def test_lane_inputs_are_what_they_claim():
    for name, blocks in (("lanes-3", (61, 62, 63)), ("lanes-1", (63,))):
        d, plants = INPUTS[name], CLAIMS[name]
        at = tokens_at(d)
        assert [p for p, _, _ in plants] == [64 * b for b in blocks]
        for p, q, n in plants:
            assert lcp(d, q, p) == n and d[p - 1] != d[q - 1]
            assert at[p] == (p - q, n - 3), (name, p, at.get(p))


def test_ladders_are_what_they_claim():
    for name, first, nearest_len in (("ladder-up", 3, 3), ("ladder-down", 40, 40)):
        d, (P, cands) = INPUTS[name], CLAIMS[name]
        assert len(cands) >= 72 and cands[0][1] == first and all(a[0] > b[0] for a, b in zip(cands, cands[1:]))
        assert sorted({n for _, n in cands}) == list(range(3, 41))
        for pos, n in cands:
            assert lcp(d, pos, P) == n, (name, pos, n)
        # level 6 (nice_length 128, chain 128): the longest, the nearest among equals; the tuned row stops at the first candidate of 32 bytes or more
        best = next(pos for pos, n in cands if n == 40)
        assert tokens_at(d)[P] == (P - best, 40 - 3)
        nice = next((pos, n) for pos, n in cands[:30] if n >= 32) if name == "ladder-down" else None
        if nice:
            assert tokens_at(d, tune=CONFIGS["L6-tuned"][2])[P] == (P - nice[0], nice[1] - 3)


def test_lazy_inputs_are_what_they_claim():
    d, (p, b) = INPUTS["lazy-near"], CLAIMS["lazy-near"]
    at = tokens_at(d)
    assert at[p] == (0, d[p]) and at[p + 1] == (p + 1 - b, 203 - 3)
    # the two distances of a search's first candidate: MAX_DIST is within reach, MAX_DIST + 1 is not
    for D, seeded, n in ((32506, 0, 40), (32507, 0, 40), (32506, 1, 4), (32507, 1, 4)):
        d, (p, q) = INPUTS["first-%d-%s" % (D, "seeded" if seeded else "plain")], CLAIMS["first-%d-%s" % (D, "seeded" if seeded else "plain")]
        assert p - q == D and lcp(d, q, p) == n and d[p - 1] != d[q - 1]
        assert tokens_at(d)[p] == ((D, n - 3) if D == 32506 else (0, d[p])), (D, seeded)
    # a second candidate: MAX_DIST is out of reach
    for D in (32505, 32506):
        d, (p, b) = INPUTS["lazy-far-%d" % D], CLAIMS["lazy-far-%d" % D]
        at = tokens_at(d)
        assert p + 1 - b == D and lcp(d, b, p + 1) == 63 and lcp(d, p - 100, p) == 4
        if D == 32505:
            assert at[p] == (0, d[p]) and at[p + 1] == (D, 63 - 3)
        else:
            assert at[p] == (100, 4 - 3)
