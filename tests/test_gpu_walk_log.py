"""walk_kernel<1> hands its games to the fused parse as one log per window of 8192 positions (zgpu_lz_parse.h, LOG).  These inputs sit on the
edges of that geometry: lengths around a window and a chunk, matches and games that straddle a window edge, logs that are nearly full (walkers
that do not meet) and logs that are empty.  Every case goes through the default path in independent 64 KiB chunks and is compared byte for byte
with the compiled reference where oracle/_ref is there (the CPU restatement otherwise), and with the same input through LZ_SORTED, which shares
none of the log code.  Bit-exact or fail."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

from oracle import cases, oracle_py as O, refzlib as R  # noqa: E402

WIN, CHUNK = 8192, 65536
Z_FILTERED, Z_FIXED = 1, 4
# name -> (level, strategy, deflateTune).  The tuned row is level 5's (deflate.c:137-149) on a level 6 stream: a raw chunk depends on the level only
# through that row and the compress function, so the CPU restatement of level 5 stands in where the compiled reference is missing.
CONFIGS = {"L4": (4, 0, None), "L6": (6, 0, None), "L9": (9, 0, None), "L6-filtered": (6, Z_FILTERED, None), "L6-fixed": (6, Z_FIXED, None),
           "L6-tuned": (6, 0, (8, 16, 32, 32))}
TUNED_AS_LEVEL = 5

LENGTHS = [0, 1, 2, 3, WIN - 1, WIN, WIN + 1, WIN + 258, 2 * WIN, CHUNK - 1, CHUNK]


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


def straddle():
    """Text with (a) a 258-byte repeat whose match starts at 8192 - 3 and ends in the next window, and (b) a game that starts at 16383, the last
    position of window 1, while the match it ends with starts at 16384 (a four-byte match at 16383 that the lazy evaluation gives up for a long
    one at 16384: the deferred token).  The bytes in front of both are unique, so both positions are reached with nothing in hand."""
    d = bytearray(cases.make("text", CHUNK, 77))
    rep = cases.make("rand", 258, 5)
    d[999] = 0xFE
    d[1000:1258] = rep
    d[WIN - 4] = 0xFF
    d[WIN - 3: WIN - 3 + 258] = rep
    s = cases.make("rand", 200, 6)
    u = bytes([0xF0, 0xF1, 0xF2, 0xF3])
    d[2000:2005] = u + b"\xF4"          # u0 u1 u2 u3, then a byte that is not s[0]
    d[3000:3003 + 200] = u[1:] + s      # u1 u2 u3 s
    d[2 * WIN - 2] = 0xFD
    d[2 * WIN - 1: 2 * WIN + 3 + 200] = u + s
    return bytes(d)


def build_inputs():
    ins = {"len-%d" % n: cases.make("text", n, 3) for n in LENGTHS}
    ins["straddle"] = straddle()
    ins["zeros"] = bytes(CHUNK)
    ins["period2"] = (b"xy" * (CHUNK // 2 + 1))[:CHUNK]
    ins["period5"] = (b"abcde" * (CHUNK // 5 + 1))[:CHUNK]
    ins["run-then-rand"] = b"r" * WIN + cases.make("rand", CHUNK - WIN, 9)
    # walkers that never meet: every 6-gram of B(6, 6) is new and (almost) every 5-gram has been seen, so the match at every position is five
    # bytes long -- a step that is odd, while walkers start 64 apart: paths from different blocks cover every position of a window before they
    # coincide.  (Zeros and short periods step by 258 and fill exactly the even half of a log.)  Measured with scripts/walk_log_stats.py: the fullest
    # log of this input holds 7397 of 8192 entries at level 6 (90%) and all 8192 at level 9; zeros and the periods 4096 to 4128, text about 1250.
    ins["debruijn"] = bytes(97 + v for v in debruijn(6, 6))
    ins["rand"] = cases.make("rand", CHUNK, 4)
    return ins


INPUTS = build_inputs()
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
            z = O.deflate_chunk(data, TUNED_AS_LEVEL if tune else level, last, strategy=strategy)
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


def check_group(eng, cfg, names):
    from zlib_amd import gpu
    for last in (0, 1):
        want = [reference(cfg, n, bool(last)) for n in names]
        got = run_segments(eng, cfg, names, last, gpu.LZ_AUTO)
        sorted_ = run_segments(eng, cfg, names, last, gpu.LZ_SORTED)
        for n, w, g, s in zip(names, want, got, sorted_):
            assert g == w, (cfg, n, last, "default path differs from the reference", len(g), len(w))
            assert s == g, (cfg, n, last, "default path differs from LZ_SORTED")


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_lengths_around_window_and_chunk(eng, cfg):
    check_group(eng, cfg, ["len-%d" % n for n in LENGTHS])


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_two_chunks_second_nearly_empty(eng, cfg):
    """65536 + 5 bytes through the chunked call: the second chunk's logs hold nothing (or one game)."""
    from zlib_amd import gpu
    level, strategy, tune = CONFIGS[cfg]
    data = cases.make("text", CHUNK + 5, 3)
    eng.set_tuning(tune)
    try:
        outs = [eng.deflate_host(data, level, flags=gpu.F_FINAL, lz_impl=impl, want_offsets=True, strategy=strategy) for impl in (gpu.LZ_AUTO, gpu.LZ_SORTED)]
    finally:
        eng.set_tuning(None)
    (z, offs), (zs, offs_s) = outs
    INPUTS.setdefault("two-a", data[:CHUNK]); INPUTS.setdefault("two-b", data[CHUNK:])
    want = reference(cfg, "two-a", False) + reference(cfg, "two-b", True)
    assert z == want, (cfg, len(z), len(want))
    assert [int(o) for o in offs] == [0, len(reference(cfg, "two-a", False)), len(want)]
    assert zs == z and list(offs_s) == list(offs)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_match_and_game_across_a_window_edge(eng, cfg):
    check_group(eng, cfg, ["straddle"])


def test_straddle_input_is_what_it_claims():
    """The level 6 tokens of the straddle input (CPU restatement): a 258-byte match at 8192 - 3, a literal at 16383 and a match at 16384."""
    _, _, toks = O.deflate_chunk(INPUTS["straddle"], 6, True, want_tokens=True)
    pos, at = 0, {}
    for dist, lc in toks:
        at[pos] = (dist, lc)
        pos += lc + 3 if dist else 1
    assert at[WIN - 3] == (WIN - 3 - 1000, 258 - 3)
    assert at[2 * WIN - 1][0] == 0 and at[2 * WIN] == (2 * WIN - 3000, 203 - 3)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_full_and_empty_logs(eng, cfg):
    check_group(eng, cfg, ["zeros", "period2", "period5", "run-then-rand", "debruijn", "rand"])


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_sixteen_chunks_full_and_empty_side_by_side(eng, cfg):
    """One launch of 16 chunks that mixes all of the above: the stream, the chunk offsets and the Adler-32 against the reference."""
    from zlib_amd import gpu
    level, strategy, tune = CONFIGS[cfg]
    full = lambda n: INPUTS[n] + cases.make("text", CHUNK - len(INPUTS[n]), 8)  # noqa: E731 (every chunk but the last is 64 KiB)
    order = ["zeros", "rand", "debruijn", "len-65536", "period2", "rand", "straddle", "zeros", "run-then-rand", "period5", "rand", "debruijn", "len-8193", "straddle",
             "rand", "len-8191"]
    chunks = [full(n) for n in order[:-1]] + [INPUTS[order[-1]]]
    data = b"".join(chunks)
    eng.set_tuning(tune)
    try:
        z, offs = eng.deflate_host(data, level, flags=gpu.F_FINAL, lz_impl=gpu.LZ_AUTO, want_offsets=True, strategy=strategy)
        adler = eng.last.adler32
        zs = eng.deflate_host(data, level, flags=gpu.F_FINAL, lz_impl=gpu.LZ_SORTED, strategy=strategy)
    finally:
        eng.set_tuning(None)
    want = []
    for k, c in enumerate(chunks):
        INPUTS["mix-%d" % k] = c
        want.append(reference(cfg, "mix-%d" % k, k == len(chunks) - 1))
    ends = [0]
    for w in want:
        ends.append(ends[-1] + len(w))
    assert [int(o) for o in offs] == ends, cfg
    for k in range(len(chunks)):
        assert z[ends[k]: ends[k + 1]] == want[k], (cfg, k, order[k])
    assert adler == (R.adler32(data) if R.available() else O.adler32(data))
    assert zs == z
