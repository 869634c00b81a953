"""The match-search catalogue (oracle/parsecases.py) through every LZ77 implementation of the device: candidates that sit ON a threshold of
longest_match / deflate_slow / deflate_fast -- chain budget (whole and quarter, multiples of eight and not), nice_length, max_lazy, TOO_FAR,
MAX_DIST for the first and for a later candidate, max_insert_length -- placed in the open, on a walker block edge, on a log window edge and,
as one continuous stream, on a tile edge.  Compared with tests/golden/parse_kat.json (the compiled reference, oracle/gen_golden_parse.py),
bit-exact; what fails is reported by case name.  One launch per (configuration, implementation, ending).

The deflateTune rows no level's row resembles (parsecases.EDGE_SLOW / EDGE_FAST: a quarter budget of 0, budgets that never run out, good_length 0..3, max_lazy 0..3,
max_lazy > nice_length, nice_length 0..3 and above 258, max_insert_length on either side of nice_length) go the same way.  The default path and the
lane-per-chunk loop serve every one of them, and so do the walkers on deflate_slow; where another implementation rests on a relation the row breaks, the plan
refuses that pair (refuses(), pinned by tests/test_deflate_plan_cpu.py) and the test asserts the refusal."""
import hashlib

import pytest

pytestmark = pytest.mark.gpu

from oracle import parsecases as P  # noqa: E402


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.set_tuning(None)
    e.close()


@pytest.fixture(scope="module")
def gold(golden):
    return golden("parse_kat.json")["cases"]


def candidates(cfg):
    """Every implementation of the configuration's compress function and strategy (zgpu_deflate_plan.h plan_deflate: LZ_PARALLEL the default strategy only; Z_RLE is
    a chain budget of the all-position search, so neither the walkers nor the level 1-3 kernels on sorted buckets take it)."""
    from zlib_amd import gpu
    k = P.CONFIGS[cfg]
    if k.level <= 3:
        return [gpu.LZ_AUTO, gpu.LZ_SERIAL] + ([] if k.strategy == P.Z_RLE else [gpu.LZ_FAST, gpu.LZ_FASTWIN])
    if k.strategy == P.Z_RLE:
        return [gpu.LZ_AUTO, gpu.LZ_SORTED, gpu.LZ_SERIAL]
    return [gpu.LZ_AUTO, gpu.LZ_WALK, gpu.LZ_SORTED, gpu.LZ_SERIAL] + ([gpu.LZ_PARALLEL] if k.strategy == 0 else [])


def refuses(cfg, impl):
    """The (row, implementation) pairs plan_deflate refuses with a message of its own (records_refuse, fast_refuse, fastwin_row_serves): the relation between
    deflateTune's four parameters that the implementation rests on, restated from the row.  Never the default path, the loop or the walkers."""
    from zlib_amd import gpu
    k = P.CONFIGS[cfg]
    if not k.tune or k.strategy in (P.Z_RLE, 2):
        return False
    good, lazy, nice, chain = k.tune
    nice, chain = min(nice, P.MAXM), chain or 0xffffffff
    if impl in (gpu.LZ_SORTED, gpu.LZ_PARALLEL):
        return chain < 4 or (lazy > nice and nice < P.MAXM) or (chain > 4096 and impl == gpu.LZ_SORTED)
    if impl == gpu.LZ_FAST:
        return lazy > 7 or good <= 2
    if impl == gpu.LZ_FASTWIN:
        return not (good == 4 and lazy < nice and (chain, nice) in ((4, 8), (8, 16), (32, 32)))
    return False


def impls(cfg):
    """Every implementation the plan serves the configuration with."""
    return [i for i in candidates(cfg) if not refuses(cfg, i)]


def serial_ok(cfg, case):
    """The one exclusion: the serial kernel walks the ladders of levels 8 and 9 (1024 and 4096 decoys, every one of them a search through all
    the decoys in front of it) with one lane -- minutes.  Every other implementation runs them, the default path and LZ_WALK run every case."""
    ladder = case.family in ("chain", "quarter") or (case.family == "placed" and case.name.startswith("chain-"))
    return not (ladder and cfg in ("L8", "L9"))


def test_only_the_stated_exclusion():
    from zlib_amd import gpu
    cat = P.catalogue()
    for cfg in P.CONFIGS:
        assert gpu.LZ_AUTO in impls(cfg) and (P.CONFIGS[cfg].level <= 3 or P.CONFIGS[cfg].strategy == P.Z_RLE or gpu.LZ_WALK in impls(cfg))
    left_out = [(cfg, c.name) for c in cat for cfg in c.cfgs if not serial_ok(cfg, c)]
    assert left_out and all(cfg in ("L8", "L9") and ("chain-" in n or "quarter-" in n) for cfg, n in left_out)
    assert {cfg for c in cat for cfg in c.cfgs} == set(P.CONFIGS)
    # the rows no level's row resembles: the default path and the loop run every one, the walkers every one on deflate_slow; what is refused is this table
    for cfg in list(P.EDGE_SLOW) + list(P.EDGE_FAST):
        assert gpu.LZ_AUTO in impls(cfg) and gpu.LZ_SERIAL in impls(cfg) and (cfg in P.EDGE_FAST or gpu.LZ_WALK in impls(cfg)), cfg
    records = {"Q3", "Q2", "Q1", "Q3-L4", "Q3-L9", "LN258", "LN64", "N0", "N2", "N3"}
    table = {(cfg, i) for cfg in records for i in (gpu.LZ_SORTED, gpu.LZ_PARALLEL)} | {("U0", gpu.LZ_SORTED), ("U70000", gpu.LZ_SORTED)}
    table |= {(cfg, gpu.LZ_FAST) for cfg in ("I8", "I258", "I31-L3", "I32-L3", "I258-L3", "FG2", "FG2U")}
    table |= {(cfg, gpu.LZ_FASTWIN) for cfg in ("I8", "I258", "I32-L3", "I258-L3", "FG2", "FG2U")}
    assert {(cfg, i) for cfg in P.CONFIGS for i in candidates(cfg) if refuses(cfg, i)} == table
    assert not any(refuses(cfg, i) for cfg in P.CONFIGS if cfg not in P.EDGE_SLOW and cfg not in P.EDGE_FAST for i in candidates(cfg))


@pytest.mark.parametrize("cfg", list(P.CONFIGS))
def test_chunk_cases_vs_golden(eng, gold, cfg):
    from zlib_amd import gpu
    k = P.CONFIGS[cfg]
    cases = [c for c in P.catalogue() if cfg in c.cfgs and not c.cont]
    assert cases
    bad = []
    eng.set_tuning(k.tune)
    try:
        for impl in impls(cfg):
            cs = [c for c in cases if impl != gpu.LZ_SERIAL or serial_ok(cfg, c)]
            for last in (0, 1):
                flags = (gpu.F_FINAL if last else 0) | (gpu.F_POS0_ALL if k.p0 else 0)
                segs = eng.deflate_segments_host([c.data for c in cs], k.level, flags=flags, lz_impl=impl, strategy=k.strategy)
                for c, z in zip(cs, segs):
                    want = gold[c.name]["out"][cfg][last]
                    if [len(z), h16(z)] != want:
                        bad.append((c.name, "impl %d" % impl, "last %d" % last, len(z), want[0]))
        for impl in candidates(cfg):
            if refuses(cfg, impl):  # an explicit request for an implementation that rests on a relation the row breaks fails cleanly
                with pytest.raises(gpu.EngineError, match="deflateTune|ZGPU_LZ_FASTWIN serves"):
                    eng.deflate_segments_host([c.data for c in cases[:2]], k.level, flags=gpu.F_FINAL, lz_impl=impl, strategy=k.strategy)
    finally:
        eng.set_tuning(None)
    assert not bad, (cfg, len(bad), bad[:24])


@pytest.mark.parametrize("cfg", ["L%d" % k for k in range(1, 10)] + P.CONT_EDGE)
def test_placed_cases_as_one_continuous_stream(eng, gold, cfg):
    from zlib_amd import gpu
    k = P.CONFIGS[cfg]
    cases = [c for c in P.catalogue() if cfg in c.cfgs and (c.cont or cfg in gold[c.name].get("cont", {}))]
    assert (cfg not in P.CONT_CFGS + P.CONT_EDGE or sum(c.cont for c in cases) >= 12) and sum(not c.cont for c in cases) >= 12
    bad = []
    eng.set_tuning(k.tune)
    try:
        for c in cases:
            z = eng.deflate_host(c.data, k.level, flags=gpu.F_FINAL | gpu.F_CONTINUOUS, strategy=k.strategy)
            want = gold[c.name]["out" if c.cont else "cont"][cfg]
            if [len(z), h16(z)] != want:
                bad.append((c.name, len(z), want[0]))
    finally:
        eng.set_tuning(None)
    assert not bad, (cfg, len(bad), bad[:24])


def host_tuned(data, level, tune):
    """The host library as an application drives it: deflateInit2 (raw), deflateTune, one deflate(Z_FINISH)."""
    import ctypes as C

    import zhost
    L = zhost.lib()
    L.deflateTune.argtypes = [C.POINTER(zhost.ZStream), C.c_int, C.c_int, C.c_int, C.c_int]
    s = zhost.ZStream()
    assert L.deflateInit2_(C.byref(s), level, 8, -15, 8, 0, b"1.2.3", C.sizeof(zhost.ZStream)) == zhost.Z_OK
    try:
        assert L.deflateTune(C.byref(s), *tune) == zhost.Z_OK
        cap = len(data) + (len(data) >> 3) + 1024
        out, src = C.create_string_buffer(cap), C.create_string_buffer(data, max(len(data), 1))
        s.next_in, s.avail_in, s.next_out, s.avail_out = C.addressof(src), len(data), C.addressof(out), cap
        assert L.deflate(C.byref(s), zhost.Z_FINISH) == zhost.Z_STREAM_END and s.avail_in == 0
        return out.raw[: s.total_out]
    finally:
        L.deflateEnd(C.byref(s))


@pytest.mark.parametrize("cfg", P.CONT_EDGE + list(P.EDGE_FAST))
def test_host_library_behind_deflateTune(gold, cfg):
    """deflateInit2 + deflateTune(row) + deflate(Z_FINISH) of the host library.  A level 6 row: the reference's one continuous stream (the golden file's).  A
    level 1-3 row: served in independent chunks -- every case here is one chunk, so the stream is the restatement's chunk stream under the tuned row, which
    the golden file holds as the reference's own as well."""
    from oracle import oracle_py as O
    k = P.CONFIGS[cfg]
    bad = []
    if k.level > 3:
        cases = [c for c in P.catalogue() if cfg in c.cfgs and (c.cont or cfg in gold[c.name].get("cont", {}))]
        assert len(cases) >= 24
        for c in cases:
            z = host_tuned(c.data, k.level, k.tune)
            want = gold[c.name]["out" if c.cont else "cont"][cfg]
            if [len(z), h16(z)] != want:
                bad.append((c.name, len(z), want[0]))
    else:
        cases = [c for c in P.catalogue() if cfg in c.cfgs and not c.cont]
        assert len(cases) >= 4 and all(len(c.data) <= 65536 for c in cases)
        for c in cases:
            z = host_tuned(c.data, k.level, k.tune)
            want = O.deflate_chunk(c.data, k.level, True, tune=k.tune)
            assert [len(want), h16(want)] == gold[c.name]["out"][cfg][1], c.name
            if z != want:
                bad.append((c.name, len(z), len(want)))
    assert not bad, (cfg, len(bad), bad[:24])
