"""The match-search catalogue (oracle/parsecases.py) through every LZ77 implementation of the device: candidates that sit ON a threshold of
longest_match / deflate_slow / deflate_fast -- chain budget (whole and quarter, multiples of eight and not), nice_length, max_lazy, TOO_FAR,
MAX_DIST for the first and for a later candidate, max_insert_length -- placed in the open, on a walker block edge, on a log window edge and,
as one continuous stream, on a tile edge.  Compared with tests/golden/parse_kat.json (the compiled reference, oracle/gen_golden_parse.py),
bit-exact; what fails is reported by case name.  One launch per (configuration, implementation, ending)."""
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


def impls(cfg):
    """Every implementation that serves the configuration (zgpu_deflate_plan.h plan_deflate: LZ_PARALLEL the default strategy only; Z_RLE is a chain budget of
    the all-position search, so neither the walkers nor the level 1-3 kernels on sorted buckets take it)."""
    from zlib_amd import gpu
    k = P.CONFIGS[cfg]
    if k.level <= 3:
        return [gpu.LZ_AUTO, gpu.LZ_SERIAL] + ([] if k.strategy == P.Z_RLE else [gpu.LZ_FAST, gpu.LZ_FASTWIN])
    if k.strategy == P.Z_RLE:
        return [gpu.LZ_AUTO, gpu.LZ_SORTED, gpu.LZ_SERIAL]
    return [gpu.LZ_AUTO, gpu.LZ_WALK, gpu.LZ_SORTED, gpu.LZ_SERIAL] + ([gpu.LZ_PARALLEL] if k.strategy == 0 else [])


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
    finally:
        eng.set_tuning(None)
    assert not bad, (cfg, len(bad), bad[:24])


@pytest.mark.parametrize("cfg", ["L%d" % k for k in range(1, 10)])
def test_placed_cases_as_one_continuous_stream(eng, gold, cfg):
    from zlib_amd import gpu
    k = P.CONFIGS[cfg]
    cases = [c for c in P.catalogue() if cfg in c.cfgs and (c.cont or cfg in gold[c.name].get("cont", {}))]
    assert (cfg not in P.CONT_CFGS or sum(c.cont for c in cases) >= 12) and sum(not c.cont for c in cases) >= 12
    bad = []
    for c in cases:
        z = eng.deflate_host(c.data, k.level, flags=gpu.F_FINAL | gpu.F_CONTINUOUS, strategy=k.strategy)
        want = gold[c.name]["out" if c.cont else "cont"][cfg]
        if [len(z), h16(z)] != want:
            bad.append((c.name, len(z), want[0]))
    assert not bad, (cfg, len(bad), bad[:24])
