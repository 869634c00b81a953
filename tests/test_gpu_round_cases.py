"""The round catalogue (oracle/roundcases.py) through the level 1-3 tile rounds of the one continuous stream (zgpu_lz_fastwin.hip fastwin_tile_kernel,
zgpu_deflate_cont.hip lz_tiles_fast): streams whose warm-up guesses a history bit wrong, whose deciding candidate sits exactly MAX_DIST behind the
first token that can still see a changed bit, whose predecessor's exit moves between rounds, and whose repair travels one tile per round.  Compared with
tests/golden/round_kat.json (the compiled reference, oracle/gen_golden_rounds.py) bit for bit; a mismatch is reported as the first differing TOKEN.
Which way a tile went is read from the engine's counters (Engine.fast_round_counts, ZGPU_FAST_STATS): the conditions below follow from how the cases
are built, they are not measurements.  tests/test_round_cases_cpu.py shows, without a GPU, that every guess IS wrong where its case says."""
import hashlib
import os
import subprocess
import sys
import zlib

import pytest

pytestmark = pytest.mark.gpu

from oracle import blockwalk as BW, oracle_py as O, parsecases as P, roundcases as RC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("ZGPU_FAST_RUN", "ZGPU_CONT_BATCH_TILES", "ZGPU_CONT_PIPE", "ZGPU_FAST_STATS", "ZGPU_FAST_TRACE", "ZGPU_FW_RING", "ZGPU_FAST_KEEP", "ZGPU_FAST_FORCE_ROUNDS")


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gold(golden):
    return golden("round_kat.json")["cases"]


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def stream(eng, c, cfg):
    from zlib_amd import gpu
    return eng.deflate_host(c.data, RC.level_of(cfg), flags=gpu.F_FINAL | gpu.F_CONTINUOUS)


def explain(c, cfg, z):
    """the first token of z that is not the restatement's"""
    st, ln, dist = RC.starts_of(O.deflate_cont_tokens(c.data, RC.level_of(cfg))[1])
    return BW.first_token_difference(z, list(zip(st.tolist(), dist.tolist(), ln.tolist())))


def differing(eng, gold, cases, what=""):
    """[(case, level, first differing token)] over the cases at every level they are for"""
    bad = []
    for c in cases:
        for cfg in c.cfgs:
            z = stream(eng, c, cfg)
            if [len(z), h16(z)] != gold[c.name]["out"][cfg]:
                bad.append((what, c.name, cfg, explain(c, cfg, z)))
    return bad


@pytest.mark.parametrize("cfg", P.FAST)
def test_catalogue_vs_golden(eng, gold, cfg):
    bad = []
    for c in RC.catalogue():
        z = stream(eng, c, cfg)
        if [len(z), h16(z)] != gold[c.name]["out"][cfg]:
            bad.append((c.name, explain(c, cfg, z)))
        else:
            assert zlib.decompress(z, -15) == c.data, c.name
    assert not bad, (cfg, len(bad), bad[:8])


def test_paths_by_counter(eng, gold, monkeypatch, capsys):
    """Conditions of the construction (module text of oracle/roundcases.py).  One batch per call (at most 8 tiles), ZGPU_FAST_RUN unset: K = 1."""
    monkeypatch.setenv("ZGPU_FAST_STATS", "1")
    seen, bad = {}, []
    for c in RC.catalogue():
        nt = RC.ntiles(len(c.data))
        for cfg in c.cfgs:
            a = eng.fast_round_counts()
            z = stream(eng, c, cfg)
            b = eng.fast_round_counts()
            d = {k: b[k] - a[k] for k in b}
            assert [len(z), h16(z)] == gold[c.name]["out"][cfg], (c.name, cfg, explain(c, cfg, z))
            seen.setdefault(c.family, []).append((c.name, cfg, d["rounds"], d["tile_parses"], d["same_entry"], d["stopped_early"], d["different_token"]))
            if d["rounds"] > nt + 1:   # a tile is exact after as many rounds as its index, plus the round that finds no change
                bad.append((c.name, cfg, "rounds", d["rounds"], nt))
            # out of reach: tile 1 (nothing changed) and the probe's tile (nothing within reach) stop early -- but for a probe in the tile's last window, behind
            # which no window's top is left to stop at
            last_window = c.probe >= RC.own(c.tile) + RC.TILE - 64
            if c.family == "reach" and c.probe - c.guess["k"] == P.MAX_DIST + 1 and d["stopped_early"] < (1 if last_window else 2):
                bad.append((c.name, cfg, "no early stop", d))
            if c.family == "reach" and c.probe - c.guess["k"] == P.MAX_DIST and d["different_token"] < 1:
                bad.append((c.name, cfg, "no different token", d))
            if c.family == "guess" and c.tile == 1 and c.guess["stream"] != c.guess["warm"] and c.probe - c.guess["q"] <= P.MAX_DIST and d["different_token"] < 1:
                bad.append((c.name, cfg, "no different token", d))
            if c.family == "entry" and d["stopped_early"] != 0:  # tile 1 meets a different token, tile 2 is entered anew twice
                bad.append((c.name, cfg, "an early stop", d))
            if c.family == "entry" and d["rounds"] < 3:
                bad.append((c.name, cfg, "rounds", d))
            if "exits3" in c.guess and (d["rounds"] < 4 or d["different_token"] < 2):  # the tile behind the one whose exit moves back is entered three times, in rounds 1, 2, 3;
                bad.append((c.name, cfg, "rounds", d))                                  # the tile whose exit moves meets a different token in rounds 1 and 2
            if c.family == "chain" and d["rounds"] < c.guess["travel"]:
                bad.append((c.name, cfg, "rounds", d["rounds"], c.guess["travel"]))
    with capsys.disabled():
        for fam, rows in sorted(seen.items()):
            for key, label in ((2, "rounds"), (5, "stopped early"), (6, "different token")):
                vals = sorted({r[key] for r in rows})
                print("round cases, %s: %s %s" % (fam, label, vals))
    assert not bad, (len(bad), bad[:8])
    monkeypatch.delenv("ZGPU_FAST_STATS")
    a = eng.fast_round_counts()
    stream(eng, RC.catalogue()[0], "L1")
    b = eng.fast_round_counts()
    assert b["rounds"] > a["rounds"] and b["tile_parses"] > a["tile_parses"] and all(b[k] == a[k] for k in list(b)[2:])  # (without the knob the kernel counts nothing)
    assert eng.L.zgpu_deflate_fast_count(eng.h, 99) == 0 and eng.L.zgpu_deflate_fast_count(None, 0) == 0


def test_round_zero_in_phases(eng, gold, monkeypatch):
    """ZGPU_FAST_RUN = K: tile c is a run's head (parsed from a guess) iff c % K == 0 (zgpu_deflate_plan.h plan_fast_phases takes the knob at its word,
    tests/test_deflate_plan_cpu.py), a follower otherwise (parsed in round 0 from the tile in front).  Every probe's tile is both across these values.  With K at
    least the number of tiles (7 here, and 3 for the streams of two or three tiles) the batch is ONE run parsed tile by tile and no round follows: fast_round0_phases
    leaves no head to parse again.  Tile 1 is a head only for K = 1; the tiles 2 and 3 of the longer streams are heads behind the first for K = 2 and 3."""
    runs = (1, 2, 3, 7)
    for c in RC.catalogue():
        roles = {c.tile % k == 0 for k in runs}
        assert roles == {True, False}, c.name
    bad = []
    for k in runs:
        monkeypatch.setenv("ZGPU_FAST_RUN", str(k))
        bad += differing(eng, gold, RC.catalogue(), "K=%d" % k)
    assert not bad, (len(bad), bad[:8])


def test_first_tile_of_a_batch(eng, gold, monkeypatch):
    """The probe's tile as a batch's first: never warm, entered where tg.entry says, its history's bits prev_ins.  A batch's first tile never takes the same-entry
    path (the kernel asks c != 0), so what a reach case shows there is that the candidate is taken from prev_ins or not, nothing about the early stop; the reach
    cases sit on tile 2, a batch's first for batches of 1 and 2 tiles, the guess cases on the tiles 1, 2 and 3."""
    cat = RC.catalogue()
    for bt in (1, 2, 3):
        assert any(c.tile % bt == 0 for c in cat if c.family == "guess") and (bt == 3 or any(c.tile % bt == 0 for c in cat if c.family == "reach"))
    bad = []
    for bt in ("1", "2", "3", None):
        for pipe in ("0", "2"):
            if bt is None:
                monkeypatch.delenv("ZGPU_CONT_BATCH_TILES", raising=False)
            else:
                monkeypatch.setenv("ZGPU_CONT_BATCH_TILES", bt)
            monkeypatch.setenv("ZGPU_CONT_PIPE", pipe)
            bad += differing(eng, gold, cat, "batch %s pipe %s" % (bt, pipe))
    assert not bad, (len(bad), bad[:8])


def test_first_tile_of_a_feed(gold, monkeypatch):
    """deflate() of the host library, the input cut 0, 1, 31, 32, 33 positions in front of the probe's tile (a feed of its own: ZAMD_FEED_BYTES), and a
    sync flush (the window stays: the plain stream's claim) and a full flush (the window is forgotten: a stream of its own, the candidate not taken) there."""
    import zhost as Z
    monkeypatch.setenv("ZAMD_FEED_BYTES", "1024")
    bad = []
    for c in RC.feed_cases():
        for tag, calls, _ in RC.feed_rows(c):
            (cut, flush), = calls
            for cfg in c.cfgs:
                z, codes, info = Z.deflate_stream(c.data, RC.level_of(cfg), [(cut, flush), (len(c.data) - cut, Z.Z_FINISH)], window_bits=-15)
                want = O.cont_stream(c.data, RC.level_of(cfg), calls, wbits=-15)
                assert [len(want), h16(want)] == gold[c.name]["feed"][tag][cfg]
                if z != want:
                    bad.append((c.name, tag, cfg, BW.first_difference(z, want)))
    assert not bad, (len(bad), bad[:8])


_died = []


@pytest.mark.parametrize("knob,value", [("ZGPU_FW_RING", "0"), ("ZGPU_FW_RING", "1"), ("ZGPU_FAST_KEEP", "0"), ("ZGPU_FAST_KEEP", "1"), ("ZGPU_FAST_FORCE_ROUNDS", "3")])
def test_forms_read_once_per_process(knob, value):
    """The whole catalogue in a fresh child per setting, one at a time; every setting gives the golden bytes, so ZGPU_FAST_KEEP=0 (every active tile parsed
    to its end) gives the bytes of =1.  After a child that died on a signal or ran out its time no further child is started."""
    assert not _died, "an earlier child died: %s" % _died
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env[knob] = value
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    try:
        p = subprocess.run([sys.executable, "-m", "round_cases_child"], cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _died.append((knob, value, "time limit"))
        raise
    if p.returncode < 0:
        _died.append((knob, value, p.returncode))
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert lines and lines[-1] == "DONE %d" % (3 * len(RC.catalogue())), lines[-3:]
    assert [ln for ln in lines if ln.startswith("DIFFERS")] == []
