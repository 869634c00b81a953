"""CPU: the tree fixture (tests/golden/tree_kat.json, written by oracle/gen_golden_trees.py from the compiled reference) against the restatement, and the
condition it stands on: every overflow row of oracle/treecases.py sends the tree it is named for through gen_bitlen's repair (trees.c:525-566), the
control reaches 15 bits without it, and the block-type sweep lands on every block type and on both equalities of the choice (trees.c:967, 978).
tests/test_gpu_trees.py runs the same rows through the HIP kernels."""
import json
import os

import pytest

from oracle import gen_golden_trees as G, oracle_py as O, refzlib as R, treecases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "tree_kat.json")))
ROWS = {(r["name"], r["level"]): r for r in KAT["rows"]}
CASES = list(T.all_cases())
PINNED = ("name", "family", "strategy", "level", "n", "input_sha", "chunk_len", "chunk_sha", "cont_len", "cont_sha", "btypes", "repairs", "overflow", "longest",
          "blocks", "tie_static", "tie_stored")


def test_fixture_has_a_row_for_every_case_and_level():
    assert sorted(ROWS) == sorted((c.name, lv) for c in CASES for lv in c.levels)
    assert len(ROWS) == len(KAT["rows"])
    for c in CASES:
        if c.strategy == 2:
            assert set(c.levels) <= {1, 6, 9}
        if c.family in ("lit", "control"):
            assert c.strategy == 2 and c.levels == (1, 6, 9)
        if c.family in ("dist", "both"):
            assert c.strategy == 0 and c.levels == (1, 3, 4, 6, 9)
        assert len(c.data) <= (1 << 20)
        if len(c.data) <= 65536:  # one chunk: the chunk function and the one continuous stream write the same bytes
            assert all(ROWS[(c.name, lv)]["chunk_sha"] == ROWS[(c.name, lv)]["cont_sha"] for lv in c.levels)


def test_restatement_reproduces_the_fixture():
    bad = []
    for c in CASES:
        for lv in c.levels:
            got, want = G.row_of(c, lv, reference=False), ROWS[(c.name, lv)]
            bad += [(c.name, lv, k, got[k], want[k]) for k in PINNED if got[k] != want[k]]
            if "hex" in want:
                assert O.deflate_cont(c.data, lv, (), c.strategy).hex() == want["hex"], (c.name, lv)
    assert not bad, bad[:10]


def test_overflow_rows_are_repaired_and_the_control_is_not():
    """On a fresh run of the restatement AND in the fixture: a row that stops repairing is a failure."""
    fresh = [G.row_of(c, lv, reference=False) for c in CASES if c.family in ("lit", "dist", "both", "control") for lv in c.levels]
    for rows in (fresh, KAT["rows"]):
        G.check_rows([r for r in rows if r["family"] != "btype"] + [r for r in KAT["rows"] if r["family"] == "btype"])
        fam = {f: [r for r in rows if r["family"] == f] for f in ("lit", "dist", "both", "control")}
        assert all(fam.values())
        assert all(r["repairs"][0] >= 1 for r in fam["lit"]) and all(r["repairs"][1] >= 1 for r in fam["dist"])
        assert all(r["repairs"][0] >= 1 and r["repairs"][1] >= 1 for r in fam["both"])
        assert all(r["repairs"][:2] == [0, 0] and r["longest"][0] == 15 for r in fam["control"])
        # the repair loop runs once (overflow 2) and several times; both trees of a "both" row are repaired in ONE block (its only block with matches)
        assert {2, 4, 6, 8} <= {r["overflow"][0] for r in fam["lit"]} and max(r["overflow"][0] for r in fam["lit"]) >= 16
        assert all(r["blocks"] == [0, 0, 2] and r["btypes"] == [2, 2] for r in fam["both"])
        # the repaired block alone, first, in the middle and last in its stream
        pos = {r["name"]: r for r in fam["lit"] if r["level"] == 6}
        assert pos["lit-pos-2of3"]["blocks"][2] == 3 and pos["lit-pos-3of4"]["blocks"] == [0, 1, 3] and pos["lit-pos-1-and-3of4-64k"]["repairs"][0] == 3


def test_block_type_sweep_lands_on_every_type_and_both_equalities():
    bt = [G.row_of(c, lv, reference=False) for c in T.btype_cases() for lv in c.levels]
    s = G.check_rows(bt)
    assert s == KAT["summary"] and all(v > 0 for v in s.values()), (s, KAT["summary"])
    for alpha in (2, 16, 64, 256):
        assert any(r["name"].startswith("btype-a%d-" % alpha) for r in bt)


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libzref.so is built only where the reference tree is mounted")
def test_fixture_equals_a_fresh_run_of_the_reference():
    for c in CASES:
        for lv in c.levels:
            assert G.row_of(c, lv, reference=True) == {k: v for k, v in ROWS[(c.name, lv)].items() if k != "hex"}, (c.name, lv)
            if "hex" in ROWS[(c.name, lv)]:
                assert R.deflate_calls(c.data, lv, (), -15, c.strategy).hex() == ROWS[(c.name, lv)]["hex"]
