"""The sizing form of the piece path (the sizing pass of the sizes call and of the packed call, batch_pieces_sizes_run) as far as plain numbers decide
it: pieces_sizes_chain, the verdict over one item's end records, needs and starts, and the sizing round plan (zlib_amd/csrc/zgpu_inflate_pieces_plan.h).
tests/tools/inflate_sizes_pieces_model.cpp includes the header -- the chain and the selection are the functions the device runs -- and is built for the
host only, with the host sanitizers, and run as a program.

The catalogue part fixes, without a GPU, what tests/test_gpu_batch_sizes_pieces.py must see in the counters: for every case of oracle/piececases.py an
IDEAL block finder (tests/piece_fixtures.py), the tool's selection, per-piece counts and needs worked out here from the case's block list, and the chain
over those: clean exactly where the case says it is sized in pieces."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from oracle import deflate_writer as W
from oracle import piececases as P
from tests.piece_fixtures import HDR, SPACING, ideal_finder, rounds_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN = 256
SCRATCH_CAP = 2 * 2 ** 30 - 1
LIMIT = 0xFFFF0000
PER_PIECE = 32 + 16 + 16 + 8 + 4   # row, end record, status, output start, need
PER_TARGET = 24 + 16               # a finder's row and its two results
TOO_FAR, OUTPUT = 10, 12           # the decoder's messages "invalid distance too far back" and "segment decodes to more than ..." as error bits of an end record
ROUND_SLOTS = 7                    # ZGPU_BATCH_PIECES_SIZES_ROUND_SLOTS of the rounds test: no three items of rounds_batch() fit, nor two of four slots


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sizes_pieces") / "inflate_sizes_pieces_model")
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "inflate_sizes_pieces_model.cpp")], check=True, timeout=300)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (args[:1], out.returncode, out.stderr[-2000:])
        return [dict(w.split("=", 1) for w in line.split()) for line in out.stdout.splitlines()]
    return run


def lst(v):
    return ",".join("-" if x is None else str(x) for x in v) if v else "-"


def chain(model, body_lo, in_hi, starts, ends, needs, data="-"):
    """starts: [(bit, stored?)], ends: [(end_bit, out_bytes, flags) or None], needs: [int]"""
    r = model("chain", body_lo, in_hi, ",".join("%d%s" % (b, "s" if s else "") for b, s in starts), ",".join("0:0:-" if e is None else "%d:%d:%d" % e for e in ends),
              lst(needs), data)[0]
    return int(r["total"]), int(r["end_bit"]), int(r["used"]), r["clean"] == "1"


# ---------------------------------------------------------------------------- the catalogue
def piece_records(case, starts, bit0):
    """What the counting kernel would write for the pieces that begin at `starts` ([(bit of the stream, "d" | "s")], the first at bit 0): per piece
    (end_bit, out_bytes, flags) and need, from the block list alone.  A piece runs from its first block to the block in front of the next start."""
    first_block = {case.start_of(i): i for i in range(len(case.blocks))}
    cuts = [0] + [first_block[b] for b, _ in starts[1:]] + [len(case.blocks)]
    ends, needs = [], []
    for p, (a, z) in enumerate(zip(cuts, cuts[1:])):
        count, need, err = 0, 0, 0
        for i in range(a, z):
            blk = case.blocks[i]
            if blk["t"] == "stored":
                count += len(blk["data"])
                continue
            t = blk["toks"]
            lens = np.where(t.kind == W.LIT, 1, np.where(t.kind == W.MATCH, t.a, 0)).astype(np.int64)
            before = count + np.cumsum(lens) - lens
            m = t.kind == W.MATCH
            reach = t.b[m].astype(np.int64) - before[m]
            if m.any() and reach.max() > 0:
                if p == 0:
                    err = TOO_FAR  # a first piece has nothing in front of it
                else:
                    need = max(need, int(reach.max()))
            count += int(lens.sum())
        assert count == sum(case.block_out[a:z])
        ends.append((bit0 + case.block_bits[z], 0 if err else count, err << 8 if err else (1 if z == len(case.blocks) else 0)))
        needs.append(need)
    return ends, needs


def sized(model, case, wrap, lead, tmp_path):
    buf = bytes(lead) + case.wrapped(wrap)
    body_lo, end = lead + HDR[wrap], len(buf)
    dyn, sto, _ = ideal_finder(case, buf, body_lo, end)
    path = tmp_path / "item.bin"
    path.write_bytes(buf)
    got = model("select", SPACING, body_lo * 8, end, (end - body_lo) * 8 // (6 * SPACING) + 1, lst(dyn), lst(sto), "@%s" % path)[0]["starts"]
    sel = [(int(w.rstrip("s")), w.endswith("s")) for w in got.split(",")]
    rel = [(b - body_lo * 8, "s" if s else "d") for b, s in sel]
    ends, needs = piece_records(case, rel, body_lo * 8)
    return chain(model, body_lo, end, sel, ends, needs, "@%s" % path), len(sel)


@pytest.mark.parametrize("case", P.catalogue() + P.pool(), ids=lambda c: c.name)
def test_catalogue_verdicts(model, case, tmp_path):
    assert case.kind in ("ok", "bad")  # (a cut case would need a model of the counting kernel's own end)
    for wrap in case.wraps:
        for lead in (0, 13):
            (total, end_bit, used, clean), npieces = sized(model, case, wrap, lead, tmp_path)
            assert npieces >= 2, (wrap, lead)
            if case.went is None:
                continue
            assert clean == (case.went == (1, 0)), (wrap, lead, total, used)
            if clean:
                assert total == len(case.expect) and used == npieces
                assert end_bit == (lead + HDR[wrap]) * 8 + case.block_bits[-1]


def test_the_reach_rule_at_its_edge(model, tmp_path):
    want = {"p3_25200_reach_25200": True, "p3_25200_reach_25201": False, "p3_32768_reach_32768": True, "p3_32767_reach_32768": False}
    for name, ok in want.items():
        (total, _, _, clean), _ = sized(model, P.by_name(name), "zlib", 0, tmp_path)
        assert clean == ok, (name, total)


# ---------------------------------------------------------------------------- synthetic record lists
def three(total_last=1000, flags=(0, 0, 1), needs=(0, 0, 0), ends=(8000, 16000, 24000), starts=(80, 8000, 16000), outs=None):
    outs = outs or (1000, 1000, total_last)
    return [(s, False) for s in starts], [(e, o, f) for e, o, f in zip(ends, outs, flags)], list(needs)


def test_chain_plain(model):
    s, e, n = three()
    assert chain(model, 10, 4000, s, e, n) == (3000, 24000, 3, True)
    # the need of a piece is held against what the pieces in front of it counted: exactly that much is clean, one byte more is not
    assert chain(model, 10, 4000, *three(needs=(0, 1000, 2000)))[3]
    assert not chain(model, 10, 4000, *three(needs=(0, 1001, 0)))[3]
    assert not chain(model, 10, 4000, *three(needs=(0, 0, 2001)))[3]
    assert chain(model, 10, 4000, *three(needs=(99999, 0, 0)))[3]  # (a first piece has no need: its reach is its own error)


def test_chain_total_at_the_item_limit(model):
    outs = (LIMIT - 2000, 1000, 1000)
    assert chain(model, 10, 4000, *three(outs=outs)) == (LIMIT, 24000, 3, True)
    assert not chain(model, 10, 4000, *three(outs=(LIMIT - 2000, 1000, 1001)))[3]
    assert not chain(model, 10, 4000, *three(outs=(LIMIT, LIMIT, LIMIT)))[3]  # (the sum is taken in 64 bits)


def test_chain_a_piece_with_an_error(model):
    for at in range(3):
        flags = [0, 0, 1]
        flags[at] = OUTPUT << 8  # the counting stopped at the item limit
        assert not chain(model, 10, 4000, *three(flags=tuple(flags)))[3], at
    s, e, n = three()
    e[1] = None  # never written
    assert not chain(model, 10, 4000, s, e, n)[3]


def test_chain_broken_links(model):
    assert not chain(model, 10, 4000, *three(ends=(8001, 16000, 24000)))[3]   # the first link
    assert not chain(model, 10, 4000, *three(ends=(8000, 15999, 24000)))[3]   # a middle one (of three pieces: the last link)
    s, e, n = three()
    s.append((24000, False)); e[2] = (24000, 1000, 0); e.append((32008, 1000, 1)); n.append(0)
    assert chain(model, 10, 4100, s, e, n) == (4000, 32008, 4, True)
    e[2] = (24001, 1000, 0)
    assert not chain(model, 10, 4100, s, e, n)[3]                             # the last link of four
    s, e, n = three(flags=(0, 0, 0))
    assert not chain(model, 10, 4000, s, e, n)[3]                             # no piece saw the final block


def test_chain_stored_hand_over(model):
    # a stored start at bit 8000 (byte 1000): the piece in front ends 3 .. 10 bits before it, and those bits are zeros
    for gap in range(0, 13):
        s, e, n = three(ends=(8000 - gap, 16000, 24000))
        s[1] = (8000, True)
        assert chain(model, 10, 4000, s, e, n)[3] == (3 <= gap <= 10), gap
    s, e, n = three(ends=(7992, 16000, 24000))
    s[1] = (8000, True)
    assert chain(model, 10, 4000, s, e, n, "998:255")[3]          # (bits in front of the hand-over do not count)
    assert not chain(model, 10, 4000, s, e, n, "999:1")[3]        # BFINAL of the stored block's header
    assert not chain(model, 10, 4000, s, e, n, "999:128")[3]      # its last padding bit


def test_chain_final_block_in_a_middle_piece(model):
    s, e, n = three(flags=(0, 1, OUTPUT << 8), needs=(0, 0, 99999), ends=(8000, 15000, 1))
    assert chain(model, 10, 4000, s, e, n) == (2000, 15000, 2, True)  # the piece behind the final block is ignored, whatever it says


def test_chain_end_behind_the_item(model):
    assert chain(model, 10, 3000, *three())[3]                        # the final block ends with the item's last bit
    assert not chain(model, 10, 2999, *three())[3]
    assert not chain(model, 3001, 4000, *three())[3]                  # ... and not in front of its body


# ---------------------------------------------------------------------------- the round plan
@pytest.mark.parametrize("shape", [(1, 3, 3), (7, 27, 23), (1100, 5000, 4000), (2 ** 32 - 2, 2 ** 32 - 2, 2 ** 32 - 2)])
def test_scratch_regions_are_aligned_and_disjoint(model, shape):
    nitems, ntargets, npieces = shape
    f = model("plan", *shape)[0]
    want = {"targets": ntargets * 24, "found": ntargets * 16, "rows": npieces * 32, "ends": npieces * 16, "status": npieces * 16, "ostart": npieces * 8, "need": npieces * 4}
    at = 0
    for name, size in want.items():  # (the plan's own order)
        off, nbytes = (int(x) for x in f[name].split(":"))
        assert nbytes == size and off % ALIGN == 0 and off >= at, name
        at = off + nbytes
    assert at <= int(f["total"]) < 2 ** 63
    assert int(f["total"]) <= npieces * PER_PIECE + ntargets * PER_TARGET + len(want) * ALIGN


def test_scratch_total_is_monotone(model):
    rnd = random.Random(9)
    for _ in range(40):
        a = [rnd.randrange(1, 5000), rnd.randrange(3, 20000), rnd.randrange(1, 20000)]
        base = int(model("plan", *a)[0]["total"])
        for i in range(3):
            b = list(a)
            b[i] += rnd.randrange(1, 300)
            assert int(model("plan", *b)[0]["total"]) >= base, (a, b)


def test_a_round_that_cannot_be_counted_is_declined(model):
    for shape in ((2 ** 32 - 1, 10, 10), (10, 2 ** 32 - 1, 10), (10, 10, 2 ** 32 - 1)):
        assert model("plan", *shape)[0]["total"] == "0", shape
    assert model("plan", 2 ** 32 - 2, 2 ** 32 - 2, 2 ** 32 - 2)[0]["total"] != "0"


def test_round_split_by_hand(model):
    rows = model("rounds", 7, "3:3", "3:4", "5:4", "3:3", "30:9", "3:3", "3:3", "3:3")
    assert [(int(r["first"]), int(r["last"])) for r in rows] == [(0, 2), (2, 4), (4, 5), (5, 7), (7, 8)]  # (nine slots alone pass the cap: a round of its own)
    rows = model("rounds", 0, *["3:3"] * 50)
    assert [(int(r["first"]), int(r["last"])) for r in rows] == [(0, 50)]  # no cap
    # scratch: 20,000,000 slots are 1.5 GB of records -- two such items pass 2 GiB
    rows = model("rounds", 0, *["1000:20000000"] * 3)
    assert [(int(r["first"]), int(r["last"])) for r in rows] == [(0, 1), (1, 2), (2, 3)]


def test_round_split_covers_every_item_once_and_keeps_the_caps(model):
    rnd = random.Random(5)
    for cap in (0, 1, 7, 50, 4000):
        items = [(rnd.randrange(3, 2000), rnd.randrange(1, 700)) for _ in range(300)]
        rows = model("rounds", cap, *["%d:%d" % it for it in items])
        nxt = 0
        for r in rows:
            first, last = int(r["first"]), int(r["last"])
            assert first == nxt and last > first
            nxt = last
            slots = sum(it[1] for it in items[first:last])
            assert slots == int(r["slots"]) and sum(it[0] for it in items[first:last]) == int(r["targets"])
            if last - first > 1 and cap:
                assert slots <= cap
            if last < len(items) and cap:  # greedy: the next item would not have fitted
                assert slots + items[last][1] > cap
            assert int(model("plan", last - first, r["targets"], r["slots"])[0]["total"]) <= SCRATCH_CAP
        assert nxt == len(items)
        if cap == 0:
            assert len(rows) == 1


def test_the_rounds_batch_under_the_slot_cap(model):
    """tests/test_gpu_batch_sizes_pieces.py, rounds: with ZGPU_BATCH_PIECES_SIZES_ROUND_SLOTS=7 the seven items of rounds_batch() make four rounds or more in
    whatever order the list of long items holds them -- every item has three slots or four, so no round holds three --, and sizing, which has no rooms,
    takes the items whose ROOM the decode's test made too small or too large: five sized in pieces, the cut item and the reach item fall back."""
    batch = rounds_batch("zlib")
    caps = []
    for data, *_ in batch:
        g = model("geom", P.MIN_BYTES, len(data) - HDR["zlib"])[0]
        assert g["long"] == "1"
        caps.append((int(g["ntargets"]), int(g["cap"])))
    assert all(c in (3, 4) for _, c in caps) and 3 * min(c for _, c in caps) > ROUND_SLOTS
    for order in (list(range(7)), [6, 5, 4, 3, 2, 1, 0], [3, 0, 6, 1, 5, 2, 4]):
        rows = model("rounds", ROUND_SLOTS, *["%d:%d" % caps[k] for k in order])
        assert len(rows) >= 4 and all(int(r["last"]) - int(r["first"]) <= 2 for r in rows), rows
    assert sizing_went(batch) == (5, 2)


def sizing_went(batch):
    """what a sizing pass adds to its counters for the items of rounds_batch(): an item that is good in a room of its size is sized in pieces"""
    done = sum(1 for b in batch if b[3] in (0, -5))   # good, or only its room was wrong
    return done, len(batch) - done
