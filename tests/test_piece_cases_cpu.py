"""The hand-built long items of oracle/piececases.py stand where they claim -- shown without a GPU.  Every case is judged by Python's zlib and by the
writer's plain expansion; tests/tools/inflate_pieces_plan_model.cpp (the header the device runs, built for the host with the host sanitizers) says the
item is long at ZGPU_BATCH_PIECES_MIN_BYTES=49153; and what an IDEAL block finder would report of it (tests/piece_fixtures.py: worked out from the block
list), put through the tool's `select` -- the function pieces_select_kernel runs --, yields exactly the piece starts the case means to have selected,
behind every wrapper's header and at several places of a buffer (the finders' regions are cut at 16 bytes of the buffer, not of the item)."""
import os
import shutil
import subprocess

import pytest

from oracle import deflate_writer as W
from oracle import piececases as P
from tests.piece_fixtures import HDR, ROUND_BYTES, SPACING, ideal_finder, rounds_batch, zlib_verdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEADS = {"raw": (0, 5, 15, 100), "zlib": (0, 13), "gzip": (0, 7)}  # bytes of other items in front of the item in its buffer


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("piececases") / "inflate_pieces_plan_model")
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "inflate_pieces_plan_model.cpp")], check=True, timeout=300)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (args, out.returncode, out.stderr[-2000:])
        return [dict(w.split("=", 1) for w in line.split()) for line in out.stdout.splitlines()]
    return run


def every_case():
    return P.catalogue() + P.pool()


def predicted_starts(model, case, wrap, lead):
    """the piece starts of the item `lead` bytes into a buffer, as bits of the STREAM: ideal finders, then the tool's selection"""
    buf = bytes(lead) + case.wrapped(wrap)
    body_lo, end = lead + HDR[wrap], len(buf)
    dyn, sto, lens = ideal_finder(case, buf, body_lo, end)
    lst = lambda v: ",".join("-" if x is None else str(x) for x in v) if v else "-"
    got = model("select", SPACING, body_lo * 8, end, (end - body_lo) * 8 // (6 * SPACING) + 1, lst(dyn), lst(sto), ",".join("%d:%d" % p for p in lens) if lens else "-")[0]["starts"]
    out = []
    for w in got.split(","):
        out.append((int(w.rstrip("s")) - body_lo * 8, "s" if w.endswith("s") else "d"))
    return out


def test_names_fields_and_sizes():
    cs = every_case()
    assert len({c.name for c in cs}) == len(cs)
    assert len({c.expect for c in cs if c.kind == "ok"}) == sum(1 for c in cs if c.kind == "ok")  # no two plaintexts are equal
    for c in cs:
        assert c.kind in ("ok", "bad", "cut") and c.went in ((1, 0), (0, 1), None) and (c.expect is None) == (c.kind != "ok"), c.name
        assert (c.msg != "") == (c.kind == "bad"), c.name
        assert 50000 <= len(c.stream) <= 120 * 1024 or c.group in ("P2", "pool"), (c.name, len(c.stream))
    for g in ("P1", "P2", "P3", "P4", "P6", "P7"):
        assert any(c.group == g for c in cs), g
    bodies = [len(c.stream) for c in P.pool()]
    assert len(bodies) >= 8 and min(bodies) == P.MIN_BYTES and 81921 <= max(bodies) <= 83000 and all(c.kind == "ok" and c.went == (1, 0) for c in P.pool())


def test_the_writer_says_where_blocks_start():
    """block_starts() is read off the same fields stream() packs (that stream() writes what it wrote is tests/test_handmade_cpu.py's: the stream hashes
    of oracle/handmade.py's catalogue); here the starts of a mixed block list are what a walk of the stream finds"""
    blocks = [W.fixed(W.literals(b"abc")), W.stored(b"hello"), W.dynamic(W.literals(b"xyzzy" * 20)), W.stored(b"", final=True)]
    starts = W.block_starts(blocks)
    s = W.stream(blocks)
    assert starts[0] == 0 and starts[1] == 3 + 3 * 8 + 7 and starts[2] == ((starts[1] + 3 + 7) // 8 + 4 + 5) * 8 and starts[-1] == len(s) * 8
    assert (s[starts[3] >> 3] >> (starts[3] & 7)) & 7 == 1  # the last block's header: final, stored
    assert (s[starts[2] >> 3] >> (starts[2] & 7)) & 7 == 4  # not final, dynamic


@pytest.mark.parametrize("case", every_case(), ids=lambda c: c.name)
def test_case_is_what_it_claims(model, case):
    ok, msg, out, used = zlib_verdict(case.stream, "raw")
    assert ok == (case.kind == "ok"), (case.kind, msg)
    if case.kind == "ok":
        assert out == case.expect and used == case.deflate_bytes == len(case.stream) - len(case.tail)
        toks = None
        for b in case.blocks:
            t = W.literals(b["data"]) if b["t"] == "stored" else b["toks"]
            toks = t if toks is None else toks + t
        assert W.expand(toks) == case.expect and sum(case.block_out) == len(case.expect)
    elif case.kind == "bad":
        assert msg == case.msg
    else:
        assert msg == "cut"
    for wrap in case.wraps:
        item = case.wrapped(wrap)
        body = len(item) - HDR[wrap]
        g = model("geom", P.MIN_BYTES, body)[0]
        assert g["long"] == "1" and int(g["spacing"]) == SPACING and int(g["fspacing"]) == 16384, (wrap, g)
        if case.kind == "ok":
            v = zlib_verdict(item, wrap)
            assert v[0] and v[2] == case.expect and v[3] == len(item) - len(case.tail), wrap
        for lead in LEADS[wrap]:
            got = predicted_starts(model, case, wrap, lead)
            assert got == [(0, "d")] + case.starts, (wrap, lead, got, case.starts)


def test_p1_padding_is_what_the_names_say():
    for c in P.catalogue():
        if c.group != "P1":
            continue
        p = int(c.name.split("pad")[1][0])
        hdr, len_bit = c.block_bits[1], c.start_of(1)
        assert len_bit - hdr == 3 + p and len_bit // 8 >= 24576, c.name
        byte = c.stream[len_bit // 8 - 1]
        pad = byte >> (8 - p) if p else 0
        if c.name.endswith("low_bit_set"):
            assert p >= 4 and pad == 1 and byte >> 5 == 0
        elif c.name.endswith("top_bit_set"):
            assert p >= 1 and byte >> 5 != 0
        else:
            assert pad == 0 and byte >> 5 == 0
    assert sorted(int(c.name[6]) for c in P.catalogue() if c.name.startswith("p1_pad") and len(c.name) == 7) == list(range(8))


def test_p2_pieces_are_shorter_than_the_window():
    c = P.by_name("p2_short_pieces")
    cuts = c.start_blocks + [len(c.blocks)]
    outs = [sum(c.block_out[a:b]) for a, b in zip(cuts, cuts[1:])]
    assert len(outs) >= 4 and all(2048 + 24000 < o < 32768 for o in outs), outs
    # (the piece in front of them decodes to 32768 bytes or more: the first far matches are valid)
    assert sum(c.block_out[: cuts[0]]) >= 32768
    for i in c.start_blocks:
        t = c.blocks[i]["toks"]
        assert [int(d) for d in t.b[t.kind == W.MATCH][:4]] == [32768, 32767, 25601, 1]
        assert (c.block_bits[i + 1] - c.block_bits[i]) // 8 < 1024


def test_p3_p4_second_piece_starts_at_the_second_block():
    for c in P.catalogue():
        if c.group in ("P3", "P4"):
            assert c.start_blocks == [1] and c.starts == [(c.block_bits[1], "d")] and c.block_bits[1] // 8 >= 24576, c.name
    a, b = P.by_name("p3_25200_reach_25200"), P.by_name("p3_25200_reach_25201")
    assert a.block_out[0] == b.block_out[0] == 25200
    assert P.by_name("p3_32768_reach_32768").block_out[0] == 32768 and P.by_name("p3_32767_reach_32768").block_out[0] == 32767
    for d in (1, 7):
        c = P.by_name("p4_flood_dist%d" % d)
        t = c.blocks[1]["toks"]
        assert (t.kind[: P.FLOOD] == W.MATCH).all() and (t.a[: P.FLOOD] == 258).all() and (t.b[: P.FLOOD] == d).all() and c.block_out[1] >= 258 * P.FLOOD


def test_p6_final_block_ends_at_every_bit():
    got = sorted(c.block_bits[-1] % 8 for c in P.catalogue() if c.group == "P6")
    assert got == list(range(8))
    for c in P.catalogue():
        if c.group == "P6":
            assert len(c.tail) == 3 and c.blocks[-1]["t"] == "fixed" and c.deflate_bytes == (c.block_bits[-1] + 7) // 8


def test_pool_geometry(model):
    rows = [model("geom", P.MIN_BYTES, len(c.stream))[0] for c in P.pool()]
    assert {int(r["ntargets"]) for r in rows} == {3, 4, 5} and {int(r["cap"]) for r in rows} == {3, 4}, rows


def test_the_rounds_batch_makes_three_rounds_or_more(model):
    """tests/test_gpu_batch_pieces_built.py, rounds: every item is long, the split at ROUND_BYTES has three rounds or more -- in item order here, and in
    any order, for no three rooms fit one round --, and the item with four times its room makes a round of its own"""
    for wrap in ("raw", "zlib", "gzip"):
        batch = rounds_batch(wrap)
        costs = []
        for data, room, *_ in batch:
            g = model("geom", P.MIN_BYTES, len(data) - HDR[wrap])[0]
            assert g["long"] == "1", (wrap, g)
            costs.append("%d:%s:%s" % (room, g["ntargets"], g["cap"]))
        rows = model("rounds", ROUND_BYTES, *costs)
        assert len(rows) >= 3 and (int(rows[-1]["first"]), int(rows[-1]["last"])) == (6, 7), rows
        rooms = sorted(b[1] for b in batch)
        assert sum(rooms[:3]) > ROUND_BYTES and rooms[-1] > ROUND_BYTES
        assert [b[5] for b in batch] == [(1, 0), (0, 1), (1, 0), (0, 1), (0, 1), (1, 0), (1, 0)]
        assert zlib_verdict(batch[3][0], wrap)[1] == "cut" and zlib_verdict(batch[4][0], wrap)[1] == "invalid distance too far back"
