"""The verify form of the piece path (the blocking integrity test, batch_pieces_verify_run) as far as plain numbers decide it: the round plan and its
memory bound, the rounds under the slot cap, pieces_verify_chain over an item's tails records, and pieces_verify_confirm, which confirms the check records
and joins the pieces' check values (zlib_amd/csrc/zgpu_inflate_pieces_plan.h, zgpu_common.h).  tests/tools/inflate_verify_pieces_model.cpp includes the
headers -- the chain, the confirmation, the join and the selection are the functions the device runs -- and is built for the host only, with the host
sanitizers, and run as a program.

The catalogue part fixes, without a GPU, what tests/test_gpu_batch_verify_pieces.py must see in the counters: for every case of oracle/piececases.py an
IDEAL block finder (tests/piece_fixtures.py), the tool's selection, the tails records and the check records worked out here from the case's block list --
the check pass knows where every piece starts, so a match that reaches in front of the item is its error, exactly -- and chain and confirmation over
those: clean exactly where the case says it goes in pieces, with Python zlib's check values of the whole."""
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

from oracle import deflate_writer as W
from oracle import piececases as P
from oracle.handmade import rnd
from tests.piece_fixtures import HDR, SPACING, ideal_finder, rounds_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN = 256
RING = 32768
SCRATCH_CAP = 2 * 2 ** 30 - 1
LIMIT = 0xFFFF0000
PER_PIECE = 2 * RING + RING + 32 + 16 + 16 + 8 + 32   # tail, window, row, end record, status, output start, check record
PER_TARGET = 24 + 16                                   # a finder's row and its two results
DEFAULT_CAP = 1024                                     # one residency of the check kernel: four workgroups on each of 256 CUs
TOO_FAR = 10                                           # the decoder's message "invalid distance too far back" as the error bits of a record
ROUND_SLOTS = 7                                        # ZGPU_BATCH_PIECES_VERIFY_ROUND_SLOTS of the rounds test
REGIONS = ("targets", "found", "rows", "ends", "status", "ostart", "checks", "ranges", "entry", "windows", "tails")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("verify_pieces") / "inflate_verify_pieces_model")
    # host code only, with the host sanitizers: the program makes no HIP call (zgpu_common.h wants the HIP front end, as tests/tools/fold_model.cpp does)
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "tools", "inflate_verify_pieces_model.cpp")], check=True, timeout=300)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (args[:1], out.returncode, out.stderr[-2000:])
        return [dict(w.split("=", 1) for w in line.split()) for line in out.stdout.splitlines()]
    return run


def lst(v):
    return ",".join("-" if x is None else str(x) for x in v) if v else "-"


def verdict(model, body_lo, in_hi, starts, ends, checks, do=3, data="-"):
    """starts: [(bit, stored?)], ends: [(end_bit, out_bytes, flags) or None], checks: [(end_bit, out_bytes, flags, adler32, crc32) or None]"""
    r = model("verdict", body_lo, in_hi, ",".join("%d%s" % (b, "s" if s else "") for b, s in starts), ",".join("0:0:-" if e is None else "%d:%d:%d" % e for e in ends),
              ",".join("0:0:-:0:0" if c is None else "%d:%d:%d:%d:%d" % c for c in checks), do, data)[0]
    return {"chain": r["chain"] == "1", "used": int(r["used"]), "total": int(r["total"]), "end_bit": int(r["end_bit"]),
            "ostart": [] if r["ostart"] == "-" else [int(x) for x in r["ostart"].split(",")], "clean": r["clean"] == "1", "adler": int(r["adler"]), "crc": int(r["crc"])}


# ---------------------------------------------------------------------------- layout
@pytest.mark.parametrize("shape", [(1, 3, 3), (7, 27, 23), (78, 4914, 1014), (1100, 5000, 4000), (2 ** 32 - 2, 2 ** 32 - 2, 2 ** 32 - 2)])
def test_scratch_regions_tile_the_scratch_in_order(model, shape):
    nitems, ntargets, npieces = shape
    f = model("plan", *shape)[0]
    assert int(f["per"]) == PER_PIECE and PER_PIECE - 3 * RING < 128  # under 128 bytes of records a slot
    want = {"targets": ntargets * 24, "found": ntargets * 16, "rows": npieces * 32, "ends": npieces * 16, "status": npieces * 16, "ostart": npieces * 8,
            "checks": npieces * 32, "ranges": nitems * 8, "entry": RING, "windows": npieces * RING, "tails": npieces * RING * 2}
    assert tuple(want) == REGIONS
    at = 0
    for name, size in want.items():  # (the plan's own order)
        off, nbytes = (int(x) for x in f[name].split(":"))
        assert nbytes == size and off % ALIGN == 0 and at <= off < at + ALIGN, name  # no overlap, and no gap but the alignment's
        at = off + nbytes
    assert at <= int(f["total"]) < at + ALIGN and int(f["total"]) < 2 ** 63
    assert int(f["total"]) <= npieces * PER_PIECE + ntargets * PER_TARGET + nitems * 8 + RING + len(want) * ALIGN


def test_a_round_that_cannot_be_counted_is_declined(model):
    for shape in ((2 ** 32 - 1, 10, 10), (10, 2 ** 32 - 1, 10), (10, 10, 2 ** 32 - 1)):
        assert model("plan", *shape)[0]["total"] == "0", shape
    assert model("plan", 2 ** 32 - 2, 2 ** 32 - 2, 2 ** 32 - 2)[0]["total"] != "0"


def test_scratch_total_is_monotone(model):
    r = random.Random(9)
    for _ in range(40):
        a = [r.randrange(1, 5000), r.randrange(3, 20000), r.randrange(1, 20000)]
        base = int(model("plan", *a)[0]["total"])
        for i in range(3):
            b = list(a)
            b[i] += r.randrange(1, 300)
            assert int(model("plan", *b)[0]["total"]) >= base, (a, b)


# ---------------------------------------------------------------------------- memory bound and rounds
def test_memory_bound_of_256_items_of_1_mib(model):
    """256 items of 1 MiB that compress to 300,000 bytes each (level 6 of the rate scripts' corpus gives about that): 13 slots an item.  Under the default cap
    no round's plan exceeds 1024 slots' bytes plus the regions' alignment -- whatever the items decode to, and however many there are: four times as many
    items make four times as many rounds of the same size."""
    g = model("geom", 131072, 300000)[0]
    assert (g["long"], int(g["cap"])) == ("1", 13)
    item = "%s:%s" % (g["ntargets"], g["cap"])
    for n in (256, 1024):
        rows = model("rounds", 0, *[item] * n)
        assert all(int(r["cap"]) == DEFAULT_CAP for r in rows)
        assert sum(int(r["last"]) - int(r["first"]) for r in rows) == n
        for r in rows:
            assert int(r["slots"]) <= DEFAULT_CAP
            assert 0 < int(r["plan"]) <= DEFAULT_CAP * PER_PIECE + len(REGIONS) * ALIGN, r
        assert len(rows) == -(-n // (DEFAULT_CAP // 13))
    assert DEFAULT_CAP * PER_PIECE < 97 << 20  # about 96 MiB


def test_round_split_by_hand(model):
    rows = model("rounds", 7, "3:3", "3:4", "5:4", "3:3", "30:9", "3:3", "3:3", "3:3")
    assert [(int(r["first"]), int(r["last"])) for r in rows] == [(0, 2), (2, 4), (4, 5), (5, 7), (7, 8)]  # (nine slots alone pass the cap: a round of its own)
    rows = model("rounds", 0, *["3:3"] * 400)
    assert [(int(r["first"]), int(r["last"])) for r in rows] == [(0, 341), (341, 400)]  # the default cap: 1024 slots
    # the knob cannot ask for a round whose scratch would pass 2 GiB
    rows = model("rounds", 10 ** 9, *["100:5000"] * 5)
    assert all(int(r["plan"]) <= SCRATCH_CAP and 0 < int(r["cap"]) < 10 ** 9 for r in rows) and len(rows) >= 2


def test_round_split_covers_every_item_once_and_keeps_the_cap(model):
    r = random.Random(5)
    for cap in (1, 7, 50, 1024, 4000):
        items = [(r.randrange(3, 2000), r.randrange(1, 700)) for _ in range(300)]
        rows = model("rounds", cap, *["%d:%d" % it for it in items])
        nxt = 0
        for row in rows:
            first, last = int(row["first"]), int(row["last"])
            assert first == nxt and last > first  # every long item lands in exactly one round
            nxt = last
            slots = sum(it[1] for it in items[first:last])
            assert slots == int(row["slots"]) and sum(it[0] for it in items[first:last]) == int(row["targets"])
            if last - first > 1:
                assert slots <= cap
            else:
                assert slots <= cap or items[first][1] > cap  # an item larger than the cap is alone in its round
            if last < len(items):  # greedy: the next item would not have fitted
                assert slots + items[last][1] > cap
            assert 0 < int(row["plan"]) <= max(cap, max(it[1] for it in items)) * PER_PIECE + 2000 * 300 * PER_TARGET + 300 * 8 + RING + len(REGIONS) * ALIGN
        assert nxt == len(items)


def test_the_rounds_batch_under_the_slot_cap(model):
    """tests/test_gpu_batch_verify_pieces.py, rounds: with ZGPU_BATCH_PIECES_VERIFY_ROUND_SLOTS=7 the seven items of rounds_batch() make four rounds or more in
    whatever order the list of long items holds them -- every item has three slots or four, so no round holds three"""
    caps = []
    for data, *_ in rounds_batch("zlib"):
        g = model("geom", P.MIN_BYTES, len(data) - HDR["zlib"])[0]
        assert g["long"] == "1"
        caps.append((int(g["ntargets"]), int(g["cap"])))
    assert all(c in (3, 4) for _, c in caps) and 3 * min(c for _, c in caps) > ROUND_SLOTS
    for order in (list(range(7)), [6, 5, 4, 3, 2, 1, 0], [3, 0, 6, 1, 5, 2, 4]):
        rows = model("rounds", ROUND_SLOTS, *["%d:%d" % caps[k] for k in order])
        assert len(rows) >= 4 and all(int(r["last"]) - int(r["first"]) <= 2 for r in rows), rows


# ---------------------------------------------------------------------------- join
def piece_values(data, cuts):
    """the pieces' own check values, each started from 1 and 0, as the check pass leaves them"""
    edges = [0] + list(cuts) + [len(data)]
    return ["%d:%d:%d" % (z - a, zlib.adler32(data[a:z]), zlib.crc32(data[a:z])) for a, z in zip(edges, edges[1:])]


def test_join_equals_zlib(model):
    r = random.Random(21)
    mix = rnd(70000, 77).tobytes()
    ff = b"\xff" * ((1 << 24) + 1 + 16385 + 5)
    cases = [(mix, []), (mix, [0]), (mix, [len(mix)]), (mix, [0, 0, 1, 1, 2]), (mix, [1]), (mix, [16385]), (mix, [16385, 2 * 16385, 2 * 16385]), (b"", []), (b"", [0, 0]),
             (b"a", []), (ff, [(1 << 24) + 1]), (ff, [0, 1, (1 << 24) + 2]), (ff, [16385])]
    cases += [(mix, sorted(r.randrange(0, len(mix) + 1) for _ in range(r.randrange(1, 12)))) for _ in range(20)]
    for data, cuts in cases:
        for do in (1, 2, 3):
            got = model("join", do, *piece_values(data, cuts))[0]
            want = (zlib.adler32(data) if do & 1 else 1, zlib.crc32(data) if do & 2 else 0)
            assert (got["clean"], int(got["adler"]), int(got["crc"])) == ("1",) + want, (len(data), cuts, do)


# ---------------------------------------------------------------------------- chain and confirmation on record lists
def three(flags=(0, 0, 1), ends=(8000, 16000, 24000), starts=(80, 8000, 16000), outs=(1000, 1000, 1000)):
    s = [(b, False) for b in starts]
    e = [(b, o, f) for b, o, f in zip(ends, outs, flags)]
    data = bytes(range(256)) * 12
    c, at = [], 0
    for b, o, f in e:
        c.append((b, o, f, zlib.adler32(data[at: at + o]), zlib.crc32(data[at: at + o])))
        at += o
    return s, e, c, data[:at]


def test_verdict_plain(model):
    s, e, c, data = three()
    v = verdict(model, 10, 4000, s, e, c)
    assert v == {"chain": True, "used": 3, "total": 3000, "end_bit": 24000, "ostart": [0, 1000, 2000], "clean": True, "adler": zlib.adler32(data), "crc": zlib.crc32(data)}
    assert verdict(model, 10, 4000, s, e, c, do=1)["crc"] == 0 and verdict(model, 10, 4000, s, e, c, do=2)["adler"] == 1


def test_verdict_has_no_need_term_but_confirms_every_check(model):
    s, e, c, _ = three()
    for at in range(3):  # an error of the check pass (a reach in front of the item, found there exactly), a check never written
        for bad in ((c[at][0], 0, TOO_FAR << 8, 1, 0), None):
            cc = list(c)
            cc[at] = bad
            v = verdict(model, 10, 4000, s, e, cc)
            assert v["chain"] and not v["clean"], (at, bad)
    for at in range(3):  # a check that ended elsewhere, counted otherwise, or disagrees about the final block
        for k, d in ((0, 1), (1, 1), (2, 1)):
            cc = list(c)
            t = list(c[at])
            t[k] ^= d
            cc[at] = tuple(t)
            assert not verdict(model, 10, 4000, s, e, cc)["clean"], (at, k)


def test_verdict_chain_rules(model):
    s, e, c, _ = three(outs=(LIMIT - 2000, 1000, 1000))
    assert verdict(model, 10, 4000, s, e, c)["chain"]                                   # the total at the item limit
    assert not verdict(model, 10, 4000, *three(outs=(LIMIT - 2000, 1000, 1001))[:3])["chain"]
    assert not verdict(model, 10, 4000, *three(ends=(8001, 16000, 24000))[:3])["chain"]  # a broken link
    assert not verdict(model, 10, 4000, *three(flags=(0, 0, 0))[:3])["chain"]            # no piece saw the final block
    assert not verdict(model, 10, 4000, *three(flags=(0, TOO_FAR << 8, 1))[:3])["chain"]  # a piece of the tails pass with an error
    s, e, c, _ = three()
    e[1] = None
    assert not verdict(model, 10, 4000, s, e, c)["chain"]                               # never written
    assert verdict(model, 10, 3000, *three()[:3])["chain"] and not verdict(model, 10, 2999, *three()[:3])["chain"]  # the final block ends inside the item
    assert not verdict(model, 3001, 4000, *three()[:3])["chain"]
    # the final block in a middle piece: the piece behind it is not used, whatever it says, and neither is its check
    s, e, c, data = three(flags=(0, 1, TOO_FAR << 8), ends=(8000, 15000, 1))
    c[2] = None
    v = verdict(model, 10, 4000, s, e, c)
    assert (v["clean"], v["used"], v["total"], v["end_bit"], v["adler"]) == (True, 2, 2000, 15000, zlib.adler32(data[:2000]))
    # a stored start: the piece in front ends 3 .. 10 zero bits before it
    for gap in range(0, 13):
        s, e, c, _ = three(ends=(8000 - gap, 16000, 24000))
        s[1] = (8000, True)
        assert verdict(model, 10, 4000, s, e, c)["chain"] == (3 <= gap <= 10), gap


# ---------------------------------------------------------------------------- the catalogue
def piece_records(case, starts, bit0):
    """What the two passes would write for the pieces that begin at `starts` ([(bit of the stream, "d" | "s")], the first at bit 0), from the block list
    alone.  The tails pass: (end_bit, out_bytes, flags) per piece; only a first piece knows that nothing lies in front of it.  The check pass: the same
    end with the piece's own Adler-32 and CRC-32 -- or "invalid distance too far back" where a match reaches in front of the item's first byte."""
    first_block = {case.start_of(i): i for i in range(len(case.blocks))}
    cuts = [0] + [first_block[b] for b, _ in starts[1:]] + [len(case.blocks)]
    ends, checks, at = [], [], 0
    for p, (a, z) in enumerate(zip(cuts, cuts[1:])):
        count, far = 0, False
        for i in range(a, z):
            blk = case.blocks[i]
            if blk["t"] == "stored":
                count += len(blk["data"])
                continue
            t = blk["toks"]
            lens = np.where(t.kind == W.LIT, 1, np.where(t.kind == W.MATCH, t.a, 0)).astype(np.int64)
            before = at + count + np.cumsum(lens) - lens  # bytes of the ITEM in front of every token
            m = t.kind == W.MATCH
            far = far or bool(m.any() and (t.b[m].astype(np.int64) > before[m]).any())
            count += int(lens.sum())
        assert count == sum(case.block_out[a:z])
        end_bit, last = bit0 + case.block_bits[z], 1 if z == len(case.blocks) else 0
        ends.append((end_bit, 0, TOO_FAR << 8) if far and p == 0 else (end_bit, count, last))
        if far or case.expect is None:
            checks.append((end_bit, 0, TOO_FAR << 8, 1, 0))
        else:
            own = case.expect[at: at + count]
            checks.append((end_bit, count, last, zlib.adler32(own), zlib.crc32(own)))
        at += count
    return ends, checks


def verified(model, case, wrap, lead, tmp_path):
    buf = bytes(lead) + case.wrapped(wrap)
    body_lo, end = lead + HDR[wrap], len(buf)
    dyn, sto, _ = ideal_finder(case, buf, body_lo, end)
    path = tmp_path / "item.bin"
    path.write_bytes(buf)
    got = model("select", SPACING, body_lo * 8, end, (end - body_lo) * 8 // (6 * SPACING) + 1, lst(dyn), lst(sto), "@%s" % path)[0]["starts"]
    sel = [(int(w.rstrip("s")), w.endswith("s")) for w in got.split(",")]
    rel = [(b - body_lo * 8, "s" if s else "d") for b, s in sel]
    ends, checks = piece_records(case, rel, body_lo * 8)
    return verdict(model, body_lo, end, sel, ends, checks, 3, "@%s" % path), len(sel)


@pytest.mark.parametrize("case", P.catalogue() + P.pool(), ids=lambda c: c.name)
def test_catalogue_verdicts(model, case, tmp_path):
    assert case.kind in ("ok", "bad")  # (a cut case would need a model of the decoder's own end)
    for wrap in case.wraps:
        for lead in (0, 13):
            v, npieces = verified(model, case, wrap, lead, tmp_path)
            assert npieces >= 2, (wrap, lead)
            if case.went is None:
                continue
            assert v["clean"] == (case.went == (1, 0)), (wrap, lead, v)
            if v["clean"]:
                assert v["total"] == len(case.expect) and v["used"] == npieces
                assert v["end_bit"] == (lead + HDR[wrap]) * 8 + case.block_bits[-1]
                assert (v["adler"], v["crc"]) == (zlib.adler32(case.expect), zlib.crc32(case.expect))


def test_the_reach_rule_at_its_edge(model, tmp_path):
    want = {"p3_25200_reach_25200": True, "p3_25200_reach_25201": False, "p3_32768_reach_32768": True, "p3_32767_reach_32768": False}
    for name, ok in want.items():
        v, _ = verified(model, P.by_name(name), "zlib", 0, tmp_path)
        assert v["clean"] == ok and v["chain"], (name, v)  # (the tails pass cannot know: the chain holds, the check pass finds the reach)
