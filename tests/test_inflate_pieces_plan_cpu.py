"""What the piece path of the blocking batch decode decides from plain numbers (zlib_amd/csrc/zgpu_inflate_pieces_plan.h): which bodies are long and how far
apart their pieces and finders stand, a round's scratch layout, the split into rounds, and the selection of piece starts from what the finders report.
tests/tools/inflate_pieces_plan_model.cpp includes the header -- the selection is the function the device runs -- and is built for the host only, with the
host sanitizers, and run as a program.  The expected values are worked out by hand from the rules (inflate_spec_run's for one stream): spacing = body / 4096
rounded up to 4096 and at least 32768; finders a quarter of that apart, rounded up to 4096 and at least 16384; starts 6 * spacing bits apart or more and more
than 2 * spacing bits before the end; a dynamic start inside a vouched stored block is struck."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING, HALF, ALIGN = 32768, 16384, 256
SCRATCH_CAP = 2 * 2 ** 30 - 1
PER_PIECE = 2 * RING + RING + 2 * HALF + 32 + 16 + 16 + 8
PER_TARGET = 24 + 16


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pieces") / "inflate_pieces_plan_model")
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "inflate_pieces_plan_model.cpp")], check=True, timeout=300)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (args, out.returncode, out.stderr[-2000:])
        return [dict(w.split("=", 1) for w in line.split()) for line in out.stdout.splitlines()]
    return run


def test_formulas(model):
    rows = {int(r["body"]): r for r in model("geom", 131072, 131071, 131072, 2 ** 30, 2 ** 29 - 1, 2 ** 29, 200 * 2 ** 20)}
    assert rows[131071]["long"] == "0"
    r = rows[131072]
    assert (r["long"], r["spacing"], r["fspacing"], r["ntargets"]) == ("1", "32768", "16384", "7")
    assert r["cap"] == str(131072 * 8 // (6 * 32768) + 1)
    r = rows[2 ** 30]
    assert (r["spacing"], r["fspacing"], r["ntargets"]) == ("262144", "65536", "16383")
    assert r["long"] == "0" and rows[2 ** 29]["long"] == "0" and rows[2 ** 29 - 1]["long"] == "1"  # the one-workgroup decoder's own limit of an item
    r = rows[200 * 2 ** 20]  # 51200 -> 53248; a quarter, 13312, is below the floor of 16384
    assert (r["spacing"], r["fspacing"], r["ntargets"]) == ("53248", "16384", str((200 * 2 ** 20 - 1) // 16384))
    # the threshold is a knob: 0 switches the feature off, a small one still wants three finders
    assert model("geom", 0, 2 ** 20)[0]["long"] == "0"
    assert [r["long"] for r in model("geom", 1000, 49152, 49153)] == ["0", "1"]


@pytest.mark.parametrize("shape", [(1, 7, 6, 131072), (256, 5000, 4000, 2 ** 28), (3, 100, 50, 0), (2 ** 32 - 2, 2 ** 32 - 2, 2 ** 31, 2 ** 43)])
def test_scratch_regions_are_aligned_disjoint_and_do_not_wrap(model, shape):
    nitems, ntargets, npieces, room = shape
    f = model("plan", *shape)[0]
    pages = room // HALF + npieces + 2
    want = {"targets": ntargets * 24, "found": ntargets * 16, "rows": npieces * 32, "ends": npieces * 16, "status": npieces * 16, "ostart": npieces * 8, "ranges": nitems * 8,
            "cnt": 64, "owner": pages * 8, "windows": npieces * RING, "entry": RING, "tails": npieces * RING * 2, "mid": pages * HALF * 2}
    assert int(f["page_cap"]) == pages
    at = 0
    for name, size in want.items():  # (the plan's own order)
        off, nbytes = (int(x) for x in f[name].split(":"))
        assert nbytes == size, name  # exactly the records: nothing wrapped
        assert off % ALIGN == 0 and off >= at, name
        at = off + nbytes
    assert at <= int(f["total"]) < 2 ** 63


def test_a_round_that_cannot_be_counted_is_declined(model):
    for shape in ((2 ** 32 - 1, 10, 10, 10), (10, 2 ** 32 - 1, 10, 10), (10, 10, 2 ** 32 - 1, 10), (10, 10, 10, 2 ** 44), (10, 10, 2 ** 31, 2 ** 32 * HALF)):
        assert model("plan", *shape)[0]["total"] == "0", shape


def test_round_split_by_hand(model):
    rooms = [40, 40, 40, 150, 10, 90, 10]
    rows = model("rounds", 100, *["%d:7:6" % r for r in rooms])
    assert [(int(r["first"]), int(r["last"])) for r in rows] == [(0, 2), (2, 3), (3, 4), (4, 6), (6, 7)]
    assert [int(r["room"]) for r in rows] == [80, 40, 150, 100, 10]
    # scratch: 10,000 slots are 1.3 GB of tails, windows and pages -- two such items pass 2 GiB whatever their rooms
    rows = model("rounds", 2 ** 40, *["1000:40000:10000"] * 3)
    assert [(int(r["first"]), int(r["last"])) for r in rows] == [(0, 1), (1, 2), (2, 3)]


def test_round_split_covers_every_item_once_and_keeps_the_cap(model):
    rnd = random.Random(5)
    for cap in (1, 1 << 20, 64 << 20):
        items = [(rnd.choice((0, 1, 1000, 1 << 20, 3 << 20, 100 << 20)), rnd.randrange(3, 2000), rnd.randrange(1, 700)) for _ in range(300)]
        rows = model("rounds", cap, *["%d:%d:%d" % it for it in items])
        nxt = 0
        for r in rows:
            first, last = int(r["first"]), int(r["last"])
            assert first == nxt and last > first
            nxt = last
            room = sum(it[0] for it in items[first:last])
            scratch = sum(it[0] * 2 + it[0] // HALF * 8 + it[2] * PER_PIECE + it[1] * PER_TARGET + 16 for it in items[first:last])
            assert (room, scratch) == (int(r["room"]), int(r["scratch"]))
            if last - first > 1:
                assert room <= cap and scratch <= SCRATCH_CAP
            if last < len(items):  # greedy: the next item would not have fitted
                nx = items[last]
                assert room + nx[0] > cap or scratch + nx[0] * 2 + nx[0] // HALF * 8 + nx[2] * PER_PIECE + nx[1] * PER_TARGET + 16 > SCRATCH_CAP
        assert nxt == len(items)


def select(model, spacing, first_bit, end, cap, dyn, sto, lens):
    lst = lambda v: ",".join("-" if x is None else str(x) for x in v) if v else "-"
    return model("select", spacing, first_bit, end, cap, lst(dyn), lst(sto), ",".join("%d:%d" % p for p in lens) if lens else "-")[0]["starts"]


def test_selection_keeps_the_distance_and_the_end(model):
    # spacing 1000: starts 6000 bits apart, more than 2000 bits before bit 80000
    got = select(model, 1000, 16, 10000, 20, [3000, 6100, 12200, 13000, 77000, 78500], [None] * 6, [])
    assert got == "16,6100,12200,77000"
    assert select(model, 1000, 16, 10000, 20, [6015, 6016], [None, None], []) == "16,6016"  # exactly 6 * spacing behind the first bit
    assert select(model, 1000, 16, 10000, 20, [77999, 78000], [None, None], []) == "16,77999"  # bit 78000 is 2 * spacing before the end, not more


def test_selection_strikes_starts_inside_a_vouched_stored_block(model):
    # a stored block whose LEN lies at byte 1000: its bytes are bits [8000, (1000 + 4 + LEN) * 8)
    assert select(model, 1000, 16, 10000, 20, [None, 9000, 14500], [None, 1000, None], [(1000, 500)]) == "16,8000s,14500"
    assert select(model, 1000, 16, 10000, 20, [None, 9000, 14500], [None, 1000, None], [(1000, 900)]) == "16,8000s"
    # the vouched block is looked up from a later finder too
    assert select(model, 100, 16, 10000, 20, [None, None, 20000], [None, 1000, None], [(1000, 2000)]) == "16,8000s"
    assert select(model, 100, 16, 10000, 20, [None, None, 20000], [None, 1000, None], [(1000, 1000)]) == "16,8000s,20000"
    # a stored start keeps its flag and obeys the same distances; at one finder the earlier position goes first
    assert select(model, 1000, 16, 10000, 20, [7000], [1000], [(1000, 0)]) == "16,7000"
    assert select(model, 1000, 16, 10000, 20, [8100], [1000], [(1000, 0)]) == "16,8000s"


def test_selection_always_begins_with_the_first_bit_and_respects_the_cap(model):
    assert select(model, 32768, 80, 200000, 6, [], [], []) == "80"
    assert select(model, 1000, 16, 10000, 1, [6100, 12200], [None, None], []) == "16"
    assert select(model, 1000, 16, 10000, 2, [6100, 12200], [None, None], []) == "16,6100"
    assert select(model, 1000, 16, 10000, 20, [None, None], [None, None], []) == "16"
