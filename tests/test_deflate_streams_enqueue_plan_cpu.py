"""What the stream-ordered batch compress of items of any length decides from plain numbers (zlib_amd/csrc/zgpu_deflate_streams_plan.h, the part behind
"the stream-ordered call"): the host's upper bound of the tiles, the workspace, the rooms' bound, and the plan the DEVICE makes from the caller's tables --
item states, the tiles and checksum pieces in front of every item, the rows of the padded tile list, the parts of every round.  The kernels call these
functions lane by lane; tests/tools/deflate_streams_enqueue_plan_model.cpp calls them in loops and compares the device's judgement of the tables with the
host's (streams_tile_scan, streams_tile_row) and the round plan both calls share (streams_round_plan, streams_part_args) with a derivation by brute force
written out in the tool.  No GPU is used.  The model is built twice, once with ASan + UBSan."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "deflate_streams_enqueue_plan_model.cpp")
TILE, CHUNK, SLOT = 32512, 65536, 65792
EDGES = [0, 1, 65024, 65025, 97536, 97537, 2 ** 32 - 1]
FINAL, ZLIB, GZIP = 1, 2, 16


def build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g"] + extra + ["-o", exe, SRC], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("senq_plan")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    return build(tmp, "model", []), build(tmp, "model_san", san)


@pytest.fixture(scope="module")
def model(exes):
    def run(rows, san=False):
        out = subprocess.run([exes[1 if san else 0]] + rows, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = out.stdout.splitlines()
        assert len(lines) == len(rows)
        return lines
    return run


def kv(line):
    return dict(w.split("=", 1) for w in line.split()[1:])


def ntiles(n):
    return 0 if n == 0 else 1 if n <= 2 * TILE else -(-(n - 2 * TILE) // TILE) + 1


def test_ntiles_max_bounds_the_tile_count(model):
    """streams_ntiles(L) <= L / kTileStride + 1 at the edges and at random lengths, so in_bytes / kTileStride + n bounds the tiles of a table that runs forward"""
    rng = random.Random(3)
    lens = EDGES + [rng.randrange(2 ** 32) for _ in range(200)] + [rng.randrange(300000) for _ in range(200)] + [TILE * k + d for k in range(1, 8) for d in (-1, 0, 1)]
    got = kv(model(["ntiles " + " ".join(map(str, lens))])[0])
    for L in lens:
        nt, bound = map(int, got[str(L)].split(","))
        assert nt == ntiles(L) and bound == L // TILE + 1 and nt <= bound, L
    assert got[str(2 ** 32 - 1)].split(",")[0] == str(ntiles(2 ** 32 - 1))
    for _ in range(200):  # tables: the sum of the items' tiles against the host's bound
        sizes = [rng.choice(EDGES[:-1] + [rng.randrange(400000)]) for _ in range(rng.randrange(1, 30))]
        assert sum(ntiles(s) for s in sizes) <= sum(sizes) // TILE + len(sizes)


def ws(model, n, in_bytes, batch):
    d = kv(model(["ws %d %d %d" % (n, in_bytes, batch)])[0])
    regions = [(k, tuple(map(int, v.split(",")))) for k, v in d.items() if "," in v]
    return d, regions


def test_workspace(model):
    """a function of (n, in_bytes, batch_tiles) alone, monotone in each; regions disjoint and 256-aligned; room for a round whose every tile is a stream"""
    names = ["cnt", "state", "tile0", "piece0", "rows", "entry", "st", "check", "ckpart", "round", "parts", "tokoff", "blk_item", "exits", "comp", "gentry", "carry",
             "T", "blk", "pos", "slots", "tokens", "meta", "sorted"]
    for n, in_bytes, batch in [(1, 1, 0), (21, 1783000, 0), (21, 1783000, 3), (4096, 4096 * 98304, 0), (5, 0, 7), (100000, 10 ** 9, 40000), (1, 2 ** 40, 1), (3, 100, 64)]:
        d, regions = ws(model, n, in_bytes, batch)
        assert [k for k, _ in regions] == names
        ntiles_max = in_bytes // TILE + n
        b = min(batch or 2048, 32768, ntiles_max)
        assert (int(d["ntiles_max"]), int(d["batch"]), int(d["rounds"])) == (ntiles_max, b, -(-ntiles_max // b))
        at = 0
        for name, (off, size) in regions:
            assert off % 256 == 0 and off >= at, name
            at = off + size
        assert at <= int(d["total"]) and int(d["total"]) % 256 == 0
        r = dict(regions)
        for need in ("parts", "tokoff", "blk_item", "T", "blk", "pos", "slots"):
            assert r[need][1] >= int(d["need_" + need]), need
        nt = int(d["rounds"]) * b
        assert r["rows"][1] == 32 * nt and r["entry"][1] >= 2 * (nt + 1) and r["ckpart"][1] >= 12 * ntiles_max and r["st"][1] == 64 * n and r["state"][1] == 4 * n
        assert r["tile0"][1] == 8 * (n + 1) == r["piece0"][1] and r["tokens"][1] == 4 * CHUNK * b and r["exits"][1] == 1040 * b and r["meta"][1] == 32 * b
        assert r["sorted"][1] == 256 + 1058832 * b + 1024 and r["slots"][1] == 7 * SLOT * b and r["T"][1] == 4 * 81920 * b
    total = lambda n, i, b: int(ws(model, n, i, b)[0]["total"])  # noqa: E731
    assert total(2 ** 32, 0, 0) == 0 and total(2 ** 32 - 1, 0, 1) > 0
    for n, i, b in [(1, 0, 1), (10, 500000, 4), (1000, 10 ** 8, 512)]:
        assert total(n, i, b) <= total(n + 1, i, b) and total(n, i, b) <= total(n, i + TILE, b) and total(n, i, b) <= total(n, i, b + 1)
        assert total(n, i, b) <= total(n + 1000, i, b) and total(n, i, b) < total(n, i + 10 ** 7, b)
    assert total(10, 500000, 0) == total(10, 500000, 2048) == total(10, 500000, 25) and total(10 ** 6, 10 ** 10, 32768) == total(10 ** 6, 10 ** 10, 10 ** 6)


def test_rooms_bound(model):
    """at least streams_layout's total on random tables that end inside in_bytes; tightest -- equal -- for one item of in_bytes"""
    rng = random.Random(5)
    rows, slack = [], []
    for _ in range(300):
        sizes = [rng.choice([0, 1, 7, 8, 63, 64, 16382, 16383, 16384, rng.randrange(300000)]) for _ in range(rng.randrange(1, 40))]
        s = rng.choice([0, 0, rng.randrange(100000)])
        slack.append(s)
        rows.append("rooms %d %d %s" % (rng.choice([FINAL, FINAL | ZLIB, FINAL | GZIP]), sum(sizes) + s, " ".join(map(str, sizes))))
    for row, line in zip(rows, model(rows)):
        d = kv(line)
        assert int(d["bound"]) >= int(d["total"]) and int(d["bound"]) % 4 == 0, row
    for flags in (FINAL, FINAL | ZLIB, FINAL | GZIP):
        for L in (0, 1, 16383, 65536, 300007, 2 ** 32 - 1):
            d = kv(model(["rooms %d %d %d" % (flags, L, L)])[0])
            assert d["bound"] == d["total"], (flags, L)


def test_scan_of_explicit_tables(model):
    """states (0 served, 1 bad, 2 too long), tile0 and piece0 of tables written out by hand"""
    big = 2 ** 33
    rows = [
        "scan 300000 1000 0 70000 50000 120000 / 0 100 200 300",        # item 1 backwards
        "scan 300000 1000 0 300000 0 300000 / 0 100 200 300",           # overlapping: 9 + 9 tiles asked for, 9 + 3 laid out
        "scan 1000 1000 0 10 1001 / 0 100 200",                         # past in_bytes
        "scan 1000 1000 0 10 20 30 40 / 0 100 96 200 1004",             # room backwards (item 1), room past out_cap (item 3)
        "scan 1000 1000 0 10 20 / 0 102 200",                           # room not at a multiple of 4 (item 1)
        "scan %d 1000 0 %d %d / 0 100 200" % (big, 2 ** 32, 2 ** 32 + 5),  # 4 GiB: too long
        "scan 200000 1000 0 0 1 4097 69633 200000 / 0 100 200 300 400 500",
    ]
    got = [kv(x) for x in model(rows)]
    assert (got[0]["states"], got[0]["tile0"]) == ("0,1,0", "0,2,2,4")
    assert (got[1]["states"], got[1]["tile0"]) == ("0,1,1", "0,9,9,9")
    assert (got[2]["states"], got[2]["tile0"]) == ("0,1", "0,1,1")
    assert got[3]["states"] == "0,1,0,1" and got[4]["states"] == "0,1"
    assert (got[5]["states"], got[5]["tile0"]) == ("2,0", "0,0,1")
    assert (got[6]["states"], got[6]["tile0"], got[6]["piece0"]) == ("0,0,0,0,0", "0,0,1,2,4,%d" % (4 + ntiles(130367)), "0,0,0,0,1,3")


# (batch, seed, count): tables, tiles, rounds, parts, open_parts, pad_rows -- what the tool printed of these tables while the blocking call still had a
# part arithmetic of its own, which was the other side of the comparison then; the brute-force derivation must walk the very same tables and parts
PLAN_COUNTS = {
    (1, 12, 400): (400, 16548, 21697, 16548, 12659, 5149),
    (2, 13, 400): (400, 17251, 11291, 10578, 6625, 5325),
    (3, 14, 400): (400, 17875, 7827, 8606, 4547, 5582),
    (7, 18, 400): (400, 19103, 3676, 6171, 2048, 6558),
    (64, 75, 400): (400, 19098, 606, 4232, 97, 12149),
    (3, 5, 150): (150, 6764, 2958, 3239, 1707, 2109),
    (64, 6, 150): (150, 7073, 227, 1661, 38, 4616),
}


def plan_counts(d):
    return tuple(int(d[k]) for k in ("tables", "tiles", "rounds", "parts", "open_parts", "pad_rows"))


@pytest.mark.parametrize("batch", [1, 2, 3, 7, 64])
def test_device_plan_equals_the_host_plan(model, batch):
    d = kv(model(["plan %d %d 400" % (batch, 11 + batch)])[0])
    assert int(d["mismatches"]) == 0, d
    assert plan_counts(d) == PLAN_COUNTS[(batch, 11 + batch, 400)], d
    assert int(d["tables"]) == 400 and int(d["parts"]) > 400 and int(d["pad_rows"]) > 0, d
    if batch < 64:
        assert int(d["open_parts"]) > 0, d  # rounds that end inside streams


def test_overlapping_ranges_never_grow_the_list(model):
    d = kv(model(["overlap 7 3000"])[0])
    assert int(d["mismatches"]) == 0 and int(d["tables"]) == 3000 and int(d["capped_items"]) > 0 and int(d["failed_items"]) > 0, d


def test_model_under_the_sanitizers(model):
    """the same program built with -fsanitize=address,undefined (a stand-alone program, its own main)"""
    rows = ["plan 3 5 150", "plan 64 6 150", "overlap 9 500", "ws 21 1783000 3", "rooms 3 500000 1 65536 300007", "ntiles 0 1 65024 65025 4294967295",
            "scan 300000 1000 0 300000 0 300000 / 0 100 200 300"]
    plain, san = model(rows), model(rows, san=True)
    assert plain == san
    assert all(int(kv(x)["mismatches"]) == 0 for x in san[:3])
    assert plan_counts(kv(san[0])) == PLAN_COUNTS[(3, 5, 150)] and plan_counts(kv(san[1])) == PLAN_COUNTS[(64, 6, 150)]
