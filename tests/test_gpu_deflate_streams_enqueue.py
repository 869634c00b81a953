"""The stream-ordered batch compress of items of any length, zgpu_deflate_streams_enqueue (+ _workspace_bytes, _rooms_bound, _layout_enqueue): what
zgpu_deflate_streams_device makes, enqueued on the caller's stream with a caller-owned workspace and nothing read back.  The yardstick is the blocking
call of the same build -- record for record, byte for byte -- which tests/test_gpu_deflate_streams.py pins to the reference; one test here goes to the
compiled reference directly.  The sizes sit on the tile and block edges that file uses.  Device memory is held in torch tensors: the destination between
two 64-byte guards of 0xA5, records (with 64 spare bytes behind them) and summary pre-filled with 0xEE, 256 spare bytes of 0xEE behind the workspace;
results() checks every guard after every call.  Every call here is followed by a synchronize of the test's own."""
import ctypes as C
import hashlib
import json
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import blockcases as BC, cases, refzlib as R  # noqa: E402

OK, ERRNO, STREAM_ERROR, BUF_ERROR = 0, -1, -2, -5
FILL, GUARD, SPARE = 0xA5, 64, 256
REC = np.dtype([("code", "<i4"), ("data_type", "<u4"), ("out_lo", "<u8"), ("out_bytes", "<u8"), ("in_bytes", "<u4"), ("adler32", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])
F_FINAL, F_ZLIB, F_GZIP, F_CRC32 = 1, 2, 16, 32
WRAP_FLAGS = {"raw": F_FINAL, "zlib": F_FINAL | F_ZLIB, "gzip": F_FINAL | F_GZIP}
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
WRAP_OF = {-15: "raw", 15: "zlib", 31: "gzip"}
SIZES = (0, 1, 2, 3, 65023, 65024, 65025, 65535, 65536, 65537, 97535, 97536, 97537, 98047, 98048, 98049, 130047, 130048, 130049, 200000, 300007)
ITEMS = [cases.make(("text", "rand", "runs")[i % 3], n, 40 + i) for i, n in enumerate(SIZES)]
SMALL = [ITEMS[k] for k in (5, 9, 12, 1, 0, 18)]  # 65024, 65537, 97537, 1, 0, 130049 bytes
FAILED = (STREAM_ERROR, 2, 0, 0, 0, 1, 0)  # the record of an item the table check has failed
KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "block_kat.json")))["cases"]
TILE = 32512


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.set_exact_sort(0)
    e.close()


def table(sizes):
    return [0] + [int(x) for x in np.cumsum(sizes)]


def dev_u64(values):
    import torch
    return torch.tensor(np.array(values, dtype=np.uint64).view(np.int64), device="cuda:0")


def fields(r):
    return tuple(int(r[f]) for f in ("code", "data_type", "out_lo", "out_bytes", "in_bytes", "adler32", "crc32"))


_blocking = {}


def blocking(eng, items, level, flags, strategy=0):
    """zgpu_deflate_streams_device over the same items in rooms of the layout, once per (items, level, flags, strategy): (streams, records without out_lo)"""
    import torch
    key = (tuple((len(b), hash(b)) for b in items), level, flags, strategy)
    if key not in _blocking:
        n = len(items)
        offs = table([len(b) for b in items])
        oo, total = eng.deflate_streams_layout(offs, flags)
        d_in = torch.tensor(np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8), device="cuda:0")
        d_io, d_oo = dev_u64(offs), dev_u64(oo)
        d_out = torch.zeros(max(total, 4), dtype=torch.uint8, device="cuda:0")
        d_items = torch.zeros(max(n, 1) * REC.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        eng.deflate_streams_device(d_in.data_ptr(), offs[-1], d_io.data_ptr(), n, level, d_out.data_ptr(), total, d_oo.data_ptr(), d_items.data_ptr(), flags=flags, strategy=strategy)
        recs = [fields(r) for r in np.frombuffer(d_items.cpu().numpy().tobytes(), dtype=REC, count=n)]
        out = d_out.cpu().numpy()
        assert all(r[0] == OK for r in recs)
        _blocking[key] = ([out[int(oo[k]): int(oo[k]) + recs[k][3]].tobytes() for k in range(n)], [r[:2] + r[3:] for r in recs])
    return _blocking[key]


class Dev:
    """One call in device memory.  in_offs / in_bytes: a table of the caller's own over the blob; oo: the rooms (None: the layout's); out_cap: None = oo[n]"""

    def __init__(self, eng, items, flags, oo=None, in_offs=None, in_bytes=None, out_cap=None, batch_tiles=0, ws_short=0, ws_shift=0, out_shift=0):
        import torch
        from zlib_amd import gpu
        self.eng, self.flags, self.batch_tiles = eng, flags, batch_tiles
        offs = table([len(b) for b in items]) if in_offs is None else list(in_offs)
        self.n = len(offs) - 1
        blob = np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8)
        self.in_bytes = len(blob) - 1 if in_bytes is None else in_bytes
        if oo is None:
            oo = [int(x) for x in eng.deflate_streams_layout(offs, flags)[0]]
        self.oo = list(oo)
        self.out_cap = self.oo[-1] if out_cap is None else out_cap
        self.d_in = torch.tensor(blob, device="cuda:0")
        self.d_io, self.d_oo = dev_u64(offs), dev_u64(self.oo)
        self.d_items = torch.full((self.n * REC.itemsize + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
        self.d_sum = torch.full((C.sizeof(gpu.DeflateBatchSummary),), 0xEE, dtype=torch.uint8, device="cuda:0")
        need = eng.deflate_streams_workspace_bytes(self.n, self.in_bytes, batch_tiles)
        self.ws_bytes = need - ws_short
        self.d_ws = torch.full((need + ws_shift + SPARE,), 0xEE, dtype=torch.uint8, device="cuda:0")
        assert self.d_ws.data_ptr() % 256 == 0
        self.ws_ptr, self.ws_shift = self.d_ws.data_ptr() + ws_shift, ws_shift
        self.d_buf = torch.full((self.out_cap + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        assert self.d_buf.data_ptr() % 4 == 0
        self.d_out = self.d_buf.data_ptr() + GUARD + out_shift
        torch.cuda.synchronize()

    def enqueue(self, level, stream=None, strategy=0, flags=None, d_items="own", n=None, **kw):
        self.eng.deflate_streams_enqueue(self.d_in.data_ptr(), self.in_bytes, self.d_io.data_ptr(), self.n if n is None else n, level, self.d_out, self.out_cap,
                                         self.d_oo.data_ptr(), self.d_items.data_ptr() if d_items == "own" else d_items, self.ws_ptr, self.ws_bytes,
                                         flags=self.flags if flags is None else flags, strategy=strategy, batch_tiles=self.batch_tiles, d_summary=self.d_sum.data_ptr(),
                                         stream=stream, **kw)

    def results(self):
        """after a synchronize: the records' fields, the summary (nfailed, nbad_offsets, ntoo_long, total, overflow, sort_fault), the destination without its
        guards -- which are checked here, as the spare bytes behind the records and behind the workspace are"""
        import torch
        torch.cuda.synchronize()
        raw = self.d_items.cpu().numpy()
        assert (raw[self.n * REC.itemsize:] == 0xEE).all(), "a byte behind the records was written"
        recs = [fields(r) for r in np.frombuffer(raw.tobytes(), dtype=REC, count=self.n)]
        summary = struct.unpack("<QQQQII", self.d_sum.cpu().numpy().tobytes())
        buf = self.d_buf.cpu().numpy()
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + self.out_cap:] == FILL).all(), "a byte outside the destination was written"
        assert (self.d_ws[self.ws_shift + self.ws_bytes:].cpu().numpy() == 0xEE).all(), "a byte behind the workspace was written"
        return recs, summary, buf[GUARD: GUARD + self.out_cap]

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.d_buf == FILL).all()) and bool((self.d_items == 0xEE).all()) and bool((self.d_sum == 0xEE).all()) and bool((self.d_ws == 0xEE).all())


def check_equal(d, streams, brecs, which=None):
    """the call's streams, records and summary are the blocking call's (which: the items to look at, all by default)"""
    recs, summary, out = d.results()
    ks = range(d.n) if which is None else which
    for k in ks:
        assert recs[k] == brecs[k][:2] + (d.oo[k],) + brecs[k][2:], (k, recs[k], brecs[k])
        assert out[d.oo[k]: d.oo[k] + len(streams[k])].tobytes() == streams[k], k
    if which is None:
        assert summary == (0, 0, 0, sum(len(s) for s in streams), 0, 0)
    return recs, summary, out


def run(eng, items, level, flags, strategy=0, batch_tiles=0):
    streams, brecs = blocking(eng, items, level, flags, strategy)
    d = Dev(eng, items, flags, batch_tiles=batch_tiles)
    d.enqueue(level, strategy=strategy)
    check_equal(d, streams, brecs)
    return streams


PARAMS = [(lv, w, 0) for lv in (4, 6, 9) for w in ("raw", "zlib", "gzip")] + [(6, "raw", s) for s in (1, 2, 3, 4)]


@pytest.mark.parametrize("level,wrap,strategy", PARAMS, ids=lambda v: str(v))
def test_catalogue_equals_the_blocking_call(eng, level, wrap, strategy):
    """1. streams, records and summary, byte for byte"""
    streams = run(eng, ITEMS, level, WRAP_FLAGS[wrap] | (F_CRC32 if wrap == "raw" else 0), strategy)
    assert len(streams) == len(ITEMS)


@pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref) is not here")
@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
def test_catalogue_equals_the_reference(eng, wrap):
    want = [R.compress2(d, 6) if wrap == "zlib" else R.deflate_wbits(d, 6, WBITS[wrap]) for d in ITEMS]
    d = Dev(eng, ITEMS, WRAP_FLAGS[wrap])
    d.enqueue(6)
    recs, summary, out = d.results()
    assert summary == (0, 0, 0, sum(len(z) for z in want), 0, 0)
    bad = [k for k, z in enumerate(want) if out[d.oo[k]: d.oo[k] + len(z)].tobytes() != z or recs[k][:5] != (OK, recs[k][1], d.oo[k], len(z), len(ITEMS[k]))]
    assert not bad, bad


def padded_items():
    """twenty empty and twenty 1-byte items among large ones: ntiles_max = in_bytes / 32512 + n exceeds the real tile count by more than thirty"""
    items = []
    for i in range(20):
        items += [b"", ITEMS[4 + i % 15], cases.make("text", 1, i)]
    return items


@pytest.mark.parametrize("batch_tiles", [1, 2, 3, 7, 0])
def test_rounds_give_the_same_bytes(eng, batch_tiles):
    """2. rounds that end inside streams, and whole rounds of padding rows behind the last real tile"""
    items = padded_items()
    real = sum(0 if len(b) == 0 else 1 if len(b) <= 2 * TILE else -(-(len(b) - 2 * TILE) // TILE) + 1 for b in items)
    ntiles_max = sum(len(b) for b in items) // TILE + len(items)
    assert ntiles_max - real >= 3 * 3  # several whole rounds of padding at batch_tiles = 3
    run(eng, items, 6, WRAP_FLAGS["zlib"], batch_tiles=batch_tiles)
    run(eng, ITEMS, 6, WRAP_FLAGS["gzip"], batch_tiles=batch_tiles)


@pytest.mark.parametrize("batch_tiles", [0, 259, 260])
def test_a_part_longer_than_the_scans_lanes(eng, batch_tiles):
    """2b. an item of 301 tiles and some 370 blocks among short ones (tests/streams_long_fixtures.py): the batched scans' 256 lanes take runs of tiles and
    of blocks.  One round (a part of 301 tiles), rounds of 259 (the long item's first part: 256 tiles) and of 260 (257).  Every item is the product's
    one-call continuous stream of that item, every record ZGPU_OK with zlib's adler32, and zlib gives the item back"""
    import streams_long_fixtures as LF
    LF.one_call_streams(eng)
    d = Dev(eng, list(LF.items()), WRAP_FLAGS["zlib"], batch_tiles=batch_tiles)
    d.enqueue(6)
    recs, summary, out = d.results()
    assert summary[:3] == (0, 0, 0) and summary[4:] == (0, 0), summary
    LF.check([out[d.oo[k]: d.oo[k] + recs[k][3]].tobytes() for k in range(d.n)], [(r[0], r[5]) for r in recs])


@pytest.mark.parametrize("batch_tiles", [0, 1])
def test_block_catalogue_as_one_call(eng, batch_tiles):
    """3. the rows test_block_catalogue_as_one_batch selects, grouped by (level, strategy, wbits), one enqueue per group: (len, sha) of tests/golden/block_kat.json"""
    rows = [c for c in BC.catalogue() if not c.calls and c.level >= 4]
    assert {c.family for c in rows} == {"phase", "full", "edge", "many"}
    groups = {}
    for c in rows:
        groups.setdefault((c.level, c.strategy, c.wbits), []).append(c)
    bad = []
    for (level, strategy, wbits), cs in sorted(groups.items()):
        d = Dev(eng, [c.data for c in cs], WRAP_FLAGS[WRAP_OF[wbits]], batch_tiles=batch_tiles)
        d.enqueue(level, strategy=strategy)
        recs, summary, out = d.results()
        assert summary[:3] == (0, 0, 0) and summary[4:] == (0, 0)
        for k, c in enumerate(cs):
            s = out[d.oo[k]: d.oo[k] + recs[k][3]].tobytes()
            if recs[k][0] != OK or (len(s), hashlib.sha256(s).hexdigest()[:16]) != (KAT[c.name]["len"], KAT[c.name]["sha"]):
                bad.append("%s: code %d, %d bytes, owed %d" % (c.name, recs[k][0], len(s), KAT[c.name]["len"]))
    assert not bad, "%d of %d rows\n" % (len(bad), len(rows)) + "\n".join(bad[:40])


def test_bad_tables_fail_their_item_alone(eng):
    """4. the neighbours of a bad entry are byte-equal to a call of their own"""
    blob = cases.make("text", 300000, 9)
    flags = WRAP_FLAGS["gzip"]
    room = [int(x) for x in eng.deflate_streams_layout([0, 300000], flags)[0]][1]

    def served(lo, hi):
        streams, brecs = blocking(eng, [blob[lo:hi]], 6, flags)
        return streams[0], brecs[0]

    def rooms(n):
        return [k * room for k in range(n + 1)]

    r3 = rooms(3)
    cases_ = {
        # name: (in_offsets, in_bytes, out_offsets, out_cap, items that fail)
        "input backwards": ([0, 70000, 50000, 120000], None, r3, None, [1]),                  # items 0 and 2 are good, and they overlap
        "input past in_bytes": ([0, 1000, 300001], None, rooms(2), None, [1]),
        "input past the in_bytes argument": ([0, 1000, 70000], 69999, rooms(2), None, [1]),
        "overlapping ranges over ntiles_max": ([0, 300000, 0, 300000], None, r3, None, [1, 2]),  # 9 + 9 tiles asked for, 9 + 3 laid out: the second range fails too
        "room backwards": ([0, 70000, 140000, 210000], None, [0, 2 * room, room, 3 * room], None, [1]),
        "room past out_cap": ([0, 70000, 140000, 210000], None, r3, 3 * room - 4, [2]),
        "room not at a multiple of 4": ([0, 70000, 140000, 210000], None, [0, room, 2 * room + 2, 3 * room], None, [2]),
    }
    for name, (io, in_bytes, oo, out_cap, failing) in cases_.items():
        n = len(io) - 1
        d = Dev(eng, [blob], flags, oo=oo, in_offs=io, in_bytes=in_bytes, out_cap=out_cap)
        d.enqueue(6)
        recs, summary, out = d.results()
        total = 0
        for k in range(n):
            if k in failing:
                assert recs[k] == FAILED, (name, k, recs[k])
            else:
                z, b = served(io[k], io[k + 1])
                assert recs[k] == b[:2] + (oo[k],) + b[2:], (name, k)
                assert out[oo[k]: oo[k] + len(z)].tobytes() == z, (name, k)
                total += len(z)
        assert summary == (len(failing), len(failing), 0, total, 0, 0), (name, summary)
        if name == "input past in_bytes":
            assert (out[oo[1]: oo[2]] == FILL).all()  # a failed item's room is left alone


@pytest.mark.parametrize("room", [8, 64])
def test_a_room_too_small_fails_its_item_alone(eng, room):
    """5. ZGPU_BUF_ERROR with out_bytes = 0 for the item, everything else as with room enough"""
    flags = WRAP_FLAGS["zlib"]
    streams, brecs = blocking(eng, SMALL, 6, flags)
    oo = [int(x) for x in eng.deflate_streams_layout(table([len(b) for b in SMALL]), flags)[0]]
    short = 2
    rooms = oo[: short + 1] + [x - (oo[short + 1] - oo[short]) + room for x in oo[short + 1:]]
    d = Dev(eng, SMALL, flags, oo=rooms)
    d.enqueue(6)
    recs, summary, out = check_equal(d, streams, brecs, which=[k for k in range(len(SMALL)) if k != short])
    assert recs[short][0] == BUF_ERROR and recs[short][3] == 0 and recs[short][4:] == brecs[short][3:]
    assert summary == (1, 0, 0, sum(len(s) for k, s in enumerate(streams) if k != short), 0, 0)
    if room == 8:
        assert (out[rooms[short]: rooms[short + 1]] == FILL).all(), "a room too small for the smallest stream is left alone"


def test_degenerate_batches(eng):
    """6. n = 0 (at most the summary is written), n = 1, only empty items"""
    flags = WRAP_FLAGS["zlib"]
    d = Dev(eng, [], flags, oo=[0], out_cap=16)
    d.enqueue(6)
    _, summary, out = d.results()
    assert summary == (0, 0, 0, 0, 0, 0) and (out == FILL).all()
    assert bool((d.d_items == 0xEE).all()) and bool((d.d_ws == 0xEE).all())
    run(eng, [ITEMS[12]], 6, flags)
    run(eng, [b""], 6, flags)
    empties = run(eng, [b""] * 5, 6, WRAP_FLAGS["gzip"])
    assert all(len(s) == 20 for s in empties)


def test_refusals_touch_nothing(eng):
    """8. every refusal of the blocking call's list, and what the host can judge of the arguments: ZGPU_STREAM_ERROR, nothing enqueued"""
    from zlib_amd import gpu
    flags = WRAP_FLAGS["raw"]

    def refused(d=None, level=6, **kw):
        d = d or Dev(eng, SMALL, flags)
        with pytest.raises(gpu.EngineError) as ei:
            d.enqueue(level, **kw)
        assert ei.value.code == STREAM_ERROR, kw
        assert d.untouched(), kw
        return d

    d = refused(level=1)
    for kw in (dict(level=3), dict(level=0), dict(level=10), dict(flags=F_FINAL | F_ZLIB | F_GZIP), dict(flags=0), dict(flags=F_FINAL | 64), dict(flags=F_FINAL | 128),
               dict(flags=F_FINAL | 4), dict(flags=F_FINAL | 8), dict(lz_impl=gpu.LZ_WALK), dict(strategy=5), dict(strategy=-1), dict(prime=(3 << 16) | 5), dict(d_items=None),
               dict(n=2 ** 32)):
        refused(d, **kw)
    eng.set_geometry(14, 8)
    try:
        refused(d)
    finally:
        eng.set_geometry(15, 8)
    refused(Dev(eng, SMALL, flags, ws_short=1))
    refused(Dev(eng, SMALL, flags, ws_shift=128))
    refused(Dev(eng, SMALL, flags, out_shift=2))
    assert eng.deflate_streams_workspace_bytes(2 ** 32, 0) == 0
    d.enqueue(6)  # and the same object, unchanged, is served
    recs, summary, _ = d.results()
    assert summary[0] == 0 and all(r[0] == OK for r in recs)


def test_sort_self_check(eng):
    """9. zgpu_debug_inject_sort_fault() sets a flag: the next launch of the fast sort is followed by a memset that raises the fault word (nothing faults).
    The call spans several rounds; the word is raised in the first and read behind the last"""
    flags = WRAP_FLAGS["zlib"]
    streams, brecs = blocking(eng, SMALL, 6, flags)
    try:
        assert eng.L.zgpu_debug_sort_fallback(eng.h) == 0
        eng.L.zgpu_debug_inject_sort_fault.restype = None
        eng.L.zgpu_debug_inject_sort_fault()
        d = Dev(eng, SMALL, flags, batch_tiles=2)
        assert eng.deflate_streams_workspace_bytes(d.n, d.in_bytes, 2) < eng.deflate_streams_workspace_bytes(d.n, d.in_bytes, 4)  # (more than two tiles: more than one round)
        d.enqueue(6)
        recs, summary, _ = d.results()
        assert summary[0] == len(SMALL) and summary[5] == 1
        assert [r[0] for r in recs] == [ERRNO] * len(SMALL)
        assert eng.L.zgpu_debug_sort_fallback(eng.h) == 0  # the host cannot do it for the caller
        eng.set_exact_sort(1)
        d = Dev(eng, SMALL, flags, batch_tiles=2)
        d.enqueue(6)
        check_equal(d, streams, brecs)
    finally:
        eng.set_exact_sort(0)
    assert eng.L.zgpu_debug_sort_fallback(eng.h) == 0


def test_two_calls_in_flight(eng):
    """10. two streams, two workspaces, one engine"""
    import torch
    flags = WRAP_FLAGS["gzip"]
    batches = []
    for seed in (1, 2):
        items = [cases.make(("text", "runs")[seed - 1], 30000 + 27000 * k, 10 * seed + k) for k in range(6)]
        streams, brecs = blocking(eng, items, 6, flags)
        batches.append((streams, brecs, Dev(eng, items, flags, batch_tiles=3), torch.cuda.Stream()))
    for streams, brecs, d, s in batches:
        d.enqueue(6, stream=s.cuda_stream)
    for streams, brecs, d, s in batches:
        s.synchronize()
    for streams, brecs, d, s in batches:
        check_equal(d, streams, brecs)


def test_call_is_stream_ordered_and_captures_into_a_graph(eng):
    """11. The input arrives by a device copy on the same stream directly in front of the enqueue, with no synchronize in between.  Then a warmed call is
    captured: a synchronize, an allocation or a blocking copy inside it would fail the capture in the global error mode.  Replayed twice over other inputs
    of the same offsets it gives their streams"""
    import torch
    sizes = [1000, 65025, 0, 130049]
    flags = WRAP_FLAGS["zlib"]
    inputs = [[cases.make(kind, n, seed + k) for k, n in enumerate(sizes)] for kind, seed in (("text", 50), ("runs", 60), ("rand", 70))]
    wants = [blocking(eng, x, 6, flags) for x in inputs]
    d = Dev(eng, [bytes(sum(sizes))], flags, in_offs=table(sizes), oo=[int(x) for x in eng.deflate_streams_layout(table(sizes), flags)[0]], batch_tiles=2)
    srcs = [torch.tensor(np.frombuffer(b"".join(x) + b"\0", dtype=np.uint8), device="cuda:0") for x in inputs]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d.d_in.copy_(srcs[0], non_blocking=True)
        d.enqueue(6, stream=s.cuda_stream)  # (also the warm-up: code objects load on first use)
    check_equal(d, *wants[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # (capture_error_mode "global", the default)
        d.enqueue(6, stream=torch.cuda.current_stream().cuda_stream)
    for which in (1, 2):
        d.d_in.copy_(srcs[which])
        d.d_buf.fill_(FILL)
        d.d_items.fill_(0xEE)
        d.d_sum.fill_(0xEE)  # (the summary asserted below is this replay's)
        torch.cuda.synchronize()
        g.replay()
        check_equal(d, *wants[which])


def test_layout_enqueue(eng):
    """12. the rooms' table made on the device: zgpu_deflate_streams_layout's for a good table, a room of 0 for a bad entry; the closed form bounds the total"""
    import torch
    for flags in WRAP_FLAGS.values():
        offs = table(SIZES)
        want, total = eng.deflate_streams_layout(offs, flags)
        d_io = dev_u64(offs)
        d_oo = torch.full((len(offs) + 8,), 0x5A5A, dtype=torch.int64, device="cuda:0")
        eng.deflate_streams_layout_enqueue(d_io.data_ptr(), len(SIZES), offs[-1], flags, d_oo.data_ptr())
        torch.cuda.synchronize()
        got = d_oo.cpu().numpy()
        assert [int(x) for x in got[: len(offs)].view(np.uint64)] == [int(x) for x in want] and (got[len(offs):] == 0x5A5A).all()
        assert total <= eng.deflate_streams_rooms_bound(len(SIZES), offs[-1], flags)
        assert eng.deflate_streams_rooms_bound(1, 300007, flags) == int(eng.deflate_streams_layout([0, 300007], flags)[1])
    bad = [0, 1000, 500, 70000, 90001, 90001]  # entry 1 runs backwards, entry 3 leaves in_bytes = 90000
    flags = WRAP_FLAGS["zlib"]
    d_io = dev_u64(bad)
    d_oo = torch.zeros(len(bad), dtype=torch.int64, device="cuda:0")
    eng.deflate_streams_layout_enqueue(d_io.data_ptr(), len(bad) - 1, 90000, flags, d_oo.data_ptr())
    torch.cuda.synchronize()
    got = [int(x) for x in d_oo.cpu().numpy().view(np.uint64)]
    bound = eng.L.zgpu_deflate_streams_bound
    rooms = [int(bound(1000, flags)), 0, int(bound(69500, flags)), 0, 0]
    assert got == table(rooms)
