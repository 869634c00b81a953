"""The stream-ordered batch deflate, zgpu_deflate_batch_enqueue / zgpu_deflate_batch_packed_enqueue: many items of at most 64 KiB compressed on the caller's
stream with a caller-owned workspace, nothing read back.  The truth is the reference's one-stream bytes (oracle.refzlib: compress2, or deflateInit2 +
Z_FINISH for raw and gzip) and, differentially, the blocking segment call: record k must equal the record zgpu_deflate_segments_items_host gives segment
k, field for field.  Device memory is held in torch tensors: the destination between two 64-byte guards of 0xA5, records and summary pre-filled with 0xEE,
256 spare bytes behind the workspace that must stay 0xEE.  Every call here is followed by a synchronize of the test's own."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cases, refzlib as R  # noqa: E402

OK, ERRNO, STREAM_ERROR, BUF_ERROR = 0, -1, -2, -5
FILL, GUARD, SPARE = 0xA5, 64, 256
REC = np.dtype([("code", "<i4"), ("data_type", "<u4"), ("out_lo", "<u8"), ("out_bytes", "<u8"), ("in_bytes", "<u4"), ("adler32", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])
F_FINAL, F_ZLIB, F_GZIP, F_CRC32, F_BGZF = 1, 2, 16, 32, 128
WRAP_FLAGS = {"raw": F_FINAL, "zlib": F_FINAL | F_ZLIB, "gzip": F_FINAL | F_GZIP, "bgzf": F_FINAL | F_BGZF}
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
SIZES = (0, 1, 2, 3, 100, 4096, 65535, 65536)
ITEMS = [cases.make(kind, n, 7 + i) for i, kind in enumerate(("text", "rand", "runs")) for n in SIZES]
FAILED = (STREAM_ERROR, 2, 0, 0, 1, 0)  # code, data_type, out_bytes, in_bytes, adler32, crc32 of an item the table check has failed


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.set_exact_sort(0)
    e.close()


_blocking = {}


def blocking(eng, items, level, flags):
    """the blocking segment call over the same items, computed once per (items, level, flags): (streams, records)"""
    key = (tuple((len(b), hash(b)) for b in items), level, flags)
    if key not in _blocking:
        _blocking[key] = eng.deflate_segments_host(items, level, flags=flags, want_items=True)
    return _blocking[key]


def table(sizes):
    return [0] + [int(x) for x in np.cumsum(sizes)]


def dev_u64(values):
    import torch
    return torch.tensor(np.array(values, dtype=np.uint64).view(np.int64), device="cuda:0")


class Dev:
    """One batch in device memory.  in_offs / in_bytes: a table of the caller's own over the blob; oo: the ranges entry's table (None: the packed entry)."""

    def __init__(self, eng, items, out_cap, oo=None, in_offs=None, in_bytes=None, batch_items=0, ws_short=0, ws_shift=0):
        import torch
        from zlib_amd import gpu
        self.eng, self.packed, self.batch_items = eng, oo is None, batch_items
        offs = table([len(b) for b in items]) if in_offs is None else list(in_offs)
        self.n = len(offs) - 1
        blob = np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8)
        self.in_bytes = len(blob) - 1 if in_bytes is None else in_bytes
        self.d_in = torch.tensor(blob, device="cuda:0")
        self.d_io = dev_u64(offs)
        self.d_items = torch.full((max(self.n, 1) * REC.itemsize,), 0xEE, dtype=torch.uint8, device="cuda:0")
        self.d_sum = torch.full((C.sizeof(gpu.DeflateBatchSummary),), 0xEE, dtype=torch.uint8, device="cuda:0")
        need = eng.deflate_batch_workspace_bytes(self.n, batch_items)
        self.ws_bytes = need - ws_short
        self.d_ws = torch.full((need + ws_shift + SPARE,), 0xEE, dtype=torch.uint8, device="cuda:0")
        assert self.d_ws.data_ptr() % 256 == 0
        self.ws_ptr, self.ws_shift = self.d_ws.data_ptr() + ws_shift, ws_shift
        self.out_cap = out_cap
        self.d_buf = torch.full((out_cap + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        self.d_out = self.d_buf.data_ptr() + GUARD
        self.d_oo = dev_u64(oo) if oo is not None else torch.full((self.n + 1,), 0xDEAD, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()

    def enqueue(self, level, flags, stream=None, strategy=0, prime=0, d_items="own"):
        fn = self.eng.deflate_batch_packed_enqueue if self.packed else self.eng.deflate_batch_enqueue
        fn(self.d_in.data_ptr(), self.in_bytes, self.d_io.data_ptr(), self.n, level, self.d_out, self.out_cap, self.d_oo.data_ptr(),
           self.d_items.data_ptr() if d_items == "own" else d_items, self.ws_ptr, self.ws_bytes, flags=flags, strategy=strategy, batch_items=self.batch_items,
           d_summary=self.d_sum.data_ptr(), stream=stream, prime=prime)

    def results(self):
        """after a synchronize: records as (code, data_type, out_lo, out_bytes, in_bytes, adler32, crc32), the summary as (nfailed, nbad_offsets, ntoo_long,
        total, overflow, sort_fault), the destination without its guards (which are checked here, as the spare bytes behind the workspace are), the offsets"""
        import torch
        torch.cuda.synchronize()
        arr = np.frombuffer(self.d_items.cpu().numpy().tobytes(), dtype=REC, count=self.n)
        recs = [tuple(int(r[f]) for f in ("code", "data_type", "out_lo", "out_bytes", "in_bytes", "adler32", "crc32")) for r in arr]
        summary = struct.unpack("<QQQQII", self.d_sum.cpu().numpy().tobytes())
        buf = self.d_buf.cpu().numpy()
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + self.out_cap:] == FILL).all(), "a byte outside the destination was written"
        assert (self.d_ws[self.ws_shift + self.ws_bytes:].cpu().numpy() == 0xEE).all(), "a byte behind the workspace was written"
        return recs, summary, buf[GUARD: GUARD + self.out_cap], [int(x) for x in self.d_oo.cpu().numpy().view(np.uint64)]

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.d_buf == FILL).all()) and bool((self.d_items == 0xEE).all()) and bool((self.d_sum == 0xEE).all()) and bool((self.d_ws == 0xEE).all())


def want_records(brecs, out_lo=None):
    """the blocking call's records (out_lo, out_bytes, in_bytes, data_type, adler32, crc32) in the enqueue's order of fields"""
    return [(OK, dt, lo if out_lo is None else out_lo[k], nb, ib, a, c) for k, (lo, nb, ib, dt, a, c) in enumerate(brecs)]


def run_both(eng, items, level, flags, batch_items=0, slack=3):
    """the packed entry, then the ranges entry with `slack` spare bytes a range: both must give the blocking call's streams and records.  Returns the streams"""
    segs, brecs = blocking(eng, items, level, flags)
    total = sum(len(s) for s in segs)
    d = Dev(eng, items, total, batch_items=batch_items)
    d.enqueue(level, flags)
    recs, summary, out, oo = d.results()
    assert summary == (0, 0, 0, total, 0, 0)
    assert oo == table([len(s) for s in segs])
    assert recs == want_records(brecs)
    assert out.tobytes() == b"".join(segs)
    rooms = table([len(s) + slack for s in segs])
    d = Dev(eng, items, rooms[-1], oo=rooms, batch_items=batch_items)
    d.enqueue(level, flags)
    recs, summary, out, oo = d.results()
    assert summary == (0, 0, 0, 0, 0, 0) and oo == rooms  # (the table is the caller's: read, never written)
    assert recs == want_records(brecs, rooms)
    for k, s in enumerate(segs):
        assert out[rooms[k]: rooms[k] + len(s)].tobytes() == s, k
        assert (out[rooms[k] + len(s): rooms[k + 1]] == FILL).all(), k
    return segs


@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
@pytest.mark.parametrize("level", [1, 4, 6, 9])
def test_catalogue_equals_the_blocking_call(eng, level, wrap):
    segs = run_both(eng, ITEMS, level, WRAP_FLAGS[wrap])
    empty = blocking(eng, ITEMS, level, WRAP_FLAGS[wrap])[1][0]
    assert empty[2] == 0 and empty[3] == 2  # the empty item: in_bytes 0, data_type Z_UNKNOWN
    assert len(segs) == len(ITEMS)


@pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref) is not here")
@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
@pytest.mark.parametrize("level", [1, 4, 6, 9])
def test_catalogue_equals_the_reference(eng, level, wrap):
    want = [R.compress2(d, level) if wrap == "zlib" else R.deflate_wbits(d, level, WBITS[wrap]) for d in ITEMS]
    total = sum(len(z) for z in want)
    d = Dev(eng, ITEMS, total)
    d.enqueue(level, WRAP_FLAGS[wrap])
    recs, summary, out, oo = d.results()
    assert summary == (0, 0, 0, total, 0, 0)
    bad = [k for k, z in enumerate(want) if out[oo[k]: oo[k + 1]].tobytes() != z]
    assert not bad, bad
    assert [(r[0], r[4]) for r in recs] == [(OK, len(x)) for x in ITEMS]
    # ... and the ranges entry: the same streams, each at the head of a room with five bytes to spare
    rooms = table([len(z) + 5 for z in want])
    d = Dev(eng, ITEMS, rooms[-1], oo=rooms)
    d.enqueue(level, WRAP_FLAGS[wrap])
    recs, summary, out, _ = d.results()
    assert summary == (0, 0, 0, 0, 0, 0)
    bad = [k for k, z in enumerate(want) if out[rooms[k]: rooms[k] + len(z)].tobytes() != z or recs[k][:4] != (OK, recs[k][1], rooms[k], len(z))]
    assert not bad, bad


def test_crc32_flag_and_strategies(eng):
    items = ITEMS[4:7] + ITEMS[12:15]
    run_both(eng, items, 6, F_FINAL | F_CRC32)
    for strategy in (1, 4):  # Z_FILTERED, Z_FIXED
        segs, brecs = eng.deflate_segments_host(items, 6, flags=F_FINAL | F_ZLIB, want_items=True, strategy=strategy)
        d = Dev(eng, items, sum(len(s) for s in segs))
        d.enqueue(6, F_FINAL | F_ZLIB, strategy=strategy)
        recs, summary, out, _ = d.results()
        assert recs == want_records(brecs) and out.tobytes() == b"".join(segs) and summary[0] == 0, strategy


def test_bgzf_blocks(eng):
    blocks = [cases.make("text", 1, 3), cases.make("text", 65280, 4)]
    segs, brecs = eng.deflate_segments_host(blocks, 6, flags=WRAP_FLAGS["bgzf"], want_items=True)
    over = cases.make("text", 65281, 5)
    items = blocks + [over]
    total = sum(len(s) for s in segs)
    for oo in (None, table([len(s) for s in segs] + [70000])):
        d = Dev(eng, items, total if oo is None else oo[-1], oo=oo)
        d.enqueue(6, WRAP_FLAGS["bgzf"])
        recs, summary, out, offs = d.results()
        assert summary == (1, 0, 1, total if oo is None else 0, 0, 0)
        assert recs[:2] == want_records(brecs) and recs[2][:2] + recs[2][3:] == FAILED
        assert out[:total].tobytes() == b"".join(segs)
        for k, s in enumerate(segs):  # BSIZE: the block's length - 1
            assert struct.unpack_from("<H", s, 16)[0] == len(s) - 1
        if oo is None:
            assert offs == table([len(s) for s in segs] + [0])
        else:
            assert (out[total:] == FILL).all()


def test_ranges_room(eng):
    items = [cases.make("text", 3000, 1), cases.make("rand", 500, 2), cases.make("runs", 9000, 3), cases.make("text", 100, 4), cases.make("text", 700, 5)]
    flags = WRAP_FLAGS["zlib"]
    segs, brecs = blocking(eng, items, 6, flags)
    L = [len(s) for s in segs]
    # item 0: room exact; item 1: one byte short; item 2: room 0; item 3: enough; item 4: a range that leaves out_cap
    rooms = [L[0], L[1] - 1, 0, L[3] + 5, L[4]]
    oo = table(rooms)
    cap = oo[-1] - 1
    d = Dev(eng, items, cap, oo=oo)
    d.enqueue(6, flags)
    recs, summary, out, _ = d.results()
    want = want_records(brecs, oo)
    assert recs[0] == want[0] and recs[3] == want[3]
    assert recs[1] == (BUF_ERROR,) + want[1][1:] and recs[2] == (BUF_ERROR,) + want[2][1:]  # out_bytes: the size needed
    assert recs[4][:2] + recs[4][3:] == FAILED
    assert summary == (3, 1, 0, 0, 0, 0)
    assert out[oo[0]: oo[1]].tobytes() == segs[0] and out[oo[3]: oo[3] + L[3]].tobytes() == segs[3]
    assert (out[oo[1]: oo[3]] == FILL).all() and (out[oo[3] + L[3]:] == FILL).all()
    # the neighbours are what they are with room enough
    full = table([n + 2 for n in L])
    d2 = Dev(eng, items, full[-1], oo=full)
    d2.enqueue(6, flags)
    recs2, summary2, out2, _ = d2.results()
    assert summary2[0] == 0 and recs2 == want_records(brecs, full)
    for k in (0, 3):
        assert out2[full[k]: full[k] + L[k]].tobytes() == out[oo[k]: oo[k] + L[k]].tobytes()


@pytest.mark.parametrize("packed", [True, False])
def test_bad_tables_fail_their_item_alone(eng, packed):
    blob = cases.make("text", 70000, 9)
    flags = WRAP_FLAGS["gzip"]

    def served(lo, hi):
        segs, brecs = eng.deflate_segments_host([blob[lo:hi]], 6, flags=flags, want_items=True)
        return segs[0], brecs[0]

    tables = {
        "backwards": ([0, 100, 50, 200], None, (1, 0)),       # item 1 runs backwards; items 0 and 2 are good, and they overlap
        "beyond": ([0, 300, 70001], None, (1, 0)),            # an entry beyond in_bytes
        "too long": ([0, 65537, 65600], None, (0, 1)),        # an item of 65537 bytes
        "beyond in_bytes argument": ([0, 300, 600], 500, (1, 0)),
    }
    for name, (io, in_bytes, (nbad, nlong)) in tables.items():
        n = len(io) - 1
        limit = 70000 if in_bytes is None else in_bytes
        good = [k for k in range(n) if io[k] <= io[k + 1] <= limit and io[k + 1] - io[k] <= 65536]
        assert len(good) == n - nbad - nlong, name
        want = {k: served(io[k], io[k + 1]) for k in good}
        sizes = [len(want[k][0]) if k in want else 0 for k in range(n)]
        oo = None if packed else table([s + 4 for s in sizes])
        d = Dev(eng, [blob], sum(sizes) if packed else oo[-1], oo=oo, in_offs=io, in_bytes=in_bytes)
        d.enqueue(6, flags)
        recs, summary, out, offs = d.results()
        assert summary == (nbad + nlong, nbad, nlong, sum(sizes) if packed else 0, 0, 0), name
        if packed:
            assert offs == table(sizes), name  # a failed item has an empty range, the others lie back to back
        for k in range(n):
            if k in want:
                z, (lo, nb, ib, dt, a, c) = want[k]
                assert recs[k] == (OK, dt, offs[k], nb, ib, a, c), (name, k)
                assert out[offs[k]: offs[k] + len(z)].tobytes() == z, (name, k)
            else:
                assert recs[k][:2] + recs[k][3:] == FAILED, (name, k)
                if packed:
                    assert recs[k][2] == offs[k]
                else:
                    assert (out[offs[k]: offs[k + 1]] == FILL).all(), (name, k)


def test_no_items_and_one_item(eng):
    for oo in (None, [0]):
        d = Dev(eng, [], 16, oo=oo)
        d.enqueue(6, WRAP_FLAGS["zlib"])
        _, summary, out, _ = d.results()
        assert summary == (0, 0, 0, 0, 0, 0) and (out == FILL).all()  # at most the summary is written
        assert bool((d.d_items == 0xEE).all()) and bool((d.d_ws == 0xEE).all())
    run_both(eng, [ITEMS[5]], 6, WRAP_FLAGS["zlib"])


def test_rounds_carry_the_total(eng):
    items = [cases.make(("text", "rand", "runs")[k % 3], 500 + 3777 * k, 20 + k) for k in range(10)]
    for wrap in ("raw", "gzip"):
        a = run_both(eng, items, 6, WRAP_FLAGS[wrap], batch_items=4)  # three rounds: 4 + 4 + 2
        b = run_both(eng, items, 6, WRAP_FLAGS[wrap], batch_items=16)
        assert a == b


@pytest.mark.parametrize("packed", [True, False])
def test_failed_items_in_later_rounds(eng, packed):
    """n = 10 in rounds of 4: item 5 (second round) runs backwards, item 9 (third round) is too long; items 4 and 6 overlap.  The layout of a round, the
    carried total and the records' indices must all skip the failed items of the rounds behind the first."""
    blob = cases.make("text", 100000, 13)
    flags = WRAP_FLAGS["gzip"]
    io = [0, 1000, 3000, 6000, 10000, 15000, 12000, 20000, 27000, 27100, 95000]
    good = [k for k in range(10) if k not in (5, 9)]
    want = {}
    for k in good:
        segs, brecs = eng.deflate_segments_host([blob[io[k]: io[k + 1]]], 6, flags=flags, want_items=True)
        want[k] = (segs[0], brecs[0])
    sizes = [len(want[k][0]) if k in want else 0 for k in range(10)]
    oo = None if packed else table([s + 7 for s in sizes])
    d = Dev(eng, [blob], sum(sizes) if packed else oo[-1], oo=oo, in_offs=io, batch_items=4)
    d.enqueue(6, flags)
    recs, summary, out, offs = d.results()
    assert summary == (2, 1, 1, sum(sizes) if packed else 0, 0, 0)
    if packed:
        assert offs == table(sizes)
    for k in range(10):
        if k in want:
            z, (lo, nb, ib, dt, a, c) = want[k]
            assert recs[k] == (OK, dt, offs[k], nb, ib, a, c), k
            assert out[offs[k]: offs[k] + len(z)].tobytes() == z, k
        else:
            assert recs[k][:2] + recs[k][3:] == FAILED, k
            if not packed:
                assert (out[offs[k]: offs[k + 1]] == FILL).all(), k


def test_packed_overflow(eng):
    items = [cases.make("text", 2000 + 500 * k, 30 + k) for k in range(6)]
    flags = WRAP_FLAGS["zlib"]
    segs, brecs = blocking(eng, items, 6, flags)
    offs = table([len(s) for s in segs])
    cap = offs[3] + len(segs[3]) // 2  # out_cap in the middle of item 3
    d = Dev(eng, items, cap)
    d.enqueue(6, flags)
    recs, summary, out, oo = d.results()
    want = want_records(brecs)
    assert summary == (3, 0, 0, offs[-1], 1, 0) and oo == offs
    assert recs[:3] == want[:3] and recs[3:] == [(BUF_ERROR,) + w[1:] for w in want[3:]]
    assert out[: offs[3]].tobytes() == b"".join(segs[:3]) and (out[offs[3]:] == FILL).all()


def test_arguments_the_host_judges(eng):
    items = ITEMS[4:7]
    flags = WRAP_FLAGS["zlib"]
    from zlib_amd.gpu import EngineError

    def refused(d, level=6, flags=flags, **kw):
        with pytest.raises(EngineError) as err:
            d.enqueue(level, flags, **kw)
        assert err.value.code == STREAM_ERROR
        assert d.untouched()

    refused(Dev(eng, items, 70000, ws_short=1))
    refused(Dev(eng, items, 70000, ws_shift=128))
    refused(Dev(eng, items, 70000, oo=[0, 100, 200, 70000], ws_short=1))
    refused(Dev(eng, items, 70000), d_items=None)
    refused(Dev(eng, items, 70000), strategy=3)           # Z_RLE
    refused(Dev(eng, items, 70000), strategy=2)           # Z_HUFFMAN_ONLY
    refused(Dev(eng, items, 70000), flags=F_ZLIB)         # ZGPU_F_FINAL missing
    refused(Dev(eng, items, 70000), flags=F_FINAL, prime=(3 << 16) | 5)
    refused(Dev(eng, items, 70000), flags=F_FINAL | 8)    # ZGPU_F_POS0_ALL
    assert eng.deflate_batch_workspace_bytes(2 ** 32) == 0


def test_sort_self_check(eng):
    """zgpu_debug_inject_sort_fault() sets a flag: the next launch of the fast sort is followed by a memset that raises the fault word (nothing faults)."""
    items = ITEMS[4:7]
    flags = WRAP_FLAGS["zlib"]
    segs, brecs = blocking(eng, items, 6, flags)
    total = sum(len(s) for s in segs)
    try:
        assert eng.L.zgpu_debug_sort_fallback(eng.h) == 0
        eng.L.zgpu_debug_inject_sort_fault.restype = None
        eng.L.zgpu_debug_inject_sort_fault()
        d = Dev(eng, items, total)
        d.enqueue(6, flags)
        recs, summary, _, _ = d.results()
        assert summary[0] == 3 and summary[5] == 1
        assert [r[0] for r in recs] == [ERRNO] * 3
        assert eng.L.zgpu_debug_sort_fallback(eng.h) == 0  # the host cannot do it for the caller
        eng.set_exact_sort(1)
        assert eng.L.zgpu_debug_sort_fallback(eng.h) != 0
        d = Dev(eng, items, total)
        d.enqueue(6, flags)
        recs, summary, out, _ = d.results()
        assert summary == (0, 0, 0, total, 0, 0) and recs == want_records(brecs) and out.tobytes() == b"".join(segs)
    finally:
        eng.set_exact_sort(0)
    assert eng.L.zgpu_debug_sort_fallback(eng.h) == 0


def test_two_calls_in_flight(eng):
    import torch
    flags = WRAP_FLAGS["gzip"]
    batches = []
    for seed in (1, 2):
        items = [cases.make(("text", "runs")[seed - 1], 3000 + 7000 * k, 10 * seed + k) for k in range(8)]
        segs, brecs = eng.deflate_segments_host(items, 6, flags=flags, want_items=True)
        batches.append((segs, brecs, Dev(eng, items, sum(len(s) for s in segs)), torch.cuda.Stream()))
    for segs, brecs, d, s in batches:
        d.enqueue(6, flags, stream=s.cuda_stream)
    for segs, brecs, d, s in batches:
        s.synchronize()
    for segs, brecs, d, s in batches:
        recs, summary, out, _ = d.results()
        assert summary[0] == 0 and recs == want_records(brecs) and out.tobytes() == b"".join(segs)


def test_call_is_stream_ordered_and_captures_into_a_graph(eng):
    """The input arrives by a device copy on the same stream directly in front of the enqueue, with no synchronize in between.  Then a warmed call is
    captured: a synchronize, an allocation or a blocking copy inside it would fail the capture in the global error mode.  The captured work reads its
    buffers when it runs: replayed over other inputs of the same offsets it gives their streams."""
    import torch
    sizes = [1000, 40000, 65536]
    flags = WRAP_FLAGS["zlib"]
    inputs = [[cases.make(kind, n, seed + k) for k, n in enumerate(sizes)] for kind, seed in (("text", 50), ("runs", 60), ("rand", 70))]
    wants = [eng.deflate_segments_host(x, 6, flags=flags, want_items=True) for x in inputs]
    rooms = table([n + 100 for n in sizes])
    d = Dev(eng, [bytes(sum(sizes))], rooms[-1], oo=rooms, in_offs=table(sizes))
    srcs = [torch.tensor(np.frombuffer(b"".join(x) + b"\0", dtype=np.uint8), device="cuda:0") for x in inputs]
    torch.cuda.synchronize()

    def check(which):
        segs, brecs = wants[which]
        recs, summary, out, _ = d.results()
        print("input", which, "summary", summary, "records", recs)  # (shown when the test fails)
        assert summary == (0, 0, 0, 0, 0, 0) and recs == want_records(brecs, rooms), which
        for k, s in enumerate(segs):
            assert out[rooms[k]: rooms[k] + len(s)].tobytes() == s, (which, k)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d.d_in.copy_(srcs[0], non_blocking=True)
        d.enqueue(6, flags, stream=s.cuda_stream)  # (also the warm-up: code objects load on first use)
    check(0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # (capture_error_mode "global", the default)
        d.enqueue(6, flags, stream=torch.cuda.current_stream().cuda_stream)
    for which in (1, 2):
        d.d_in.copy_(srcs[which])
        d.d_buf.fill_(FILL)
        d.d_items.fill_(0xEE)
        d.d_sum.fill_(0xEE)  # (the summary asserted below is this replay's)
        torch.cuda.synchronize()
        g.replay()
        check(which)
