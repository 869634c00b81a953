"""Batch compress of items of any length, zgpu_deflate_streams_device / zgpu_deflate_streams_host: many continuous streams whose tiles share the launches.
Item k must be, byte for byte, what the reference's one-call stream gives for that item alone (oracle.refzlib: compress2 for a zlib wrapper,
deflateInit2 + Z_FINISH for gzip and raw), whatever its neighbours are and wherever the batches of tiles end; the block catalogue of
oracle/blockcases.py owes the bytes of tests/golden/block_kat.json when its rows are the items of one call.  Device memory is held in torch tensors:
the destination pre-filled with a pattern between two guards.  The sizes sit on the tile geometry: 65024 (one tile's range), 97536 (= 65024 + 32512, two
tiles), 98048 (+ 512, the slack), 130048 (three tiles)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import blockcases as BC, cases, refzlib as R  # noqa: E402

OK, STREAM_ERROR, BUF_ERROR = 0, -2, -5
F_FINAL, F_ZLIB, F_GZIP, F_CRC32 = 1, 2, 16, 32
WRAP_FLAGS = {"raw": F_FINAL, "zlib": F_FINAL | F_ZLIB, "gzip": F_FINAL | F_GZIP}
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
WRAP_OF = {-15: "raw", 15: "zlib", 31: "gzip"}
REC = np.dtype([("code", "<i4"), ("data_type", "<u4"), ("out_lo", "<u8"), ("out_bytes", "<u8"), ("in_bytes", "<u4"), ("adler32", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])
FILL, GUARD = 0xA5, 64
SIZES = (0, 1, 2, 3, 65023, 65024, 65025, 65535, 65536, 65537, 97535, 97536, 97537, 98047, 98048, 98049, 130047, 130048, 130049, 200000, 300007)
KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "block_kat.json")))["cases"]
needs_ref = pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref) is not here")


def _items():
    out = [cases.make("mix", n, 100 + i) for i, n in enumerate(SIZES)]
    out += [cases.make(kind, 150000, 31 + i) for i, kind in enumerate(cases.KINDS)]
    out.append(np.random.RandomState(5).randint(0, 256, 100000, dtype=np.uint8).tobytes())  # stored blocks of 65,535 bytes and the veto
    out.append(bytes(400000))                                                                # blocks that span many tiles, matches of 258, the NIL position
    return out


ITEMS = _items()
PARAMS = [(lv, w, 0) for lv in (4, 6, 9) for w in ("raw", "zlib", "gzip")] + [(6, "raw", s) for s in (1, 2, 3, 4)]


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


_want = {}


def want(level, wrap, strategy):
    """the reference's streams of ITEMS and what zlib says of each item (adler32, crc32), made once per parameter set"""
    key = (level, wrap, strategy)
    if key not in _want:
        _want[key] = [R.compress2(d, level) if (wrap == "zlib" and strategy == 0) else R.deflate_wbits(d, level, WBITS[wrap], strategy) for d in ITEMS]
    return _want[key]


_got = {}


def got(eng, level, wrap, strategy):
    """the product's call over ITEMS with every knob at its default, made once per parameter set: (streams, records, result)"""
    key = (level, wrap, strategy)
    if key not in _got:
        z, recs = eng.deflate_streams_host(ITEMS, level, wrap=wrap, strategy=strategy, flags=F_CRC32, want_items=True)
        _got[key] = (z, recs, (eng.last.out_bytes, eng.last.nchunks, eng.last.reserved, eng.last.adler32, eng.last.crc32))
    return _got[key]


def ntiles(n):
    return 0 if n == 0 else 1 if n <= 65024 else -(-(n - 65024) // 32512) + 1


@needs_ref
@pytest.mark.parametrize("level,wrap,strategy", PARAMS, ids=lambda v: str(v))
def test_items_are_the_references_streams(eng, level, wrap, strategy):
    """1. one call per parameter set: every item's bytes, its record, and the stream back through the product's batch inflate"""
    z, recs, res = got(eng, level, wrap, strategy)
    ref = want(level, wrap, strategy)
    bad = [(k, len(d), len(a), len(b)) for k, (d, a, b) in enumerate(zip(ITEMS, z, ref)) if a != b]
    assert not bad, "(item, bytes, got, want) %s" % bad[:10]
    at = 0
    for k, (d, r) in enumerate(zip(ITEMS, recs)):
        assert (r.code, r.out_lo, r.out_bytes, r.in_bytes, r.adler32, r.crc32) == (OK, at, len(ref[k]), len(d), R.adler32(d), R.crc32(d)), k
        at += len(ref[k])
    assert res == (at, sum(ntiles(len(d)) for d in ITEMS), 0, R.adler32(ITEMS[-1]), R.crc32(ITEMS[-1]))
    back = eng.inflate_batch_host(z, [len(d) + 8 for d in ITEMS], wrap=wrap)
    for k, (d, b) in enumerate(zip(ITEMS, back)):
        assert b[0] == 0 and b[2] == d, (k, b[0], b[1])


def test_items_are_the_one_call_streams(eng):
    """1. (no reference needed; data_type) every item equals the product's own one-call continuous stream of that item -- which the existing suites pin to the
    reference -- and the record's data_type is that call's strm->data_type: Z_TEXT / Z_BINARY from the first block, Z_UNKNOWN for the empty item"""
    from zlib_amd import gpu
    z, recs, res = got(eng, 6, "zlib", 0)
    for k, (d, r) in enumerate(zip(ITEMS, recs)):
        one = eng.deflate_host(d, 6, flags=gpu.F_FINAL | gpu.F_CONTINUOUS | gpu.F_ZLIB_WRAP)
        assert one == z[k], (k, len(d))
        assert (r.data_type, r.adler32) == (eng.last.data_type, eng.last.adler32), (k, len(d))
    assert recs[0].data_type == 2 and {r.data_type for r in recs} == {0, 1, 2}


def test_streams_inflate_with_zlib(eng):
    """(no reference needed) every stream of the level-6 calls is a valid stream of its item"""
    import zlib
    for wrap in ("raw", "zlib", "gzip"):
        z, recs, res = got(eng, 6, wrap, 0)
        for k, (d, s) in enumerate(zip(ITEMS, z)):
            assert zlib.decompress(s, WBITS[wrap]) == d, (wrap, k)


def test_neighbours_do_not_matter(eng):
    """2. the same items reversed, and with an empty item between every two: the same bytes per item"""
    z, _, _ = got(eng, 6, "zlib", 0)
    rev = eng.deflate_streams_host(ITEMS[::-1], 6, wrap="zlib")
    assert rev[::-1] == z
    spaced = []
    for d in ITEMS:
        spaced += [d, b""]
    sp = eng.deflate_streams_host(spaced, 6, wrap="zlib")
    assert sp[0::2] == z and all(s == sp[1] for s in sp[1::2]) and len(sp[1]) == 8


@pytest.mark.parametrize("tiles", ["1", "3", None])
def test_batch_ends_inside_streams(eng, monkeypatch, tiles):
    """3. ZGPU_CONT_BATCH_TILES = 1, 3, unset: batches that end inside streams give the same bytes"""
    z, _, _ = got(eng, 6, "raw", 0)  # (made with the knob unset: got() is first called from a test without it, or here before it is set)
    if tiles is None:
        monkeypatch.delenv("ZGPU_CONT_BATCH_TILES", raising=False)
    else:
        monkeypatch.setenv("ZGPU_CONT_BATCH_TILES", tiles)
    again, recs = eng.deflate_streams_host(ITEMS, 6, wrap="raw", want_items=True)
    assert again == z
    assert all(r.code == OK for r in recs)
    if R.available():
        assert z == want(6, "raw", 0)


@pytest.mark.parametrize("tiles", [None, "259", "260"])
def test_a_part_longer_than_the_scans_lanes(eng, monkeypatch, tiles):
    """3b. an item of 301 tiles and some 370 blocks among short ones (tests/streams_long_fixtures.py): the batched scans' 256 lanes take runs of tiles and
    of blocks.  One batch (a part of 301 tiles), batches of 259 (the long item's first part: 256 tiles) and of 260 (257).  Every item is the product's
    one-call continuous stream of that item, every record ZGPU_OK with zlib's adler32, and zlib gives the item back"""
    import streams_long_fixtures as LF
    LF.one_call_streams(eng)  # (made with the knob unset or not: the one-stream path does not read the streams' parts)
    if tiles is None:
        monkeypatch.delenv("ZGPU_CONT_BATCH_TILES", raising=False)
    else:
        monkeypatch.setenv("ZGPU_CONT_BATCH_TILES", tiles)
    z, recs = eng.deflate_streams_host(list(LF.items()), 6, wrap="zlib", want_items=True)
    assert eng.last.nchunks == 307
    LF.check(z, [(r.code, r.adler32) for r in recs])


def catalogue_rows():
    return [c for c in BC.catalogue() if not c.calls and c.level >= 4]


@pytest.mark.parametrize("tiles", [None, "1"])
def test_block_catalogue_as_one_batch(eng, monkeypatch, tiles):
    """4. every row of the block catalogue that is one Z_FINISH call at a level of 4 or more, grouped by (level, strategy, wbits), one call per group: every
    item owes (len, sha) of tests/golden/block_kat.json"""
    if tiles is None:
        monkeypatch.delenv("ZGPU_CONT_BATCH_TILES", raising=False)
    else:
        monkeypatch.setenv("ZGPU_CONT_BATCH_TILES", tiles)
    rows = catalogue_rows()
    assert {c.family for c in rows} == {"phase", "full", "edge", "many"}
    groups = {}
    for c in rows:
        groups.setdefault((c.level, c.strategy, c.wbits), []).append(c)
    bad = []
    for (level, strategy, wbits), cs in sorted(groups.items()):
        z = eng.deflate_streams_host([c.data for c in cs], level, wrap=WRAP_OF[wbits], strategy=strategy)
        for c, s in zip(cs, z):
            if (len(s), hashlib.sha256(s).hexdigest()[:16]) != (KAT[c.name]["len"], KAT[c.name]["sha"]):
                bad.append("%s: %d bytes, owed %d" % (c.name, len(s), KAT[c.name]["len"]))
    assert not bad, "%d of %d rows\n" % (len(bad), len(rows)) + "\n".join(bad[:40])


class Dev:
    """One call of the device entry in device memory: the destination pre-filled with FILL between two guards"""

    def __init__(self, items, flags, rooms=None):
        import torch
        self.n = len(items)
        offs = [0] + [int(x) for x in np.cumsum([len(b) for b in items])]
        self.in_bytes = offs[-1]
        self.d_in = torch.tensor(np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8), device="cuda:0")
        self.d_io = torch.tensor(np.array(offs, dtype=np.uint64).view(np.int64), device="cuda:0")
        self.oo = rooms
        self.out_cap = rooms[-1]
        self.d_oo = torch.tensor(np.array(rooms, dtype=np.uint64).view(np.int64), device="cuda:0")
        self.d_buf = torch.full((self.out_cap + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        assert self.d_buf.data_ptr() % 4 == 0
        self.d_out = self.d_buf.data_ptr() + GUARD
        self.d_items = torch.full((max(self.n, 1) * REC.itemsize,), 0xEE, dtype=torch.uint8, device="cuda:0")
        self.flags = flags
        torch.cuda.synchronize()

    def call(self, eng, level, strategy=0, flags=None, lz_impl=0):
        return eng.deflate_streams_device(self.d_in.data_ptr(), self.in_bytes, self.d_io.data_ptr(), self.n, level, self.d_out, self.out_cap, self.d_oo.data_ptr(),
                                          self.d_items.data_ptr(), flags=self.flags if flags is None else flags, strategy=strategy, lz_impl=lz_impl)

    def results(self):
        import torch
        torch.cuda.synchronize()
        recs = np.frombuffer(self.d_items.cpu().numpy().tobytes(), dtype=REC, count=self.n)
        buf = self.d_buf.cpu().numpy()
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + self.out_cap:] == FILL).all(), "a byte outside the destination was written"
        return recs, buf[GUARD: GUARD + self.out_cap]

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.d_buf == FILL).all()) and bool((self.d_items == 0xEE).all())


SMALL = [ITEMS[k] for k in (5, 9, 12, 1, 0, 18)]  # 65024, 65537, 97537, 1, 0, 130049 bytes


@pytest.mark.parametrize("room", [8, 64])
def test_a_room_too_small_fails_its_item_alone(eng, room):
    """5. one item in the middle gets 8 bytes of room (less than the smallest stream needs) or 64 (a header and a few words of the first block fit): its record is
    ZGPU_BUF_ERROR, all others are exact, nothing is written outside a room"""
    flags = WRAP_FLAGS["zlib"]
    oo, total = eng.deflate_streams_layout([0] + list(np.cumsum([len(d) for d in SMALL])), flags)
    oo = [int(x) for x in oo]
    assert all(x % 4 == 0 for x in oo) and total == oo[-1]
    full = Dev(SMALL, flags, oo + [oo[-1] + 256])  # (one more entry than the call reads: 256 bytes behind oo[n] that belong to no room)
    res = full.call(eng, 6)
    recs, out = full.results()
    whole = [bytes(out[oo[k]: oo[k] + int(recs[k]["out_bytes"])]) for k in range(len(SMALL))]
    assert res.reserved == 0 and all(int(r["code"]) == OK for r in recs)
    assert (out[oo[-1]:] == FILL).all(), "the pattern behind oo[n] is gone"
    short = 2
    rooms = oo[: short + 1] + [x - (oo[short + 1] - oo[short]) + room for x in oo[short + 1:]]
    d = Dev(SMALL, flags, rooms + [rooms[-1] + 256])
    res = d.call(eng, 6)
    recs, out = d.results()
    assert res.reserved == 1
    for k in range(len(SMALL)):
        if k == short:
            assert (int(recs[k]["code"]), int(recs[k]["out_bytes"])) == (BUF_ERROR, 0)
        else:
            assert int(recs[k]["code"]) == OK and int(recs[k]["out_lo"]) == rooms[k]
            assert bytes(out[rooms[k]: rooms[k] + int(recs[k]["out_bytes"])]) == whole[k], k
    if room == 8:
        assert (out[rooms[short]: rooms[short + 1]] == FILL).all(), "a room too small for the smallest stream is left alone"
    assert (out[rooms[-1]:] == FILL).all(), "the pattern behind oo[n] is gone"
    if R.available():
        assert whole == [R.compress2(x, 6) for x in SMALL]


def test_refusals_touch_nothing(eng):
    """6. level 1, level 0, a set geometry, both wrappers (and what else the call names): ZGPU_STREAM_ERROR, the output untouched"""
    from zlib_amd import gpu
    flags = WRAP_FLAGS["raw"]
    oo, total = eng.deflate_streams_layout([0] + list(np.cumsum([len(d) for d in SMALL])), F_FINAL | F_GZIP)
    d = Dev(SMALL, flags, [int(x) for x in oo])

    def refused(**kw):
        level = kw.pop("level", 6)
        with pytest.raises(gpu.EngineError) as ei:
            d.call(eng, level, **kw)
        assert ei.value.code == STREAM_ERROR, kw
        assert d.untouched(), kw

    refused(level=1)
    refused(level=3)
    refused(level=0)
    refused(flags=F_FINAL | F_ZLIB | F_GZIP)
    refused(flags=0)                      # no FINAL
    refused(flags=F_FINAL | 64)           # CONTINUOUS
    refused(flags=F_FINAL | 128)          # BGZF_WRAP
    refused(flags=F_FINAL | 4)            # POS0
    refused(lz_impl=gpu.LZ_WALK)
    refused(strategy=5)
    eng.set_geometry(14, 8)
    try:
        refused()
    finally:
        eng.set_geometry(15, 8)
    # tables: a room that is no multiple of 4, a table that leaves the destination
    import torch
    good = d.d_oo.clone()
    bad = [int(x) for x in oo]
    bad[2] += 2
    d.d_oo = torch.tensor(np.array(bad, dtype=np.uint64).view(np.int64), device="cuda:0")
    refused()
    d.d_oo = good
    d.out_cap -= 4
    refused()
    d.out_cap += 4
    d.call(eng, 6)  # and the same object, unchanged, is served
    recs, out = d.results()
    assert all(int(r["code"]) == OK for r in recs)


def _batch_args(datas, caps):
    n = len(datas)
    src = [C.create_string_buffer(x, max(len(x), 1)) for x in datas]
    dst = [C.create_string_buffer(max(c, 1)) for c in caps]
    A = C.c_void_p * n
    return src, dst, A(*[C.addressof(x) for x in dst]), (C.c_ulong * n)(*caps), A(*[C.addressof(x) for x in src]), (C.c_ulong * n)(*[len(x) for x in datas]), (C.c_int * n)()


@pytest.mark.parametrize("wbits", [15, 31, -15])
def test_host_library_batch(wbits):
    """7. zamd_compress2_batch: the large items at levels 6 and 9 equal the library's own one-item streams and have gone through ONE streams call"""
    import zhost as Z
    L = Z.lib()
    P, U = C.POINTER(C.c_void_p), C.POINTER(C.c_ulong)
    L.zamd_compress2_batch.argtypes = [P, U, P, U, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.zamd_compress2_batch_count.argtypes = [C.c_int]
    L.zamd_compress2_batch_count.restype = C.c_ulonglong
    datas = [cases.make("mix", n, 70 + i) for i, n in enumerate((0, 100, 65536, 65537, 200000, (1 << 20) + 1))]
    for level in (6, 9):
        own = [Z.compress2(x, level)[1] if wbits == 15 else Z.deflate_stream(x, level, [(len(x), Z.Z_FINISH)], window_bits=wbits)[0] for x in datas]
        caps = [int(L.compressBound(len(x))) + 32 for x in datas]
        caps[4] = 1000  # a short destLen on a large item
        src, dst, dp, dl, sp, sl, st = _batch_args(datas, caps)
        calls0, one0 = L.zamd_compress2_batch_count(0), L.zamd_compress2_batch_count(1)
        rc = L.zamd_compress2_batch(dp, dl, sp, sl, len(datas), level, wbits, st)
        assert (L.zamd_compress2_batch_count(0) - calls0, L.zamd_compress2_batch_count(1) - one0) == (1, 0), "the three large items are one streams call, nothing goes one by one"
        assert rc == Z.Z_BUF_ERROR
        for k, x in enumerate(datas):
            if k == 4:
                assert (st[k], dl[k]) == (Z.Z_BUF_ERROR, 1000)
            else:
                assert st[k] == Z.Z_OK and dst[k].raw[: dl[k]] == own[k], (level, k)
        if R.available() and wbits == 15:
            assert own[5] == R.compress2(datas[5], level)
