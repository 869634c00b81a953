"""BGZF (blocked gzip) on the GPU: the encode (every 65 280 bytes one block, byte for byte what bgzip's deflate calls give), the device's block finder
(mark, compact, link, reach from byte 0 by pointer doubling, order) against a header chase in Python and the host library's walk, the batched
decode against gzip.decompress, false headers inside stored payloads, damaged files and damaged blocks, and the zlib-style host entry points."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cases, refzlib as R  # noqa: E402
from tests import bgzf_fixtures as F, zhost  # noqa: E402

OK, STREAM_ERROR, DATA_ERROR, BUF_ERROR = 0, -2, -3, -5


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


class Block(C.Structure):
    _fields_ = [("coffset", C.c_ulonglong), ("uoffset", C.c_ulonglong)]


@pytest.fixture(scope="module")
def L():
    lib = zhost.lib()
    U = C.POINTER(C.c_ulong)
    lib.zamd_bgzf_bound.argtypes = [C.c_ulong]
    lib.zamd_bgzf_bound.restype = C.c_ulong
    lib.zamd_bgzf_compress.argtypes = [C.c_char_p, U, C.c_char_p, C.c_ulong, C.c_int]
    lib.zamd_bgzf_uncompress.argtypes = [C.c_char_p, U, C.c_char_p, C.c_ulong]
    lib.zamd_bgzf_index.argtypes = [C.c_char_p, C.c_ulong, C.POINTER(Block), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    lib.zamd_bgzf_uncompress_range.argtypes = [C.c_char_p, C.c_char_p, C.c_ulong, C.POINTER(Block), C.c_size_t, C.c_ulonglong, C.c_ulong]
    return lib


def host_index(L, f):
    n, eof = C.c_size_t(0), C.c_int(-1)
    rc = L.zamd_bgzf_index(f, len(f), None, 0, C.byref(n), C.byref(eof))
    if rc != zhost.Z_BUF_ERROR:
        return rc, None, None
    blocks = (Block * (n.value + 1))()
    rc = L.zamd_bgzf_index(f, len(f), blocks, n.value + 1, C.byref(n), C.byref(eof))
    return rc, blocks, ([b.coffset for b in blocks], [b.uoffset for b in blocks], bool(eof.value))


def device_index(eng, f, cap=None):
    """zgpu_bgzf_index_device on torch buffers -> (rc, (starts, sums, eof) or None, the device tensors)"""
    import torch
    dev = torch.device("cuda", 0)
    cap = len(f) // 28 if cap is None else cap  # (the header's rule: no block is shorter than 28 bytes)
    d_in = torch.tensor(np.frombuffer(f + b"\0", dtype=np.uint8), device=dev)
    d_io = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
    d_oo = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
    rc, n, total, eof = eng.bgzf_index_device(d_in.data_ptr(), len(f), d_io.data_ptr(), d_oo.data_ptr(), cap)
    if rc != OK:
        return rc, n, (d_in, d_io, d_oo)
    got = ([int(x) for x in d_io[: n + 1].cpu()], [int(x) for x in d_oo[: n + 1].cpu()], bool(eof))
    assert got[1][-1] == total
    return rc, got, (d_in, d_io, d_oo)


# ---- encode ----
ENCODE = [("mix", n, 0) for n in (0, 1, 65279, 65280, 65281, 2 * 65280, 3 * 65280 + 17)] + [("rand", 65280, 0), ("mix", 10000, 4096)]


def _encode_data(kind, n):
    return cases.make(kind, n, 5) if n else b""


@pytest.mark.parametrize("kind,n,bs", ENCODE)
def test_encode_reads_back_and_offsets(eng, kind, n, bs):
    data = _encode_data(kind, n)
    size = bs or 65280
    for level in (1, 6, 9):
        f, offs = eng.bgzf_deflate_host(data, level, block_size=bs, want_offsets=True)
        assert gzip.decompress(f) == data, level
        want = F.chase(f)
        assert want is not None and want[2]
        assert [int(x) for x in offs] == want[0], level
        assert want[1] == [min(k * size, n) for k in range((n + size - 1) // size + 1)] + [n]
        assert all(b - a <= 65536 for a, b in zip(want[0], want[0][1:]))
        assert eng.last.out_bytes == len(f) and eng.last.nchunks == (n + size - 1) // size and eng.last.crc32 == zlib.crc32(data)


@pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref) is not here")
@pytest.mark.parametrize("kind,n,bs", ENCODE)
def test_encode_matches_reference(eng, kind, n, bs):
    data = _encode_data(kind, n)
    size = bs or 65280
    for level in (1, 6, 9):
        want = b"".join(F.block(data[i: i + size], body=R.deflate_wbits(data[i: i + size], level, -15)) for i in range(0, n, size)) + F.EOF_BLOCK
        assert eng.bgzf_deflate_host(data, level, block_size=bs) == want, level


def _segments(eng, bufs, level, flags):
    from zlib_amd import gpu
    offs = np.zeros(len(bufs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(b) for b in bufs])
    blob = np.frombuffer(b"".join(bufs) + b"\0", dtype=np.uint8)
    cap = int(eng.L.zgpu_deflate_segments_bound(len(bufs), int(offs[-1]), flags))
    out = np.empty(cap, dtype=np.uint8)
    ooffs = np.zeros(len(bufs) + 1, dtype=np.uint64)
    p = gpu._Params(level, 0, flags, gpu.LZ_AUTO, 0, 0)
    res = gpu.DeflateResult()
    rc = eng.L.zgpu_deflate_segments_host(eng.h, blob.ctypes.data, offs.ctypes.data, len(bufs), C.byref(p), out.ctypes.data, cap, ooffs.ctypes.data, C.byref(res))
    raw = out[: res.out_bytes].tobytes() if rc == OK else b""
    return rc, [raw[int(ooffs[i]): int(ooffs[i + 1])] for i in range(len(bufs))]


def test_segments_flag_frames_the_raw_segments(eng):
    from zlib_amd import gpu
    bufs = [cases.make("mix", n, 9 + i) for i, n in enumerate((0, 1, 100, 4096, 65279, 65280))] + [cases.make("rand", 65280, 3)]
    for level in (1, 6):
        rc, raw = _segments(eng, bufs, level, gpu.F_FINAL)
        rc2, blk = _segments(eng, bufs, level, gpu.F_FINAL | gpu.F_BGZF_WRAP)
        assert rc == OK and rc2 == OK
        for d, r, b in zip(bufs, raw, blk):
            assert b == F.block(d, body=r)
    assert eng.L.zgpu_deflate_segments_bound(7, 1000, gpu.F_FINAL | gpu.F_BGZF_WRAP) == eng.L.zgpu_deflate_segments_bound(7, 1000, gpu.F_FINAL) + 7 * 26


def test_segments_flag_refusals(eng):
    from zlib_amd import gpu
    good = cases.make("mix", 65280, 1)
    assert _segments(eng, [good, cases.make("mix", 65281, 2)], 6, gpu.F_FINAL | gpu.F_BGZF_WRAP)[0] == STREAM_ERROR
    assert _segments(eng, [good], 6, gpu.F_BGZF_WRAP)[0] == STREAM_ERROR                                   # needs FINAL
    assert _segments(eng, [good], 6, gpu.F_FINAL | gpu.F_BGZF_WRAP | gpu.F_GZIP_WRAP)[0] == STREAM_ERROR   # no other wrapper
    assert _segments(eng, [good], 6, gpu.F_FINAL | gpu.F_BGZF_WRAP | gpu.F_ZLIB_WRAP)[0] == STREAM_ERROR
    eng.set_geometry(14, 8)
    try:
        assert _segments(eng, [good], 6, gpu.F_FINAL | gpu.F_BGZF_WRAP)[0] == STREAM_ERROR
    finally:
        eng.set_geometry(15, 8)
    assert _segments(eng, [good], 6, gpu.F_FINAL | gpu.F_BGZF_WRAP)[0] == OK
    # the flag belongs to segment calls: the other deflate entries refuse it
    for flags in (gpu.F_FINAL | gpu.F_BGZF_WRAP, gpu.F_FINAL | gpu.F_BGZF_WRAP | gpu.F_CONTINUOUS):
        with pytest.raises(gpu.EngineError) as ei:
            eng.deflate_host(good, 6, flags=flags)
        assert ei.value.code == STREAM_ERROR


def test_encode_device_entry(eng):
    import torch
    dev = torch.device("cuda", 0)
    data = cases.make("mix", 2 * 65280 + 500, 12)
    cap = int(eng.L.zgpu_bgzf_bound(len(data), 0))
    d_in = torch.tensor(np.frombuffer(data, dtype=np.uint8), device=dev)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(3 + 2, dtype=torch.int64, device=dev)
    res = eng.bgzf_deflate_device(d_in.data_ptr(), len(data), 6, d_out.data_ptr(), cap, d_offsets=d_off.data_ptr())
    f = d_out[: res.out_bytes].cpu().numpy().tobytes()
    assert f == eng.bgzf_deflate_host(data, 6)
    assert [int(x) for x in d_off.cpu()] == F.chase(f)[0]


# ---- decode ----
WELL = sorted(F.well_formed())


@pytest.mark.parametrize("name", WELL)
def test_decode_well_formed(eng, L, name):
    f = F.well_formed()[name]
    want = F.chase(f)
    data = gzip.decompress(f) if f else b""
    rc, got, items = eng.bgzf_inflate_host(f)
    assert rc == OK and got == data
    assert eng.last_inflate.out_bytes == len(data) and eng.last_inflate.first_bad_chunk == -1
    n = len(want[0]) - 1
    for k in range(n):
        assert (items[k].code, items[k].out_bytes, items[k].in_used) == (OK, want[1][k + 1] - want[1][k], want[0][k + 1] - want[0][k]), k
    rc, dev, _ = device_index(eng, f)
    assert rc == OK and dev == want
    rc, _, host = host_index(L, f)
    assert rc == zhost.Z_OK and host == want
    if name == "many":
        assert n >= 1500  # (twelve doubling rounds, several workgroups of every kernel of the finder)


def test_items_sized_by_the_headers_rule(eng):
    """in_bytes / 28 records are enough for any file: the smallest blocks there are fill them exactly, and shorter ones are no blocks"""
    import zlib_amd.gpu as G
    f = F.well_formed()["smallest"]
    n = len(f) // 28
    arr = np.frombuffer(f, dtype=np.uint8)
    raw = np.full((n + 1) * C.sizeof(G.InflateItem), 0xA5, dtype=np.uint8)  # one record of guard behind the n the rule gives
    res = G.InflateResult()
    rc = eng.L.zgpu_bgzf_inflate_host(eng.h, arr.ctypes.data, len(f), None, 0, raw.ctypes.data, C.byref(res))
    assert rc == OK and res.out_bytes == 0
    items = [G.InflateItem.from_buffer_copy(raw.tobytes(), k * C.sizeof(G.InflateItem)) for k in range(n)]
    assert all((it.code, it.out_bytes, it.in_used) == (OK, 0, 28) for it in items)
    assert (raw[n * C.sizeof(G.InflateItem):] == 0xA5).all()
    g = F.malformed()["no_body"]
    assert len(g) // 26 > len(g) // 28
    raw[:] = 0xA5
    rc = eng.L.zgpu_bgzf_inflate_host(eng.h, np.frombuffer(g, dtype=np.uint8).ctypes.data, len(g), None, 0, raw.ctypes.data, C.byref(res))
    assert rc == DATA_ERROR and res.first_bad_chunk == -1 and (raw == 0xA5).all()


def test_decode_capacity(eng):
    f = F.well_formed()["three"]
    data = gzip.decompress(f)
    rc, got, _ = eng.bgzf_inflate_host(f, out_cap=len(data) - 1)
    assert rc == BUF_ERROR and eng.last_inflate.out_bytes == len(data)
    rc, got, _ = eng.bgzf_inflate_host(f, out_cap=len(data))
    assert rc == OK and got == data
    rc, n, _ = device_index(eng, f, cap=3)  # four blocks
    assert rc == BUF_ERROR and n == 4


def test_index_then_batch_on_device_buffers(eng):
    import torch
    import zlib_amd.gpu as G
    f = F.well_formed()["many"]
    data = gzip.decompress(f)
    rc, got, (d_in, d_io, d_oo) = device_index(eng, f)
    assert rc == OK
    n = len(got[0]) - 1
    dev = torch.device("cuda", 0)
    d_out = torch.zeros(len(data) + 1, dtype=torch.uint8, device=dev)
    d_items = torch.zeros(n * C.sizeof(G.InflateItem), dtype=torch.uint8, device=dev)
    failed = eng.inflate_batch_device(d_in.data_ptr(), len(f), d_io.data_ptr(), n, d_out.data_ptr(), len(data), d_oo.data_ptr(), d_items.data_ptr(), wrap="gzip")
    assert failed == 0
    assert d_out[: len(data)].cpu().numpy().tobytes() == data
    # the whole decode on device buffers gives the same
    d_out2 = torch.zeros(len(data) + 1, dtype=torch.uint8, device=dev)
    rc, res = eng.bgzf_inflate_device(d_in.data_ptr(), len(f), d_out2.data_ptr(), len(data), d_items.data_ptr())
    assert rc == OK and res.out_bytes == len(data) and d_out2[: len(data)].cpu().numpy().tobytes() == data


@pytest.mark.parametrize("name", sorted(F.malformed()))
def test_malformed_files(eng, L, name):
    f = F.malformed()[name]
    rc, got, _ = eng.bgzf_inflate_host(f)
    r = eng.last_inflate
    assert rc == DATA_ERROR and (r.first_bad_chunk, r.error_code) == (-1, DATA_ERROR)
    assert eng.L.zgpu_inflate_message(r.error_msg) == b"invalid BGZF block chain"
    assert device_index(eng, f)[0] == DATA_ERROR
    assert host_index(L, f)[0] == zhost.Z_DATA_ERROR


def test_finder_agrees_with_the_chase_on_mutated_headers(eng):
    for f in F.mutations(60):
        want = F.chase(f)
        rc, got, _ = device_index(eng, f)
        assert (rc == OK) == (want is not None)
        if want is not None:
            assert got == want


def _blocks_decode(eng, f):
    """the per-block view of a decode: rc, [(code, msg, bytes of the block's range)]"""
    co, uo, _ = F.chase(f)
    rc, got, items = eng.bgzf_inflate_host(f)
    return rc, [(items[k].code, eng.L.zgpu_inflate_message(items[k].msg).decode(), got[uo[k]: uo[k + 1]]) for k in range(len(co) - 1)]


def test_damaged_crc_is_that_blocks_alone(eng):
    blocks = F.six_blocks()
    rc, good = _blocks_decode(eng, b"".join(blocks) + F.EOF_BLOCK)
    assert rc == OK and [g[2] for g in good[:6]] == F.SIX
    b2 = blocks[2]
    blocks[2] = b2[:-8] + struct.pack("<I", zlib.crc32(F.SIX[2]) ^ 0x10) + b2[-4:]
    rc, got = _blocks_decode(eng, b"".join(blocks) + F.EOF_BLOCK)
    assert rc == DATA_ERROR
    assert got[2][:2] == (DATA_ERROR, "incorrect data check")
    r = eng.last_inflate
    assert (r.first_bad_chunk, r.error_code, eng.L.zgpu_inflate_message(r.error_msg)) == (2, DATA_ERROR, b"incorrect data check")
    for k in (0, 1, 3, 4, 5, 6):
        assert got[k] == good[k], k


def test_isize_below_what_the_block_decodes_to(eng):
    blocks = F.six_blocks()
    b4 = blocks[4]
    blocks[4] = b4[:-4] + struct.pack("<I", len(F.SIX[4]) - 1)
    rc, got = _blocks_decode(eng, b"".join(blocks) + F.EOF_BLOCK)
    assert rc == DATA_ERROR and eng.last_inflate.first_bad_chunk == 4
    assert got[4][:2] == (DATA_ERROR, "incorrect length check")
    for k in (0, 1, 2, 3, 5):
        assert got[k] == (OK, "", F.SIX[k]), k
    assert got[6] == (OK, "", b"")


# ---- the host library ----
def _compress(L, data, level, cap=None):
    n = C.c_ulong(L.zamd_bgzf_bound(len(data)) if cap is None else cap)
    out = C.create_string_buffer(max(n.value, 1))
    rc = L.zamd_bgzf_compress(out, C.byref(n), data, len(data), level)
    return rc, out.raw[: n.value]


def _uncompress(L, f, cap):
    n = C.c_ulong(cap)
    out = C.create_string_buffer(max(cap, 1))
    rc = L.zamd_bgzf_uncompress(out, C.byref(n), f, len(f))
    return rc, n.value, out.raw[: n.value] if rc == zhost.Z_OK else b""


def test_host_library_round_trip(eng, L):
    for data in (b"", cases.make("mix", 1, 2), cases.make("mix", 3 * 65280 + 17, 3)):
        rc, f = _compress(L, data, 6)
        assert rc == zhost.Z_OK and f == eng.bgzf_deflate_host(data, 6) and gzip.decompress(f) == data
        assert _uncompress(L, f, len(data)) == (zhost.Z_OK, len(data), data)
        if data:
            assert _uncompress(L, f, len(data) - 1)[:2] == (zhost.Z_BUF_ERROR, len(data))
            assert _compress(L, data, 6, cap=len(f) - 1)[0] == zhost.Z_BUF_ERROR
    assert _compress(L, b"abc", 0)[0] == zhost.Z_STREAM_ERROR  # no level 0
    assert _compress(L, b"abc", -1)[1] == _compress(L, b"abc", 6)[1]
    assert _uncompress(L, F.malformed()["cut"], 1 << 20)[0] == zhost.Z_DATA_ERROR


@pytest.mark.parametrize("name", ["many", "three", "concat"])
def test_host_library_ranges(L, name):
    f = F.well_formed()[name]
    data = gzip.decompress(f)
    rc, blocks, (co, uo, _) = host_index(L, f)
    assert rc == zhost.Z_OK
    n = len(co) - 1
    empties = [k for k in range(1, n - 1) if uo[k] == uo[k + 1]]
    ranges = [(uo[1] + 1, 5), (uo[2] - 3, 10), (len(data) - 1, 1), (100, 0), (len(data), 0), (0, len(data)), (uo[1], uo[3] - uo[1])]
    if name == "concat":
        assert empties
        ranges.append((uo[empties[0]] - 7, 20))  # across the empty block in the middle
    for lo, ln in ranges:
        out = C.create_string_buffer(max(ln, 1))
        assert L.zamd_bgzf_uncompress_range(out, f, len(f), blocks, n, lo, ln) == zhost.Z_OK, (lo, ln)
        assert out.raw[:ln] == data[lo: lo + ln], (lo, ln)
    out = C.create_string_buffer(16)
    assert L.zamd_bgzf_uncompress_range(out, f, len(f), blocks, n, len(data) - 1, 2) == zhost.Z_BUF_ERROR
    assert L.zamd_bgzf_uncompress_range(out, f, len(f), blocks, n, len(data) + 1, 0) == zhost.Z_BUF_ERROR


def test_gzread_reads_what_bgzf_compress_wrote(L, tmp_path):
    data = cases.make("text", 2 * 65280 + 999, 8)
    rc, f = _compress(L, data, 6)
    assert rc == zhost.Z_OK
    path = tmp_path / "x.gz"
    path.write_bytes(f)
    L.gzopen.restype = C.c_void_p
    L.gzopen.argtypes = [C.c_char_p, C.c_char_p]
    L.gzread.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
    L.gzclose.argtypes = [C.c_void_p]
    g = L.gzopen(str(path).encode(), b"rb")
    assert g
    buf = C.create_string_buffer(len(data) + 100)
    got = b""
    while True:
        k = L.gzread(g, buf, len(data) + 100)
        if k <= 0:
            break
        got += buf.raw[:k]
    assert k == 0 and L.gzclose(g) == 0
    assert got == data
