"""The packed batch decode, zgpu_inflate_batch_packed_* (sizing pass, layout on the device, decode into that layout), and the host library's
zamd_uncompress_sizes_batch / zamd_uncompress_batch_packed.  The truth is Python's zlib; the decoder the layout is handed to when the output is too
small is the project's existing zgpu_inflate_batch_host."""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cases  # noqa: E402
from tests import batch_sizes_fixtures as F  # noqa: E402
from tests.batch_sizes_fixtures import BUF_ERROR, DATA_ERROR, NEED_DICT, OK, STREAM_ERROR, TRUNCATED  # noqa: E402
from tests.test_gpu_batch_sizes import _damage_items, _trailer_items  # noqa: E402


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


def _mixed():
    """good items of every size class with the damaged ones of the sizes tests among them: (streams, decoded bytes or None)"""
    good, damaged, _ = _damage_items()
    pairs = F.streams("auto")
    zs = [z + F.JUNK for _, z in pairs]
    want = [d for d, _ in pairs]
    for k in sorted(damaged):
        at = 3 + 5 * k
        zs.insert(at, damaged[k][0]); want.insert(at, None)
    return zs, want, {3 + 5 * k: damaged[k][1:] for k in damaged}


def _check_layout(offs, recs, want, align, total):
    assert offs[0] == 0 and total == offs[-1]
    for k, (r, d) in enumerate(zip(recs, want)):
        size = len(d) if d is not None else 0
        assert offs[k] % align == 0, (k, offs[k])
        assert offs[k + 1] >= offs[k] + size, (k, offs[k], offs[k + 1], size)
        assert offs[k + 1] - (offs[k] + size) < align, (k, "a gap wider than the alignment")
    last = len(want) - 1
    assert offs[-1] == offs[last] + (len(want[last]) if want[last] is not None else 0)


@pytest.mark.parametrize("align", [1, 16])
def test_packed_decode(eng, align):
    zs, want, verdicts = _mixed()
    rc, total, failed, offs, recs, out = F.packed_call(eng, zs, "auto", checks=3, align=align)
    assert rc == OK and failed == len(verdicts)
    _check_layout(offs, recs, want, align, total)
    bad = []
    for k, (r, d, z) in enumerate(zip(recs, want, zs)):
        if d is None:
            if r != verdicts[k] + (0, 0, 1, 0) or offs[k + 1] - offs[k] >= align:
                bad.append((k, r, verdicts[k]))
        elif r != (OK, "", len(d), len(z) - len(F.JUNK), zlib.adler32(d), zlib.crc32(d)) or out[offs[k]: offs[k] + len(d)].tobytes() != d:
            bad.append((k, r[:4], len(d)))
    assert not bad, bad[:10]
    assert (out[total:] == 0xA5).all()
    # the Python wrapper: the same bytes and records, the buffer sized by a first call
    datas, precs = eng.inflate_batch_packed_host(zs[:40], wrap="auto", checks=3, align=align)
    assert datas == [d if d is not None else b"" for d in want[:40]] and precs == recs[:40]
    assert eng.last_offsets[:40] == offs[:40]


def test_output_too_small(eng):
    zs, want, verdicts = _mixed()
    rc, total, failed, offs, recs, out = F.packed_call(eng, zs, "auto", checks=3)
    assert rc == OK
    rc2, total2, failed2, offs2, sized, out2 = F.packed_call(eng, zs, "auto", checks=3, cap=total - 1)
    assert rc2 == BUF_ERROR and total2 == total and offs2 == offs and failed2 == len(verdicts)
    assert (out2 == 0xA5).all()  # nothing is decoded
    rcs, _, sizes = F.sizes_call(eng, zs, "auto")
    assert rcs == OK and sized == sizes  # the records are the sizing pass's
    # the caller allocates and hands the table to the plain batch decode
    blob, ioffs = F.pack(zs)
    from zlib_amd import gpu
    n = len(zs)
    buf = np.full(total + 1, 0xA5, dtype=np.uint8)
    items = (gpu.InflateItem * n)()
    tab = np.array(offs, dtype=np.uint64)
    nf = C.c_uint64(0)
    assert eng.L.zgpu_inflate_batch_host(eng.h, blob.ctypes.data, int(ioffs[-1]), ioffs.ctypes.data, n, gpu.WRAP_AUTO, 3, buf.ctypes.data, total, tab.ctypes.data, items,
                                         C.byref(nf)) == OK
    for k, d in enumerate(want):
        if d is not None:
            assert items[k].code == OK and buf[offs[k]: offs[k] + len(d)].tobytes() == d, k
    assert buf[: total].tobytes() == out[: total].tobytes()


def test_arguments(eng):
    z = zlib.compress(b"hello")
    for align in (3, 0, 512, 24):
        rc, total, failed, offs, recs, out = F.packed_call(eng, [z, z], "zlib", align=align, cap=64)
        assert rc == STREAM_ERROR and (out == 0xA5).all() and offs == [0xDEAD] * 3, align
    rc, total, failed, offs, recs, out = F.packed_call(eng, [], "zlib", cap=64)
    assert (rc, total, failed) == (OK, 0, 0) and (out == 0xA5).all()
    rc, total, failed, offs, recs, out = F.packed_call(eng, [z, z], "zlib", align=256, cap=1024)
    assert (rc, total, failed, offs) == (OK, 256 + 5, 0, [0, 256, 261])
    assert out[:5].tobytes() == b"hello" and out[256:261].tobytes() == b"hello" and (out[5:256] == 0xA5).all()


def test_trailer_mismatches_show_in_the_decode(eng):
    d, z, gz, flipped, wrong_isize = _trailer_items()
    zs = [z, flipped, gz, wrong_isize, z]
    rc, total, failed, offs, recs, out = F.packed_call(eng, zs, "auto", checks=3, cap=8 * len(d))
    assert rc == OK and failed == 2 and total == 5 * len(d)  # (the two were sized: their ranges are in the layout)
    assert recs[1][:4] == (DATA_ERROR, "incorrect data check", 0, 0) and recs[3][:4] == (DATA_ERROR, "incorrect length check", 0, 0)
    for k in (0, 2, 4):
        assert recs[k] == (OK, "", len(d), len(zs[k]), zlib.adler32(d), zlib.crc32(d)), k
        assert out[offs[k]: offs[k] + len(d)].tobytes() == d, k
    for k in (1, 3):  # the host entry writes only what succeeded
        assert (out[offs[k]: offs[k + 1]] == 0xA5).all(), k


def test_device_entry_matches_host(eng):
    import torch
    from zlib_amd import gpu
    zs, want, verdicts = _mixed()
    rc, total, failed, offs, recs, out = F.packed_call(eng, zs, "auto", checks=3, align=16)
    n = len(zs)
    dev = torch.device("cuda", 0)
    blob, ioffs = F.pack(zs)
    d_in = torch.tensor(blob, device=dev)
    d_io = torch.tensor(ioffs.view(np.int64), device=dev)
    d_oo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_out = torch.full((total + 1,), 0xA5, dtype=torch.uint8, device=dev)
    isz = C.sizeof(gpu.InflateItem)
    d_items = torch.zeros(n * isz, dtype=torch.uint8, device=dev)
    # too small first: the table and the total, nothing decoded
    got = eng.inflate_batch_packed_device(d_in.data_ptr(), int(ioffs[-1]), d_io.data_ptr(), n, d_out.data_ptr(), total - 1, d_oo.data_ptr(), d_items.data_ptr(),
                                          wrap="auto", checks=3, align=16)
    assert got == (BUF_ERROR, total, len(verdicts)) and d_oo.cpu().tolist() == offs and bool((d_out == 0xA5).all())
    got = eng.inflate_batch_packed_device(d_in.data_ptr(), int(ioffs[-1]), d_io.data_ptr(), n, d_out.data_ptr(), total, d_oo.data_ptr(), d_items.data_ptr(),
                                          wrap="auto", checks=3, align=16)
    assert got == (OK, total, len(verdicts)) and d_oo.cpu().tolist() == offs
    raw = d_items.cpu().numpy().tobytes()
    assert [F.record(eng, gpu.InflateItem.from_buffer_copy(raw, k * isz)) for k in range(n)] == recs
    dout = d_out.cpu().numpy()
    for k, d in enumerate(want):
        if d is not None:
            assert dout[offs[k]: offs[k] + len(d)].tobytes() == d, k
    assert dout[total] == 0xA5


# ---- the host library ----
def _lib():
    from tests import zhost
    L = zhost.lib()
    P, U = C.POINTER(C.c_void_p), C.POINTER(C.c_ulong)
    L.zamd_uncompress_sizes_batch.argtypes = [U, P, U, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    L.zamd_uncompress_sizes_batch.restype = C.c_int
    L.zamd_uncompress_batch_packed.argtypes = [C.c_void_p, U, U, P, U, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    L.zamd_uncompress_batch_packed.restype = C.c_int
    return L


def _sources(zs):
    n = len(zs)
    src = [C.create_string_buffer(z, max(len(z), 1)) for z in zs]
    return src, (C.c_void_p * n)(*[C.addressof(s) for s in src]), (C.c_ulong * n)(*[len(z) for z in zs])


@pytest.mark.parametrize("wbits,wrap", [(15, "zlib"), (31, "gzip"), (47, "auto"), (-15, "raw")])
def test_host_library(wbits, wrap):
    from tests import zhost
    L = _lib()
    pairs = list(F.streams(wrap))
    datas = [d for d, _ in pairs]
    zs = [z for _, z in pairs]
    n = len(zs)
    keep, sp, sl = _sources(zs)
    # every item good
    dl = (C.c_ulong * n)(*[7] * n)
    st = (C.c_int * n)(*[9] * n)
    assert L.zamd_uncompress_sizes_batch(dl, sp, sl, n, wbits, st) == zhost.Z_OK
    assert list(st) == [zhost.Z_OK] * n and list(dl) == [len(d) for d in datas]
    total = sum(len(d) for d in datas)
    dest = C.create_string_buffer(total + 1)
    cap = C.c_ulong(total)
    offs = (C.c_ulong * (n + 1))()
    assert L.zamd_uncompress_batch_packed(dest, C.byref(cap), offs, sp, sl, n, wbits, st) == zhost.Z_OK
    assert cap.value == total and list(st) == [zhost.Z_OK] * n
    assert list(offs) == [0] + list(np.cumsum([len(d) for d in datas]))
    assert dest.raw[:total] == b"".join(datas)
    # one damaged item (cut inside a block) in the middle
    k = 21
    zs2 = list(zs)
    zs2[k] = zs[k][: len(zs[k]) // 2]
    assert len(datas[k]) > 1000
    keep2, sp2, sl2 = _sources(zs2)
    dl = (C.c_ulong * n)(*[7] * n)
    assert L.zamd_uncompress_sizes_batch(dl, sp2, sl2, n, wbits, st) == zhost.Z_DATA_ERROR
    assert list(st) == [zhost.Z_OK] * k + [zhost.Z_DATA_ERROR] + [zhost.Z_OK] * (n - k - 1)
    assert list(dl) == [len(d) if j != k else 0 for j, d in enumerate(datas)]
    need = total - len(datas[k])
    # the room too small: the bytes needed and the table, nothing decoded
    dest = C.create_string_buffer(b"\xa5" * (total + 1), total + 1)
    cap = C.c_ulong(need - 1)
    assert L.zamd_uncompress_batch_packed(dest, C.byref(cap), offs, sp2, sl2, n, wbits, st) == zhost.Z_BUF_ERROR
    want_offs = [0] + list(np.cumsum([len(d) if j != k else 0 for j, d in enumerate(datas)]))
    assert cap.value == need and list(offs) == want_offs and dest.raw == b"\xa5" * (total + 1)
    assert st[k] == zhost.Z_DATA_ERROR
    cap = C.c_ulong(need)
    assert L.zamd_uncompress_batch_packed(dest, C.byref(cap), offs, sp2, sl2, n, wbits, st) == zhost.Z_DATA_ERROR  # the first failing item's code
    assert cap.value == need and list(offs) == want_offs
    assert list(st) == [zhost.Z_OK] * k + [zhost.Z_DATA_ERROR] + [zhost.Z_OK] * (n - k - 1)
    assert dest.raw[:need] == b"".join(d for j, d in enumerate(datas) if j != k) and dest.raw[need:] == b"\xa5" * (total + 1 - need)


def test_host_library_arguments():
    from tests import zhost
    L = _lib()
    z = zlib.compress(b"hello")
    keep, sp, sl = _sources([z])
    dl, st, cap, offs = (C.c_ulong * 1)(7), (C.c_int * 1)(9), C.c_ulong(64), (C.c_ulong * 2)(5, 5)
    dest = C.create_string_buffer(b"\xa5" * 64, 64)
    # n == 0: Z_OK in front of any engine (tests/test_batch_sizes_cpu.py asserts the same where there is no GPU to make one on)
    assert L.zamd_uncompress_sizes_batch(None, None, None, 0, 15, None) == zhost.Z_OK
    assert L.zamd_uncompress_batch_packed(None, C.byref(cap), None, None, None, 0, 15, None) == zhost.Z_OK and cap.value == 0
    cap = C.c_ulong(64)
    assert L.zamd_uncompress_sizes_batch(dl, None, sl, 1, 15, st) == zhost.Z_STREAM_ERROR
    assert L.zamd_uncompress_sizes_batch(dl, sp, sl, 1, 14, st) == zhost.Z_STREAM_ERROR
    assert L.zamd_uncompress_batch_packed(dest, C.byref(cap), offs, None, sl, 1, 15, st) == zhost.Z_STREAM_ERROR
    assert L.zamd_uncompress_batch_packed(dest, C.byref(cap), None, sp, sl, 1, 15, st) == zhost.Z_STREAM_ERROR
    assert L.zamd_uncompress_batch_packed(dest, C.byref(cap), offs, sp, sl, 1, 16, st) == zhost.Z_STREAM_ERROR
    assert (dl[0], st[0], cap.value, list(offs), dest.raw) == (7, 9, 64, [5, 5], b"\xa5" * 64)
