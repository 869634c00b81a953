"""Batch inflate without known sizes, what needs no GPU: both libraries export the entry points their headers declare, and the host library's
answers that come in front of any engine call (n == 0 is Z_OK and creates no engine -- there is no GPU here to create one on; bad arguments are
refused and touch nothing)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_GPU = ["zgpu_inflate_batch_sizes_device", "zgpu_inflate_batch_sizes_host", "zgpu_inflate_batch_packed_device", "zgpu_inflate_batch_packed_host"]
NEW_HOST = ["zamd_uncompress_sizes_batch", "zamd_uncompress_batch_packed"]


def _exported(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "zlib_amd", so)]).decode()
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def _declared(header, pattern):
    with open(os.path.join(ROOT, "include", header)) as f:
        return re.findall(pattern, f.read())


def test_entry_points_are_declared_and_exported():
    gpu, host = _declared("zamd_gpu.h", r"\b(zgpu_[a-z0-9_]+)\s*\("), _declared("zamd_batch.h", r"\b(zamd_[a-z0-9_]+)\s*\(")
    assert not [n for n in NEW_GPU if n not in gpu or n not in _exported("libzamd_gpu.so")]
    assert not [n for n in NEW_HOST if n not in host or n not in _exported("libzamd_z.so")]


def test_host_library_answers_without_an_engine():
    from tests import zhost
    L = zhost.lib()
    P, U = C.POINTER(C.c_void_p), C.POINTER(C.c_ulong)
    L.zamd_uncompress_sizes_batch.argtypes = [U, P, U, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    L.zamd_uncompress_batch_packed.argtypes = [C.c_void_p, U, U, P, U, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    cap = C.c_ulong(64)
    assert L.zamd_uncompress_sizes_batch(None, None, None, 0, 15, None) == zhost.Z_OK
    assert L.zamd_uncompress_batch_packed(None, C.byref(cap), None, None, None, 0, -15, None) == zhost.Z_OK and cap.value == 0
    src = C.create_string_buffer(b"\x78\x9c\x03\x00\x00\x00\x00\x01", 8)
    sp, sl = (C.c_void_p * 1)(C.addressof(src)), (C.c_ulong * 1)(8)
    dl, st, cap, offs = (C.c_ulong * 1)(7), (C.c_int * 1)(9), C.c_ulong(64), (C.c_ulong * 2)(5, 5)
    dest = C.create_string_buffer(b"\xa5" * 64, 64)
    assert L.zamd_uncompress_sizes_batch(dl, sp, sl, 1, 0, st) == zhost.Z_STREAM_ERROR          # no such windowBits
    assert L.zamd_uncompress_sizes_batch(dl, sp, None, 1, 15, st) == zhost.Z_STREAM_ERROR
    assert L.zamd_uncompress_sizes_batch(dl, (C.c_void_p * 1)(None), sl, 1, 15, st) == zhost.Z_STREAM_ERROR  # a length without bytes
    assert L.zamd_uncompress_batch_packed(dest, None, offs, sp, sl, 1, 15, st) == zhost.Z_STREAM_ERROR
    assert L.zamd_uncompress_batch_packed(None, C.byref(cap), offs, sp, sl, 1, 15, st) == zhost.Z_STREAM_ERROR  # room without a buffer
    assert L.zamd_uncompress_batch_packed(dest, C.byref(cap), offs, sp, sl, 1, 32, st) == zhost.Z_STREAM_ERROR
    assert (dl[0], st[0], cap.value, list(offs), dest.raw) == (7, 9, 64, [5, 5], b"\xa5" * 64)
