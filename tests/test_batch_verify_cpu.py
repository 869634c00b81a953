"""The batch integrity test, what needs no GPU: both libraries export the entry points their headers declare; the host library's answers that come
in front of any engine call (nothing to do is OK and creates no engine -- there is no GPU here to create one on; bad arguments are refused and touch
nothing); and the fold's arithmetic -- the check values of a byte string taken in pieces of 16 KiB and a ragged tail, 64 end-aligned slices a piece --
computed on the CPU by tests/tools/fold_model.cpp through the helpers the kernel itself calls (zlib_amd/csrc/zgpu_common.h), against Python's zlib."""
import ctypes as C
import os
import re
import subprocess
import zlib

import pytest

from oracle import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_GPU = ["zgpu_inflate_batch_verify_device", "zgpu_inflate_batch_verify_host", "zgpu_bgzf_verify_device", "zgpu_bgzf_verify_host"]
NEW_HOST = {"zamd_batch.h": ["zamd_uncompress_verify_batch"], "zamd_zip_test.h": ["zamd_unzip_test_batch"], "zamd_bgzf.h": ["zamd_bgzf_test"]}
PARAMERROR = -102


def _exported(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "zlib_amd", so)]).decode()
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def _declared(header, pattern):
    with open(os.path.join(ROOT, "include", header)) as f:
        return re.findall(pattern, f.read())


def test_entry_points_are_declared_and_exported():
    gpu = _declared("zamd_gpu.h", r"\b(zgpu_[a-z0-9_]+)\s*\(")
    assert not [n for n in NEW_GPU if n not in gpu or n not in _exported("libzamd_gpu.so")]
    for header, names in NEW_HOST.items():
        host = _declared(header, r"\b(zamd_[a-z0-9_]+)\s*\(")
        assert not [n for n in names if n not in host or n not in _exported("libzamd_z.so")], header


def test_host_library_answers_without_an_engine():
    from tests import zhost
    L = zhost.lib()
    P, U = C.POINTER(C.c_void_p), C.POINTER(C.c_ulong)
    L.zamd_uncompress_verify_batch.argtypes = [U, P, U, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    L.zamd_unzip_test_batch.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_long)]
    L.zamd_bgzf_test.argtypes = [C.c_char_p, C.c_ulong, U]
    # nothing to do
    assert L.zamd_uncompress_verify_batch(None, None, None, 0, 15, None) == zhost.Z_OK
    dl = C.c_ulong(7)
    assert L.zamd_bgzf_test(None, 0, C.byref(dl)) == zhost.Z_OK and dl.value == 0  # an empty file has no blocks
    assert L.zamd_bgzf_test(b"", 0, None) == zhost.Z_OK
    # bad arguments: refused, the sentinels survive
    src = C.create_string_buffer(b"\x78\x9c\x03\x00\x00\x00\x00\x01", 8)
    sp, sl = (C.c_void_p * 1)(C.addressof(src)), (C.c_ulong * 1)(8)
    dl, st = (C.c_ulong * 1)(7), (C.c_int * 1)(9)
    assert L.zamd_uncompress_verify_batch(dl, sp, sl, 1, 0, st) == zhost.Z_STREAM_ERROR          # no such windowBits
    assert L.zamd_uncompress_verify_batch(dl, sp, None, 1, 15, st) == zhost.Z_STREAM_ERROR
    assert L.zamd_uncompress_verify_batch(dl, None, sl, 1, 15, st) == zhost.Z_STREAM_ERROR
    assert L.zamd_uncompress_verify_batch(dl, sp, sl, 1, 15, None) == zhost.Z_STREAM_ERROR
    assert L.zamd_uncompress_verify_batch(dl, (C.c_void_p * 1)(None), sl, 1, 15, st) == zhost.Z_STREAM_ERROR  # a length without bytes
    assert (dl[0], st[0]) == (7, 9)
    res, idx = (C.c_long * 1)(77), (C.c_int * 1)(0)
    assert L.zamd_unzip_test_batch(None, idx, 1, res) == PARAMERROR  # no archive
    assert L.zamd_unzip_test_batch(None, None, 0, None) == PARAMERROR
    assert res[0] == 77
    one = C.c_ulong(7)
    assert L.zamd_bgzf_test(None, 5, C.byref(one)) == zhost.Z_STREAM_ERROR and one.value == 7


def test_unzip_test_batch_of_nothing_needs_no_engine(tmp_path):
    from tests import zhost
    L = zhost.lib()
    L.zamd_zip_open.restype = C.c_void_p
    L.zamd_zip_open.argtypes = [C.c_char_p]
    L.zamd_zip_close.argtypes = [C.c_void_p, C.c_char_p]
    L.zamd_unzip_open.restype = C.c_void_p
    L.zamd_unzip_open.argtypes = [C.c_char_p]
    L.zamd_unzip_close.argtypes = [C.c_void_p]
    L.zamd_unzip_test_batch.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_long)]
    path = str(tmp_path / "empty.zip").encode()
    z = L.zamd_zip_open(path)
    assert z and L.zamd_zip_close(z, None) == 0
    u = L.zamd_unzip_open(path)
    assert u
    res = (C.c_long * 1)(77)
    assert L.zamd_unzip_test_batch(u, None, 0, None) == 0  # n == 0: ZAMD_ZIP_OK
    assert L.zamd_unzip_test_batch(u, None, 1, None) == PARAMERROR  # results have nowhere to go
    idx = (C.c_int * 1)(3)
    assert L.zamd_unzip_test_batch(u, idx, 1, res) == PARAMERROR and res[0] == PARAMERROR  # no such member: that item's own code
    assert L.zamd_unzip_close(u) == 0


@pytest.fixture(scope="module")
def fold_model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fold") / "fold_model")
    # host code only, with the host sanitizers: the program makes no HIP call
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "tools", "fold_model.cpp")], check=True, timeout=300)
    return exe


@pytest.mark.parametrize("kind", ["mix", "ff"])
def test_fold_equals_zlib(fold_model, tmp_path, kind):
    for n in (0, 1, 63, 64, 65, 16383, 16384, 16385, 32768 + 5, 100000):
        d = b"\xff" * n if kind == "ff" else cases.make("mix", n, 41)  # (0xFF: a full piece's s2 does not fit 32 bits)
        path = tmp_path / ("%s_%d.bin" % (kind, n))
        path.write_bytes(d)
        out = subprocess.run([fold_model, str(path)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        assert tuple(int(x) for x in out.stdout.split()) == (zlib.adler32(d), zlib.crc32(d)), (kind, n)
