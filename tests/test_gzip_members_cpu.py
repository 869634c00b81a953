"""Multi-member gzip, what needs no GPU: both libraries export the new entry points, and zamd_gunzip's answers that come in front of any engine call
(an empty file is a valid file of no members and needs no engine; null buffers are refused)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import zhost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header, pattern):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(pattern, text)))


def _exported(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "zlib_amd", so)]).decode()
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_libraries_export_the_new_symbols():
    assert _declared("zamd_gzip.h", r"\b(zamd_[a-z0-9_]+)\s*\(") == ["zamd_gunzip"]
    assert "zamd_gunzip" in _exported("libzamd_z.so")
    declared = _declared("zamd_gpu.h", r"\b(zgpu_[a-z0-9_]+)\s*\(")
    have = _exported("libzamd_gpu.so")
    for n in ("zgpu_gzip_inflate_device", "zgpu_gzip_inflate_host", "zgpu_gzip_members_count"):
        assert n in declared and n in have, n


@pytest.fixture(scope="module")
def L():
    lib = zhost.lib()
    U = C.POINTER(C.c_ulong)
    lib.zamd_gunzip.argtypes = [C.c_char_p, U, C.c_char_p, C.c_ulong, U, U]
    return lib


def test_an_empty_file_needs_no_engine(L):
    # (a machine without a GPU cannot make an engine: any call that wanted one would answer Z_MEM_ERROR here)
    n, used, members = C.c_ulong(77), C.c_ulong(5), C.c_ulong(5)
    out = C.create_string_buffer(8)
    assert L.zamd_gunzip(out, C.byref(n), b"", 0, C.byref(used), C.byref(members)) == zhost.Z_OK
    assert (n.value, used.value, members.value) == (0, 0, 0)
    n = C.c_ulong(3)
    assert L.zamd_gunzip(None, C.byref(n), None, 0, None, None) == zhost.Z_OK and n.value == 0


def test_null_buffers_are_refused(L):
    n = C.c_ulong(16)
    out = C.create_string_buffer(16)
    f = b"\x1f\x8b\x08\x00" + bytes(16)
    assert L.zamd_gunzip(None, C.byref(n), f, len(f), None, None) == zhost.Z_STREAM_ERROR
    assert L.zamd_gunzip(out, None, f, len(f), None, None) == zhost.Z_STREAM_ERROR
    assert L.zamd_gunzip(out, C.byref(n), None, len(f), None, None) == zhost.Z_STREAM_ERROR
    assert n.value == 16


def test_counters_start_readable():
    from zlib_amd import gpu
    G = gpu.load_library()
    assert G.zgpu_gzip_members_count(2) == 0 and G.zgpu_gzip_members_count(0) >= 0
