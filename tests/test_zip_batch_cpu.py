"""ZIP archives in batches and batch checksums, what needs no GPU: the entry points include/zamd_zip_batch.h and include/zamd_batch.h declare are
exported by libzamd_z.so, the new engine entries by libzamd_gpu.so, and the argument checks that come in front of any engine call."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMERROR = -102


def _declared(header, pattern):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(pattern, text)))


def _exported(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "zlib_amd", so)]).decode()
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_host_library_exports_the_batch_entry_points():
    names = _declared("zamd_zip_batch.h", r"\b(zamd_[a-z0-9_]+)\s*\(")
    assert names == ["zamd_unzip_read_batch", "zamd_zip_add_batch"], names
    batch = _declared("zamd_batch.h", r"\b(zamd_[a-z0-9_]+)\s*\(")
    assert "zamd_crc32_batch" in batch and "zamd_adler32_batch" in batch, batch
    have = _exported("libzamd_z.so")
    assert not [n for n in names + batch if n not in have]
    assert not [n for n in have if n.startswith("zamd_batch_engine")], "the engine lock is internal"


def test_gpu_library_exports_the_new_engine_entries():
    declared = _declared("zamd_gpu.h", r"\b(zgpu_[a-z0-9_]+)\s*\(")
    want = ["zgpu_checksum_batch_device", "zgpu_checksum_batch_host", "zgpu_deflate_segments_items_device", "zgpu_deflate_segments_items_host"]
    have = _exported("libzamd_gpu.so")
    for n in want:
        assert n in declared and n in have, n


@pytest.fixture(scope="module")
def L():
    from tests import zhost
    lib = zhost.lib()
    lib.zamd_zip_open.restype = C.c_void_p
    lib.zamd_zip_open.argtypes = [C.c_char_p]
    lib.zamd_zip_close.argtypes = [C.c_void_p, C.c_char_p]
    lib.zamd_zip_add_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_ulong), C.c_int, C.POINTER(C.c_ulong),
                                       C.POINTER(C.c_char_p)]
    lib.zamd_unzip_read_batch.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_ulong), C.POINTER(C.c_long)]
    lib.zamd_crc32_batch.argtypes = [C.POINTER(C.c_ulong), C.POINTER(C.c_char_p), C.POINTER(C.c_ulong), C.c_size_t]
    lib.zamd_adler32_batch.argtypes = [C.POINTER(C.c_ulong), C.POINTER(C.c_char_p), C.POINTER(C.c_ulong), C.c_size_t]
    return lib


def test_read_batch_without_an_archive(L):
    res = (C.c_long * 1)(7)
    assert L.zamd_unzip_read_batch(None, None, 1, (C.c_void_p * 1)(), (C.c_ulong * 1)(), res) == PARAMERROR
    assert L.zamd_unzip_read_batch(None, None, 0, None, None, None) == PARAMERROR
    assert res[0] == 7


def test_add_batch_of_nothing_leaves_the_file_empty(L, tmp_path):
    p = tmp_path / "e.zip"
    z = L.zamd_zip_open(str(p).encode())
    assert z
    assert L.zamd_zip_add_batch(z, 0, None, None, None, 6, None, None) == 0
    assert L.zamd_zip_add_batch(None, 0, None, None, None, 6, None, None) == PARAMERROR
    assert os.path.getsize(p) == 0
    assert L.zamd_zip_close(z, None) == 0
    assert len(p.read_bytes()) == 22  # the end record alone


def _members(payloads):
    n = len(payloads)
    bufs = [C.create_string_buffer(d, max(len(d), 1)) for d in payloads]
    names = (C.c_char_p * n)(*[b"m%d" % k for k in range(n)])
    data = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_ulong * n)(*[len(d) for d in payloads])
    dates = (C.c_ulong * n)(*[0x32F26459] * n)
    return bufs, names, data, lens, dates


def test_add_batch_checks_every_argument_before_it_writes(L, tmp_path):
    p = tmp_path / "b.zip"
    z = L.zamd_zip_open(str(p).encode())
    keep, names, data, lens, dates = _members([b"abc", b"", b"hello hello hello"])
    assert L.zamd_zip_add_batch(z, 3, names, data, lens, 10, dates, None) == PARAMERROR  # no such level
    assert L.zamd_zip_add_batch(z, 3, names, data, lens, -2, dates, None) == PARAMERROR
    assert L.zamd_zip_add_batch(z, 3, names, None, lens, 6, dates, None) == PARAMERROR
    data[1], lens[1] = None, 5  # a length without bytes, between two valid members
    assert L.zamd_zip_add_batch(z, 3, names, data, lens, 6, dates, None) == PARAMERROR
    lens[1] = 0
    long_name = (C.c_char_p * 3)(b"a", b"x" * 70000, b"c")
    assert L.zamd_zip_add_batch(z, 3, long_name, data, lens, 6, dates, None) == PARAMERROR
    many = 0x10000  # one entry more than the end record counts
    assert L.zamd_zip_add_batch(z, many, (C.c_char_p * many)(), (C.c_void_p * many)(), (C.c_ulong * many)(), 6, (C.c_ulong * many)(), None) == PARAMERROR
    assert os.path.getsize(p) == 0
    assert L.zamd_zip_close(z, None) == 0
    assert len(p.read_bytes()) == 22
    del keep


def test_checksum_batch_arguments(L):
    assert L.zamd_crc32_batch(None, None, None, 0) == 0
    assert L.zamd_adler32_batch(None, None, None, 0) == 0
    val = (C.c_ulong * 1)(5)
    assert L.zamd_crc32_batch(val, None, (C.c_ulong * 1)(3), 1) == -2
    assert L.zamd_adler32_batch(val, (C.c_char_p * 1)(None), (C.c_ulong * 1)(3), 1) == -2  # a length without bytes
    assert val[0] == 5
