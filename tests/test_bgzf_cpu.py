"""BGZF on the host, no GPU: zamd_bgzf_bound, and zamd_bgzf_index (a walk over the block headers) against a header chase in Python on files made
with Python's zlib -- well-formed ones (other subfields, concatenated files, no end block, 1 500 tiny blocks, false headers inside stored
payloads) and files whose blocks do not chain from byte 0 to exactly the end."""
import ctypes as C

import pytest

from tests import bgzf_fixtures as F, zhost


class Block(C.Structure):
    _fields_ = [("coffset", C.c_ulonglong), ("uoffset", C.c_ulonglong)]


@pytest.fixture(scope="module")
def L():
    lib = zhost.lib()
    lib.zamd_bgzf_bound.argtypes = [C.c_ulong]
    lib.zamd_bgzf_bound.restype = C.c_ulong
    lib.zamd_bgzf_index.argtypes = [C.c_char_p, C.c_ulong, C.POINTER(Block), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    return lib


def index(L, f, cap=None):
    n, eof = C.c_size_t(0), C.c_int(-1)
    rc = L.zamd_bgzf_index(f, len(f), None, 0, C.byref(n), C.byref(eof))
    if rc != zhost.Z_BUF_ERROR:
        return rc, None
    blocks = (Block * (n.value + 1))()
    rc = L.zamd_bgzf_index(f, len(f), blocks, n.value + 1 if cap is None else cap, C.byref(n), C.byref(eof))
    return rc, ([b.coffset for b in blocks], [b.uoffset for b in blocks], bool(eof.value))


@pytest.mark.parametrize("n", [0, 1, 65280, 65281, 1 << 20])
def test_bound(L, n):
    assert L.zamd_bgzf_bound(n) >= n + 26 * ((n + 65279) // 65280) + 28


@pytest.mark.parametrize("name", sorted(F.well_formed()))
def test_index_equals_the_chase(L, name):
    f = F.well_formed()[name]
    want = F.chase(f)
    assert want is not None
    rc, got = index(L, f)
    assert rc == zhost.Z_OK
    assert got == want


@pytest.mark.parametrize("name", sorted(F.malformed()))
def test_index_refuses(L, name):
    f = F.malformed()[name]
    assert F.chase(f) is None
    assert index(L, f)[0] == zhost.Z_DATA_ERROR


def test_index_capacity(L):
    f = F.well_formed()["three"]
    rc, _ = index(L, f, cap=4)  # four blocks need five entries
    assert rc == zhost.Z_BUF_ERROR
    n = C.c_size_t(0)
    assert L.zamd_bgzf_index(f, len(f), None, 0, C.byref(n), None) == zhost.Z_BUF_ERROR and n.value == 4


def test_index_agrees_with_the_chase_on_mutated_headers(L):
    verdicts = set()
    for f in F.mutations():
        want = F.chase(f)
        rc, got = index(L, f)
        assert (rc == zhost.Z_OK) == (want is not None)
        if want is not None:
            assert got == want
        verdicts.add(rc)
    assert verdicts == {zhost.Z_OK, zhost.Z_DATA_ERROR}
