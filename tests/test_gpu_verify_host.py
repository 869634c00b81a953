"""The integrity tests of the host library (libzamd_z.so, through ctypes): zamd_uncompress_verify_batch must say of every item what
zamd_uncompress_batch says of it given enough room, zamd_unzip_test_batch what zamd_unzip_read returns member by member, zamd_bgzf_test what
zamd_bgzf_uncompress returns -- none of them with room for a decoded byte."""
import ctypes as C
import struct
import zlib

import pytest

from oracle import cases

pytestmark = pytest.mark.gpu
CRCERROR = -105


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 512), ("crc32", C.c_ulong), ("compressed_size", C.c_ulong), ("uncompressed_size", C.c_ulong), ("dos_date", C.c_ulong),
                ("local_header_offset", C.c_ulong), ("method", C.c_int), ("flag", C.c_int), ("internal_fa", C.c_int)]


@pytest.fixture(scope="module")
def L():
    from tests import zhost
    lib = zhost.lib()
    P, U = C.POINTER(C.c_void_p), C.POINTER(C.c_ulong)
    lib.zamd_uncompress_batch.argtypes = [P, U, P, U, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    lib.zamd_uncompress_verify_batch.argtypes = [U, P, U, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    lib.zamd_zip_open.restype = C.c_void_p
    lib.zamd_zip_open.argtypes = [C.c_char_p]
    lib.zamd_zip_add_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p), P, U, C.c_int, U, C.POINTER(C.c_char_p)]
    lib.zamd_zip_close.argtypes = [C.c_void_p, C.c_char_p]
    lib.zamd_unzip_open.restype = C.c_void_p
    lib.zamd_unzip_open.argtypes = [C.c_char_p]
    lib.zamd_unzip_count.argtypes = [C.c_void_p]
    lib.zamd_unzip_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(Entry)]
    lib.zamd_unzip_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_ulong]
    lib.zamd_unzip_read.restype = C.c_long
    lib.zamd_unzip_test_batch.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_long)]
    lib.zamd_unzip_close.argtypes = [C.c_void_p]
    lib.zamd_bgzf_bound.argtypes = [C.c_ulong]
    lib.zamd_bgzf_bound.restype = C.c_ulong
    lib.zamd_bgzf_compress.argtypes = [C.c_char_p, U, C.c_char_p, C.c_ulong, C.c_int]
    lib.zamd_bgzf_uncompress.argtypes = [C.c_char_p, U, C.c_char_p, C.c_ulong]
    lib.zamd_bgzf_test.argtypes = [C.c_char_p, C.c_ulong, U]
    return lib


def _flip(s, at, bit=0x10):
    at %= len(s)
    return s[:at] + bytes([s[at] ^ bit]) + s[at + 1:]


@pytest.mark.parametrize("wbits", [15, 31, 47, -15])
def test_uncompress_verify_batch(L, wbits):
    from tests import zhost
    datas = [cases.make("mix", n, 60 + i) for i, n in enumerate((0, 1, 100, 4096, 65536, 200000, 3000))]

    def stream(d, k):
        w = wbits if wbits != 47 else (15, 31)[k & 1]
        c = zlib.compressobj(6 if k != 4 else 0, zlib.DEFLATED, w)
        return c.compress(d) + c.flush()
    zs = [stream(d, k) for k, d in enumerate(datas)]
    sizes = [len(d) for d in datas]
    zs += [zs[5][: len(zs[5]) // 2], _flip(zs[3], len(zs[3]) // 2), zs[6] + b"junk"]  # cut, damaged inside, good with bytes behind it
    sizes += [200000, 4096, 3000]
    if wbits != -15:  # trailers: a byte of the check value; a stored payload byte, the deflate data still valid
        zs += [_flip(zs[5], -3), _flip(zs[4], len(zs[4]) // 2), zs[2][:-1]]
        sizes += [200000, 65536, 100]
    n = len(zs)
    src = [C.create_string_buffer(z, max(len(z), 1)) for z in zs]
    sizes = [2 * s + (1 << 20) for s in sizes]  # enough room, also for what a damaged stream may decode to before it fails
    dst = [C.create_string_buffer(s) for s in sizes]
    PA = C.c_void_p * n
    sp, sl = PA(*[C.addressof(x) for x in src]), (C.c_ulong * n)(*[len(z) for z in zs])
    dp, dl, st = PA(*[C.addressof(x) for x in dst]), (C.c_ulong * n)(*sizes), (C.c_int * n)()
    want_rc = L.zamd_uncompress_batch(dp, dl, sp, sl, n, wbits, st)
    want = [(st[k], dl[k] if st[k] == zhost.Z_OK else 0) for k in range(n)]
    assert {c for c, _ in want} == {zhost.Z_OK, zhost.Z_DATA_ERROR} and [c for c, _ in want[:7]] == [zhost.Z_OK] * 7
    vl, vs = (C.c_ulong * n)(*([12345] * n)), (C.c_int * n)(*([9] * n))
    rc = L.zamd_uncompress_verify_batch(vl, sp, sl, n, wbits, vs)
    assert [(vs[k], vl[k]) for k in range(n)] == want and rc == want_rc == zhost.Z_DATA_ERROR
    vs2 = (C.c_int * n)(*([9] * n))
    assert L.zamd_uncompress_verify_batch(None, sp, sl, n, wbits, vs2) == rc and list(vs2) == list(vs)  # the sizes are optional


def _add(L, z, members, level):
    n = len(members)
    bufs = [C.create_string_buffer(d, max(len(d), 1)) for _, d in members]
    names = (C.c_char_p * n)(*[nm.encode() for nm, _ in members])
    data = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_ulong * n)(*[len(d) for _, d in members])
    dates = (C.c_ulong * n)(*([0x5A8F6B2C] * n))
    assert L.zamd_zip_add_batch(z, n, names, data, lens, level, dates, None) == 0


def _read_and_test(L, path):
    """member by member through zamd_unzip_read; all of them through one zamd_unzip_test_batch, in order and in a shuffled order with repeats"""
    u = L.zamd_unzip_open(str(path).encode())
    assert u
    n = L.zamd_unzip_count(u)
    one = []
    for i in range(n):
        e = Entry()
        assert L.zamd_unzip_stat(u, i, C.byref(e)) == 0
        buf = C.create_string_buffer(max(e.uncompressed_size, 1))
        one.append(L.zamd_unzip_read(u, i, buf, e.uncompressed_size))
    res = (C.c_long * n)(*([77] * n))
    rc = L.zamd_unzip_test_batch(u, None, n, res)
    order = [(7 * k + 3) % n for k in range(n)] + [0, n - 1, 0]
    idx, res2 = (C.c_int * len(order))(*order), (C.c_long * len(order))()
    rc2 = L.zamd_unzip_test_batch(u, idx, len(order), res2)
    L.zamd_unzip_close(u)
    assert list(res2) == [res[i] for i in order] and rc2 == next((r for r in res2 if r < 0), 0)
    return one, rc, list(res)


def test_unzip_test_batch(L, tmp_path):
    deflated = [("d%d" % i, cases.make(k, n, 70 + i)) for i, (k, n) in enumerate([("text", 5000), ("mix", 70000), ("zeros", 40000), ("text", 0), ("rand", 900), ("mix", 200000)])]
    stored = [("s%d" % i, cases.make("rand", n, 80 + i)) for i, n in enumerate((13, 5000, 70000))]
    path = tmp_path / "a.zip"
    z = L.zamd_zip_open(str(path).encode())
    assert z
    _add(L, z, deflated[:3], 6)
    _add(L, z, stored, 0)
    _add(L, z, deflated[3:], 9)
    assert L.zamd_zip_close(z, None) == 0
    members = deflated[:3] + stored + deflated[3:]
    one, rc, res = _read_and_test(L, path)
    assert one == [len(d) for _, d in members] and res == one and rc == 0
    # a second copy: a data byte of one deflated member (d1) and of one stored member (s1) flipped
    raw = path.read_bytes()

    def body(i):  # where member i's data starts: behind its local header, name and extra field
        u = L.zamd_unzip_open(str(path).encode())
        e = Entry()
        assert u and L.zamd_unzip_stat(u, i, C.byref(e)) == 0
        L.zamd_unzip_close(u)
        lh = e.local_header_offset
        assert raw[lh: lh + 4] == b"PK\x03\x04"
        return lh + 30 + struct.unpack("<HH", raw[lh + 26: lh + 30])[0] + struct.unpack("<HH", raw[lh + 26: lh + 30])[1]
    at_d, at_s = body(1) + 200, body(4) + 100
    assert raw[at_s - 100: at_s] == stored[1][1][:100]
    bad = tmp_path / "b.zip"
    bad.write_bytes(_flip(_flip(raw, at_d), at_s))
    one, rc, res = _read_and_test(L, bad)
    assert res == one and one[1] < 0 and one[4] == CRCERROR and rc == one[1]
    assert [r for k, r in enumerate(res) if k not in (1, 4)] == [len(d) for k, (_, d) in enumerate(members) if k not in (1, 4)]


def test_bgzf_test(L):
    from tests import zhost
    data = cases.make("text", 3 * 65280 + 999, 12)
    cap = C.c_ulong(L.zamd_bgzf_bound(len(data)))
    out = C.create_string_buffer(cap.value)
    assert L.zamd_bgzf_compress(out, C.byref(cap), data, len(data), 6) == zhost.Z_OK
    f = out.raw[: cap.value]
    # block 1's header: where its body starts and where its trailer lies
    b1 = struct.unpack("<H", f[16:18])[0] + 1
    b2 = b1 + struct.unpack("<H", f[b1 + 16: b1 + 18])[0] + 1
    files = [f, f[:-28], _flip(f, b1 + 18 + 300), _flip(f, b2 - 6), f[:b2 - 4] + struct.pack("<I", 65279) + f[b2:], f[:-3], b"not a bgzf file at all......"]
    for k, g in enumerate(files):
        n, room = C.c_ulong(len(data)), C.create_string_buffer(len(data))
        want = L.zamd_bgzf_uncompress(room, C.byref(n), g, len(g))
        got_n = C.c_ulong(7)
        got = L.zamd_bgzf_test(g, len(g), C.byref(got_n))
        assert got == want and want == (zhost.Z_OK if k < 2 else zhost.Z_DATA_ERROR), (k, got, want)
        assert got_n.value == (len(data) if k < 2 else 7), k
    assert L.zamd_bgzf_test(f, len(f), None) == zhost.Z_OK
