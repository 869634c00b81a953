"""ZIP archives in batches (include/zamd_zip_batch.h): zamd_zip_add_batch must write, byte for byte, the archive zamd_zip_add writes member by member
(and so the reference's minizip archives of tests/golden/zip_kat.json); zamd_unzip_read_batch must give, member by member, what zamd_unzip_read
gives -- the bytes, and for damaged archives the codes -- without one bad member disturbing another."""
import base64
import ctypes as C
import io
import json
import os
import random
import zipfile

import pytest

from oracle import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "zip_kat.json")))
PARAMERROR, BADZIPFILE, CRCERROR = -102, -103, -105


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 512), ("crc32", C.c_ulong), ("compressed_size", C.c_ulong), ("uncompressed_size", C.c_ulong), ("dos_date", C.c_ulong),
                ("local_header_offset", C.c_ulong), ("method", C.c_int), ("flag", C.c_int), ("internal_fa", C.c_int)]


@pytest.fixture(scope="module")
def L():
    from tests import zhost
    lib = zhost.lib()
    lib.zamd_zip_open.restype = C.c_void_p
    lib.zamd_zip_open.argtypes = [C.c_char_p]
    lib.zamd_zip_add.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_ulong, C.c_int, C.c_ulong, C.c_char_p]
    lib.zamd_zip_add_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_ulong), C.c_int, C.POINTER(C.c_ulong),
                                       C.POINTER(C.c_char_p)]
    lib.zamd_zip_close.argtypes = [C.c_void_p, C.c_char_p]
    lib.zamd_unzip_open.restype = C.c_void_p
    lib.zamd_unzip_open.argtypes = [C.c_char_p]
    lib.zamd_unzip_count.argtypes = [C.c_void_p]
    lib.zamd_unzip_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(Entry)]
    lib.zamd_unzip_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_ulong]
    lib.zamd_unzip_read.restype = C.c_long
    lib.zamd_unzip_read_batch.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_ulong), C.POINTER(C.c_long)]
    lib.zamd_unzip_close.argtypes = [C.c_void_p]
    return lib


def write_batch(L, path, members, level, dates, comments=None, split=None):
    """members: (name, data); one zamd_zip_add_batch call, or two cut at `split`"""
    z = L.zamd_zip_open(str(path).encode())
    assert z
    for lo, hi in ([(0, len(members))] if split is None else [(0, split), (split, len(members))]):
        part = members[lo:hi]
        n = len(part)
        bufs = [C.create_string_buffer(d, max(len(d), 1)) for _, d in part]
        names = (C.c_char_p * n)(*[nm.encode() for nm, _ in part])
        data = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        lens = (C.c_ulong * n)(*[len(d) for _, d in part])
        dd = (C.c_ulong * n)(*dates[lo:hi])
        cc = (C.c_char_p * n)(*comments[lo:hi]) if comments else None
        assert L.zamd_zip_add_batch(z, n, names, data, lens, level, dd, cc) == 0
    assert L.zamd_zip_close(z, None) == 0
    return open(path, "rb").read()


def write_one_by_one(L, path, members, level, dates, comments=None):
    z = L.zamd_zip_open(str(path).encode())
    assert z
    for k, (name, data) in enumerate(members):
        assert L.zamd_zip_add(z, name.encode(), data, len(data), level, dates[k], comments[k] if comments else None) == 0
    assert L.zamd_zip_close(z, None) == 0
    return open(path, "rb").read()


def read_one_by_one(L, path):
    """[(code or size, bytes)] through zamd_unzip_read"""
    u = L.zamd_unzip_open(str(path).encode())
    assert u
    out = []
    for i in range(L.zamd_unzip_count(u)):
        e = Entry()
        assert L.zamd_unzip_stat(u, i, C.byref(e)) == 0
        buf = C.create_string_buffer(max(e.uncompressed_size, 1))
        n = L.zamd_unzip_read(u, i, buf, e.uncompressed_size)
        out.append((n, buf.raw[: max(n, 0)]))
    L.zamd_unzip_close(u)
    return out


def read_batch(L, path, index=None, caps=None):
    """(return value, [(code or size, bytes)]) through one zamd_unzip_read_batch; caps: {item: room} instead of the directory's size"""
    u = L.zamd_unzip_open(str(path).encode())
    assert u
    count = L.zamd_unzip_count(u)
    idx = list(range(count)) if index is None else index
    n = len(idx)
    sizes = []
    for i in idx:
        e = Entry()
        assert L.zamd_unzip_stat(u, i, C.byref(e)) == 0
        sizes.append(e.uncompressed_size)
    room = [(caps or {}).get(k, sizes[k]) for k in range(n)]
    bufs = [C.create_string_buffer(b"\xa5" * max(r, 1), max(r, 1)) for r in room]
    out = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    cap = (C.c_ulong * n)(*room)
    res = (C.c_long * n)(*[12345] * n)
    rc = L.zamd_unzip_read_batch(u, None if index is None else (C.c_int * n)(*idx), n, out, cap, res)
    L.zamd_unzip_close(u)
    return rc, [(res[k], bufs[k].raw[: max(res[k], 0)]) for k in range(n)]


@pytest.fixture(scope="module")
def kat_members():
    return [(name, cases.make(kind, n, seed)) for name, kind, n, seed in KAT["members"]]


@pytest.mark.parametrize("arc", KAT["archives"], ids=lambda a: "L%d" % a["level"])
def test_batch_writer_matches_the_reference_minizip(L, arc, kat_members, tmp_path):
    got = write_batch(L, tmp_path / "t.zip", kat_members, arc["level"], [arc["dos_date"]] * len(kat_members))
    assert got == base64.b64decode(arc["zip_b64"])


@pytest.fixture(scope="module")
def mixed_members():
    rnd = random.Random(7301)
    members = [("big.txt", cases.make("text", 3 * 65536 + 17, 21)), ("over.mix", cases.make("mix", 65537, 22)), ("empty", b""), ("tiny", b"x")]
    members += [("m/%02d.%s" % (i, k), cases.make(k, rnd.randint(1, 5000), 50 + i)) for i, k in enumerate(cases.KINDS * 6) if i < 40]
    dates = [0x32F26459 + 0x10000 * i for i in range(len(members))]
    comments = [(b"member %d" % i) if i % 3 == 0 else None for i in range(len(members))]
    return members, dates, comments


@pytest.fixture(scope="module")
def mixed_archive(L, mixed_members, tmp_path_factory):
    members, dates, comments = mixed_members
    return write_one_by_one(L, tmp_path_factory.mktemp("zipb") / "one.zip", members, 6, dates, comments)


def test_mixed_archive_equals_the_member_by_member_writer(L, mixed_members, mixed_archive, tmp_path):
    members, dates, comments = mixed_members
    assert len(members) == 44
    got = write_batch(L, tmp_path / "batch.zip", members, 6, dates, comments)
    assert got == mixed_archive
    assert write_batch(L, tmp_path / "two.zip", members, 6, dates, comments, split=7) == mixed_archive  # offsets carry over from call to call
    zf = zipfile.ZipFile(io.BytesIO(got))
    assert zf.testzip() is None
    for name, data in members:
        assert zf.read(name) == data


def test_default_level_and_stored_members_of_any_size(L, mixed_members, tmp_path):
    members, dates, _ = mixed_members
    for level in (-1, 0):
        assert write_batch(L, tmp_path / "b.zip", members[:8], level, dates[:8]) == write_one_by_one(L, tmp_path / "o.zip", members[:8], level, dates[:8])


@pytest.mark.parametrize("arc", KAT["archives"], ids=lambda a: "L%d" % a["level"])
def test_batch_reader_reads_the_reference_archives(L, arc, kat_members, tmp_path):
    p = tmp_path / "ref.zip"
    p.write_bytes(base64.b64decode(arc["zip_b64"]))
    rc, got = read_batch(L, p)
    assert rc == 0 and got == [(len(d), d) for _, d in kat_members]
    index = [5, 0, 3, 3, 2, 1, 0, 4, 5, 5]
    rc, got = read_batch(L, p, index=index)
    assert rc == 0 and got == [(len(kat_members[i][1]), kat_members[i][1]) for i in index]


@pytest.fixture(scope="module")
def foreign(tmp_path_factory):
    """a Python-zipfile archive: deflated and stored members, an empty one, 70 000 random bytes stored"""
    members = [("f1", cases.make("text", 300000, 31)), ("f2", cases.make("rand", 70000, 32)), ("f3", b""), ("f4", cases.make("runs", 200000, 33)),
               ("f5", cases.make("text", 900, 34)), ("f6", b"stored, short")]
    p = tmp_path_factory.mktemp("zipf") / "py.zip"
    with zipfile.ZipFile(p, "w", zipfile.ZIP_DEFLATED, compresslevel=7) as zf:
        for name, data in members:
            zf.writestr(zipfile.ZipInfo(name, (2005, 7, 18, 12, 34, 56)), data, zipfile.ZIP_STORED if name in ("f2", "f6") else zipfile.ZIP_DEFLATED)
    return p, members


def test_batch_reader_reads_a_foreign_archive(L, foreign):
    p, members = foreign
    rc, got = read_batch(L, p)
    assert rc == 0 and got == [(len(d), d) for _, d in members]
    index = [3, 1, 1, 0, 5, 2, 4, 3]
    rc, got = read_batch(L, p, index=index)
    assert rc == 0 and got == [(len(members[i][1]), members[i][1]) for i in index]


def _damage(raw, what):
    raw = bytearray(raw)
    cd = [i for i in range(len(raw) - 4) if raw[i:i + 4] == b"PK\x01\x02"]  # (f2's stored random bytes could hold the magic: the last six are the directory)
    cd = cd[-6:]
    if what == "crc":  # a CRC bit in the directory of f1 (deflated) and of f2 (stored)
        raw[cd[0] + 16] ^= 1
        raw[cd[1] + 16] ^= 1
    elif what == "compressed_size":
        raw[cd[0] + 20:cd[0] + 24] = (0xFFFFFF00).to_bytes(4, "little")
    elif what == "uncompressed_size":
        raw[cd[0] + 24:cd[0] + 28] = (100).to_bytes(4, "little")
    elif what == "body":  # one byte in the middle of f4's deflate data
        lh = int.from_bytes(raw[cd[3] + 42:cd[3] + 46], "little")
        csize = int.from_bytes(raw[cd[3] + 20:cd[3] + 24], "little")
        body = lh + 30 + int.from_bytes(raw[lh + 26:lh + 28], "little") + int.from_bytes(raw[lh + 28:lh + 30], "little")
        raw[body + csize // 2] ^= 0x40
    return bytes(raw)


@pytest.mark.parametrize("what", ["crc", "compressed_size", "uncompressed_size", "body"])
def test_damaged_archives_get_the_member_by_member_codes(L, foreign, what, tmp_path):
    p, members = foreign
    bad = tmp_path / "bad.zip"
    bad.write_bytes(_damage(p.read_bytes(), what))
    want = read_one_by_one(L, bad)
    rc, got = read_batch(L, bad)
    size_lie = what in ("compressed_size", "uncompressed_size")
    damaged = {"crc": (0, 1), "compressed_size": (0,), "uncompressed_size": (0,), "body": (3,)}[what]
    for k, ((wn, wd), (gn, gd)) in enumerate(zip(want, got)):
        if k in damaged:
            assert wn < 0 and gn < 0, (k, wn, gn)
            assert gn == wn or (size_lie and {gn, wn} <= {BADZIPFILE, CRCERROR}), (k, wn, gn)
        else:
            assert (gn, gd) == (len(members[k][1]), members[k][1]) == (wn, wd), k
    assert rc == next(gn for gn, _ in got if gn < 0)
    if what == "crc":
        assert [got[0][0], got[1][0]] == [CRCERROR, CRCERROR]
    if what == "compressed_size":
        assert got[0][0] == BADZIPFILE


def test_room_too_small_is_that_items_error_alone(L, foreign):
    p, members = foreign
    index = [0, 4, 1, 4]
    rc, got = read_batch(L, p, index=index, caps={1: 899, 2: 10})
    assert rc == PARAMERROR
    assert [g[0] for g in got] == [len(members[0][1]), PARAMERROR, PARAMERROR, len(members[4][1])]
    assert got[0][1] == members[0][1] and got[3][1] == members[4][1]
    u = L.zamd_unzip_open(str(p).encode())
    res = (C.c_long * 1)(12345)
    buf = C.create_string_buffer(16)
    assert L.zamd_unzip_read_batch(u, (C.c_int * 1)(99), 1, (C.c_void_p * 1)(C.addressof(buf)), (C.c_ulong * 1)(16), res) == PARAMERROR and res[0] == PARAMERROR
    assert L.zamd_unzip_read_batch(u, None, 1, None, (C.c_ulong * 1)(16), res) == PARAMERROR
    assert L.zamd_unzip_read_batch(u, None, 0, None, None, None) == 0
    L.zamd_unzip_close(u)
