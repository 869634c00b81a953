"""Multi-member gzip on the GPU (zgpu_gzip_inflate_*, zamd_gunzip): all members of a file in one batch.  The oracle is Python's zlib, member by
member (decompressobj(31) over unused_data), recording every member's extent in the file and in the decoded bytes.  Plain files (one pass), files
with gzip signatures inside stored payloads (false candidates: a second pass at most), damaged members, trailing bytes, capacities, the project's own
multi-member producers, and the zlib-style host call."""
import ctypes as C
import functools
import random
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cases  # noqa: E402
from tests import bgzf_fixtures as F, zhost  # noqa: E402

OK, DATA_ERROR, BUF_ERROR = 0, -3, -5


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def L():
    lib = zhost.lib()
    U = C.POINTER(C.c_ulong)
    lib.zamd_gunzip.argtypes = [C.c_char_p, U, C.c_char_p, C.c_ulong, U, U]
    return lib


# ---- files and the oracle ----
def member(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def member_with_fields(data, level=6):
    """a member whose header carries FEXTRA, FNAME, FCOMMENT and FHCRC, built by hand"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    head = bytes([0x1F, 0x8B, 8, 2 | 4 | 8 | 16, 1, 2, 3, 4, 0, 3]) + struct.pack("<H", 6) + b"ab\x02\x00xy" + b"name.txt\0" + b"a comment\0"
    head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data))


def is_candidate(f, p):
    return len(f) - p >= 4 and f[p: p + 3] == b"\x1f\x8b\x08" and not f[p + 3] & 0xE0


def candidates(f):
    return [p for p in range(len(f)) if f[p] == 0x1F and is_candidate(f, p)]


def walk(f):
    """(members [(in_lo, in_hi, data)], bad): the members gzread() would deliver; bad = a member on the chain failed (it begins where the last ends)"""
    pos, out = 0, []
    while pos < len(f) and is_candidate(f, pos):
        d = zlib.decompressobj(31)
        try:
            data = d.decompress(f[pos:])
        except zlib.error:
            return out, True
        if not d.eof:
            return out, True
        end = len(f) - len(d.unused_data)
        out.append((pos, end, data))
        pos = end
    return out, False


def tables(members):
    io = [m[0] for m in members] + [members[-1][1] if members else 0]
    oo = [0]
    for m in members:
        oo.append(oo[-1] + len(m[2]))
    return io, oo


def small_pieces(n, seed):
    rng = random.Random(seed)
    base = cases.make("text", 64 * 1024, 7)
    out = []
    for k in range(n):
        ln = 0 if k % 7 == 3 else rng.randrange(0, 301)
        at = rng.randrange(0, len(base) - 300)
        out.append(base[at: at + ln])
    return out


@functools.lru_cache(maxsize=None)
def plain_files():
    far = cases.make("rand", 20 * 1024, 3) * 10  # 200 KiB: more than one 64 KiB checksum piece, matches at distance 20 KiB (beyond the 8 KiB ring)
    mix = cases.make("mix", 3000, 5)
    files = {
        "one": member(cases.make("text", 250, 1)),
        "three": b"".join(member(p, lv) for p, lv in zip([cases.make("text", 300, 2), b"", cases.make("mix", 120, 3)], (1, 6, 9))),
        "thousand": b"".join(member(p, 1 + k % 9) for k, p in enumerate(small_pieces(1000, 11))),
        "far": member(mix) + member(far, 6) + member(mix[:1000], 9),
        "fields": member_with_fields(mix) + member(b"") + member_with_fields(b"", 1) + member_with_fields(mix[:77], 9),
    }
    for name, f in files.items():  # (the premise of "one pass": nothing in these files looks like a header but the members' own)
        assert candidates(f) == [m[0] for m in walk(f)[0]], name
    return files


def host_decode(eng, f, out_cap=None, cap_members=None):
    rc, data, io, oo, items = eng.gzip_inflate_host(f, out_cap=out_cap, cap_members=cap_members)
    return rc, data, io, oo, items, eng.last_members, eng.last_inflate


def device_decode(eng, f, out_cap, cap_members=None):
    import torch
    import zlib_amd.gpu as G
    dev = torch.device("cuda", 0)
    cm = len(f) // 20 if cap_members is None else cap_members
    d_in = torch.tensor(np.frombuffer(f + b"\0", dtype=np.uint8), device=dev)
    d_out = torch.zeros(out_cap + 1, dtype=torch.uint8, device=dev)
    d_io = torch.zeros(cm + 1, dtype=torch.int64, device=dev)
    d_oo = torch.zeros(cm + 1, dtype=torch.int64, device=dev)
    d_items = torch.zeros((cm + 1) * C.sizeof(G.InflateItem), dtype=torch.uint8, device=dev)
    rc, nm, res = eng.gzip_inflate_device(d_in.data_ptr(), len(f), d_out.data_ptr(), out_cap, d_io.data_ptr(), d_oo.data_ptr(), d_items.data_ptr(), cm)
    if rc not in (OK, DATA_ERROR) or nm > cm:
        return rc, b"", [], [], [], nm, res
    raw = d_items.cpu().numpy().tobytes()
    items = [G.InflateItem.from_buffer_copy(raw, k * C.sizeof(G.InflateItem)) for k in range(nm)]
    return rc, d_out[: res.out_bytes].cpu().numpy().tobytes(), [int(x) for x in d_io[: nm + 1].cpu()], [int(x) for x in d_oo[: nm + 1].cpu()], items, nm, res


def check_good(got, f):
    """a decode that succeeded, against the oracle: bytes, both tables, every member's record"""
    members, bad = walk(f)
    assert not bad
    rc, data, io, oo, items, nm, res = got
    assert rc == OK and nm == len(members)
    assert data == b"".join(m[2] for m in members)
    assert (io, oo) == tables(members)
    assert res.out_bytes == len(data) and res.in_used == (members[-1][1] if members else 0) and res.first_bad_chunk == -1
    for k, (lo, hi, d) in enumerate(members):
        it = items[k]
        assert (it.code, it.out_bytes, it.in_used, it.crc32) == (OK, len(d), hi - lo, zlib.crc32(d)), k


# ---- 1. plain files: every member decoded once ----
@pytest.mark.parametrize("name", ["one", "three", "thousand", "far", "fields"])
def test_plain_files_take_one_pass(eng, name):
    f = plain_files()[name]
    total = sum(len(m[2]) for m in walk(f)[0])
    before = eng.gzip_members_count()
    check_good(host_decode(eng, f, out_cap=total), f)
    assert eng.gzip_members_count() == (before[0] + 1, before[1])
    check_good(device_decode(eng, f, total), f)
    assert eng.gzip_members_count() == (before[0] + 2, before[1])


# ---- 2. false candidates ----
def stored(payload):
    return member(payload, 0)


@functools.lru_cache(maxsize=None)
def decoy_file():
    text = cases.make("text", 4000, 21)
    inner = member(b"a complete member held as payload " * 9, 6)
    parts = [
        member(text[:700]),
        stored(b"front " + inner + b" back"),                             # a complete valid member inside a stored block
        member(text[700:1500], 9),
        stored(b"junk follows " + b"\x1f\x8b\x08\x00" + bytes(range(40, 90))),  # a header and then nothing that decodes
        member(b""),
        stored(b"no candidate " + b"\x1f\x8b\x08\xe0" + b"reserved flag bits"),
        member(text[1500:2600], 1),
        member_with_fields(text[2600:3000]),
        member(text[3000:], 6),
        stored(b"the last member " * 5 + b"\x1f\x8b\x08\x04" + b"zz"),      # 14 bytes in front of the file's end: its header runs into the end
    ]
    f = b"".join(parts)
    members = walk(f)[0]
    starts = [m[0] for m in members]
    assert len(members) == len(parts) and len(f) - candidates(f)[-1] == 14
    assert len(candidates(f)) == len(parts) + 3 and f.index(inner) not in starts
    return f


@functools.lru_cache(maxsize=None)
def plausible_decoy_file():
    """the planted signature's neighbourhood makes both wrong guesses nonzero and plausible: the word in front of it (the guess of the member that
    holds it) says 50, and it is far enough from the next member for that member's ISIZE to be taken as its own"""
    text = cases.make("text", 3000, 22)
    payload = b"A" * 96 + struct.pack("<I", 50) + b"\x1f\x8b\x08\x00" + b"B" * 60
    f = member(text[:900]) + stored(payload) + member(text[900:2000], 9) + member(text[2000:], 1)
    assert len(walk(f)[0]) == 4 and len(candidates(f)) == 5
    return f


def test_false_candidates_are_no_members(eng):
    f = decoy_file()
    total = sum(len(m[2]) for m in walk(f)[0])
    for decode in (lambda: host_decode(eng, f, out_cap=total), lambda: device_decode(eng, f, total)):
        before = eng.gzip_members_count()
        check_good(decode(), f)
        after = eng.gzip_members_count()
        assert sum(after) == sum(before) + 1


def test_plausible_wrong_guess_takes_the_second_pass(eng):
    f = plausible_decoy_file()
    total = sum(len(m[2]) for m in walk(f)[0])
    for decode in (lambda: host_decode(eng, f, out_cap=total), lambda: device_decode(eng, f, total)):
        before = eng.gzip_members_count()
        check_good(decode(), f)
        assert eng.gzip_members_count() == (before[0], before[1] + 1)


# ---- 3. verdicts ----
@functools.lru_cache(maxsize=None)
def ten():
    text = cases.make("text", 20000, 23)
    parts = [member(text[2000 * k: 2000 * k + 1000 + 97 * k], 1 + k % 9) for k in range(10)]
    starts = [0]
    for p in parts:
        starts.append(starts[-1] + len(p))
    return parts, starts


@functools.lru_cache(maxsize=None)
def damaged_files():
    """name -> (file, the failed member, its message or None when the decoder's own text is not pinned)"""
    parts, starts = ten()
    good = b"".join(parts)

    def with5(p5):
        return b"".join(parts[:5]) + p5 + b"".join(parts[6:])
    p5 = parts[5]
    mid = 10 + (len(p5) - 18) // 2
    crc, isize = struct.unpack("<II", p5[-8:])
    return {
        "data": (with5(p5[:mid] + bytes([p5[mid] ^ 0x55]) + p5[mid + 1:]), 5, None),
        "crc": (with5(p5[:-8] + struct.pack("<II", crc ^ 0x100, isize)), 5, "incorrect data check"),
        "isize_up": (with5(p5[:-4] + struct.pack("<I", isize + 1)), 5, "incorrect length check"),
        "isize_down": (with5(p5[:-4] + struct.pack("<I", isize - 1)), 5, "incorrect length check"),
        "cut": (good[: starts[9] + len(parts[9]) // 2], 9, None),
    }


@pytest.mark.parametrize("name", ["data", "crc", "isize_up", "isize_down", "cut"])
def test_a_damaged_member_ends_the_file(eng, name):
    f, k, msg = damaged_files()[name]
    parts, starts = ten()
    members, bad = walk(f)
    assert bad and len(members) == k and [m[0] for m in members] == starts[:k]
    want = b"".join(m[2] for m in members)
    for got in (host_decode(eng, f, out_cap=30000), device_decode(eng, f, 30000)):
        rc, data, io, oo, items, nm, res = got
        assert rc == DATA_ERROR and nm == k
        assert (res.first_bad_chunk, res.error_code, res.out_bytes, res.in_used) == (k, DATA_ERROR, len(want), starts[k])
        assert res.error_msg != 0
        if msg:
            assert eng.L.zgpu_inflate_message(res.error_msg).decode() == msg
        assert data == want
        assert (io, oo) == (starts[: k + 1], tables(members)[1])
        for j, (lo, hi, d) in enumerate(members):
            assert (items[j].code, items[j].out_bytes, items[j].in_used, items[j].crc32) == (OK, len(d), hi - lo, zlib.crc32(d)), j


def test_bytes_behind_the_last_member_are_ignored(eng):
    parts, starts = ten()
    good = b"".join(parts)
    f = good + bytes(512)
    for got in (host_decode(eng, f, out_cap=30000), device_decode(eng, f, 30000)):
        check_good(got, f)
        assert got[6].in_used == len(good) < len(f)


def test_a_file_that_begins_with_no_member(eng):
    parts, _ = ten()
    f = b"\x1f\x8b\x07" + b"".join(parts)[3:]
    for got in (host_decode(eng, f, out_cap=30000), device_decode(eng, f, 30000)):
        rc, data, io, oo, items, nm, res = got
        assert rc == DATA_ERROR and nm == 0 and data == b""
        assert (res.first_bad_chunk, res.out_bytes, res.in_used) == (0, 0, 0)
        assert eng.L.zgpu_inflate_message(res.error_msg) == b"incorrect header check"


# ---- 4. capacities ----
def test_capacities(eng):
    f = plain_files()["far"]
    members = walk(f)[0]
    total = sum(len(m[2]) for m in members)
    for decode in (host_decode, lambda e, g, out_cap, cap_members=None: device_decode(e, g, out_cap, cap_members)):
        rc, *_, res = decode(eng, f, out_cap=total - 1)
        assert rc == BUF_ERROR and res.out_bytes == total
        check_good(decode(eng, f, out_cap=total), f)
        rc, data, io, oo, items, nm, res = decode(eng, f, out_cap=total, cap_members=len(members) - 1)
        assert rc == BUF_ERROR and nm == len(members)
        check_good(decode(eng, f, out_cap=total, cap_members=len(members)), f)
    # the file with false candidates, one byte short: the size needed is still exact
    g = decoy_file()
    gtotal = sum(len(m[2]) for m in walk(g)[0])
    rc, *_, res = host_decode(eng, g, out_cap=gtotal - 1)
    assert rc == BUF_ERROR and res.out_bytes == gtotal
    check_good(host_decode(eng, g), g)  # (out_cap=None: asks for the size with no room, then decodes)


def test_empty_input(eng):
    for got in (host_decode(eng, b"", out_cap=0), device_decode(eng, b"", 0, cap_members=0)):
        rc, data, io, oo, items, nm, res = got
        assert (rc, nm, data, res.out_bytes, res.in_used) == (OK, 0, b"", 0, 0)
        assert (io, oo) == ([0], [0])


# ---- 5. the project's own multi-member producers ----
@pytest.mark.parametrize("name", ["three", "concat"])
def test_a_bgzf_file_is_multi_member_gzip(eng, name):
    f = F.well_formed()[name]
    rc, want, _ = eng.bgzf_inflate_host(f)
    assert rc == OK
    got = host_decode(eng, f)
    check_good(got, f)
    assert got[1] == want and got[2] == F.chase(f)[0]


def test_gzip_segments_read_back(eng):
    base = cases.make("mix", 64 * 3000, 31)
    bufs = [base[3000 * k: 3000 * k + 1 + (k * 613) % 2999] for k in range(64)]
    f = b"".join(eng.deflate_batch_host(bufs, 6, wrap="gzip"))
    got = host_decode(eng, f)
    assert got[0] == OK and got[5] == 64 and got[1] == b"".join(bufs)
    check_good(got, f)


# ---- 6. the host library ----
def _gunzip(L, f, cap):
    n, used, members = C.c_ulong(cap), C.c_ulong(0), C.c_ulong(0)
    out = C.create_string_buffer(max(cap, 1))
    rc = L.zamd_gunzip(out, C.byref(n), f, len(f), C.byref(used), C.byref(members))
    return rc, n.value, used.value, members.value, out.raw[: n.value] if rc in (zhost.Z_OK, zhost.Z_DATA_ERROR) else b""


def test_zamd_gunzip(eng, L):
    f = plain_files()["thousand"]
    members = walk(f)[0]
    want = b"".join(m[2] for m in members)
    assert _gunzip(L, f, len(want)) == (zhost.Z_OK, len(want), len(f), 1000, want)
    assert _gunzip(L, f, len(want) - 1)[:2] == (zhost.Z_BUF_ERROR, len(want))
    n = C.c_ulong(len(want))
    out = C.create_string_buffer(len(want))
    assert L.zamd_gunzip(out, C.byref(n), f, len(f), None, None) == zhost.Z_OK and out.raw == want
    _, starts = ten()
    for name, (g, k, _msg) in sorted(damaged_files().items()):
        front = b"".join(m[2] for m in walk(g)[0])
        assert _gunzip(L, g, 30000) == (zhost.Z_DATA_ERROR, len(front), starts[k], k, front), name
    assert _gunzip(L, b"\x1f\x8b\x07" + f[3:], 30000)[:4] == (zhost.Z_DATA_ERROR, 0, 0, 0)
