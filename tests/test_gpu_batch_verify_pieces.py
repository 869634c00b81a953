"""The verify form of the piece path (batch_pieces_verify_run, zgpu_inflate_batch_pieces.hip): the long items of a blocking integrity test --
zgpu_inflate_batch_verify_host / _device and what stands on them -- checked in pieces, on the hand-built long items of oracle/piececases.py with the
threshold at 49153, the smallest body that can be long.

The rule of every test is that of tests/test_gpu_batch_sizes_pieces.py: the call runs with the feature on and, in the same process, with the threshold 0.
With it off the new counters (Engine.batch_verify_piece_counts()) rise by (0, 0).  Every record is equal both ways -- code, message, out_bytes, in_used,
adler32, crc32 --, and Python zlib is the judge of good items, check values included.  With it on the new counters rise by exactly what the catalogue's
`went` says (bounded from below where a case leaves its way open).  The fallback verifies anything right, so two things expose a piece path that is wrong
or that declines what it should take: the counters, and -- for raw items with checks=3, which have no trailer to be caught by -- the reported check
values.  The decode's and the sizing pass's counters do not move in a verify call.
tests/test_inflate_verify_pieces_plan_cpu.py works the same verdicts out without a GPU."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from oracle import piececases as P
from oracle.handmade import rint, rnd
from tests.piece_fixtures import HDR, rounds_batch, zlib_verdict

pytestmark = pytest.mark.gpu

OK, DATA_ERROR = 0, -3
MINK, VK, SLOTK, NOSCR = "ZGPU_BATCH_PIECES_MIN_BYTES", "ZGPU_BATCH_PIECES_VERIFY_MIN_BYTES", "ZGPU_BATCH_PIECES_VERIFY_ROUND_SLOTS", "ZGPU_BATCH_PIECES_NO_SCRATCH"
KNOBS = (MINK, VK, SLOTK, NOSCR, "ZGPU_BATCH_PIECES_ROUND_BYTES", "ZGPU_BATCH_PIECES_SIZES_MIN_BYTES", "ZGPU_BATCH_PIECES_SIZES_ROUND_SLOTS")
ROUND_SLOTS = 7  # (tests/test_inflate_verify_pieces_plan_cpu.py: four rounds or more of the seven items of rounds_batch)


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def piece_knobs():
    """the shared threshold at the smallest long body: the integrity test follows it"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ[MINK] = str(P.MIN_BYTES)
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


class Item:
    """one item of a call: its bytes and what it adds to the verify counters ((0, 0): it is not long; None: either way)"""

    def __init__(self, data, went=(0, 0), name=""):
        self.data, self.went, self.name = data, went, name


def of_case(c, wrap):
    return Item(c.wrapped(wrap), c.went, c.name)


def small_item(wrap, length, seed):
    """a good item of exactly `length` bytes: one final stored block of seeded bytes in the wrapper"""
    data = rnd(length - HDR[wrap] - 5 - {"raw": 0, "zlib": 4, "gzip": 8}[wrap], 9700 + seed).tobytes()
    body = b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data
    s = {"raw": body, "zlib": b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(data)),
         "gzip": b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + struct.pack("<II", zlib.crc32(data), len(data))}[wrap]
    assert len(s) == length
    return Item(s, name="small")


def verify_host(eng, items, wrap, checks):
    """zgpu_inflate_batch_verify_host; one (code, msg, out_bytes, in_used, adler32, crc32) per item"""
    res = eng.inflate_batch_verify_host([i.data for i in items], wrap, checks=checks)
    assert eng.last_failed == sum(1 for r in res if r[0] != OK)
    return res


def want_counts(items):
    lo = (sum(i.went[0] for i in items if i.went), sum(i.went[1] for i in items if i.went))
    free = sum(1 for i in items if i.went is None)
    return (lo if not free else None), lo, lo[0] + lo[1] + free


def check_counts(items, went):
    exact, lo, total = want_counts(items)
    if exact is not None:
        assert went == exact, (went, exact)
    else:
        assert went[0] >= lo[0] and went[1] >= lo[1] and went[0] + went[1] == total, (went, lo, total)


def check_records(items, res, wrap, checks):
    """Python zlib is the judge: a good item's out_bytes, in_used and check values are zlib's (a check neither asked for nor needed by the wrapper stays at
    its start value); an item zlib refuses is a data error, with zlib's message where it has one"""
    for k, (it, r) in enumerate(zip(items, res)):
        tag = (k, it.name, r)
        w = wrap if wrap != "auto" else ("gzip" if it.data[:2] == b"\x1f\x8b" else "zlib")
        ok, msg, out, used = zlib_verdict(it.data, w)
        if ok:
            adler = zlib.adler32(out) if (checks & 1) or wrap in ("zlib", "auto") else 1
            crc = zlib.crc32(out) if (checks & 2) or wrap in ("gzip", "auto") else 0
            assert r == (OK, "", len(out), used, adler, crc), tag
        else:
            assert r[0] != OK and r[2] == 0 and r[3] == 0, tag
            if msg != "cut" and len(it.data) > 16:
                assert r[0] == DATA_ERROR and r[1] == msg, tag


def delta(now, before):
    return now[0] - before[0], now[1] - before[1]


def others(eng):
    return eng.batch_piece_counts() + eng.batch_size_piece_counts()


def both_ways(eng, call):
    """call() with the knobs as they stand and with the feature off (the shared threshold 0): (on, off, rise of the verify counters)"""
    before, rest = eng.batch_verify_piece_counts(), others(eng)
    on = call()
    went = delta(eng.batch_verify_piece_counts(), before)
    keep = {k: os.environ.pop(k, None) for k in (MINK, VK)}
    os.environ[MINK] = "0"
    try:
        before = eng.batch_verify_piece_counts()
        off = call()
        assert delta(eng.batch_verify_piece_counts(), before) == (0, 0)
    finally:
        os.environ.pop(MINK, None)
        for k, v in keep.items():
            if v is not None:
                os.environ[k] = v
    assert others(eng) == rest  # (a verify call decodes nothing into memory and sizes nothing)
    return on, off, went


def verify_checked(eng, items, wrap, checks):
    on, off, went = both_ways(eng, lambda: verify_host(eng, items, wrap, checks))
    check_records(items, off, wrap, checks)
    for k, (a, b) in enumerate(zip(on, off)):
        assert a == b, (k, items[k].name, a, b)
    check_counts(items, went)
    return on, went


def catalogue_items(wrap):
    items = []
    for c in P.catalogue():
        if wrap not in c.wraps:
            continue
        items.append(of_case(c, wrap))
        if len(items) == 3:
            items.append(small_item(wrap, 100, 1))  # a 100-byte item between neighbours
        if len(items) == 9:
            items.append(Item(b"", name="empty"))   # an empty item between neighbours
    assert all(len(i.data) - HDR[wrap] >= P.MIN_BYTES for i in items if i.went != (0, 0))
    return items


# ---------------------------------------------------------------------------- 1
@pytest.mark.parametrize("checks", [0, 3])
@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
def test_catalogue(eng, wrap, checks):
    verify_checked(eng, catalogue_items(wrap), wrap, checks)


# ---------------------------------------------------------------------------- 2
def test_the_reach_rule_at_its_edge(eng):
    names = ("p3_25200_reach_25200", "p3_25200_reach_25201", "p3_32768_reach_32768", "p3_32767_reach_32768")
    for n, want in zip(names, ((1, 0), (0, 1), (1, 0), (0, 1))):
        c = P.by_name(n)
        assert c.went == want
        res, went = verify_checked(eng, [of_case(c, "zlib")], "zlib", 0)
        assert went == want, n
        if want == (0, 1):
            assert res[0][:2] == (DATA_ERROR, "invalid distance too far back")


# ---------------------------------------------------------------------------- 3
def flip(s, at):
    at %= len(s)
    return s[:at] + bytes([s[at] ^ 0x04]) + s[at + 1:]


def test_a_wrong_trailer_on_a_long_item_stays_in_pieces(eng):
    """one bit flipped in the Adler-32 of a zlib item, in the CRC-32 of a gzip item and in its ISIZE: the deflate data is clean, so the item is checked in
    pieces, and the finish kernel -- the code that compares every trailer -- says what is wrong"""
    pool = P.pool()
    z, g = pool[4].wrapped("zlib"), pool[6].wrapped("gzip")
    for wrap, data, msg in (("zlib", flip(z, -2), "incorrect data check"), ("gzip", flip(g, -6), "incorrect data check"), ("gzip", flip(g, -3), "incorrect length check")):
        items = [small_item(wrap, 100, 5), Item(data, (1, 0), msg), of_case(pool[1], wrap)]
        res, went = verify_checked(eng, items, wrap, 0)
        assert went == (2, 0)
        assert res[1][:4] == (DATA_ERROR, msg, 0, 0), res[1]
        assert res[0][0] == OK and res[2][0] == OK


def test_failed_short_items_beside_long_ones(eng):
    """a call with long items runs the merge and the finish kernel a second time over ALL items: a short item with a wrong trailer, a damaged short
    item and a cut short item keep the records of the first time"""
    pool = P.pool()
    good = small_item("zlib", 3000, 11).data
    items = [of_case(pool[0], "zlib"), Item(flip(good, -1), name="short, wrong Adler-32"), Item(flip(good, 4), name="short, bad stored length"),
             of_case(pool[3], "zlib"), Item(good[:1500], name="short, cut"), small_item("zlib", 100, 12)]
    res, went = verify_checked(eng, items, "zlib", 3)
    assert went == (2, 0)
    assert [r[0] for r in res] == [OK, DATA_ERROR, DATA_ERROR, OK, DATA_ERROR, OK]
    assert res[1][1] == "incorrect data check" and res[2][1] == "invalid stored block lengths"
    assert eng.last_failed == 3


# ---------------------------------------------------------------------------- 4
def test_the_window_across_a_piece_start(eng):
    """the P3 cases and the cases that end with far_tail: matches at distance 32768 and at distance 1 straddle a piece start.  Raw items with checks=3 have
    no trailer: the check values come from the pieces alone, and a wrong entry window shows in them"""
    cases = [c for c in P.catalogue() if c.group in ("P1", "P3") and c.went == (1, 0) and "raw" in c.wraps]
    assert sum(1 for c in cases if c.group == "P3") >= 2 and sum(1 for c in cases if c.group == "P1") >= 2
    items = [of_case(c, "raw") for c in cases]
    res, went = verify_checked(eng, items, "raw", 3)
    assert went == (len(items), 0)
    for c, r in zip(cases, res):
        assert r[4:] == (zlib.adler32(c.expect), zlib.crc32(c.expect)), c.name


# ---------------------------------------------------------------------------- 5
def test_rounds_under_the_slot_cap(eng):
    """ZGPU_BATCH_PIECES_VERIFY_ROUND_SLOTS=7: every item has three slots or four, so the seven items make four rounds or more in whatever order the list
    holds them; the cut item and the reach item fall back inside their own rounds, and the items whose ROOM the decode's test makes too small or too
    large are good here -- an integrity test has no rooms."""
    os.environ[SLOTK] = str(ROUND_SLOTS)
    items = []
    for data, _room, _plain, code, _msg, _went, name in rounds_batch("zlib"):
        items.append(Item(data, (0, 1) if code == DATA_ERROR else (1, 0), name))
    res, went = verify_checked(eng, items, "zlib", 0)
    assert went == (5, 2)
    assert [r[0] for r in res] == [OK, OK, OK, DATA_ERROR, DATA_ERROR, OK, OK]


def test_three_hundred_items_under_the_default_cap(eng):
    """300 long items drawn from the pool, three slots or four each: more than the default cap of 1024 slots holds, so the call makes rounds on its own"""
    pool = P.pool()
    wrapped = [c.wrapped("gzip") for c in pool]
    order = rint(300, 0, len(pool), 5151).tolist()
    items = [Item(wrapped[j], (1, 0), pool[j].name) for j in order]
    assert 15 << 20 < sum(len(i.data) for i in items) < 25 << 20
    on, off, went = both_ways(eng, lambda: verify_host(eng, items, "gzip", 3))
    truth = [(OK, "", len(c.expect), len(w), zlib.adler32(c.expect), zlib.crc32(c.expect)) for c, w in zip(pool, wrapped)]
    for k, (j, a, b) in enumerate(zip(order, on, off)):
        assert a == b == truth[j], (k, pool[j].name, a, b)
    assert went == (300, 0), went


# ---------------------------------------------------------------------------- 6
def test_every_alignment_of_an_item_and_an_input_that_is_not_aligned(eng):
    """The finders read the buffer in 16-byte vectors: one call holds 16 long items at every offset mod 16.  The same bytes handed over at base + 4 and
    base + 1 of the allocation: the path declines an input that is not 16-byte aligned, the records are the same."""
    import torch
    import zlib_amd.gpu as G
    cases = [c for c in P.catalogue() if c.went == (1, 0) and c.group in ("P1", "P3", "P6", "P7")][:8] + P.pool()[:8]
    items, at = [], 0
    for r, c in enumerate(cases):
        f = 5 + (r - at - 5) % 16  # a filler item of 5 .. 20 bytes puts the long one at offset r mod 16
        items.append(small_item("raw", f, r)); at += f
        assert at % 16 == r
        items.append(of_case(c, "raw")); at += len(c.stream)
    n = len(items)
    blob = np.frombuffer(b"".join(i.data for i in items), dtype=np.uint8)
    ioffs = np.zeros(n + 1, dtype=np.uint64); ioffs[1:] = np.cumsum([len(i.data) for i in items])
    dev = torch.device("cuda", 0)
    d_buf = torch.zeros(len(blob) + 64, dtype=torch.uint8, device=dev)
    assert d_buf.data_ptr() % 16 == 0
    d_io = torch.tensor(ioffs.view(np.int64), device=dev)
    recs = []
    for shift in (0, 4, 1):
        d_buf[shift: shift + len(blob)] = torch.from_numpy(blob.copy()).to(dev)
        d_items = torch.zeros(n * C.sizeof(G.InflateItem), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        before = eng.batch_verify_piece_counts()
        failed = eng.inflate_batch_verify_device(d_buf.data_ptr() + shift, len(blob), d_io.data_ptr(), n, d_items.data_ptr(), wrap="raw", checks=3)
        went = delta(eng.batch_verify_piece_counts(), before)
        raw = d_items.cpu().numpy().tobytes()
        res = []
        for k in range(n):
            it = G.InflateItem.from_buffer_copy(raw, k * C.sizeof(G.InflateItem))
            res.append((it.code, eng.L.zgpu_inflate_message(it.msg).decode(), it.out_bytes, it.in_used, it.adler32, it.crc32))
        assert failed == 0
        check_records(items, res, "raw", 3)
        recs.append(res)
        assert went == ((16, 0) if shift == 0 else (0, 0)), (shift, went)
    assert recs[0] == recs[1] == recs[2]


# ---------------------------------------------------------------------------- 7
def test_the_verify_knob_overrides_the_shared_one(eng):
    items = [of_case(P.by_name(n), "zlib") for n in ("p1_pad3", "p2_short_pieces", "pool8_82000")]
    ref = verify_host(eng, items, "zlib", 0)
    for shared, own, want in ((str(P.MIN_BYTES), "0", (0, 0)), ("0", str(P.MIN_BYTES), (3, 0)), (str(P.MIN_BYTES), "100000", (1, 0)), ("0", None, (0, 0))):
        os.environ[MINK] = shared
        os.environ.pop(VK, None)
        if own is not None:
            os.environ[VK] = own
        before = eng.batch_verify_piece_counts()
        assert verify_host(eng, items, "zlib", 0) == ref
        assert delta(eng.batch_verify_piece_counts(), before) == want, (shared, own)


def test_no_scratch_every_long_item_falls_back(eng):
    os.environ[NOSCR] = "1"
    items = catalogue_items("zlib")
    nlong = sum(1 for i in items if i.went != (0, 0))
    for i in items:
        if i.went != (0, 0):
            i.went = (0, 1)
    _, went = verify_checked(eng, items, "zlib", 0)
    assert went == (0, nlong)


def test_default_threshold_and_an_input_below_it(eng):
    """the threshold at its default: a call whose whole input is shorter than 128 KiB has no long item, whatever its items are"""
    os.environ.pop(MINK, None)
    items = [of_case(P.by_name("pool0_49153"), "zlib"), small_item("zlib", 100, 3), of_case(P.by_name("p1_pad0"), "zlib")]
    for i in items:
        i.went = (0, 0)
    assert sum(len(i.data) for i in items) < 131072
    before = eng.batch_verify_piece_counts()
    res = verify_host(eng, items, "zlib", 0)
    assert delta(eng.batch_verify_piece_counts(), before) == (0, 0)
    check_records(items, res, "zlib", 0)
    os.environ[MINK] = "0"
    assert verify_host(eng, items, "zlib", 0) == res
    assert delta(eng.batch_verify_piece_counts(), before) == (0, 0)


# ---------------------------------------------------------------------------- 8
def test_the_host_library_over_long_and_short_items(eng):
    """zamd_uncompress_verify_batch (libzamd_z.so) over a mix of long and short items: statuses and destLen are the per-item truth, and the engine's counters
    show that the long items went in pieces"""
    from tests import zhost
    L = zhost.lib()
    P_, U = C.POINTER(C.c_void_p), C.POINTER(C.c_ulong)
    L.zamd_uncompress_verify_batch.argtypes = [U, P_, U, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    pool = P.pool()
    cut = pool[7].wrapped("zlib")
    items = [of_case(pool[0], "zlib"), small_item("zlib", 100, 7), of_case(P.by_name("p3_32768_reach_32768"), "zlib"), Item(b"", name="empty"),
             Item(cut[: len(cut) * 2 // 3], (0, 1), "cut"), of_case(pool[8], "zlib"), Item(flip(pool[2].wrapped("zlib"), -1), (1, 0), "adler")]
    n = len(items)
    src = [C.create_string_buffer(i.data, max(len(i.data), 1)) for i in items]
    sp, sl = (C.c_void_p * n)(*[C.addressof(x) for x in src]), (C.c_ulong * n)(*[len(i.data) for i in items])
    vl, vs = (C.c_ulong * n)(*([12345] * n)), (C.c_int * n)(*([9] * n))
    before, rest = eng.batch_verify_piece_counts(), others(eng)
    rc = L.zamd_uncompress_verify_batch(vl, sp, sl, n, 15, vs)
    went = delta(eng.batch_verify_piece_counts(), before)
    want = []
    for it in items:
        ok, _msg, out, _used = zlib_verdict(it.data, "zlib")
        want.append((zhost.Z_OK, len(out)) if ok else (zhost.Z_BUF_ERROR if not it.data else zhost.Z_DATA_ERROR, 0))
    got = [(vs[k], vl[k]) for k in range(n)]
    assert [g[0] == zhost.Z_OK for g in got] == [w[0] == zhost.Z_OK for w in want], got
    assert [g for g in got if g[0] == zhost.Z_OK] == [w for w in want if w[0] == zhost.Z_OK]
    assert all(g[1] == 0 for g in got if g[0] != zhost.Z_OK) and rc != zhost.Z_OK
    assert went == (4, 1), went
    assert others(eng) == rest
