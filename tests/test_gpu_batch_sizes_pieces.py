"""The sizing form of the piece path (batch_pieces_sizes_run, zgpu_inflate_batch_pieces.hip): the long items of a sizing pass -- the sizes call and the
sizing half of the packed call -- counted in pieces, on the hand-built long items of oracle/piececases.py with the threshold at 49153, the smallest body
that can be long.

The rule of every test: the call runs with the feature on and with it off in the same process.  With it off the new counters
(Engine.batch_size_piece_counts()) rise by (0, 0).  Every record is equal both ways -- code, message, out_bytes, in_used, adler32 == 1, crc32 == 0 --, and a
good item's out_bytes and in_used are Python zlib's.  With it on the new counters rise by exactly what the catalogue's `went` says (bounded from below
where a case leaves its way open): the fallback sizes anything right, so only the counters show a path that declines what it should take.
tests/test_inflate_sizes_pieces_plan_cpu.py works the same verdicts out without a GPU."""
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
MINK, SZK, SLOTK, NOSCR = "ZGPU_BATCH_PIECES_MIN_BYTES", "ZGPU_BATCH_PIECES_SIZES_MIN_BYTES", "ZGPU_BATCH_PIECES_SIZES_ROUND_SLOTS", "ZGPU_BATCH_PIECES_NO_SCRATCH"
KNOBS = (MINK, SZK, SLOTK, NOSCR, "ZGPU_BATCH_PIECES_ROUND_BYTES")
ROUND_SLOTS = 7  # (tests/test_inflate_sizes_pieces_plan_cpu.py: four rounds or more of the seven items of rounds_batch)


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def piece_knobs():
    """the shared threshold at the smallest long body: the sizing pass follows it, and so does the decode half of a packed call"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ[MINK] = str(P.MIN_BYTES)
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


class Item:
    """one item of a call: its bytes and what it adds to the sizing counters ((0, 0): it is not long; None: either way)"""

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


def sizes_host(eng, items, wrap):
    """zgpu_inflate_batch_sizes_host; one (code, msg, out_bytes, in_used, adler32, crc32) per item"""
    import zlib_amd.gpu as G
    n = len(items)
    blob, ioffs = eng._pack_streams([i.data for i in items])
    recs = (G.InflateItem * max(n, 1))()
    failed = C.c_uint64(0)
    eng._check(eng.L.zgpu_inflate_batch_sizes_host(eng.h, blob.ctypes.data, int(ioffs[-1]), ioffs.ctypes.data, n, G._WRAPS[wrap], recs, C.byref(failed)))
    out = [(r.code, eng.L.zgpu_inflate_message(r.msg).decode(), r.out_bytes, r.in_used, r.adler32, r.crc32) for r in recs[:n]]
    assert failed.value == sum(1 for r in out if r[0] != OK)
    return out


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


def check_size_records(items, res, wrap):
    """Python zlib is the judge: a good item's out_bytes and in_used are zlib's; one zlib refuses is a data error, with zlib's message where it has one"""
    for k, (it, r) in enumerate(zip(items, res)):
        tag = (k, it.name, r)
        w = wrap if wrap != "auto" else ("gzip" if it.data[:2] == b"\x1f\x8b" else "zlib")
        ok, msg, out, used = zlib_verdict(it.data, w)
        assert r[4] == 1 and r[5] == 0, tag  # a sizing pass computes no check
        if ok:
            assert r[:4] == (OK, "", len(out), used), tag
        else:
            assert r[0] != OK and r[2] == 0 and r[3] == 0, tag
            if msg != "cut" and len(it.data) > 16:
                assert r[0] == DATA_ERROR and r[1] == msg, tag


def delta(now, before):
    return now[0] - before[0], now[1] - before[1]


def both_ways(eng, call):
    """call() with the knobs as they stand and with the feature off (the shared threshold 0): (on, off, rise of the sizing counters, of the decode's)"""
    bs, bd = eng.batch_size_piece_counts(), eng.batch_piece_counts()
    on = call()
    went_s, went_d = delta(eng.batch_size_piece_counts(), bs), delta(eng.batch_piece_counts(), bd)
    keep = {k: os.environ.pop(k, None) for k in (MINK, SZK)}
    os.environ[MINK] = "0"
    try:
        bs, bd = eng.batch_size_piece_counts(), eng.batch_piece_counts()
        off = call()
        assert delta(eng.batch_size_piece_counts(), bs) == (0, 0) and delta(eng.batch_piece_counts(), bd) == (0, 0)
    finally:
        os.environ.pop(MINK, None)
        for k, v in keep.items():
            if v is not None:
                os.environ[k] = v
    return on, off, went_s, went_d


def sizes_checked(eng, items, wrap):
    before_d = eng.batch_piece_counts()
    on, off, went, went_d = both_ways(eng, lambda: sizes_host(eng, items, wrap))
    assert went_d == (0, 0) and eng.batch_piece_counts() == before_d  # (a sizes call decodes nothing)
    check_size_records(items, off, wrap)
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
@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
def test_catalogue_sizes(eng, wrap):
    items = catalogue_items(wrap)
    sizes_checked(eng, items, wrap)


def test_the_reach_rule_at_its_edge(eng):
    names = ("p3_25200_reach_25200", "p3_25200_reach_25201", "p3_32768_reach_32768", "p3_32767_reach_32768")
    for n, want in zip(names, ((1, 0), (0, 1), (1, 0), (0, 1))):
        c = P.by_name(n)
        assert c.went == want
        res, went = sizes_checked(eng, [of_case(c, "zlib")], "zlib")
        assert went == want, n
        if want == (0, 1):
            assert res[0][:2] == (DATA_ERROR, "invalid distance too far back")


def test_the_sizing_knob_overrides_the_shared_one(eng):
    items = [of_case(P.by_name(n), "zlib") for n in ("p1_pad3", "p2_short_pieces", "pool8_82000")]
    ref = sizes_host(eng, items, "zlib")
    for shared, own, want in ((str(P.MIN_BYTES), "0", (0, 0)), ("0", str(P.MIN_BYTES), (3, 0)), (str(P.MIN_BYTES), "100000", (1, 0)), ("0", None, (0, 0))):
        os.environ[MINK] = shared
        os.environ.pop(SZK, None)
        if own is not None:
            os.environ[SZK] = own
        before = eng.batch_size_piece_counts()
        assert sizes_host(eng, items, "zlib") == ref
        assert delta(eng.batch_size_piece_counts(), before) == want, (shared, own)


# ---------------------------------------------------------------------------- 2
@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
def test_catalogue_packed(eng, wrap):
    """the packed call: its sizing half and its decode half each count the long items on their own counters.  An item the sizing pass refuses (a reach in
    front of the item) has no room: the decode half's piece path falls back on it too, and the record stays the sizing pass's."""
    items = catalogue_items(wrap)
    streams = [i.data for i in items]

    def call():
        datas, recs = eng.inflate_batch_packed_host(streams, wrap, checks=3)
        return datas, recs, list(eng.last_offsets)
    (d_on, r_on, o_on), (d_off, r_off, o_off), went_s, went_d = both_ways(eng, call)
    assert r_on == r_off and d_on == d_off and o_on == o_off  # records, bytes, offsets and total
    for k, (it, r, d) in enumerate(zip(items, r_off, d_off)):
        ok, msg, out, used = zlib_verdict(it.data, wrap)
        if ok:
            assert r == (OK, "", len(out), used, zlib.adler32(out), zlib.crc32(out)) and d == out, (k, it.name, r)
        else:
            assert r[0] != OK and d == b"", (k, it.name, r)
            if msg != "cut" and it.data:
                assert r[:2] == (DATA_ERROR, msg), (k, it.name, r)
    assert o_off[-1] == sum(len(d) for d in d_off)
    check_counts(items, went_s)
    check_counts(items, went_d)
    far = next(k for k, i in enumerate(items) if i.name == "p3_25200_reach_25201")
    assert r_on[far][:4] == (DATA_ERROR, "invalid distance too far back", 0, 0)


# ---------------------------------------------------------------------------- 3
def gzip_header(extra, name):
    h = b"\x1f\x8b\x08" + bytes([4 | 8 | 2]) + b"\x00\x00\x00\x00\x00\x03" + struct.pack("<H", len(extra)) + extra + name + b"\x00"
    return h + struct.pack("<H", zlib.crc32(h) & 0xFFFF)


def test_wrap_auto_behind_gzip_headers_of_odd_lengths(eng):
    """zlib items and gzip items whose headers carry FEXTRA, FNAME and FHCRC: the body begins at an odd offset that differs from item to item"""
    items, lens = [], []
    for i, n in enumerate(("p1_pad1", "p1_pad6", "p2_short_pieces", "p3_32768_reach_32768", "p6_final_ends_at_bit3", "p7_dynamic_block_inside_stored", "pool1_52801", "pool7_78000")):
        c = P.by_name(n)
        if i % 4 == 0:
            items.append(of_case(c, "zlib"))
            continue
        hdr = gzip_header(bytes(rnd(2 * i + 3, 9100 + i)), b"m" * (2 * i + 1))
        lens.append(len(hdr))
        assert len(hdr) % 2 == 1
        items.append(Item(hdr + c.wrapped("gzip")[10:], c.went, n))
    assert len(set(lens)) == len(lens) == 6
    _, went = sizes_checked(eng, items, "auto")
    assert went == (8, 0)


# ---------------------------------------------------------------------------- 4
def test_rounds_under_the_slot_cap(eng):
    """ZGPU_BATCH_PIECES_SIZES_ROUND_SLOTS=7: every item has three slots or four, so the seven items make four rounds or more in whatever order the list
    holds them; the cut item and the reach item fall back inside their own rounds, and the items whose ROOM the decode's test makes too small or too
    large are good here -- sizing has no rooms."""
    os.environ[SLOTK] = str(ROUND_SLOTS)
    items = []
    for data, _room, _plain, code, _msg, _went, name in rounds_batch("zlib"):
        items.append(Item(data, (0, 1) if code == DATA_ERROR else (1, 0), name))
    res, went = sizes_checked(eng, items, "zlib")
    assert went == (5, 2)
    assert [r[0] for r in res] == [OK, OK, OK, DATA_ERROR, DATA_ERROR, OK, OK]


# ---------------------------------------------------------------------------- 5
def test_more_long_items_than_the_round_kernel_has_threads(eng):
    """1100 long items in one round: pieces_round_kernel's threads take two items each.  A 100-byte item follows every seventh; two items beyond the
    1024th are cut at two thirds and fall back."""
    pool = P.pool()
    wrapped = [c.wrapped("zlib") for c in pool]
    order = rint(1100, 0, len(pool), 4343).tolist()
    cut_at = (1031, 1092)
    big = len(pool) - 1  # (two thirds of the longest are still a long item)
    items, src = [], []
    for k, j in enumerate(order):
        if k in cut_at:
            d = wrapped[big][: len(wrapped[big]) * 2 // 3]
            assert len(d) - 2 >= P.MIN_BYTES
            items.append(Item(d, (0, 1), "cut")); src.append(None)
        else:
            items.append(Item(wrapped[j], (1, 0), pool[j].name)); src.append(j)
        if k % 7 == 6:
            items.append(small_item("zlib", 100, k)); src.append(-1)
    assert sum(len(i.data) for i in items) < 80 << 20
    on, off, went, _ = both_ways(eng, lambda: sizes_host(eng, items, "zlib"))
    truth = [(OK, "", len(c.expect), len(w), 1, 0) for c, w in zip(pool, wrapped)]
    for k, (it, a, b) in enumerate(zip(items, on, off)):
        assert a == b, (k, it.name, a, b)
        if src[k] is None:
            assert a[0] == DATA_ERROR, (k, a)
        elif src[k] >= 0:
            assert a == truth[src[k]], (k, it.name, a)
        else:
            assert a[:4] == (OK, "", len(it.data) - 2 - 5 - 4, len(it.data)), (k, a)
    assert went == (1098, 2), went


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
        before = eng.batch_size_piece_counts()
        failed = eng.inflate_batch_sizes_device(d_buf.data_ptr() + shift, len(blob), d_io.data_ptr(), n, d_items.data_ptr(), wrap="raw")
        went = delta(eng.batch_size_piece_counts(), before)
        raw = d_items.cpu().numpy().tobytes()
        res = []
        for k in range(n):
            it = G.InflateItem.from_buffer_copy(raw, k * C.sizeof(G.InflateItem))
            res.append((it.code, eng.L.zgpu_inflate_message(it.msg).decode(), it.out_bytes, it.in_used, it.adler32, it.crc32))
        assert failed == 0
        check_size_records(items, res, "raw")
        recs.append(res)
        assert went == ((16, 0) if shift == 0 else (0, 0)), (shift, went)
    assert recs[0] == recs[1] == recs[2]


# ---------------------------------------------------------------------------- 7
def test_no_scratch_every_long_item_falls_back(eng):
    os.environ[NOSCR] = "1"
    items = catalogue_items("zlib")
    nlong = sum(1 for i in items if i.went != (0, 0))
    for i in items:
        if i.went != (0, 0):
            i.went = (0, 1)
    _, went = sizes_checked(eng, items, "zlib")
    assert went == (0, nlong)


# ---------------------------------------------------------------------------- 8
def test_default_threshold_and_an_input_below_it(eng):
    """the threshold at its default: a call whose whole input is shorter than 128 KiB has no long item, whatever its items are"""
    os.environ.pop(MINK, None)
    items = [of_case(P.by_name("pool0_49153"), "zlib"), small_item("zlib", 100, 3), of_case(P.by_name("p1_pad0"), "zlib")]
    for i in items:
        i.went = (0, 0)
    assert sum(len(i.data) for i in items) < 131072
    before = eng.batch_size_piece_counts()
    res = sizes_host(eng, items, "zlib")
    assert delta(eng.batch_size_piece_counts(), before) == (0, 0)
    check_size_records(items, res, "zlib")
    os.environ[MINK] = "0"
    assert sizes_host(eng, items, "zlib") == res
    assert delta(eng.batch_size_piece_counts(), before) == (0, 0)
