"""The piece path of the blocking batch decode (zgpu_inflate_batch_pieces.hip) on the hand-built long items of oracle/piececases.py, with
ZGPU_BATCH_PIECES_MIN_BYTES=49153, the smallest body that can be long.  tests/test_gpu_batch_pieces.py feeds the path what zlib's encoder emits; these items
are what it never emits at such sizes: a stored start behind every count of padding bits (and padding that is not zero), pieces that decode to less than
the window, a reach of the second piece exactly to and one byte past the item's first byte, megabytes of copies of one unknown byte, a final block that
ends at every bit of its byte, finder decoys, a page pool a neighbour starves, rounds in which some items fall back, more long items than the round
kernel has threads, and every alignment of an item in its buffer.  tests/test_piece_cases_cpu.py shows without a GPU that the cases stand where they claim.

The rule of every test: bytes, out_bytes, in_used, Adler-32 and CRC-32 of a good item are Python zlib's; code and message of a bad one are the case's;
every record equals the record of the same call with the feature off (ZGPU_BATCH_PIECES_MIN_BYTES=0), whose counters stay (0, 0); and the counters of
Engine.batch_piece_counts() rise by exactly what the cases say -- the fallback decodes anything right, so only the counters show a piece path that
declines what it should take.  With the knob 0 for the whole process the feature is off throughout: the counters must then stay where they are, the
bytes and records are checked all the same."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from oracle import piececases as P
from oracle.handmade import rint, rnd
from tests.piece_fixtures import HDR, rounds_batch, zlib_verdict
from tests.test_gpu_batch_pieces import BUF_ERROR, DATA_ERROR, KNOBS, OK, delta, run_host

pytestmark = pytest.mark.gpu

MINK = "ZGPU_BATCH_PIECES_MIN_BYTES"
PIECES_ON = os.environ.get(MINK) != "0"  # (the whole file can be run with the feature off: see the docstring)


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def piece_knobs():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ[MINK] = str(P.MIN_BYTES) if PIECES_ON else "0"
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


class Item:
    """one item of a call: its bytes, its room, and what is expected of it -- plain: the bytes of a good item (None: not good); code, msg: of one that is
    not good (None: the one-workgroup decoder's, whatever it is); went: what it adds to the counters ((0, 0): it is not long)"""

    def __init__(self, data, room, plain=None, code=OK, msg=None, went=(0, 0), name=""):
        self.data, self.room, self.plain, self.code, self.msg, self.went, self.name = data, room, plain, code, msg, went, name


def of_case(c, wrap, room=None):
    if c.kind == "ok":
        return Item(c.wrapped(wrap), len(c.expect) if room is None else room, c.expect, went=c.went, name=c.name)
    return Item(c.wrapped(wrap), 65536 if room is None else room, None, DATA_ERROR, c.msg if c.kind == "bad" else None, c.went, c.name)


def small_item(wrap, length, seed):
    """a good item of exactly `length` bytes: one final stored block of seeded bytes in the wrapper"""
    data = rnd(length - HDR[wrap] - 5 - {"raw": 0, "zlib": 4, "gzip": 8}[wrap], 9500 + seed).tobytes()
    body = b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data
    s = {"raw": body, "zlib": b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(data)),
         "gzip": b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + struct.pack("<II", zlib.crc32(data), len(data))}[wrap]
    assert len(s) == length
    return Item(s, len(data), data, name="small")


def too_small(c, wrap, room=None):
    """the item in a room one byte too small (or `room`): Z_BUF_ERROR with the size that was needed, from the one-workgroup decoder"""
    return Item(c.wrapped(wrap), len(c.expect) - 1 if room is None else room, None, BUF_ERROR, None, (0, 1), c.name + " (room too small)")


def want_counts(items):
    """(exact, lo, total): the counters' rise if every item's way is known, else None; the least each counter rises by; the rise of their sum"""
    lo = (sum(i.went[0] for i in items if i.went), sum(i.went[1] for i in items if i.went))
    free = sum(1 for i in items if i.went is None)
    return (lo if not free else None), lo, lo[0] + lo[1] + free


def check_counts(items, went):
    exact, lo, total = want_counts(items)
    if not PIECES_ON:
        assert went == (0, 0), went
    elif exact is not None:
        assert went == exact, (went, exact)
    else:
        assert went[0] >= lo[0] and went[1] >= lo[1] and went[0] + went[1] == total, (went, lo, total)


def check_records(items, res, wrap, checks=3):
    adler_done = bool(checks & 1) or wrap in ("zlib", "auto")
    crc_done = bool(checks & 2) or wrap in ("gzip", "auto")
    for k, (it, r) in enumerate(zip(items, res)):
        tag = (k, it.name, r[:6])
        if it.plain is not None:
            w = wrap if wrap != "auto" else ("gzip" if it.data[:2] == b"\x1f\x8b" else "zlib")
            ok, _, out, used = zlib_verdict(it.data, w)
            assert ok and out == it.plain, tag  # (the judge itself)
            assert r[:4] == (OK, "", len(out), used), tag
            assert r[4] == (zlib.adler32(out) if adler_done else 1) and r[5] == (zlib.crc32(out) if crc_done else 0), tag
            assert r[6] == out, tag
        elif it.code is None:
            assert r[0] != OK, tag
        else:
            assert r[0] == it.code, tag
            if it.msg is not None:
                assert r[1] == it.msg, tag
            if it.code == BUF_ERROR:
                assert r[2] == len(zlib_verdict(it.data, wrap)[2]), tag  # out_bytes: the size that was needed


def run_checked(eng, items, wrap, checks=3, run=None):
    """the call with the feature as the fixture set it and with the feature off: every record is checked and equal both ways; the counters' rise"""
    run = run or (lambda: run_host(eng, [i.data for i in items], [i.room for i in items], wrap, checks))
    before = eng.batch_piece_counts()
    on = run()
    went = delta(eng, before)
    keep = os.environ[MINK]
    os.environ[MINK] = "0"
    try:
        before = eng.batch_piece_counts()
        off = run()
        assert delta(eng, before) == (0, 0)
    finally:
        os.environ[MINK] = keep
    check_records(items, off, wrap, checks)
    for k, (a, b) in enumerate(zip(on, off)):
        assert a[:6] == b[:6] and a[6] == b[6], (k, items[k].name, a[:6], b[:6])
    check_counts(items, went)
    return on, went


# ---------------------------------------------------------------------------- 1
@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
def test_catalogue(eng, wrap):
    items = []
    for c in P.catalogue():
        if wrap not in c.wraps:
            continue
        items.append(of_case(c, wrap))
        if c.group == "P4":
            items.append(too_small(c, wrap))
        if len(items) == 3:
            items.append(small_item(wrap, 100, 1))  # a 100-byte item between neighbours
        if len(items) == 9:
            items.append(Item(b"", 16, None, None, None, name="empty"))  # an empty item: not a good one, the record the one-workgroup decoder writes
    assert all(len(i.data) - HDR[wrap] >= P.MIN_BYTES for i in items if i.went != (0, 0))
    run_checked(eng, items, wrap)


# ---------------------------------------------------------------------------- 2
def test_a_flood_starves_the_page_pool(eng):
    """The flood in 64 KiB of room: its piece takes pages from the round's pool until there is none.  Its own record is the one-workgroup decoder's (the
    room is too small); its neighbours are right whichever way they went; each of the three is counted once."""
    flood, a, b = P.by_name("p4_flood_dist1"), P.by_name("p1_pad2"), P.by_name("p2_short_pieces")
    items = [too_small(flood, "zlib", 65536), of_case(a, "zlib"), of_case(b, "zlib")]
    items[0].went = (0, 1)
    items[1].went = items[2].went = None
    run_checked(eng, items, "zlib")


# ---------------------------------------------------------------------------- 3
@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
@pytest.mark.parametrize("checks", [0, 1, 2, 3])
def test_checks(eng, wrap, checks):
    items = [of_case(P.by_name(n), wrap) for n in ("p1_pad3", "p2_short_pieces", "p3_32768_reach_32768", "pool8_82000")]
    _, went = run_checked(eng, items, wrap, checks)
    assert went == ((4, 0) if PIECES_ON else (0, 0))


# ---------------------------------------------------------------------------- 4
def gzip_header(extra, name):
    h = b"\x1f\x8b\x08" + bytes([4 | 8 | 2]) + b"\x00\x00\x00\x00\x00\x03" + struct.pack("<H", len(extra)) + extra + name + b"\x00"
    return h + struct.pack("<H", zlib.crc32(h) & 0xFFFF)


def test_wrap_auto_behind_headers_of_every_length(eng):
    """zlib items and gzip items whose headers carry FEXTRA, FNAME and FHCRC: the body begins at an odd offset that differs from item to item"""
    items, lens = [], []
    for i, n in enumerate(("p1_pad0", "p1_pad7", "p2_short_pieces", "p3_25200_reach_25200", "p6_final_ends_at_bit5", "p7_dynamic_block_inside_stored", "pool0_49153", "pool6_74001")):
        c = P.by_name(n)
        if i % 4 == 0:
            items.append(of_case(c, "zlib"))
            continue
        hdr = gzip_header(bytes(rnd(2 * i + 1, 9000 + i)), b"n" * (2 * i + 1))
        lens.append(len(hdr))
        assert len(hdr) % 2 == 1 and zlib_verdict(hdr + c.wrapped("gzip")[10:], "gzip")[2] == c.expect
        items.append(Item(hdr + c.wrapped("gzip")[10:], len(c.expect), c.expect, went=c.went, name=n))
    assert len(set(lens)) == len(lens) == 6
    run_checked(eng, items, "auto")


# ---------------------------------------------------------------------------- 5
def test_rounds_in_which_items_fall_back(eng):
    """ZGPU_BATCH_PIECES_ROUND_BYTES=131072: no three of these rooms fit one round, so the seven items make four rounds or more in whatever order the
    list of long items holds them (tests/test_piece_cases_cpu.py runs the split); items 1, 3 and 4 fall back, each in a round that has its own part of
    the fallback's segment table, item numbers and records."""
    os.environ["ZGPU_BATCH_PIECES_ROUND_BYTES"] = "131072"
    specs = rounds_batch("zlib")
    items = [Item(d, room, plain, code, msg, went, name) for d, room, plain, code, msg, went, name in specs]
    _, went = run_checked(eng, items, "zlib")
    assert went == ((4, 3) if PIECES_ON else (0, 0))


# ---------------------------------------------------------------------------- 6
def test_more_long_items_than_the_round_kernel_has_threads(eng):
    """1100 long items in one round: pieces_round_kernel's threads take two items each.  A 100-byte item follows every seventh; two items beyond the
    1024th are cut at two thirds and fall back."""
    pool = P.pool()
    wrapped = [c.wrapped("zlib") for c in pool]
    order = rint(1100, 0, len(pool), 4242).tolist()
    cut_at = (1030, 1093)
    big = len(pool) - 1  # (two thirds of the longest are still a long item)
    items, src = [], []
    for k, j in enumerate(order):
        if k in cut_at:
            d = wrapped[big][: len(wrapped[big]) * 2 // 3]
            assert len(d) - 2 >= P.MIN_BYTES
            items.append(Item(d, len(pool[big].expect), None, DATA_ERROR, None, (0, 1), "cut")); src.append(None)
        else:
            items.append(Item(wrapped[j], len(pool[j].expect), None, OK, None, (1, 0), pool[j].name)); src.append(j)
        if k % 7 == 6:
            items.append(small_item("zlib", 100, k)); src.append(-1)
    assert sum(len(i.data) for i in items) < 80 << 20
    streams, caps = [i.data for i in items], [i.room for i in items]
    before = eng.batch_piece_counts()
    on = run_host(eng, streams, caps, "zlib", 0)
    went = delta(eng, before)
    os.environ[MINK] = "0"
    before = eng.batch_piece_counts()
    off = run_host(eng, streams, caps, "zlib", 0)
    assert delta(eng, before) == (0, 0)
    truth = [(OK, "", len(c.expect), len(w), zlib.adler32(c.expect), 0) for c, w in zip(pool, wrapped)]
    for k, (it, a, b) in enumerate(zip(items, on, off)):
        assert a[:6] == b[:6], (k, it.name, a[:6], b[:6])
        if src[k] is None:
            assert a[0] == DATA_ERROR, (k, a[:6])
        elif src[k] >= 0:
            assert a[:6] == truth[src[k]] and a[6] == b[6] == pool[src[k]].expect, (k, it.name, a[:6])
        else:
            assert a[0] == OK and a[6] == b[6] == it.plain, (k, a[:6])
    assert went == ((1098, 2) if PIECES_ON else (0, 0)), went


# ---------------------------------------------------------------------------- 7
def test_every_alignment_of_an_item_and_an_input_that_is_not_aligned(eng):
    """The finders read the buffer in 16-byte vectors and their regions are cut at 16 bytes of the BUFFER: one call holds 16 long items at every offset
    mod 16.  The same bytes handed over at base + 4 and base + 1 of the allocation: the piece path declines an input that is not 16-byte aligned, the
    records are the same."""
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
    ooffs = np.zeros(n + 1, dtype=np.uint64); ooffs[1:] = np.cumsum([i.room for i in items])
    dev = torch.device("cuda", 0)
    d_buf = torch.zeros(len(blob) + 64, dtype=torch.uint8, device=dev)
    assert d_buf.data_ptr() % 16 == 0
    d_io = torch.tensor(ioffs.view(np.int64), device=dev)
    d_oo = torch.tensor(ooffs.view(np.int64), device=dev)
    recs = []
    for shift in (0, 4, 1):
        d_buf[shift: shift + len(blob)] = torch.from_numpy(blob.copy()).to(dev)
        d_out = torch.zeros(int(ooffs[-1]) + 1, dtype=torch.uint8, device=dev)
        d_items = torch.zeros(n * C.sizeof(G.InflateItem), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        before = eng.batch_piece_counts()
        failed = eng.inflate_batch_device(d_buf.data_ptr() + shift, len(blob), d_io.data_ptr(), n, d_out.data_ptr(), int(ooffs[-1]), d_oo.data_ptr(), d_items.data_ptr(),
                                          wrap="raw", checks=3)
        went = delta(eng, before)
        raw = d_items.cpu().numpy().tobytes()
        out = d_out.cpu().numpy()
        res = []
        for k in range(n):
            it = G.InflateItem.from_buffer_copy(raw, k * C.sizeof(G.InflateItem))
            data = out[int(ooffs[k]): int(ooffs[k]) + it.out_bytes].tobytes() if it.code == OK else b""
            res.append((it.code, eng.L.zgpu_inflate_message(it.msg).decode(), it.out_bytes, it.in_used, it.adler32, it.crc32, data))
        assert failed == 0
        check_records(items, res, "raw")
        recs.append(res)
        assert went == ((16, 0) if PIECES_ON and shift == 0 else (0, 0)), (shift, went)
    assert recs[0] == recs[1] == recs[2]
