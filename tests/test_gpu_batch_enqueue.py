"""The stream-ordered batch inflate, zgpu_inflate_batch_*_enqueue: the four batch jobs put on the caller's stream with a caller-owned workspace, nothing
read back, the decode through the decoder's fused mode (every item's check values folded in the flush that stores its bytes).  The truth is Python's zlib
(bytes, sizes, Adler-32, CRC-32) and, differentially, the blocking entry point of the same job: record k must equal its record k field for field.
Device memory is held in torch tensors; every call here is followed by a synchronize of the test's own."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cases, handmade as H  # noqa: E402
from tests import batch_sizes_fixtures as F  # noqa: E402
from tests.batch_sizes_fixtures import BUF_ERROR, DATA_ERROR, OK, STREAM_ERROR, TRUNCATED  # noqa: E402
from tests.test_gpu_batch_sizes import _damage_items  # noqa: E402
from tests.test_gpu_batch_verify import RING_SIZES, _truth_without_dictionary  # noqa: E402

ADLER, CRC = 1, 2
DECODE, SIZES, VERIFY, PACKED = 0, 1, 2, 3
FILL = 0xA5
GUARD = 64
REC = np.dtype([("code", "<i4"), ("msg", "<u4"), ("out_bytes", "<u8"), ("in_used", "<u8"), ("adler32", "<u4"), ("crc32", "<u4")])
BAD_OFFSETS = (STREAM_ERROR, "", 0, 0, 1, 0)


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


def _records(eng, raw, n):
    """n zgpu_inflate_item in `raw` (bytes or a uint8 array) as (code, message, out_bytes, in_used, adler32, crc32)"""
    arr = np.frombuffer(bytes(raw), dtype=REC, count=n)
    text = {m: eng.L.zgpu_inflate_message(int(m)).decode() for m in np.unique(arr["msg"])}
    return [(int(r["code"]), text[r["msg"]], int(r["out_bytes"]), int(r["in_used"]), int(r["adler32"]), int(r["crc32"])) for r in arr]


class Dev:
    """One batch in device memory: the input, its offsets, records filled with 0xEE, a summary filled with 0xEE, a workspace; for the jobs with a
    destination a buffer of out_cap bytes between two guards of 64, all filled with 0xA5."""

    def __init__(self, eng, job, zs, out_cap=0, in_offs=None, in_bytes=None, ws_short=0):
        import torch
        from zlib_amd import gpu
        self.eng, self.job = eng, job
        self.n = len(zs) if in_offs is None else len(in_offs) - 1  # (a table of its own may name the pieces of the blob more than once)
        dev = torch.device("cuda", 0)
        blob, offs = F.pack(zs)
        if in_offs is not None:
            offs = np.array(in_offs, dtype=np.uint64)
        self.in_bytes = int(offs[-1]) if in_bytes is None else in_bytes
        self.d_in = torch.tensor(blob, device=dev)
        self.d_io = torch.tensor(offs.view(np.int64), device=dev)
        self.d_items = torch.full((max(self.n, 1) * REC.itemsize,), 0xEE, dtype=torch.uint8, device=dev)
        self.d_sum = torch.full((C.sizeof(gpu.InflateBatchSummary),), 0xEE, dtype=torch.uint8, device=dev)
        self.ws_bytes = eng.inflate_batch_workspace_bytes(job, self.n) - ws_short
        self.d_ws = torch.full((self.ws_bytes + ws_short + 256,), 0xEE, dtype=torch.uint8, device=dev)
        assert self.d_ws.data_ptr() % 256 == 0 and self.d_in.data_ptr() % 256 == 0
        self.out_cap = out_cap
        self.d_buf = torch.full((out_cap + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert self.d_buf.data_ptr() % 256 == 0
        self.d_out = self.d_buf.data_ptr() + GUARD
        self.d_oo = torch.full((self.n + 1,), 0xDEAD, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

    def set_out_offsets(self, ooffs):
        import torch
        self.d_oo.copy_(torch.tensor(np.array(ooffs, dtype=np.uint64).view(np.int64)))
        torch.cuda.synchronize()

    def enqueue(self, wrap, checks=0, align=1, stream=None, ws_ptr=None):
        e, ws = self.eng, self.d_ws.data_ptr() if ws_ptr is None else ws_ptr
        common = dict(wrap=wrap, d_summary=self.d_sum.data_ptr(), stream=stream)
        if self.job == DECODE:
            e.inflate_batch_enqueue(self.d_in.data_ptr(), self.in_bytes, self.d_io.data_ptr(), self.n, self.d_out, self.out_cap, self.d_oo.data_ptr(), self.d_items.data_ptr(), ws,
                                    self.ws_bytes, checks=checks, **common)
        elif self.job == SIZES:
            e.inflate_batch_sizes_enqueue(self.d_in.data_ptr(), self.in_bytes, self.d_io.data_ptr(), self.n, self.d_items.data_ptr(), ws, self.ws_bytes, **common)
        elif self.job == VERIFY:
            e.inflate_batch_verify_enqueue(self.d_in.data_ptr(), self.in_bytes, self.d_io.data_ptr(), self.n, self.d_items.data_ptr(), ws, self.ws_bytes, checks=checks, **common)
        else:
            e.inflate_batch_packed_enqueue(self.d_in.data_ptr(), self.in_bytes, self.d_io.data_ptr(), self.n, self.d_out, self.out_cap, self.d_oo.data_ptr(), self.d_items.data_ptr(), ws,
                                           self.ws_bytes, checks=checks, align=align, **common)

    def results(self):
        """after a synchronize: (records, (nfailed, nbad_offsets, total, overflow, reserved), destination with its guards, output offsets)"""
        import torch
        torch.cuda.synchronize()
        recs = _records(self.eng, self.d_items.cpu().numpy(), self.n)
        summary = struct.unpack("<QQQII", self.d_sum.cpu().numpy().tobytes())
        return recs, summary, self.d_buf.cpu().numpy(), [int(x) for x in self.d_oo.cpu().numpy().view(np.uint64)]


def run_decode(eng, zs, ooffs, wrap, checks=0, **kw):
    d = Dev(eng, DECODE, zs, out_cap=kw.pop("out_cap", int(ooffs[-1])), **kw)
    d.set_out_offsets(ooffs)
    d.enqueue(wrap, checks)
    recs, summary, buf, _ = d.results()
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + d.out_cap:] == FILL).all()  # nothing outside the destination
    return recs, summary, buf[GUARD:]


def blocking_decode(eng, zs, ooffs, wrap, checks=0):
    """zgpu_inflate_batch_host with the same output table: (rc, nfailed, records, destination)"""
    from zlib_amd import gpu
    n = len(zs)
    blob, offs = F.pack(zs)
    cap = int(ooffs[-1])
    out = np.full(cap + 1, FILL, dtype=np.uint8)
    tab = np.array(ooffs, dtype=np.uint64)
    recs = (gpu.InflateItem * max(n, 1))()
    failed = C.c_uint64(99)
    rc = eng.L.zgpu_inflate_batch_host(eng.h, blob.ctypes.data, int(offs[-1]), offs.ctypes.data, n, gpu._WRAPS[wrap], checks, out.ctypes.data, cap, tab.ctypes.data, recs, C.byref(failed))
    return rc, failed.value, [F.record(eng, recs[k]) for k in range(n)], out


def table(caps):
    return [0] + [int(x) for x in np.cumsum(caps)]


def odd_table(sizes):
    """item k starts at an address = k mod 16 (the destination itself is 256-byte aligned + 64): both the vector path and the byte path of the flush run"""
    return table([s + ((1 - s) % 16) for s in sizes])


@pytest.mark.parametrize("wrap,checks", [("raw", 0), ("raw", ADLER | CRC), ("zlib", 0), ("gzip", ADLER), ("auto", 0)])
def test_whole_catalogue(eng, wrap, checks):
    pairs = F.streams(wrap)
    zs = [z + F.JUNK for _, z in pairs]
    caps = [len(d) for d, _ in pairs]
    ooffs = table(caps)
    recs, summary, out = run_decode(eng, zs, ooffs, wrap, checks)
    want = [(c, m, len(data), used, a, crc) for c, m, data, used, a, crc in eng.inflate_batch_host(zs, caps, wrap=wrap, checks=checks)]
    assert recs == want
    assert summary == (eng.last_failed, 0, 0, 0, 0) and eng.last_failed == 0
    bad = [k for k, (d, _) in enumerate(pairs) if recs[k][0] != OK or out[ooffs[k]: ooffs[k] + len(d)].tobytes() != d]
    assert not bad, bad[:10]


RINGS = ["8", "16", "32"]  # ZGPU_INF_RING_KB: the fused decoder has the rings the batch decoder has, and picks among them as it does (8 unless set)


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_ring_boundaries(eng, wrap, ring, monkeypatch):
    """decoded sizes around every half of the 32 KiB ring (and so of the smaller ones), text / stored / zeros, every item at an odd address"""
    monkeypatch.setenv("ZGPU_INF_RING_KB", ring)
    pairs = []
    for n in RING_SIZES:
        for kind, level in (("text", 6), ("rand", 0), ("zeros", 9)):
            d = cases.make(kind, n, 13)
            pairs.append((d, F.deflate(d, level, wrap)))
    zs = [z for _, z in pairs]
    ooffs = odd_table([len(d) for d, _ in pairs])
    recs, summary, out = run_decode(eng, zs, ooffs, wrap, ADLER | CRC)
    assert summary == (0, 0, 0, 0, 0)
    bad = []
    for k, (d, z) in enumerate(pairs):
        if recs[k] != (OK, "", len(d), len(z), zlib.adler32(d), zlib.crc32(d)) or out[ooffs[k]: ooffs[k] + len(d)].tobytes() != d or not (out[ooffs[k] + len(d): ooffs[k + 1]] == FILL).all():
            bad.append((k, len(d), recs[k]))
    assert not bad, bad[:5]
    rc, failed, want, _ = blocking_decode(eng, zs, ooffs, wrap, ADLER | CRC)
    assert rc == OK and failed == 0 and recs == want


def _flip(s, at, bit=0x10):
    at %= len(s)
    return s[:at] + bytes([s[at] ^ bit]) + s[at + 1:]


def test_trailers_and_truncation(eng):
    d = cases.make("text", 5000, 21)
    z, gz = zlib.compress(d, 6), F.gzip_member(F.deflate(d, 6, "raw"), d)
    broken = [_flip(z, -4), _flip(z, -3), _flip(z, -2), _flip(z, -1),  # each byte of the Adler-32
              _flip(gz, -7), gz[:-4] + struct.pack("<I", len(d) + 1),  # CRC-32, ISIZE
              z[: len(z) - 40], gz[: len(gz) - 30],                    # cut inside the last block
              z[:-2], gz[:-3]]                                         # cut inside the trailer
    want_msg = ["incorrect data check"] * 5 + ["incorrect length check"] + [TRUNCATED] * 4
    zs = [z]
    for k, b in enumerate(broken):
        zs += [b, gz if k & 1 else z]  # a good neighbour on both sides of every broken item
    ooffs = odd_table([len(d)] * len(zs))
    recs, summary, out = run_decode(eng, zs, ooffs, "auto", 0)
    rc, failed, want, _ = blocking_decode(eng, zs, ooffs, "auto", 0)
    assert rc == OK and recs == want
    assert summary == (len(broken), 0, 0, 0, 0) and failed == len(broken)
    assert [(r[0], r[1]) for r in recs[1::2]] == [(DATA_ERROR, m) for m in want_msg]
    for k in range(0, len(zs), 2):
        assert recs[k] == (OK, "", len(d), len(zs[k]), zlib.adler32(d), zlib.crc32(d)), k
        assert out[ooffs[k]: ooffs[k] + len(d)].tobytes() == d and (out[ooffs[k] + len(d): ooffs[k + 1]] == FILL).all(), k


@pytest.mark.parametrize("ring", RINGS)
def test_ranges_too_small(eng, ring, monkeypatch):
    """capacity 0, size - 1 and exactly half a ring short, each between two guard items of 64 bytes that decode to nothing"""
    monkeypatch.setenv("ZGPU_INF_RING_KB", ring)
    half = int(ring) * 512
    guard = zlib.compress(b"")
    datas = [cases.make("text", 40000, 5), cases.make("mix", 70000, 6), cases.make("zeros", 100000, 7), cases.make("rand", 50000, 8)]
    items = []  # (stream, data, capacity)
    for d in datas:
        z = zlib.compress(d, 0 if d is datas[3] else 6)
        items += [(z, d, 0), (z, d, len(d) - 1), (z, d, len(d) - half), (z, d, len(d))]
    zs, caps = [guard], [GUARD]
    for z, _, cap in items:
        zs += [z, guard]
        caps += [cap, GUARD]
    ooffs = table(caps)
    recs, summary, out = run_decode(eng, zs, ooffs, "zlib", ADLER)
    rc, failed, want, _ = blocking_decode(eng, zs, ooffs, "zlib", ADLER)
    assert rc == OK and recs == want
    nshort = sum(1 for _, d, cap in items if cap < len(d))
    assert summary == (nshort, 0, 0, 0, 0) and failed == nshort
    for k, (z, d, cap) in enumerate(items):
        at = 2 * k + 1
        if cap < len(d):
            assert recs[at] == (BUF_ERROR, "", len(d), 0, 1, 0), (k, recs[at])  # the size that would have been needed
            assert out[ooffs[at]: ooffs[at + 1]].tobytes() == d[:cap], k     # (what fits is the item's own to write)
        else:
            assert recs[at] == (OK, "", len(d), len(z), zlib.adler32(d), 0) and out[ooffs[at]: ooffs[at + 1]].tobytes() == d, k
        assert recs[at - 1][:3] == (OK, "", 0)
        assert (out[ooffs[at - 1]: ooffs[at]] == FILL).all() and (out[ooffs[at + 1]: ooffs[at + 2]] == FILL).all(), k  # 64 guard bytes on each side


@pytest.mark.parametrize("ring", RINGS)
def test_small_ring_far_matches(eng, ring, monkeypatch):
    """matches at distances around 8 KiB, 16 KiB and the farthest, of every kind of length: a ring shorter than the distance reads the flushed bytes
    back from the destination, at odd addresses here, and a destination that ends early is not read past its end"""
    from tests.test_gpu_inflate import far_match_data
    monkeypatch.setenv("ZGPU_INF_RING_KB", ring)
    data = far_match_data(77)
    chunks = [data[k: k + 65536] for k in range(0, len(data), 65536)]
    pairs = [(d, zlib.compress(d, level)) for level in (9, 6, 1) for d in chunks]
    short = [(d, z) for d, z in pairs[:3]]  # the same items into ranges that end 40000 bytes early
    zs = [z for _, z in pairs + short]
    ooffs = odd_table([len(d) for d, _ in pairs] + [len(d) - 40000 for d, _ in short])
    recs, summary, out = run_decode(eng, zs, ooffs, "zlib", ADLER | CRC)
    assert summary == (len(short), 0, 0, 0, 0)
    for k, (d, z) in enumerate(pairs):
        assert recs[k] == (OK, "", len(d), len(z), zlib.adler32(d), zlib.crc32(d)), (k, recs[k])
        assert out[ooffs[k]: ooffs[k] + len(d)].tobytes() == d and (out[ooffs[k] + len(d): ooffs[k + 1]] == FILL).all(), k
    for j, (d, z) in enumerate(short):
        k = len(pairs) + j
        assert recs[k] == (BUF_ERROR, "", len(d), 0, 1, 0), (k, recs[k])
        room = ooffs[k + 1] - ooffs[k]  # (the range is the item's to fill: the bytes that keep the next start odd belong to it)
        assert len(d) - 40000 <= room < len(d) - 40000 + 16 and out[ooffs[k]: ooffs[k + 1]].tobytes() == d[:room], k
    rc, failed, want, _ = blocking_decode(eng, zs, ooffs, "zlib", ADLER | CRC)
    assert rc == OK and failed == len(short) and recs == want


def test_hand_built_streams(eng):
    cat = H.catalogue()
    zs = [c.stream for c in cat]
    kinds = [_truth_without_dictionary(c) for c in cat]
    ooffs = table([n if kind in ("ok", "trailing") else 0 for kind, n in kinds])
    recs, summary, _ = run_decode(eng, zs, ooffs, "raw", ADLER | CRC)
    rc, failed, want, _ = blocking_decode(eng, zs, ooffs, "raw", ADLER | CRC)
    assert rc == OK
    bad = [(c.name, r, w) for c, r, w in zip(cat, recs, want) if r != w]
    assert not bad, bad[:10]
    assert summary == (failed, 0, 0, 0, 0) and failed == sum(1 for r in recs if r[0] != OK)


def test_bad_offsets_fail_their_items_only(eng):
    """one item that runs backwards in the input (and, its neighbour leaving the output, in the output too), one that leaves the output, one that
    leaves the input, among good items: three STREAM_ERROR records, everything else as the blocking decode of the batch without them"""
    datas = [cases.make("text", 3000 + 500 * k, 40 + k) for k in range(4)]
    z = [zlib.compress(d, 6) for d in datas]
    pieces = [z[0], z[1], z[2], z[3], b"\x01\x02\x03\x04\x05\x06\x07\x08"]
    s = table([len(x) for x in pieces])
    in_bytes = s[4] + 4  # (the buffer itself is four bytes longer still: nothing the call could read lies outside it)
    # items:   0     1     2 (stream 2, its output leaves)   3 (backwards)   4 (stream 2 again)   5 (stream 3)   6 (leaves the input)
    in_offs = [s[0], s[1], s[2], s[3], s[2], s[3], s[4], in_bytes + 2]
    sizes = [len(datas[0]), len(datas[1]), len(datas[2]), 0, len(datas[2]), len(datas[3]), 16]
    out_cap = sum(sizes) + 100
    o = table(sizes[:2])
    big = out_cap + 7
    # item 2 = [o2, big) leaves the output, item 3 = [big, o2) runs backwards, item 4 starts where item 2 would have
    ooffs = [o[0], o[1], o[2], big, o[2], o[2] + sizes[4], o[2] + sizes[4] + sizes[5], o[2] + sizes[4] + sizes[5] + sizes[6]]
    assert ooffs[-1] <= out_cap
    d = Dev(eng, DECODE, pieces, out_cap=out_cap, in_offs=in_offs, in_bytes=in_bytes)
    assert d.n == 7
    d.set_out_offsets(ooffs)
    d.enqueue("zlib", ADLER | CRC)
    recs, summary, buf, _ = d.results()
    out = buf[GUARD:]
    assert [recs[k] for k in (2, 3, 6)] == [BAD_OFFSETS] * 3
    assert summary == (3, 3, 0, 0, 0)
    good = [0, 1, 4, 5]
    gz, gd = [z[0], z[1], z[2], z[3]], [datas[0], datas[1], datas[2], datas[3]]
    rc, failed, want, _ = blocking_decode(eng, gz, table([len(x) for x in gd]), "zlib", ADLER | CRC)
    assert rc == OK and failed == 0 and [recs[k] for k in good] == want
    for k, data in zip(good, gd):
        assert out[ooffs[k]: ooffs[k] + len(data)].tobytes() == data, k
    assert (out[ooffs[6]:] == FILL).all() and (buf[:GUARD] == FILL).all()  # the bad items wrote nothing


def test_no_items_one_item_and_two_launch_rounds(eng):
    from zlib_amd import gpu
    # n = 0: at most the summary's memset
    d = Dev(eng, DECODE, [], out_cap=16)
    d.enqueue("zlib")
    recs, summary, buf, _ = d.results()
    assert recs == [] and summary == (0, 0, 0, 0, 0) and (buf == FILL).all() and (d.d_items.cpu().numpy() == 0xEE).all()
    # n = 1
    data = cases.make("mix", 20000, 9)
    recs, summary, out = run_decode(eng, [zlib.compress(data)], [0, len(data)], "zlib", CRC)
    assert recs == [(OK, "", len(data), len(zlib.compress(data)), zlib.adler32(data), zlib.crc32(data))] and out[: len(data)].tobytes() == data
    # n = 65,537: two launches of the decoder
    small = cases.make("text", 100, 5)
    e, last = zlib.compress(b""), zlib.compress(small)
    n = 65537
    recs, summary, out = run_decode(eng, [e] * (n - 1) + [last], [0] * n + [len(small)], "zlib")
    assert summary == (0, 0, 0, 0, 0)
    assert set(recs[: n - 1]) == {(OK, "", 0, len(e), 1, 0)}
    assert recs[n - 1] == (OK, "", len(small), len(last), zlib.adler32(small), 0) and out[: len(small)].tobytes() == small
    # a workspace one byte short, a misaligned workspace: refused, nothing touched
    for kw, ws_off in ((dict(ws_short=1), 0), (dict(), 128)):
        d = Dev(eng, DECODE, [last, last], out_cap=2 * len(small), **kw)
        d.set_out_offsets([0, len(small), 2 * len(small)])
        with pytest.raises(gpu.EngineError) as ex:
            d.enqueue("zlib", ws_ptr=d.d_ws.data_ptr() + ws_off)
        assert ex.value.code == STREAM_ERROR
        _, _, buf, _ = d.results()
        assert (buf == FILL).all() and (d.d_items.cpu().numpy() == 0xEE).all() and (d.d_sum.cpu().numpy() == 0xEE).all() and (d.d_ws.cpu().numpy() == 0xEE).all()
    # what else the host can see
    d = Dev(eng, DECODE, [last], out_cap=len(small))
    d.set_out_offsets([0, len(small)])
    for bad in (dict(wrap=4), dict(wrap="zlib", checks=4)):
        with pytest.raises(gpu.EngineError) as ex:
            d.enqueue(**bad)
        assert ex.value.code == STREAM_ERROR
    dp = Dev(eng, PACKED, [last], out_cap=len(small))
    for align in (0, 3, 512):
        with pytest.raises(gpu.EngineError) as ex:
            dp.enqueue("zlib", align=align)
        assert ex.value.code == STREAM_ERROR
    assert (d.results()[2] == FILL).all() and (dp.d_ws.cpu().numpy() == 0xEE).all()


def _mixed():
    """the catalogue with damaged items among it: (streams, decoded bytes or None)"""
    good, damaged, _ = _damage_items()
    pairs = F.streams("auto")
    zs = [z + F.JUNK for _, z in pairs]
    want = [d for d, _ in pairs]
    for k in sorted(damaged):
        zs.insert(3 + 5 * k, damaged[k][0]); want.insert(3 + 5 * k, None)
    return zs, want


def test_sizes_enqueue(eng):
    zs, _ = _mixed()
    d = Dev(eng, SIZES, zs)
    d.enqueue("auto")
    recs, summary, _, _ = d.results()
    rc, failed, want = F.sizes_call(eng, zs, "auto")
    assert rc == OK and recs == want and summary == (failed, 0, 0, 0, 0) and failed > 0


@pytest.mark.parametrize("checks", [0, ADLER | CRC])
def test_verify_enqueue(eng, checks):
    from zlib_amd import gpu
    zs, _ = _mixed()
    d = Dev(eng, VERIFY, zs)
    d.enqueue("auto", checks)
    recs, summary, _, _ = d.results()
    blob, offs = F.pack(zs)
    items = (gpu.InflateItem * len(zs))()
    failed = C.c_uint64(99)
    assert eng.L.zgpu_inflate_batch_verify_host(eng.h, blob.ctypes.data, int(offs[-1]), offs.ctypes.data, len(zs), gpu.WRAP_AUTO, checks, items, C.byref(failed)) == OK
    assert recs == [F.record(eng, items[k]) for k in range(len(zs))] and summary == (failed.value, 0, 0, 0, 0) and failed.value > 0


@pytest.mark.parametrize("align", [1, 256])
def test_packed_enqueue(eng, align):
    zs, want = _mixed()
    rc, total, failed, offs, brecs, bout = F.packed_call(eng, zs, "auto", checks=3, align=align)
    assert rc == OK
    d = Dev(eng, PACKED, zs, out_cap=total + 1000)
    d.enqueue("auto", 3, align=align)
    recs, summary, buf, ooffs = d.results()
    assert recs == brecs and ooffs == offs and summary == (failed, 0, total, 0, 0)
    out = buf[GUARD:]
    for k, data in enumerate(want):
        if data is not None:
            assert out[offs[k]: offs[k] + len(data)].tobytes() == data, k
    assert (out[total:] == FILL).all() and (buf[:GUARD] == FILL).all()


def test_packed_enqueue_overflow_is_decided_on_the_device(eng):
    zs, _ = _mixed()
    rc, total, failed, offs, sized, bout = F.packed_call(eng, zs, "auto", checks=3, cap=0)
    assert rc == BUF_ERROR  # (the blocking call's answer: the sizing records, the offsets, the total)
    d = Dev(eng, PACKED, zs, out_cap=total - 1)
    d.enqueue("auto", 3)
    recs, summary, buf, ooffs = d.results()
    assert summary == (failed, 0, total, 1, 0)
    assert ooffs == offs and recs == sized
    assert (buf == FILL).all()  # no decoded byte is written


def test_two_calls_in_flight(eng):
    import torch
    batches = []
    for seed in (1, 2):
        datas = [cases.make(("text", "mix")[seed - 1], 30000 + 7000 * k, 10 * seed + k) for k in range(12)]
        zs = [zlib.compress(x, 6) for x in datas]
        d = Dev(eng, DECODE, zs, out_cap=sum(len(x) for x in datas))
        d.set_out_offsets(table([len(x) for x in datas]))
        batches.append((datas, zs, d, torch.cuda.Stream()))
    for datas, zs, d, s in batches:
        d.enqueue("zlib", ADLER | CRC, stream=s.cuda_stream)
    for datas, zs, d, s in batches:
        s.synchronize()
    for datas, zs, d, s in batches:
        recs, summary, buf, _ = d.results()
        assert summary == (0, 0, 0, 0, 0)
        assert recs == [(OK, "", len(x), len(z), zlib.adler32(x), zlib.crc32(x)) for x, z in zip(datas, zs)]
        assert buf[GUARD: GUARD + d.out_cap].tobytes() == b"".join(datas)


def test_call_is_stream_ordered_and_captures_into_a_graph(eng):
    """A synchronize, an allocation or a blocking copy inside the call would fail a capture in the global error mode: that the capture succeeds is the
    test of the call's claim.  The captured work reads its buffers when it runs, not when it was captured: replayed over a second batch of the same
    offsets it gives the second batch's output and records."""
    import torch
    sizes = [1000, 40000, 70000]
    first = [cases.make("rand", n, 50 + k) for k, n in enumerate(sizes)]
    second = [cases.make("text", n, 60 + k) for k, n in enumerate(sizes)]
    z1, z2 = [zlib.compress(x, 0) for x in first], [zlib.compress(x, 0) for x in second]  # stored blocks: the same offsets for both
    assert [len(a) for a in z1] == [len(b) for b in z2]
    d = Dev(eng, DECODE, z1, out_cap=sum(sizes))
    d.set_out_offsets(table(sizes))
    d.enqueue("zlib", ADLER | CRC)  # the ordinary warm-up call: code objects load on first use
    recs, _, buf, _ = d.results()
    assert buf[GUARD: GUARD + d.out_cap].tobytes() == b"".join(first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # (capture_error_mode "global", the default)
        d.enqueue("zlib", ADLER | CRC, stream=torch.cuda.current_stream().cuda_stream)
    blob2, _ = F.pack(z2)
    d.d_in.copy_(torch.tensor(blob2))
    d.d_buf.fill_(FILL)
    d.d_items.fill_(0xEE)
    torch.cuda.synchronize()
    g.replay()
    recs, summary, buf, _ = d.results()
    assert summary == (0, 0, 0, 0, 0)
    assert recs == [(OK, "", len(x), len(z), zlib.adler32(x), zlib.crc32(x)) for x, z in zip(second, z2)]
    assert buf[GUARD: GUARD + d.out_cap].tobytes() == b"".join(second)
