"""Batch of independent streams in one call: zgpu_deflate_segments_* with a zlib / gzip wrapper (one complete stream per segment) and
zgpu_inflate_batch_* (one verdict per item).  Encode must give, item by item, what the reference's compress2() / deflate() with windowBits 31 or
-15 gives for that item alone; decode must give each item's bytes, its in_used and its checks, and a bad item must never change what its
neighbours produce."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cases, handmade as H, refzlib as R  # noqa: E402

OK, NEED_DICT, DATA_ERROR, BUF_ERROR = 0, 2, -3, -5
SIZES = [0, 1, 2, 3, 100, 4096, 65535, 65536]
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


def _items():
    out = [cases.make("mix", n, 3) for n in SIZES]
    out += [cases.make(k, 5000 + 977 * i, 11 + i) for i, k in enumerate(cases.KINDS)]
    return out


ITEMS = _items()


def _own_compress2(data, level):
    from tests import zhost
    L = zhost.lib()
    n = C.c_ulong(len(data) + (len(data) >> 8) + 1024)
    out = C.create_string_buffer(n.value)
    src = C.create_string_buffer(data, max(len(data), 1))
    assert L.compress2(out, C.byref(n), src, len(data), level) == zhost.Z_OK
    return out.raw[: n.value]


def _want(data, level, wrap, strategy=0):
    """the reference's one-stream bytes for one item"""
    if wrap == "zlib" and strategy == 0:
        return R.compress2(data, level)
    return R.deflate_wbits(data, level, WBITS[wrap], strategy)


def _own(data, level, wrap, strategy=0):
    """this library's single-call bytes for one item: compress2(), or deflateInit2() + deflate(Z_FINISH)"""
    from tests import zhost
    if wrap == "zlib" and strategy == 0:
        return _own_compress2(data, level)
    z, _, _ = zhost.deflate_stream(data, level, [(len(data), zhost.Z_FINISH)], window_bits=WBITS[wrap], strategy=strategy)
    return z


@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
def test_encode_matches_single_calls(eng, wrap):
    bad = []
    for level in (1, 2, 3, 4, 6, 9):
        got = eng.deflate_batch_host(ITEMS, level, wrap=wrap)
        assert len(got) == len(ITEMS)
        for i, (d, z) in enumerate(zip(ITEMS, got)):
            if z != _own(d, level, wrap):
                bad.append(("own", wrap, level, i, len(d)))
            assert zlib.decompress(z, WBITS[wrap]) == d, (wrap, level, i)
    for strategy in range(5):
        got = eng.deflate_batch_host(ITEMS, 6, wrap=wrap, strategy=strategy)
        for i, (d, z) in enumerate(zip(ITEMS, got)):
            if z != _own(d, 6, wrap, strategy):
                bad.append(("own", wrap, "strategy", strategy, i, len(d)))
            assert zlib.decompress(z, WBITS[wrap]) == d
    assert not bad, bad[:10]


@pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref) is not here")
@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
def test_encode_matches_reference(eng, wrap):
    bad = []
    for level in (1, 2, 3, 4, 6, 9):
        for i, (d, z) in enumerate(zip(ITEMS, eng.deflate_batch_host(ITEMS, level, wrap=wrap))):
            if z != _want(d, level, wrap):
                bad.append((wrap, level, i, len(d)))
    for strategy in range(5):
        for i, (d, z) in enumerate(zip(ITEMS, eng.deflate_batch_host(ITEMS, 6, wrap=wrap, strategy=strategy))):
            if z != _want(d, 6, wrap, strategy):
                bad.append((wrap, "strategy", strategy, i, len(d)))
    assert not bad, bad[:10]


def test_encode_without_wrapper_unchanged(eng):
    from zlib_amd import gpu
    for level in (1, 6):
        assert eng.deflate_batch_host(ITEMS, level, wrap="raw") == eng.deflate_segments_host(ITEMS, level, flags=gpu.F_FINAL)
    # the body of every wrapped item is the raw item
    raw = eng.deflate_batch_host(ITEMS, 6, wrap="raw")
    for r, z, g in zip(raw, eng.deflate_batch_host(ITEMS, 6, wrap="zlib"), eng.deflate_batch_host(ITEMS, 6, wrap="gzip")):
        assert z[2:-4] == r and g[10:-8] == r


def _check_items(res, datas, streams, what):
    for k, (r, d, s) in enumerate(zip(res, datas, streams)):
        code, msg, data, used, adler, crc = r
        assert code == OK, (what, k, code, msg)
        assert data == d, (what, k)
        assert used == len(s), (what, k, used, len(s))
        assert adler == zlib.adler32(d) and crc == zlib.crc32(d), (what, k)


@pytest.mark.parametrize("ring", ["8", "16", "32"])
def test_decode_round_trip(eng, monkeypatch, ring):
    monkeypatch.setenv("ZGPU_INF_RING_KB", ring)
    per = {}
    for wrap in ("raw", "zlib", "gzip"):
        per[wrap] = eng.deflate_batch_host(ITEMS, 6, wrap=wrap) + eng.deflate_batch_host(ITEMS, 1, wrap=wrap)
        datas = ITEMS + ITEMS
        res = eng.inflate_batch_host(per[wrap], [len(d) for d in datas], wrap=wrap, checks=3)
        _check_items(res, datas, per[wrap], wrap)
        assert eng.last_failed == 0
    mixed = [per["zlib"][i] if i % 2 else per["gzip"][i] for i in range(len(per["zlib"]))]
    datas = ITEMS + ITEMS
    _check_items(eng.inflate_batch_host(mixed, [len(d) for d in datas], wrap="auto", checks=3), datas, mixed, "auto")


def _gzip_member(body_raw, data, name=None, extra=None, comment=None, hcrc=False):
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = bytes([0x1F, 0x8B, 8, flg]) + struct.pack("<I", 0) + bytes([0, 3])
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + body_raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def _raw(data, level=6, wbits=-15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits)
    return c.compress(data) + c.flush()


def test_other_producers(eng):
    datas, streams, wraps = [], [], []
    big1 = cases.make("text", 1 << 20, 5)
    big8 = cases.make("mix", 8 << 20, 6)
    for i, d in enumerate([cases.make("text", 100, 1), big1, cases.make("rand", 100, 2), big8, cases.make("runs", 30000, 3)]):
        for level, wb in ((1, 15), (6, 15), (9, 12), (6, 9), (0, 15), (6, 31), (9, 31)):
            c = zlib.compressobj(level, zlib.DEFLATED, wb)
            if d is big8 and level != 6:
                continue
            z = c.compress(d[: len(d) // 3]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(d[len(d) // 3: len(d) // 2]) + c.flush(zlib.Z_FULL_FLUSH) + \
                c.compress(d[len(d) // 2:]) + c.flush()
            datas.append(d); streams.append(z); wraps.append("gzip" if wb > 15 else "zlib")
    d = cases.make("mix", 7000, 9)
    for kw in ({"name": b"file.txt"}, {"extra": b"ab\x02\x00xy"}, {"comment": b"hello"},
               {"name": b"n", "extra": b"", "comment": b"c", "hcrc": True}, {"hcrc": True}):
        datas.append(d); streams.append(_gzip_member(_raw(d), d, **kw)); wraps.append("gzip")
    res = eng.inflate_batch_host(streams, [len(x) for x in datas], wrap="auto", checks=3)
    _check_items(res, datas, streams, "auto")
    # the same items through the mode of their own wrapper
    for w in ("zlib", "gzip"):
        sel = [k for k in range(len(streams)) if wraps[k] == w]
        res = eng.inflate_batch_host([streams[k] for k in sel], [len(datas[k]) for k in sel], wrap=w)
        _check_items([r[:4] + (zlib.adler32(datas[k]), zlib.crc32(datas[k])) for r, k in zip(res, sel)], [datas[k] for k in sel], [streams[k] for k in sel], w)
        # the check the wrapper needs is computed whatever `checks` says
        for r, k in zip(res, sel):
            assert (r[4] == zlib.adler32(datas[k])) if w == "zlib" else (r[5] == zlib.crc32(datas[k]))


def test_independent_verdicts(eng, golden):
    g = golden("handmade_inflate.json")["cases"]
    cat = [c for c in H.catalogue() if not c.dictionary]
    filler = [cases.make("mix", 300 + 50 * i, 40 + i) for i in range(len(cat) + 1)]
    streams, caps, want = [], [], []
    for i, c in enumerate(cat):
        streams.append(_raw(filler[i])); caps.append(len(filler[i])); want.append(("ok", filler[i], None))
        streams.append(c.stream); caps.append(len(c.expect) if c.expect is not None else 1 << 20); want.append((c.kind, c.expect, c))
    streams.append(_raw(filler[-1])); caps.append(len(filler[-1])); want.append(("ok", filler[-1], None))
    res = eng.inflate_batch_host(streams, caps, wrap="raw", checks=3)
    bad = []
    for r, s, (kind, expect, c) in zip(res, streams, want):
        code, msg, data, used = r[:4]
        name = c.name if c else "neighbour"
        if kind == "ok":
            if code != OK or data != expect or used != len(s):
                bad.append((name, code, msg, used, len(s)))
            elif r[4] != zlib.adler32(expect) or r[5] != zlib.crc32(expect):
                bad.append((name, "checks"))
        elif kind == "bad":
            if code != DATA_ERROR or msg != g[c.name]["msg"]:
                bad.append((name, code, msg, g[c.name]["msg"]))
        elif kind == "cut":
            if code != DATA_ERROR:
                bad.append((name, code, msg))
        elif kind == "trailing":
            if code != OK or data != expect or not used < len(s):
                bad.append((name, code, msg, used, len(s)))
    assert not bad, bad[:10]


def test_wrapper_errors(eng):
    d = cases.make("text", 5000, 21)
    z = zlib.compress(d, 6)
    gz = _gzip_member(_raw(d), d)
    hc = _gzip_member(_raw(d), d, name=b"x", hcrc=True)

    def zl(b0, b1):
        return bytes([b0, b1]) + z[2:]

    def fix31(b0, b1):  # b1 adjusted so that the header passes the % 31 check
        b1 &= 0xE0
        b1 |= 31 - ((b0 << 8) | b1) % 31 if ((b0 << 8) | b1) % 31 else 0
        return b0, b1
    wrong_adler = z[:-4] + struct.pack(">I", (zlib.adler32(d) ^ 1))
    items = [
        ("zlib", zl(0x78, 0x9D), DATA_ERROR, "incorrect header check"),
        ("zlib", zl(*fix31(0x77, 0x00)), DATA_ERROR, "unknown compression method"),
        ("zlib", zl(*fix31(0x88, 0x00)), DATA_ERROR, "invalid window size"),
        ("zlib", bytes(fix31(0x78, 0x20)) + b"\0\0\0\0" + z[2:], NEED_DICT, ""),
        ("zlib", wrong_adler, DATA_ERROR, "incorrect data check"),
        ("zlib", z[:-2], DATA_ERROR, None),
        ("zlib", z, OK, ""),
        ("gzip", gz[:-8] + struct.pack("<I", zlib.crc32(d) ^ 4) + gz[-4:], DATA_ERROR, "incorrect data check"),
        ("gzip", gz[:-4] + struct.pack("<I", len(d) + 1), DATA_ERROR, "incorrect length check"),
        ("gzip", hc[:12] + bytes([hc[12] ^ 1]) + hc[13:], DATA_ERROR, "header crc mismatch"),
        ("gzip", gz[:3] + bytes([0x20]) + gz[4:], DATA_ERROR, "unknown header flags set"),
        ("gzip", gz[:2] + bytes([7]) + gz[3:], DATA_ERROR, "unknown compression method"),
        ("gzip", z, DATA_ERROR, "incorrect header check"),
        ("gzip", hc, OK, ""),
    ]
    # (the member with FHCRC: name "x" at bytes 10-11, the header CRC at 12-13)
    assert hc[3] & 2
    for wrap in ("zlib", "gzip", "auto"):
        sel = [it for it in items if wrap == "auto" or it[0] == wrap]
        if wrap == "auto":  # under AUTO a zlib stream in a gzip-only slot is a valid zlib stream
            sel = [it for it in sel if not (it[0] == "gzip" and it[1] is z)]
        res = eng.inflate_batch_host([it[1] for it in sel], len(d), wrap=wrap)
        for (w, s, code, msg), r in zip(sel, res):
            assert r[0] == code, (wrap, w, msg, r[:2])
            if msg is not None:
                assert r[1] == msg, (wrap, w, r[1], msg)
            if code == OK:
                assert r[2] == d and r[3] == len(s)
            if R.available() and msg:  # the reference's verdict for the same item
                rc, _, _, rmsg, _ = R.inflate_wbits(s, {"zlib": 15, "gzip": 31, "auto": 47}[wrap], len(d) + 10)
                assert rmsg == msg, (w, rmsg, msg)


def test_capacity(eng):
    ds = [cases.make("text", 3000, 1), cases.make("mix", 9000, 2), cases.make("rand", 500, 3), b""]
    zs = [zlib.compress(d) for d in ds]
    res = eng.inflate_batch_host(zs, [len(ds[0]), len(ds[1]) - 1, len(ds[2]), 0], wrap="zlib")
    assert res[1][0] == BUF_ERROR and res[1][2] == b""
    for k in (0, 2, 3):
        assert res[k][0] == OK and res[k][2] == ds[k] and res[k][3] == len(zs[k])
    # out_bytes of the short item is the size it needs
    import zlib_amd.gpu as G
    n = len(zs)
    ioffs = np.zeros(n + 1, dtype=np.uint64); ioffs[1:] = np.cumsum([len(z) for z in zs])
    caps = [len(ds[0]), len(ds[1]) - 1, len(ds[2]), 0]
    ooffs = np.zeros(n + 1, dtype=np.uint64); ooffs[1:] = np.cumsum(caps)
    blob = np.frombuffer(b"".join(zs), dtype=np.uint8)
    out = np.full(int(ooffs[-1]) + 1, 0xA5, dtype=np.uint8)
    items = (G.InflateItem * n)()
    failed = C.c_uint64(0)
    rc = eng.L.zgpu_inflate_batch_host(eng.h, blob.ctypes.data, blob.size, ioffs.ctypes.data, n, G.WRAP_ZLIB, 0, out.ctypes.data, int(ooffs[-1]),
                                       ooffs.ctypes.data, items, C.byref(failed))
    assert rc == 0 and failed.value == 1
    assert items[1].code == BUF_ERROR and items[1].out_bytes == len(ds[1])
    assert out[int(ooffs[0]): int(ooffs[1])].tobytes() == ds[0] and out[int(ooffs[2]): int(ooffs[3])].tobytes() == ds[2]
    assert (out[int(ooffs[1]): int(ooffs[2])] == 0xA5).all()  # the failed item's room is left as it was


def test_scale_crosses_launch_batch(eng):
    n = 70000
    rng = np.random.default_rng(7)
    base = cases.make("text", 4096, 8)
    datas = []
    for k in range(n):
        m = int(rng.integers(0, 201))
        o = int(rng.integers(0, 4096 - m + 1))
        datas.append(base[o: o + m])
    zs = eng.deflate_batch_host(datas, 1, wrap="raw")
    res = eng.inflate_batch_host(zs, [len(d) for d in datas], wrap="raw")
    assert eng.last_failed == 0
    bad = [k for k in range(n) if res[k][0] != OK or res[k][2] != datas[k] or res[k][3] != len(zs[k])]
    assert not bad, bad[:10]


def test_device_entry_matches_host(eng):
    import torch
    import zlib_amd.gpu as G
    ds = [cases.make(k, 2000 + 300 * i, i) for i, k in enumerate(cases.KINDS)] + [b""]
    zs = [zlib.compress(d, 6) for d in ds]
    zs[2] = zs[2][:-1]  # one bad item
    caps = [len(d) for d in ds]
    caps[3] -= 1        # one short room
    host = eng.inflate_batch_host(zs, caps, wrap="zlib", checks=3)
    n = len(zs)
    dev = torch.device("cuda", 0)
    ioffs = np.zeros(n + 1, dtype=np.uint64); ioffs[1:] = np.cumsum([len(z) for z in zs])
    ooffs = np.zeros(n + 1, dtype=np.uint64); ooffs[1:] = np.cumsum(caps)
    d_in = torch.tensor(np.frombuffer(b"".join(zs), dtype=np.uint8), device=dev)
    d_io = torch.tensor(ioffs.view(np.int64), device=dev)
    d_oo = torch.tensor(ooffs.view(np.int64), device=dev)
    d_out = torch.zeros(int(ooffs[-1]) + 1, dtype=torch.uint8, device=dev)
    d_items = torch.zeros(n * C.sizeof(G.InflateItem), dtype=torch.uint8, device=dev)
    failed = eng.inflate_batch_device(d_in.data_ptr(), d_in.numel(), d_io.data_ptr(), n, d_out.data_ptr(), int(ooffs[-1]), d_oo.data_ptr(),
                                      d_items.data_ptr(), wrap="zlib", checks=3)
    assert failed == 2
    raw = d_items.cpu().numpy().tobytes()
    out = d_out.cpu().numpy()
    for k in range(n):
        it = G.InflateItem.from_buffer_copy(raw, k * C.sizeof(G.InflateItem))
        h = host[k]
        assert (it.code, eng.L.zgpu_inflate_message(it.msg).decode(), it.in_used, it.adler32, it.crc32) == (h[0], h[1], h[3], h[4], h[5]), k
        if it.code == OK:
            assert out[int(ooffs[k]): int(ooffs[k]) + it.out_bytes].tobytes() == h[2] == ds[k]


def _batch_args(bufs, caps):
    n = len(bufs)
    src = [C.create_string_buffer(b, max(len(b), 1)) for b in bufs]
    dst = [C.create_string_buffer(max(c, 1)) for c in caps]
    P = (C.c_void_p * n)
    return (src, dst, P(*[C.addressof(d) for d in dst]), (C.c_ulong * n)(*caps), P(*[C.addressof(x) for x in src]),
            (C.c_ulong * n)(*[len(b) for b in bufs]), (C.c_int * n)())


def test_host_library_batch():
    """zamd_compress2_batch / zamd_uncompress_batch of libzamd_z.so against the same library's compress2() / uncompress(), item by item"""
    from tests import zhost
    L = zhost.lib()
    P, U = C.POINTER(C.c_void_p), C.POINTER(C.c_ulong)
    L.zamd_compress2_batch.argtypes = [P, U, P, U, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.zamd_uncompress_batch.argtypes = [P, U, P, U, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    datas = [cases.make("mix", n, 50 + i) for i, n in enumerate((0, 1, 100, 4096, 65535, 65536, 65537, 200000, 3000, 20000))]
    for level in (0, 1, 6, 9):
        caps = [int(L.compressBound(len(d))) for d in datas]
        caps[3] = 10  # a short destLen
        src, dst, dp, dl, sp, sl, st = _batch_args(datas, caps)
        rc = L.zamd_compress2_batch(dp, dl, sp, sl, len(datas), level, 15, st)
        firsts = []
        for k, d in enumerate(datas):
            wrc, wz = zhost.compress2(d, level, caps[k])
            firsts.append(wrc)
            assert st[k] == wrc, (level, k, st[k], wrc)
            if wrc == zhost.Z_OK:
                assert dl[k] == len(wz) and dst[k].raw[: dl[k]] == wz, (level, k)
        assert rc == next((c for c in firsts if c != zhost.Z_OK), zhost.Z_OK)
    for wb, wrap in ((31, "gzip"), (-15, "raw")):
        caps = [int(L.compressBound(len(d))) + 32 for d in datas]
        src, dst, dp, dl, sp, sl, st = _batch_args(datas, caps)
        assert L.zamd_compress2_batch(dp, dl, sp, sl, len(datas), 6, wb, st) == zhost.Z_OK
        for k, d in enumerate(datas):
            assert dst[k].raw[: dl[k]] == _own(d, 6, wrap), (wrap, k)
    # uncompress: exact room, a short destLen, a truncated item, a damaged one, an item over 64 KiB
    zs = [zhost.compress2(d, 6)[1] for d in datas]
    zs[2] = zs[2][:-3]
    zs[5] = zs[5][:40] + bytes([zs[5][40] ^ 0xFF]) + zs[5][41:]
    caps = [len(d) for d in datas]
    caps[4] -= 1
    src, dst, dp, dl, sp, sl, st = _batch_args(zs, caps)
    rc = L.zamd_uncompress_batch(dp, dl, sp, sl, len(zs), 15, st)
    firsts = []
    for k, z in enumerate(zs):
        wrc, wd = zhost.uncompress(z, caps[k])
        firsts.append(wrc)
        assert st[k] == wrc, (k, st[k], wrc)
        if wrc == zhost.Z_OK:
            assert dl[k] == len(wd) and dst[k].raw[: dl[k]] == wd == datas[k], k
    assert st[2] == zhost.Z_DATA_ERROR and st[4] == zhost.Z_BUF_ERROR
    assert rc == next(c for c in firsts if c != zhost.Z_OK)
