"""Blocking batch inflate with LONG items (a deflate body of ZGPU_BATCH_PIECES_MIN_BYTES or more, 128 KiB unless set): such an item is cut into pieces at
block starts found by search and the pieces of all long items of a call share their launches (zgpu_inflate_batch_pieces.hip); short items, and long ones
that fall back, go to the one-workgroup decoder as before.  Streams come from Python's zlib.  Bytes, in_used and both checks must be Python's; verdicts on
damaged, cut and too-large items must be the one-workgroup decoder's, which the same process produces with the feature switched off; Engine.batch_piece_counts()
says which way the long items went.  Sizes are the smallest that reach the piece path at its default threshold: 150-600 KiB of compressed data per
long item.  Smaller ones -- hand-built items of 49-140 KiB behind a lowered threshold, shaped as zlib's encoder never shapes them -- are
tests/test_gpu_batch_pieces_built.py's."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIN = 131072
HDR = {"raw": 0, "zlib": 2, "gzip": 10}
OK, DATA_ERROR, BUF_ERROR = 0, -3, -5
KNOBS = ("ZGPU_BATCH_PIECES_MIN_BYTES", "ZGPU_BATCH_PIECES_ROUND_BYTES", "ZGPU_BATCH_PIECES_NO_SCRATCH")


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def default_knobs():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


@pytest.fixture(scope="module")
def text(eng):
    """8 MiB of the Silesia-like corpus, made once on the device"""
    import torch
    src = torch.empty(128 * 65536, dtype=torch.uint8, device="cuda")
    eng.corpus_fill_device(0, 0x5EED5117, 500, 128, src.data_ptr())
    return src.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(12).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=-15, zdict=None):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy, zdict) if zdict is not None else zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return co.compress(data) + co.flush()


def wrapped(body, data, wrap):
    """a raw deflate body in the wrapper `wrap`"""
    if wrap == "zlib":
        return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(data))
    if wrap == "gzip":
        return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)
    return body


def exact_body(data, filler, wrap, length):
    """(stream, plaintext): a stream in `wrap` whose bytes behind the header -- deflate data and trailer -- are exactly `length`: `data` at level 6 up to a
    full flush, then stored blocks of `filler`, the last one final"""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush(zlib.Z_FULL_FLUSH)
    left = length - {"raw": 0, "zlib": 4, "gzip": 8}[wrap] - len(body)
    assert left >= 5
    plain, at = data, 0
    while left > 5 + 65535 + 5:
        body += b"\x00" + struct.pack("<HH", 65535, 0) + filler[at: at + 65535]
        plain += filler[at: at + 65535]; at += 65535; left -= 5 + 65535
    n = left - 5
    body += b"\x01" + struct.pack("<HH", n, n ^ 0xFFFF) + filler[at: at + n]
    plain += filler[at: at + n]
    s = wrapped(body, plain, wrap)
    assert len(s) - HDR[wrap] == length
    return s, plain


def run_host(eng, streams, caps, wrap, checks=3):
    """zgpu_inflate_batch_host; one (code, msg, out_bytes, in_used, adler32, crc32, data) per item -- out_bytes of every record, data of the good ones"""
    import zlib_amd.gpu as G
    n = len(streams)
    ioffs = np.zeros(n + 1, dtype=np.uint64); ioffs[1:] = np.cumsum([len(s) for s in streams])
    ooffs = np.zeros(n + 1, dtype=np.uint64); ooffs[1:] = np.cumsum(caps)
    blob = np.frombuffer(b"".join(streams) + b"\0", dtype=np.uint8)
    out = np.zeros(int(ooffs[-1]) + 1, dtype=np.uint8)
    items = (G.InflateItem * n)()
    failed = C.c_uint64(0)
    rc = eng.L.zgpu_inflate_batch_host(eng.h, blob.ctypes.data, int(ioffs[-1]), ioffs.ctypes.data, n, G._WRAPS[wrap], checks, out.ctypes.data, int(ooffs[-1]), ooffs.ctypes.data,
                                       items, C.byref(failed))
    assert rc == 0, rc
    res = []
    for k, it in enumerate(items):
        data = out[int(ooffs[k]): int(ooffs[k]) + it.out_bytes].tobytes() if it.code == OK else b""
        res.append((it.code, eng.L.zgpu_inflate_message(it.msg).decode(), it.out_bytes, it.in_used, it.adler32, it.crc32, data))
    return res


def count_long(streams, wrap):
    return sum(1 for s in streams if len(s) - HDR[wrap] >= MIN)


def delta(eng, before):
    after = eng.batch_piece_counts()
    return after[0] - before[0], after[1] - before[1]


@pytest.fixture(scope="module")
def mixed(text, noise):
    """the raw bodies of the mixed batch and what they decode to (the two bodies of exact length depend on the wrapper: made per wrapper)"""
    K = 768 << 10
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    t7 = text[6 * K: 7 * K]
    flushed = co.compress(t7[:200000]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(t7[200000:450000]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(t7[450000:]) + co.flush()
    return [
        (raw_deflate(text[:4096]), text[:4096]),
        (raw_deflate(text[0:K], 6), text[0:K]),
        None,  # an empty input
        (raw_deflate(noise[:300000], 6), noise[:300000]),  # stored blocks
        (raw_deflate(text[K: 2 * K], 1), text[K: 2 * K]),
        (raw_deflate(text[2 * K: 3 * K], 6, zlib.Z_FIXED), text[2 * K: 3 * K]),
        (raw_deflate(text[3 * K: 5 * K], 6, wbits=-9), text[3 * K: 5 * K]),
        (flushed, t7),
    ]


@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
def test_mixed_batch_long_items_go_in_pieces(eng, mixed, text, noise, wrap):
    """Fails without the feature: the counter of items decoded in pieces must rise by the number of long items, the fallback counter by none."""
    streams, datas = [], []
    for m in mixed:
        streams.append(b"" if m is None else wrapped(m[0], m[1], wrap))
        datas.append(None if m is None else m[1])
    for length in (MIN - 1, MIN):
        s, d = exact_body(text[5 << 20: (5 << 20) + 250000], noise, wrap, length)
        streams.append(s); datas.append(d)
    nlong = count_long(streams, wrap)
    assert nlong == 7, [len(s) for s in streams]  # all but the 4 KiB item, the empty one and the body of MIN - 1
    before = eng.batch_piece_counts()
    res = run_host(eng, streams, [len(d) if d is not None else 16 for d in datas], wrap)
    got = delta(eng, before)
    for k, (r, s, d) in enumerate(zip(res, streams, datas)):
        if d is None:
            assert r[0] == DATA_ERROR, (k, r[:6])
            continue
        assert r[:6] == (OK, "", len(d), len(s), zlib.adler32(d), zlib.crc32(d)), (k, r[:6], len(s), len(d))
        assert r[6] == d, k
    assert got == (nlong, 0), got


def test_first_piece_of_an_item_has_nothing_in_front_of_it(eng, text):
    """Item 1 was compressed behind a dictionary that is the end of item 0's plaintext and begins with bytes copied from it.  Decoded with no dictionary it
    is an error, although those very bytes lie right in front of it in the output.  What this pins is the verdict, not which kernel gives it: a first
    piece decoded as if a window lay in front of it would have its markers flagged by the resolve pass and fall back to the same record."""
    first = text[: 256 << 10]
    zdict = first[-32768:]
    data = zdict[1000:9000] + text[1 << 20: (1 << 20) + (768 << 10)]
    body = raw_deflate(data, 6, zdict=zdict)
    assert len(body) >= MIN
    with pytest.raises(zlib.error):
        zlib.decompress(body, -15)
    res = run_host(eng, [raw_deflate(first), body], [len(first), len(data)], "raw")
    assert res[0][0] == OK and res[0][6] == first
    assert res[1][:2] == (DATA_ERROR, "invalid distance too far back"), res[1][:6]


def test_an_item_ends_where_its_table_says(eng, text, noise):
    """A cut item is an error and the valid stream right behind it in the buffer is not read as its continuation; noise behind a trailer is left alone.
    The verdicts are pinned; that the pieces' own reads end with the item is covered only through them (a piece that ran on would break the chain and
    fall back to the same record)."""
    K = 768 << 10
    long_data, small = text[:K], text[K: K + 50000]
    body = raw_deflate(long_data)
    cut = body[: len(body) * 2 // 3]
    assert len(cut) >= MIN
    res = run_host(eng, [cut, raw_deflate(small)], [K, len(small)], "raw")
    assert res[0][0] == DATA_ERROR, res[0][:6]
    assert res[1][0] == OK and res[1][6] == small
    z = zlib.compress(long_data, 6)
    before = eng.batch_piece_counts()
    res = run_host(eng, [z + noise[:5000], zlib.compress(small)], [K, len(small)], "zlib")
    assert res[0][:4] == (OK, "", K, len(z)) and res[0][6] == long_data
    assert res[1][0] == OK and res[1][6] == small
    assert delta(eng, before) == (1, 0)


def test_verdicts_are_the_one_workgroup_decoders(eng, text):
    """One long zlib item, damaged and in rooms of three sizes, with the feature on and off in one process: the records and bytes are equal.  Almost every
    single bit flip in this stream leaves the deflate syntax whole (the codes are complete: the bits still decode, to other bytes), so the flips AT 1/7 and
    1/2 of the body chain cleanly in pieces and fail their Adler-32, on both paths alike.  The damage that must fall back is the nearest flip behind each of
    the two places that zlib rejects while it decodes -- positions fixed for this seeded corpus, found with zlib on the CPU, and checked here against
    zlib's own message before anything is asserted about the counters."""
    K = 768 << 10
    data = text[2 << 20: (2 << 20) + K]
    z = zlib.compress(data, 6)
    body = len(z) - 6

    def flip(at, bit=0x10):
        b = bytearray(z); b[at] ^= bit
        return bytes(b)
    syntax = {"damage 1/7": "invalid stored block lengths", "damage 1/2": "invalid literal/length code"}
    variants = [("flip 1/7", flip(2 + body // 7), K), ("flip 1/2", flip(2 + body // 2), K), ("damage 1/7", flip(2 + body // 7 + 1743, 0x80), K),
                ("damage 1/2", flip(2 + body // 2 + 4318, 0x80), K), ("flip adler", flip(len(z) - 2), K), ("room - 1", z, K - 1), ("room", z, K), ("room * 64", z, 64 * K)]
    for name, s, cap in variants:
        before = eng.batch_piece_counts()
        on = run_host(eng, [s], [cap], "zlib")[0]
        went = delta(eng, before)
        os.environ["ZGPU_BATCH_PIECES_MIN_BYTES"] = "0"
        before = eng.batch_piece_counts()
        off = run_host(eng, [s], [cap], "zlib")[0]
        assert delta(eng, before) == (0, 0), name
        del os.environ["ZGPU_BATCH_PIECES_MIN_BYTES"]
        assert on == off, (name, on[:6], off[:6])
        try:
            accepted = zlib.decompress(s) == data
            why = ""
        except zlib.error as e:
            accepted, why = False, str(e)
        assert (on[0] == OK) == (accepted and cap >= K), (name, on[:6], why)
        if name in syntax:
            assert syntax[name] in why, (name, why)  # (the fixed position still is what it was found to be)
            assert on[0] == DATA_ERROR and on[1] != "incorrect data check", (name, on[:6])
        if name in syntax or name == "room - 1":
            assert went == (0, 1), (name, went, why)  # damage the decoder sees, a room too small: the item fell back
        elif name in ("room", "room * 64", "flip adler"):
            assert went == (1, 0), (name, went)
        else:
            assert went[0] + went[1] == 1, (name, went)


def test_false_starts_inside_stored_blocks(eng, text):
    inner = b"".join(zlib.compress(text[i: i + (256 << 10)], 6) for i in range(0, 2 << 20, 256 << 10))[: 600 << 10]
    streams = [raw_deflate(inner, 0), raw_deflate(inner, 6)]
    assert count_long(streams, "raw") == 2
    before = eng.batch_piece_counts()
    res = run_host(eng, streams, [len(inner)] * 2, "raw")
    went = delta(eng, before)
    for r in res:
        assert r[0] == OK and r[6] == inner, r[:6]
    assert went[0] + went[1] == 2, went


def test_rounds(eng, text):
    os.environ["ZGPU_BATCH_PIECES_ROUND_BYTES"] = str(1 << 20)
    datas = [text[i << 20: (i + 1) << 20] for i in range(6)]
    streams = [zlib.compress(d, 6) for d in datas]
    assert count_long(streams, "zlib") == 6
    before = eng.batch_piece_counts()
    res = run_host(eng, streams, [len(d) for d in datas], "zlib")
    for k, (r, s, d) in enumerate(zip(res, streams, datas)):
        assert r[:6] == (OK, "", len(d), len(s), zlib.adler32(d), zlib.crc32(d)) and r[6] == d, (k, r[:6])
    assert delta(eng, before) == (6, 0)


def test_device_entry_on_a_stream_and_the_packed_call(eng, text):
    import torch
    import zlib_amd.gpu as G
    K = 512 << 10
    datas = [text[:3000], text[K: 2 * K], text[5000:9000], text[2 * K: 3 * K], b"", text[3 * K: 4 * K + 777]]
    zs = [zlib.compress(d, 6) for d in datas]
    zs[2] = zs[2][:-1]  # one bad short item
    caps = [len(d) for d in datas]
    nlong = count_long(zs, "zlib")
    assert nlong == 3
    host = run_host(eng, zs, caps, "zlib")
    n = len(zs)
    dev = torch.device("cuda", 0)
    ioffs = np.zeros(n + 1, dtype=np.uint64); ioffs[1:] = np.cumsum([len(z) for z in zs])
    ooffs = np.zeros(n + 1, dtype=np.uint64); ooffs[1:] = np.cumsum(caps)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        d_in = torch.tensor(np.frombuffer(b"".join(zs), dtype=np.uint8), device=dev)
        d_io = torch.tensor(ioffs.view(np.int64), device=dev)
        d_oo = torch.tensor(ooffs.view(np.int64), device=dev)
        d_out = torch.zeros(int(ooffs[-1]) + 1, dtype=torch.uint8, device=dev)
        d_items = torch.zeros(n * C.sizeof(G.InflateItem), dtype=torch.uint8, device=dev)
        before = eng.batch_piece_counts()
        failed = eng.inflate_batch_device(d_in.data_ptr(), int(ioffs[-1]), d_io.data_ptr(), n, d_out.data_ptr(), int(ooffs[-1]), d_oo.data_ptr(), d_items.data_ptr(),
                                          wrap="zlib", checks=3, stream=st.cuda_stream)
        went = delta(eng, before)
        st.synchronize()
        raw = d_items.cpu().numpy().tobytes()
        out = d_out.cpu().numpy()
    assert failed == 1 and went == (nlong, 0), (failed, went)
    for k in range(n):
        it = G.InflateItem.from_buffer_copy(raw, k * C.sizeof(G.InflateItem))
        assert (it.code, eng.L.zgpu_inflate_message(it.msg).decode(), it.out_bytes, it.in_used, it.adler32, it.crc32) == host[k][:6], k
        if it.code == OK:
            assert out[int(ooffs[k]): int(ooffs[k]) + it.out_bytes].tobytes() == host[k][6] == datas[k]
    before = eng.batch_piece_counts()
    packed, recs = eng.inflate_batch_packed_host(zs, wrap="zlib", checks=3)
    assert delta(eng, before) == (nlong, 0)
    for k in range(n):
        assert recs[k][0] == host[k][0] and packed[k] == host[k][6], k


def test_gzip_file_of_long_members(eng, text):
    """zgpu_gzip_inflate_host: its trial decode (candidates that overlap in the input) stays on the one-workgroup decoder, its final decode takes the
    members in pieces.  Between the two long members lies a stored member that holds a planted signature with a plausible size in front of it (the
    shape of test_plausible_wrong_guess_takes_the_second_pass): the trial layout gives the decoy room, the layout moves, the second decode runs."""
    import gzip
    a, b = text[: 700 << 10], text[1 << 20: (1 << 20) + (900 << 10)]
    payload = b"A" * 96 + struct.pack("<I", 50) + b"\x1f\x8b\x08\x00" + b"B" * 60
    data = gzip.compress(a, 6) + gzip.compress(payload, 0) + gzip.compress(b, 6)
    passes = eng.gzip_members_count()
    before = eng.batch_piece_counts()
    rc, out, ioffs, ooffs, items = eng.gzip_inflate_host(data)
    went = delta(eng, before)
    second = eng.gzip_members_count()[1] - passes[1]
    assert rc == 0 and out == a + payload + b and eng.last_members == 3
    assert second == 1, (second, went)
    assert went == (2, 0), went


def test_a_round_without_scratch_goes_to_the_one_workgroup_decoder(eng, text):
    """ZGPU_BATCH_PIECES_NO_SCRATCH=1 declines every round as a failed reservation does: no error of the call, every long item falls back, bytes and
    records are right; the next call, with scratch, goes in pieces again."""
    datas = [text[i << 20: (i << 20) + (768 << 10)] for i in range(3)] + [text[:5000]]
    streams = [zlib.compress(d, 6) for d in datas]
    assert count_long(streams, "zlib") == 3
    for knob, want in (("1", (0, 3)), (None, (3, 0))):
        if knob:
            os.environ["ZGPU_BATCH_PIECES_NO_SCRATCH"] = knob
        before = eng.batch_piece_counts()
        try:
            res = run_host(eng, streams, [len(d) for d in datas], "zlib")
        finally:
            os.environ.pop("ZGPU_BATCH_PIECES_NO_SCRATCH", None)
        for k, (r, s, d) in enumerate(zip(res, streams, datas)):
            assert r[:6] == (OK, "", len(d), len(s), zlib.adler32(d), zlib.crc32(d)) and r[6] == d, (knob, k, r[:6])
        assert delta(eng, before) == want, knob
