"""The hand-built DEFLATE streams of oracle/handmade.py through every device path of inflate: the end-to-end decoder (32 KiB ring), segments
of at most 64 KiB through rings of 8, 16 and 32 KiB (the far-match path), the decoder of streams without a side table (the pieces decoder for
the long cases), and inflate() of the zlib API, raw and zlib-wrapped, at assorted input / output steps.  A valid stream must give exactly
expand()'s bytes (and their Adler-32 / CRC-32); an invalid one Z_DATA_ERROR with the reference's message (tests/golden/handmade_inflate.json).
What comes out in front of an error is not compared."""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import handmade as H  # noqa: E402


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cat():
    return H.catalogue()


@pytest.fixture(scope="module")
def gold(golden, cat):
    g = golden("handmade_inflate.json")["cases"]
    assert sorted(c.name for c in cat) == sorted(g)
    for c in cat:
        assert [len(c.stream), H.sha16(c.stream)] == g[c.name]["stream"], c.name
    return g


def _cap(c):
    return len(c.expect) if c.expect is not None else 1 << 20


def _verdict(c, g, call, bad, where):
    """run call(); compare with what the case must give"""
    import zlib_amd
    try:
        out = call()
    except zlib_amd.EngineError as ex:
        if c.kind == "bad" and (ex.code != -3 or g["msg"] not in str(ex)):
            bad.append((c.name, where, "error %d %s, want %s" % (ex.code, ex, g["msg"])))
        elif c.kind == "cut" and ex.code not in (-3, -5):
            bad.append((c.name, where, "error %d %s" % (ex.code, ex)))
        elif c.kind == "trailing" and "after its last block" not in str(ex):
            bad.append((c.name, where, str(ex)))
        elif c.kind == "ok":
            bad.append((c.name, where, "error %d %s" % (ex.code, ex)))
        return None
    if c.kind != "ok":
        bad.append((c.name, where, "decoded %d bytes, want an error" % len(out)))
    elif out != c.expect:
        n = min(len(out), len(c.expect))
        diff = next((i for i in range(n) if out[i] != c.expect[i]), n)
        bad.append((c.name, where, "%d bytes, want %d; first difference at %d" % (len(out), len(c.expect), diff)))
    return out


def _checks(eng, c, bad, where):
    li = eng.last_inflate
    if (li.adler32, li.crc32) != (zlib.adler32(c.expect), zlib.crc32(c.expect)):
        bad.append((c.name, where, "checks"))


def test_whole_stream_decoder(eng, cat, gold):
    """chunk_size WHOLE_STREAM: one workgroup, the 32 KiB ring where position q lands on the slot of q - 32768"""
    from zlib_amd import gpu
    bad = []
    for c in cat:
        eng.inflate_set_dictionary(c.dictionary)
        try:
            offs = np.array([0, len(c.stream)], dtype=np.uint64)
            out = _verdict(c, gold[c.name], lambda: eng.inflate_host(c.stream, offs, chunk_size=gpu.WHOLE_STREAM, out_len=_cap(c)), bad, "whole")
            if out is not None and c.kind == "ok":
                _checks(eng, c, bad, "whole")
        finally:
            eng.inflate_set_dictionary(b"")
    if bad:
        pytest.fail("%d failures:\n" % len(bad) + "\n".join("%s [%s] %s" % x for x in bad))


def _segment_cases(cat):
    """cases whose segments decode to at most 64 KiB each (all but the last to exactly 64 KiB), and small invalid ones"""
    out = []
    for c in cat:
        if c.kind in ("ok", "trailing"):
            if len(c.segs) == 2 and len(c.expect) <= 65536:
                out.append(c)
            elif len(c.segs) > 2:
                out.append(c)
        elif len(c.stream) <= 65536:
            out.append(c)
    return out


def test_segments_through_small_rings(eng, cat, gold, monkeypatch):
    """The layout of the library's own chunked streams (independent segments of 64 KiB), through rings of 8, 16 and 32 KiB: matches
    that reach farther back than the ring read the destination (32 bytes ahead when they are that short)."""
    cases = _segment_cases(cat)
    assert any(c.maxdist == 32768 and not c.dictionary for c in cases) and any(len(c.segs) > 2 for c in cases)
    bad = []
    try:
        for kb in ("8", "16", "32"):
            monkeypatch.setenv("ZGPU_INF_RING_KB", kb)
            for c in cases:
                eng.inflate_set_dictionary(c.dictionary)
                try:
                    offs = np.array(c.segs, dtype=np.uint64)
                    cap = len(c.expect) if c.expect is not None else 65536
                    out = _verdict(c, gold[c.name], lambda: eng.inflate_host(c.stream, offs, chunk_size=65536, out_len=cap), bad, "ring %s" % kb)
                    if out is not None and c.kind == "ok":
                        _checks(eng, c, bad, "ring %s" % kb)
                finally:
                    eng.inflate_set_dictionary(b"")
    finally:
        monkeypatch.delenv("ZGPU_INF_RING_KB", raising=False)
    if bad:
        pytest.fail("%d failures:\n" % len(bad) + "\n".join("%s [%s] %s" % x for x in bad))


def test_stream_decoder_and_pieces(eng, cat, gold):
    """zgpu_inflate_stream_host2 without a side table: the long cases go through the pieces decoder (asserted through spec_counts), the one
    4 MiB block with no start to find does not; the rest through marker search / one workgroup."""
    bad = []
    for c in cat:
        eng.inflate_set_dictionary(c.dictionary)
        try:
            s0, w0 = eng.spec_counts()
            out = _verdict(c, gold[c.name], lambda: eng.inflate_stream_host(c.stream, _cap(c)), bad, "stream")
            s1, w1 = eng.spec_counts()
            if out is not None and c.kind == "ok":
                _checks(eng, c, bad, "stream")
            if c.pieces is True and s1 == s0:
                bad.append((c.name, "stream", "the pieces decoder was not taken"))
            if c.pieces is False and (s1 != s0 or w1 == w0):
                bad.append((c.name, "stream", "pieces %d -> %d, one workgroup %d -> %d" % (s0, s1, w0, w1)))
            if c.kind == "trailing":  # stream mode: the stream ends with its final block, whatever follows
                got = eng.inflate_stream_host(c.stream, _cap(c), flags=1)
                if got != c.expect or eng.last_inflate.stream_end != 1:
                    bad.append((c.name, "stream mode", "%d bytes" % len(got)))
        finally:
            eng.inflate_set_dictionary(b"")
    if bad:
        pytest.fail("%d failures:\n" % len(bad) + "\n".join("%s [%s] %s" % x for x in bad))


def _api(z, wbits, dictionary, cap, in_step, out_step):
    """inflate() of libzamd_z.so driven like a streaming caller; returns (rc, bytes, msg, strm.adler)"""
    import zhost as Z
    L = Z.lib()
    L.inflateSetDictionary.argtypes = [C.POINTER(Z.ZStream), C.c_char_p, C.c_uint]
    s = Z.ZStream()
    assert L.inflateInit2_(C.byref(s), wbits, b"1.2.3", C.sizeof(Z.ZStream)) == Z.Z_OK
    if wbits < 0 and dictionary:
        assert L.inflateSetDictionary(C.byref(s), dictionary, len(dictionary)) == Z.Z_OK
    src = C.create_string_buffer(z, max(len(z), 1))
    out = C.create_string_buffer(max(cap, 1))
    ipos = opos = 0
    in_step = in_step or len(z) or 1
    out_step = out_step or cap or 1
    rc = Z.Z_OK
    for _ in range(20_000_000):
        step, room = min(in_step, len(z) - ipos), min(out_step, cap - opos)
        s.next_in = C.addressof(src) + ipos; s.avail_in = step
        s.next_out = C.addressof(out) + opos; s.avail_out = room
        rc = L.inflate(C.byref(s), Z.Z_FINISH if ipos + step == len(z) else Z.Z_NO_FLUSH)
        took, gave = step - s.avail_in, room - s.avail_out
        ipos += took; opos += gave
        if rc == Z.Z_NEED_DICT:
            assert dictionary
            assert L.inflateSetDictionary(C.byref(s), dictionary, len(dictionary)) == Z.Z_OK
            continue
        if rc == Z.Z_STREAM_END or rc not in (Z.Z_OK, Z.Z_BUF_ERROR):
            break
        if rc == Z.Z_BUF_ERROR and took == 0 and gave == 0 and (ipos == len(z) or opos == cap):
            break
    msg = s.msg.decode() if s.msg else None
    adler = s.adler & 0xFFFFFFFF
    L.inflateEnd(C.byref(s))
    return rc, out.raw[:opos], msg, adler


def _zlib_wrap(c):
    if c.dictionary:
        hdr = bytearray([0x78, 0x20])
        hdr[1] += 31 - ((hdr[0] << 8) | hdr[1]) % 31
        hdr = bytes(hdr) + zlib.adler32(c.dictionary).to_bytes(4, "big")
    else:
        hdr = b"\x78\x9c"
    return hdr + c.stream + zlib.adler32(c.expect if c.expect is not None else b"").to_bytes(4, "big")


def test_zlib_api_inflate_at_assorted_steps(cat, gold):
    """inflate(), raw (inflateSetDictionary up front) and zlib-wrapped (the dictionary when Z_NEED_DICT asks for it): input / output steps of
    everything, 4093 / 65521, and for outputs of at most 64 KiB 100003 / 7 and (short streams) 1 / 1 -- resumption at any bit offset."""
    bad = []
    for c in cat:
        g = gold[c.name]
        steps = [(None, None), (4093, 65521)]
        if c.kind != "ok" or len(c.expect) <= 65536:
            steps.append((100003, 7))
            if len(c.stream) <= 600:
                steps.append((1, 1))
        wraps = [-15] if c.kind == "trailing" else [-15, 15]
        for wbits in wraps:
            z = c.stream if wbits < 0 else _zlib_wrap(c)
            for ist, ost in steps:
                where = "api wbits %d steps %s/%s" % (wbits, ist, ost)
                rc, out, msg, adler = _api(z, wbits, c.dictionary, _cap(c), ist, ost)
                if c.kind in ("ok", "trailing"):
                    if rc != 1 or out != c.expect:
                        bad.append((c.name, where, "rc %d, %d bytes (want %d) %s" % (rc, len(out), len(c.expect), msg)))
                    elif wbits > 0 and adler != zlib.adler32(c.expect):
                        bad.append((c.name, where, "adler"))
                elif c.kind == "bad":
                    if rc != -3 or msg != g["msg"]:
                        bad.append((c.name, where, "rc %d %s, want -3 %s" % (rc, msg, g["msg"])))
                elif rc not in (-3, -5):  # cut short: the input ends before the stream does
                    bad.append((c.name, where, "rc %d %s" % (rc, msg)))
    if bad:
        pytest.fail("%d failures:\n" % len(bad) + "\n".join("%s [%s] %s" % x for x in bad))


def test_rest_of_a_stream_taken_up_at_a_bit_offset(eng, cat, monkeypatch):
    """zgpu_inflate_stream_host3 with a start bit (what inflate() hands over when a call ended inside a byte), in front of a stored block at each
    bit offset: by the pieces, and by the one-workgroup decoder they fall back to (ZGPU_SPEC_DECLINE_AT_BIT).  The stored block aligns to the
    caller's bytes; input that stops early takes nothing and keeps the start bit."""
    from oracle import deflate_writer as W
    from zlib_amd import gpu
    cases = {c.name: c for c in cat}
    bad = []
    for b in range(8):
        c = cases["stored_at_bit%d" % b]
        head = W.literals((H.rnd(20, 610 + b) % 144).tolist() + [200] * ((b - 2) % 8))  # (the case's first block, see oracle/handmade.py)
        nbits = 3 + sum(W.FIXED_LIT[int(x)] for x in head.a) + 7
        assert nbits % 8 == b
        pre = len(W.expand(head))
        for decline in (False, True):
            if decline:
                monkeypatch.setenv("ZGPU_SPEC_DECLINE_AT_BIT", "1")
            else:
                monkeypatch.delenv("ZGPU_SPEC_DECLINE_AT_BIT", raising=False)
            for cut in (0, 40):
                rest = np.frombuffer(c.stream[nbits >> 3: len(c.stream) - cut], dtype=np.uint8)
                out = np.zeros(65536, dtype=np.uint8)
                res = gpu.InflateResult()
                eng.inflate_set_dictionary(c.expect[:pre])
                try:
                    rc = eng.L.zgpu_inflate_stream_host3(eng.h, rest.ctypes.data, rest.size, b, 1, out.ctypes.data, out.size, C.byref(res))
                finally:
                    eng.inflate_set_dictionary(b"")
                got = (rc, out[: res.out_bytes].tobytes(), res.stream_end, res.in_used, res.in_used_bits)
                if cut == 0:
                    want = (0, c.expect[pre:], 1, rest.size, 0)
                else:  # (the stored block is not all there: nothing is decoded yet, the stream still begins at bit b)
                    want = (0, b"", 0, 0, b)
                if got != want:
                    bad.append((c.name, "bit %d decline %d cut %d" % (b, decline, cut), "rc %d, %d bytes, end %d, used %d.%d" % (
                        rc, len(got[1]), res.stream_end, res.in_used, res.in_used_bits)))
    monkeypatch.delenv("ZGPU_SPEC_DECLINE_AT_BIT", raising=False)
    if bad:
        pytest.fail("%d failures:\n" % len(bad) + "\n".join("%s [%s] %s" % x for x in bad))
