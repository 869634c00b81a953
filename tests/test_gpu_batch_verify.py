"""The batch integrity test, zgpu_inflate_batch_verify_* and zgpu_bgzf_verify_*: every item decoded in full inside the workgroup, its check values
folded where the decoder would flush, its trailer compared -- and no destination anywhere.  The truth is Python's zlib (sizes, Adler-32, CRC-32) and,
differentially, the project's own batch decoder given ranges of exactly the right size: record k of the test must equal the decoder's record k field
for field."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cases, handmade as H  # noqa: E402
from tests import batch_sizes_fixtures as F  # noqa: E402
from tests.batch_sizes_fixtures import DATA_ERROR, NEED_DICT, OK, STREAM_ERROR, TRUNCATED  # noqa: E402

ADLER, CRC = 1, 2
DATA_CHECK, LENGTH_CHECK = "incorrect data check", "incorrect length check"


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


def verify_call(eng, zs, wrap, checks=0):
    """zgpu_inflate_batch_verify_host through ctypes: (rc, nfailed, [(code, message, out_bytes, in_used, adler32, crc32)])"""
    from zlib_amd import gpu
    n = len(zs)
    blob, offs = F.pack(zs)
    recs = (gpu.InflateItem * max(n, 1))()
    failed = C.c_uint64(99)
    rc = eng.L.zgpu_inflate_batch_verify_host(eng.h, blob.ctypes.data, int(offs[-1]), offs.ctypes.data, n, gpu._WRAPS[wrap], checks, recs, C.byref(failed))
    return rc, failed.value, [F.record(eng, recs[k]) for k in range(n)]


def decoder_records(eng, zs, caps, wrap, checks):
    """the batch decoder's records in the shape of the test's: (code, message, out_bytes, in_used, adler32, crc32)"""
    return [(c, m, len(data), used, a, crc) for c, m, data, used, a, crc in eng.inflate_batch_host(zs, caps, wrap=wrap, checks=checks)]


def truth(d, z, wrap, checks):
    """the record of a good item: the check the wrapper needs is always computed (auto: both), the others as `checks` asks, else 1 / 0"""
    w = wrap if wrap != "auto" else "both"
    do_adler, do_crc = (checks & ADLER) or w in ("zlib", "both"), (checks & CRC) or w in ("gzip", "both")
    return (OK, "", len(d), len(z), zlib.adler32(d) if do_adler else 1, zlib.crc32(d) if do_crc else 0)


@pytest.mark.parametrize("wrap,checks", [("raw", 0), ("raw", ADLER | CRC), ("zlib", 0), ("gzip", ADLER), ("auto", 0)])
def test_whole_catalogue(eng, wrap, checks):
    pairs = F.streams(wrap)
    zs = [z + F.JUNK for _, z in pairs]
    rc, failed, recs = verify_call(eng, zs, wrap, checks)
    assert rc == OK and failed == 0
    bad = [(k, r, truth(d, z, wrap, checks)) for k, ((d, z), r) in enumerate(zip(pairs, recs)) if r != truth(d, z, wrap, checks)]
    assert not bad, bad[:5]
    assert recs == decoder_records(eng, zs, [len(d) for d, _ in pairs], wrap, checks)
    # the Python wrapper gives the same records
    assert eng.inflate_batch_verify_host(zs[:20], wrap, checks) == recs[:20] and eng.last_failed == 0


RING_SIZES = [0, 1, 63, 64, 65, 16383, 16384, 16385, 32767, 32768, 32769, 49151, 49152, 49153, 65535, 65536, 65537, 81921]


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_ring_boundaries(eng, wrap):
    """decoded sizes around every half of the 32 KiB ring: text through the token path, random bytes as stored blocks (through the ring half by
    half), zeros as chains of length-258 matches at distance 1 across every flush"""
    pairs = []
    for n in RING_SIZES:
        for kind, level in (("text", 6), ("rand", 0), ("zeros", 9)):
            d = cases.make(kind, n, 13)
            z = F.deflate(d, level, wrap)
            assert zlib.decompress(z, F.WBITS[wrap]) == d
            pairs.append((d, z))
    rc, failed, recs = verify_call(eng, [z for _, z in pairs], wrap, ADLER | CRC)
    assert rc == OK and failed == 0
    bad = [(len(d), k % 3, r, truth(d, z, wrap, ADLER | CRC)) for k, ((d, z), r) in enumerate(zip(pairs, recs)) if r != truth(d, z, wrap, ADLER | CRC)]
    assert not bad, bad[:5]


def _truth_without_dictionary(c):
    """a hand-built case as a raw item of a batch, which has no preset dictionary: (kind, decoded size) by Python's zlib where the case wants one"""
    if not c.dictionary:
        return c.kind, (len(c.expect) if c.expect is not None else None)
    o = zlib.decompressobj(-15)
    try:
        n = len(o.decompress(c.stream))
    except zlib.error:
        return "bad", None
    return ("ok" if o.eof else "cut"), n


def test_hand_built_streams(eng, golden):
    g = golden("handmade_inflate.json")["cases"]
    cat = H.catalogue()
    assert sorted(c.name for c in cat) == sorted(g)
    zs = [c.stream for c in cat]
    kinds = [_truth_without_dictionary(c) for c in cat]
    rc, failed, recs = verify_call(eng, zs, "raw", ADLER | CRC)
    assert rc == OK
    # differential, no case left out: the decoder's records for the same items, every range exactly as large as the item decodes to
    caps = [n if kind in ("ok", "trailing") else 0 for kind, n in kinds]
    dec = decoder_records(eng, zs, caps, "raw", ADLER | CRC)
    bad = [(c.name, r, d) for c, r, d in zip(cat, recs, dec) if r != d]
    assert not bad, bad[:10]
    assert failed == sum(1 for r in recs if r[0] != OK) == eng.last_failed
    assert all(r[0] in (OK, DATA_ERROR) for r in recs)
    # the good ones, wrapped: the trailer is compared against what the ring held
    good = [c for c in cat if c.kind == "ok" and not c.dictionary]
    assert len(good) > 20
    for wrap in ("zlib", "gzip"):
        ws = [(b"\x78\x9c" + c.stream + struct.pack(">I", zlib.adler32(c.expect))) if wrap == "zlib" else F.gzip_member(c.stream, c.expect) for c in good]
        rc, failed, recs = verify_call(eng, ws, wrap, ADLER | CRC)
        assert rc == OK
        bad = [(c.name, r) for c, w, r in zip(good, ws, recs) if r != truth(c.expect, w, wrap, ADLER | CRC)]
        assert not bad and failed == 0, bad[:10]


def _flip(s, at, bit=0x10):
    at %= len(s)
    return s[:at] + bytes([s[at] ^ bit]) + s[at + 1:]


def test_trailers(eng):
    """the point of the call: a stream whose deflate data is valid and whose trailer does not match what it decodes to"""
    d = cases.make("text", 5000, 21)
    z, gz = zlib.compress(d, 6), F.gzip_member(F.deflate(d, 6, "raw"), d)
    z0, gz0 = zlib.compress(d, 0), F.gzip_member(F.deflate(d, 0, "raw"), d)
    assert z0[7:7 + 100] == d[:100]  # (header 2, stored block header 5: the payload follows)
    broken = [
        (_flip(z, -2), DATA_CHECK),                                   # a byte of the Adler-32
        (_flip(gz, -7), DATA_CHECK),                                  # a byte of the CRC-32
        (gz[:-4] + struct.pack("<I", len(d) + 1), LENGTH_CHECK),      # ISIZE + 1
        (_flip(z0, 7 + 50), DATA_CHECK),                              # a payload byte of a stored block: the deflate data stays valid
        (_flip(gz0, 10 + 5 + 50), DATA_CHECK),
        (z[:-2], TRUNCATED),                                          # the final block is there, the trailer is not
        (gz[:-2], TRUNCATED),
    ]
    for s, _ in broken[:5]:  # (Python's zlib agrees that these decode and then fail their check)
        o = zlib.decompressobj(47)
        with pytest.raises(zlib.error):
            o.decompress(s)
    good = [z, gz, z0, gz0, z, gz, z, gz]
    rc, failed, clean = verify_call(eng, good, "auto")
    assert rc == OK and failed == 0
    assert clean == [truth(d, s, "auto", 0) for s in good]
    mixed = []
    for k, s in enumerate(good):
        mixed.append(s)
        if k < len(broken):
            mixed.append(broken[k][0])
    rc, failed, recs = verify_call(eng, mixed, "auto")
    assert rc == OK and failed == len(broken)
    assert [r for r in recs if r[0] == OK] == clean  # the good neighbours' records do not change
    got = [r for r in recs if r[0] != OK]
    assert [r[:4] for r in got] == [(DATA_ERROR, msg, 0, 0) for _, msg in broken]
    # ... and they are the decoder's, check values of a failed item included
    caps = [len(d)] * len(mixed)
    assert recs == decoder_records(eng, mixed, caps, "auto", 0)
    # the sizing pass sees nothing wrong with the first five: their deflate data is valid
    rc, sfailed, sized = F.sizes_call(eng, mixed, "auto")
    assert rc == OK and sfailed == 2
    assert [r[:3] for r, v in zip(sized, recs) if v[0] != OK][:5] == [(OK, "", len(d))] * 5


def _damage_items():
    d = cases.make("mix", 9000, 31)
    z = zlib.compress(d, 6)
    gz = F.gzip_member(F.deflate(d, 6, "raw"), d, name=b"file.txt", comment=b"c", hcrc=True)
    fdict = bytearray([0x78, 0x20])
    fdict[1] += 31 - ((fdict[0] << 8) | fdict[1]) % 31
    good = [z, gz, zlib.compress(b""), zlib.compress(cases.make("text", 70000, 2), 9), gz, z]
    damaged = {
        0: (z[: len(z) // 2], DATA_ERROR, TRUNCATED),                          # cut inside a block
        1: (bytes([0x78, 0x9D]) + z[2:], DATA_ERROR, "incorrect header check"),
        2: (bytes(fdict) + b"\0\0\0\1" + z[2:], NEED_DICT, ""),
        3: (b"", DATA_ERROR, TRUNCATED),
        4: (gz[:14] + bytes([gz[14] ^ 1]) + gz[15:], DATA_ERROR, "header crc mismatch"),  # (a byte of the name, under the header CRC)
        5: (z[:-2], DATA_ERROR, TRUNCATED),                                   # the final block is there, the trailer is not
    }
    sizes = [len(zlib.decompressobj(47).decompress(s)) for s in good]
    return good, damaged, sizes


def test_damage_and_headers_in_a_batch(eng):
    good, damaged, sizes = _damage_items()
    mixed, caps = [], []
    for k, s in enumerate(good):
        mixed += [s, damaged[k][0]]
        caps += [sizes[k], sizes[k] if k == 5 else 0]  # (item 5 decodes to its end: a range of exactly that size; the others fail whatever the room)
    rc, failed, recs = verify_call(eng, mixed, "auto", ADLER | CRC)
    assert rc == OK and failed == len(damaged)
    for k in range(len(good)):
        assert recs[2 * k][:4] == (OK, "", sizes[k], len(good[k])), k
        assert recs[2 * k + 1][:4] == (damaged[k][1], damaged[k][2], 0, 0), (k, recs[2 * k + 1])
    assert recs == decoder_records(eng, mixed, caps, "auto", ADLER | CRC)


def test_more_than_one_launch_round(eng):
    d = cases.make("text", 100, 5)
    e, last = zlib.compress(b""), zlib.compress(d)
    n = 65537
    rc, failed, recs = verify_call(eng, [e] * (n - 1) + [last], "zlib")
    assert rc == OK and failed == 0
    bad = [k for k in range(n - 1) if recs[k] != (OK, "", 0, len(e), 1, 0)]
    assert not bad, bad[:10]
    assert recs[n - 1] == (OK, "", len(d), len(last), zlib.adler32(d), 0)


def test_arguments(eng):
    from zlib_amd import gpu
    z = zlib.compress(b"abc")
    blob, offs = F.pack([z, z])
    recs = (gpu.InflateItem * 2)()
    failed = C.c_uint64(0)
    call = eng.L.zgpu_inflate_batch_verify_host
    assert call(eng.h, None, 0, None, 0, gpu.WRAP_ZLIB, 0, None, None) == OK  # nothing to do
    assert call(eng.h, blob.ctypes.data, int(offs[-1]), offs.ctypes.data, 2, 4, 0, recs, C.byref(failed)) == STREAM_ERROR  # no such wrapper
    assert call(eng.h, blob.ctypes.data, int(offs[-1]), offs.ctypes.data, 2, gpu.WRAP_ZLIB, 4, recs, C.byref(failed)) == STREAM_ERROR  # no such check
    assert call(eng.h, blob.ctypes.data, int(offs[-1]), offs.ctypes.data, 2, gpu.WRAP_ZLIB, 0, None, C.byref(failed)) == STREAM_ERROR
    out = np.array([0, len(z), 2 * len(z) + 1], dtype=np.uint64)  # leaves the buffer
    assert call(eng.h, blob.ctypes.data, int(offs[-1]), out.ctypes.data, 2, gpu.WRAP_ZLIB, 0, recs, C.byref(failed)) == STREAM_ERROR


def test_device_entry_matches_host(eng):
    import torch
    import zlib_amd
    from zlib_amd import gpu
    good, damaged, _ = _damage_items()
    d = cases.make("text", 5000, 21)
    zs = list(good) + [damaged[0][0], damaged[2][0], _flip(zlib.compress(d, 6), -2)] + [z + F.JUNK for _, z in F.streams("zlib")[-2:]]
    rc, failed, host = verify_call(eng, zs, "auto", ADLER | CRC)
    assert rc == OK and failed == 3
    n = len(zs)
    dev = torch.device("cuda", 0)
    blob, offs = F.pack(zs)
    d_in = torch.tensor(blob, device=dev)
    d_io = torch.tensor(offs.view(np.int64), device=dev)
    d_bad = torch.tensor(offs[::-1].copy().view(np.int64), device=dev)  # runs backwards
    isz = C.sizeof(gpu.InflateItem)
    d_items = torch.zeros(n * isz, dtype=torch.uint8, device=dev)
    assert eng.inflate_batch_verify_device(d_in.data_ptr(), int(offs[-1]), d_io.data_ptr(), n, d_items.data_ptr(), wrap="auto", checks=ADLER | CRC) == 3
    assert eng.last_failed == 3
    raw = d_items.cpu().numpy().tobytes()
    assert [F.record(eng, gpu.InflateItem.from_buffer_copy(raw, k * isz)) for k in range(n)] == host
    # a table that runs backwards is refused by both entries
    with pytest.raises(zlib_amd.EngineError) as ex:
        eng.inflate_batch_verify_device(d_in.data_ptr(), int(offs[-1]), d_bad.data_ptr(), n, d_items.data_ptr(), wrap="auto")
    assert ex.value.code == STREAM_ERROR
    back = offs[::-1].copy()
    recs = (gpu.InflateItem * n)()
    assert eng.L.zgpu_inflate_batch_verify_host(eng.h, blob.ctypes.data, int(offs[-1]), back.ctypes.data, n, gpu.WRAP_AUTO, 0, recs, None) == STREAM_ERROR


def _nblocks(f):
    """blocks of a file whose headers are the encoder's (18 bytes, BSIZE in the last two)"""
    pos, n = 0, 0
    while pos + 18 <= len(f):
        pos += struct.unpack("<H", f[pos + 16: pos + 18])[0] + 1
        n += 1
    return n


def _bgzf_both(eng, f):
    """(rc, out_bytes, first_bad_chunk, error_code, error_msg, [block records]) of the decode and of the test of the same file"""
    out = []
    for verify in (False, True):
        if verify:
            rc, items = eng.bgzf_verify_host(f)
        else:
            rc, _, items = eng.bgzf_inflate_host(f)
        r = eng.last_inflate
        ran = rc == OK or (rc == DATA_ERROR and r.first_bad_chunk >= 0)  # (else the chain was bad: no block was looked at)
        out.append((rc, r.out_bytes, r.first_bad_chunk, r.error_code, r.error_msg, [F.record(eng, items[k]) for k in range(_nblocks(f) if ran else 0)]))
    return out


def test_bgzf(eng):
    data = cases.make("text", 200000, 9)
    f, offs = eng.bgzf_deflate_host(data, 6, want_offsets=True)
    dec, ver = _bgzf_both(eng, f)
    assert ver == dec and ver[:3] == (OK, len(data), -1) and len(ver[5]) == 5  # four blocks of data and the end block
    at = int(offs[1]) + 18 + 100  # a body byte of block 1
    dec, ver = _bgzf_both(eng, _flip(f, at))
    assert ver == dec and ver[0] == DATA_ERROR and ver[2] == 1 and ver[3] == DATA_ERROR
    assert [r[0] for r in ver[5]] == [OK, DATA_ERROR, OK, OK, OK]
    # a block that decodes to more than its ISIZE says: the decode has no room for it, the test has no room at all -- one verdict
    isz_at = int(offs[2]) - 4
    short = f[:isz_at] + struct.pack("<I", struct.unpack("<I", f[isz_at:isz_at + 4])[0] - 1) + f[isz_at + 4:]
    dec, ver = _bgzf_both(eng, short)
    assert ver == dec and ver[0] == DATA_ERROR and ver[2] == 1 and eng.L.zgpu_inflate_message(ver[4]).decode() == LENGTH_CHECK
    dec, ver = _bgzf_both(eng, f[:-28])  # no end block: a valid file all the same
    assert ver == dec and ver[:3] == (OK, len(data), -1)
    dec, ver = _bgzf_both(eng, f[:-5])  # the chain does not reach the end
    assert ver[:5] == dec[:5] and ver[0] == DATA_ERROR and ver[2] == -1
