"""The sizing pass, zgpu_inflate_batch_sizes_*: every item's decoded size and the verdict of its header and deflate data, with nothing decoded into
memory.  The truth is Python's zlib (the length of what decompressobj gives) and, for verdicts, the project's own batch decoder given ranges of exactly
the right size: the sizing pass must say what that decoder says, minus the trailer checks it cannot make."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cases, handmade as H  # noqa: E402
from tests import batch_sizes_fixtures as F  # noqa: E402
from tests.batch_sizes_fixtures import BUF_ERROR, DATA_ERROR, NEED_DICT, OK, STREAM_ERROR, TRUNCATED  # noqa: E402


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip", "auto"])
def test_sizes_equal_the_truth(eng, wrap):
    pairs = F.streams(wrap)
    for d, z in pairs[:3] + pairs[-2:]:  # (the oracle's own view of these streams)
        assert len(zlib.decompressobj(47 if wrap == "auto" else F.WBITS[wrap]).decompress(z)) == len(d)
    rc, failed, recs = F.sizes_call(eng, [z + F.JUNK for _, z in pairs], wrap)
    assert rc == OK and failed == 0
    bad = [(k, r[:4], len(d), len(z)) for k, ((d, z), r) in enumerate(zip(pairs, recs)) if r != (OK, "", len(d), len(z), 1, 0)]
    assert not bad, bad[:10]
    # the Python wrapper gives the same records
    got = eng.inflate_batch_sizes_host([z + F.JUNK for _, z in pairs[:20]], wrap)
    assert got == [r[:4] for r in recs[:20]] and eng.last_failed == 0


def _truth_without_dictionary(c):
    """a hand-built case as a raw item of a batch, which has no preset dictionary: (kind, decoded size, message) by Python's zlib where the case wants one"""
    if not c.dictionary:
        return c.kind, (len(c.expect) if c.expect is not None else None), None
    o = zlib.decompressobj(-15)
    try:
        n = len(o.decompress(c.stream))
    except zlib.error as ex:
        return "bad", None, str(ex).split(": ", 1)[1]
    return ("ok" if o.eof else "cut"), n, None


def test_hand_built_streams(eng, golden):
    g = golden("handmade_inflate.json")["cases"]
    cat = H.catalogue()
    assert sorted(c.name for c in cat) == sorted(g)
    zs = [c.stream for c in cat]
    truth = [_truth_without_dictionary(c) for c in cat]
    rc, failed, recs = F.sizes_call(eng, zs, "raw")
    assert rc == OK
    # the decoder's records for the same items, every range exactly as large as the item decodes to (an item that does not decode: empty)
    caps = [n if kind in ("ok", "trailing") else 0 for kind, n, _ in truth]
    dec = eng.inflate_batch_host(zs, caps, wrap="raw")
    bad = []
    for c, (kind, n, msg), r, d in zip(cat, truth, recs, dec):
        code, m, out_bytes, used = r[:4]
        if kind == "ok" and (code, out_bytes, used) != (OK, n, len(c.stream)):
            bad.append((c.name, "truth", r[:4], n))
        if kind == "trailing" and not (code == OK and out_bytes == n and used < len(c.stream)):
            bad.append((c.name, "truth", r[:4], n))
        if kind == "bad" and (code, m) != (DATA_ERROR, msg if msg is not None else g[c.name]["msg"]):
            bad.append((c.name, "truth", r[:4], msg or g[c.name]["msg"]))
        if kind == "cut" and code != DATA_ERROR:
            bad.append((c.name, "truth", r[:4]))
        if code != OK and (out_bytes, used) != (0, 0):
            bad.append((c.name, "a failed item reports sizes", r[:4]))
        if r[4:] != (1, 0):
            bad.append((c.name, "checks", r[4:]))
        # differential: no case is left out
        if (code, m) != d[:2]:
            bad.append((c.name, "decoder says", d[:2], "sizing says", (code, m)))
        elif code == OK and (out_bytes, used) != (len(d[2]), d[3]):
            bad.append((c.name, "decoder", len(d[2]), d[3], "sizing", out_bytes, used))
    assert not bad, bad[:10]
    assert failed == sum(1 for r in recs if r[0] != OK) == eng.last_failed


def _trailer_items():
    d = cases.make("text", 5000, 21)
    z = zlib.compress(d, 6)
    gz = F.gzip_member(F.deflate(d, 6, "raw"), d)
    flipped = z[:-2] + bytes([z[-2] ^ 0x10]) + z[-1:]
    wrong_isize = gz[:-4] + struct.pack("<I", len(d) + 1)
    return d, z, gz, flipped, wrong_isize


def test_what_sizing_does_not_check(eng):
    d, z, gz, flipped, wrong_isize = _trailer_items()
    zs = [z, flipped, gz, wrong_isize, z]
    rc, failed, recs = F.sizes_call(eng, zs, "auto")
    assert rc == OK and failed == 0
    assert [r[:4] for r in recs] == [(OK, "", len(d), len(s)) for s in zs]


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
    rc, failed, clean = F.sizes_call(eng, good, "auto")
    assert rc == OK and failed == 0
    assert [r[:4] for r in clean] == [(OK, "", n, len(s)) for n, s in zip(sizes, good)]
    # all damaged items among good ones, one call
    mixed = []
    for k, s in enumerate(good):
        mixed += [s, damaged[k][0]]
    rc, failed, recs = F.sizes_call(eng, mixed, "auto")
    assert rc == OK and failed == len(damaged)
    for k in range(len(good)):
        assert recs[2 * k] == clean[k], k
        assert recs[2 * k + 1] == (damaged[k][1], damaged[k][2], 0, 0, 1, 0), (k, recs[2 * k + 1])
    # one item at a time: the neighbours' records do not change
    for k, (s, code, msg) in damaged.items():
        zs = list(good)
        zs[k] = s
        rc, failed, recs = F.sizes_call(eng, zs, "auto")
        assert rc == OK and failed == 1
        assert recs[k][:2] == (code, msg), (k, recs[k])
        assert [r for j, r in enumerate(recs) if j != k] == [r for j, r in enumerate(clean) if j != k], k


def test_more_than_one_launch_round(eng):
    d = cases.make("text", 100, 5)
    e, last = zlib.compress(b""), zlib.compress(d)
    n = 65537
    rc, failed, recs = F.sizes_call(eng, [e] * (n - 1) + [last], "zlib")
    assert rc == OK and failed == 0
    bad = [k for k in range(n - 1) if recs[k] != (OK, "", 0, len(e), 1, 0)]
    assert not bad, bad[:10]
    assert recs[n - 1] == (OK, "", len(d), len(last), 1, 0)


def test_arguments(eng):
    from zlib_amd import gpu
    z = zlib.compress(b"abc")
    blob, offs = F.pack([z, z])
    recs = (gpu.InflateItem * 2)()
    failed = C.c_uint64(0)
    call = eng.L.zgpu_inflate_batch_sizes_host
    assert call(eng.h, None, 0, None, 0, gpu.WRAP_ZLIB, None, None) == OK  # nothing to do
    assert call(eng.h, blob.ctypes.data, int(offs[-1]), offs.ctypes.data, 2, 4, recs, C.byref(failed)) == STREAM_ERROR  # no such wrapper
    assert call(eng.h, blob.ctypes.data, int(offs[-1]), offs.ctypes.data, 2, gpu.WRAP_ZLIB, None, C.byref(failed)) == STREAM_ERROR
    back = np.array([0, len(z) + 1, len(z)], dtype=np.uint64)  # runs backwards
    assert call(eng.h, blob.ctypes.data, int(offs[-1]), back.ctypes.data, 2, gpu.WRAP_ZLIB, recs, C.byref(failed)) == STREAM_ERROR
    out = np.array([0, len(z), 2 * len(z) + 1], dtype=np.uint64)  # leaves the buffer
    assert call(eng.h, blob.ctypes.data, int(offs[-1]), out.ctypes.data, 2, gpu.WRAP_ZLIB, recs, C.byref(failed)) == STREAM_ERROR


def test_device_entry_matches_host(eng):
    import torch
    from zlib_amd import gpu
    good, damaged, _ = _damage_items()
    zs = list(good) + [damaged[0][0], damaged[2][0]] + [z + F.JUNK for _, z in F.streams("zlib")[-2:]]
    rc, failed, host = F.sizes_call(eng, zs, "auto")
    assert rc == OK and failed == 2
    n = len(zs)
    dev = torch.device("cuda", 0)
    blob, offs = F.pack(zs)
    d_in = torch.tensor(blob, device=dev)
    d_io = torch.tensor(offs.view(np.int64), device=dev)
    # the offsets table that runs backwards is refused by the device entry too (the check is made on the device)
    d_bad = torch.tensor(offs[::-1].copy().view(np.int64), device=dev)
    isz = C.sizeof(gpu.InflateItem)
    d_items = torch.zeros(n * isz, dtype=torch.uint8, device=dev)
    assert eng.inflate_batch_sizes_device(d_in.data_ptr(), int(offs[-1]), d_io.data_ptr(), n, d_items.data_ptr(), wrap="auto") == 2
    raw = d_items.cpu().numpy().tobytes()
    assert [F.record(eng, gpu.InflateItem.from_buffer_copy(raw, k * isz)) for k in range(n)] == host
    import zlib_amd
    with pytest.raises(zlib_amd.EngineError) as ex:
        eng.inflate_batch_sizes_device(d_in.data_ptr(), int(offs[-1]), d_bad.data_ptr(), n, d_items.data_ptr(), wrap="auto")
    assert ex.value.code == STREAM_ERROR
