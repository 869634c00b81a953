"""What tests/test_gpu_batch_sizes.py and tests/test_gpu_batch_packed.py share: the items (the contents tests/test_gpu_batch.py builds its ITEMS
from), their streams by Python's zlib, and ctypes access to the records.  Built once per session."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np

from oracle import cases

OK, NEED_DICT, STREAM_ERROR, DATA_ERROR, BUF_ERROR = 0, 2, -2, -3, -5
SIZES = [0, 1, 2, 3, 100, 4096, 65535, 65536]
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
JUNK = b"\x07junk!\xff"  # 7 bytes that are no part of any stream
TRUNCATED = "segment ends inside a block"


@functools.lru_cache(maxsize=None)
def items():
    out = [cases.make("mix", n, 3) for n in SIZES]
    out += [cases.make(k, 5000 + 977 * i, 11 + i) for i, k in enumerate(cases.KINDS)]
    return tuple(out)


def deflate(data, level, wrap):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[wrap])
    return c.compress(data) + c.flush()


@functools.lru_cache(maxsize=None)
def streams(wrap):
    """(data, stream) for every item at levels 1, 6 and 9 (wrap "auto": zlib and gzip in turn), then 8 MiB of zeros and 3 MiB of mix at level 6"""
    pairs = []
    datas = [d for _ in (1, 6, 9) for d in items()] + [bytes(8 << 20), cases.make("mix", 3 << 20, 77)]
    levels = [lv for lv in (1, 6, 9) for _ in items()] + [6, 6]
    for k, (d, lv) in enumerate(zip(datas, levels)):
        w = wrap if wrap != "auto" else ("zlib", "gzip")[k & 1]
        pairs.append((d, deflate(d, lv, w)))
    return tuple(pairs)


def gzip_member(body_raw, data, name=None, extra=None, comment=None, hcrc=False):
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


def pack(zs):
    """blob (one spare byte behind it), offsets"""
    offs = np.zeros(len(zs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(z) for z in zs])
    return np.frombuffer(b"".join(zs) + b"\0", dtype=np.uint8), offs


def sizes_call(eng, zs, wrap):
    """zgpu_inflate_batch_sizes_host through ctypes: (rc, nfailed, [(code, message, out_bytes, in_used, adler32, crc32)])"""
    from zlib_amd import gpu
    n = len(zs)
    blob, offs = pack(zs)
    recs = (gpu.InflateItem * max(n, 1))()
    failed = C.c_uint64(99)
    rc = eng.L.zgpu_inflate_batch_sizes_host(eng.h, blob.ctypes.data, int(offs[-1]), offs.ctypes.data, n, gpu._WRAPS[wrap], recs, C.byref(failed))
    return rc, failed.value, [record(eng, recs[k]) for k in range(n)]


def packed_call(eng, zs, wrap, checks=0, align=1, cap=None, fill=0xA5):
    """zgpu_inflate_batch_packed_host through ctypes into a buffer of `cap` bytes (default 64 MiB, more than any test here decodes) filled with
    `fill`: (rc, total, nfailed, offsets, records, buffer)"""
    from zlib_amd import gpu
    n = len(zs)
    blob, offs = pack(zs)
    cap = (64 << 20) if cap is None else cap
    out = np.full(cap + 1, fill, dtype=np.uint8)
    ooffs = np.full(n + 1, 0xDEAD, dtype=np.uint64)
    recs = (gpu.InflateItem * max(n, 1))()
    failed, total = C.c_uint64(99), C.c_uint64(99)
    rc = eng.L.zgpu_inflate_batch_packed_host(eng.h, blob.ctypes.data, int(offs[-1]), offs.ctypes.data, n, gpu._WRAPS[wrap], checks, align, out.ctypes.data, cap,
                                              ooffs.ctypes.data, recs, C.byref(total), C.byref(failed))
    return rc, total.value, failed.value, [int(o) for o in ooffs], [record(eng, recs[k]) for k in range(n)], out


def record(eng, it):
    return (it.code, eng.L.zgpu_inflate_message(it.msg).decode(), it.out_bytes, it.in_used, it.adler32, it.crc32)
