#!/usr/bin/env python3
"""The match-search catalogue's golden file, by the compiled reference:  python oracle/gen_golden_parse.py -> tests/golden/parse_kat.json

Per case of oracle/parsecases.py: the input's length and SHA-256/16 (the inputs are built again from the catalogue, not stored) and, per
configuration the case is meant for, length and SHA-256/16 of the reference's raw stream -- an independent chunk with both endings
([Z_FULL_FLUSH, Z_FINISH]), or, for a case placed on a tile edge, the one continuous stream ("cont": the same for the cases placed on a
block or window edge, which go through both).  Tuned rows go through deflateTune (chunks: in front of the one call; a continuous stream: right
behind deflateInit2), position-0
matchable chunks through a three-byte preset dictionary (refzlib.deflate_chunk_raw)."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import parsecases as P, refzlib as R  # noqa: E402


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


def ref_chunk(data, cfg, last):
    k = P.CONFIGS[cfg]
    L = R.lib()
    L.deflateTune.argtypes = [C.POINTER(R.ZStream), C.c_int, C.c_int, C.c_int, C.c_int]
    s = R.ZStream()
    assert L.deflateInit2_(C.byref(s), k.level, R.Z_DEFLATED, -15, 8, k.strategy, b"1.2.3", C.sizeof(R.ZStream)) == R.Z_OK
    if k.p0:
        assert L.deflateSetDictionary(C.byref(s), b"\x00\x01\x02", 3) == R.Z_OK
    if k.tune:
        assert L.deflateTune(C.byref(s), *k.tune) == R.Z_OK
    cap = len(data) + (len(data) >> 8) + 256
    out = C.create_string_buffer(cap)
    inb = C.create_string_buffer(data, max(len(data), 1))
    s.next_in = C.addressof(inb); s.avail_in = len(data); s.next_out = C.addressof(out); s.avail_out = cap
    rc = L.deflate(C.byref(s), R.Z_FINISH if last else R.Z_FULL_FLUSH)
    assert rc == (R.Z_STREAM_END if last else R.Z_OK) and s.avail_in == 0, rc
    z = out.raw[: s.total_out]
    L.deflateEnd(C.byref(s))
    return z


def rows_of(c):
    out = {}
    for cfg in c.cfgs:
        if c.cont:
            k = P.CONFIGS[cfg]
            assert not k.p0
            z = R.deflate_calls(c.data, k.level, (), wbits=-15, strategy=k.strategy, tune=k.tune)
            out[cfg] = [len(z), h16(z)]
        else:
            out[cfg] = [[len(z), h16(z)] for z in (ref_chunk(c.data, cfg, 0), ref_chunk(c.data, cfg, 1))]
    row = {"data": [len(c.data), h16(c.data)], "out": out}
    if c.family == "placed" and not c.cont:  # the cases on a block or window edge as ONE continuous stream as well (a level's own row, or a tuned row of CONT_EDGE)
        cont = {}
        for cfg in c.cfgs:
            k = P.CONFIGS[cfg]
            if not (k.tune or k.p0) or cfg in P.CONT_EDGE:
                z = R.deflate_calls(c.data, k.level, (), wbits=-15, strategy=k.strategy, tune=k.tune)
                cont[cfg] = [len(z), h16(z)]
        if cont:
            row["cont"] = cont
    return row


if __name__ == "__main__":
    rows = {c.name: rows_of(c) for c in P.catalogue()}
    with open(os.path.join(ROOT, "tests", "golden", "parse_kat.json"), "w") as f:
        json.dump({"reference": R.version(), "cases": rows}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote parse_kat.json:", len(rows), "cases")
