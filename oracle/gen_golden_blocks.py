#!/usr/bin/env python3
"""The block-layer catalogue's golden file, by the compiled reference:
python oracle/gen_golden_blocks.py -> tests/golden/block_kat.json

Per row of oracle/blockcases.py: the input's length and SHA-256/16 (the inputs are built again from the catalogue, not stored) and the length and
SHA-256/16 of the stream the reference writes for the row's calls.  Before a row is written down its claims are checked on that stream (blockwalk),
and the stream is inflated back by the reference itself."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import blockcases as BC, blockwalk as BW, refzlib as R  # noqa: E402


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


def row_of(c):
    z = R.deflate_calls(c.data, c.level, list(c.calls), wbits=c.wbits, strategy=c.strategy)
    rc, back = R.inflate_wbits(z, c.wbits, len(c.data) + 8)[:2]
    assert rc == R.Z_STREAM_END and back == c.data, c.name
    bad = BC.check(c, BW.walk(BC.raw_of(c, z))[0])
    assert not bad, bad
    return {"family": c.family, "data": [len(c.data), h16(c.data)], "len": len(z), "sha": h16(z)}


if __name__ == "__main__":
    rows = {c.name: row_of(c) for c in BC.catalogue()}
    with open(os.path.join(ROOT, "tests", "golden", "block_kat.json"), "w") as f:
        json.dump({"reference": R.version(), "cases": rows}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote block_kat.json:", len(rows), "cases")
