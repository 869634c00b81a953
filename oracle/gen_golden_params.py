#!/usr/bin/env python3
"""The deflateParams / deflateTune / deflateReset catalogue's golden file, by the compiled reference:
python oracle/gen_golden_params.py -> tests/golden/params_kat.json

Per row of oracle/paramcases.py: the input's length and SHA-256/16 (the inputs are built again from the catalogue, not stored), every call's return
code, per stream its length, SHA-256/16, total_in, total_out, strm->adler and whether the reference's own inflate gives the input back from it
(ref_valid), and what deflateBound answered where the row asks."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import paramcases as PC, refzlib as R  # noqa: E402


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


def row_of(c):
    codes, streams, bound = R.play_steps(c)
    row = {"family": c.family, "data": [len(c.data), h16(c.data)], "codes": codes,
           "streams": [{"len": len(s["z"]), "sha": h16(s["z"]), "total_in": s["total_in"], "total_out": s["total_out"], "adler": s["adler"], "ref_valid": s["valid"]} for s in streams]}
    if bound is not None:
        row["bound"] = bound
    return row


if __name__ == "__main__":
    rows = {c.name: row_of(c) for c in PC.catalogue()}
    with open(os.path.join(ROOT, "tests", "golden", "params_kat.json"), "w") as f:
        json.dump({"reference": R.version(), "cases": rows}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote params_kat.json:", len(rows), "cases;", sum(1 for r in rows.values() if not all(s["ref_valid"] for s in r["streams"])), "with a stream the reference itself cannot read back")
