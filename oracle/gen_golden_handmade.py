#!/usr/bin/env python3
"""The hand-built streams' golden file, by the compiled reference:  python oracle/gen_golden_handmade.py -> tests/golden/handmade_inflate.json

Per case of oracle/handmade.py: the stream's length and SHA-256/16 (the streams are built again from the catalogue, not stored), and the
verdict of the reference's raw inflate() (behind the case's preset dictionary): rc, msg, bytes out, their SHA-256/16, bytes consumed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import handmade as H, refzlib as R  # noqa: E402

rows = {}
for c in H.catalogue():
    cap = len(c.expect) if c.expect is not None else 1 << 20
    rc, out, used, msg = R.inflate_raw_dict(c.stream, cap + 64, c.dictionary)
    rows[c.name] = {"stream": [len(c.stream), H.sha16(c.stream)], "rc": rc, "msg": msg, "out": [len(out), H.sha16(out)], "used": used}
with open(os.path.join(ROOT, "tests", "golden", "handmade_inflate.json"), "w") as f:
    json.dump({"reference": R.version(), "cases": rows}, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote handmade_inflate.json:", len(rows), "cases")
