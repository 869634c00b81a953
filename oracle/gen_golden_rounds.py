#!/usr/bin/env python3
"""The round catalogue's golden file, by the compiled reference:  python oracle/gen_golden_rounds.py -> tests/golden/round_kat.json

Per case of oracle/roundcases.py: the input's length and SHA-256/16 (the inputs are built again from the catalogue, not stored) and, per level the
case is for, length and SHA-256/16 of the reference's ONE continuous raw stream ("out") and the tokens the case claims ("claims": [position, dist, len],
dist 0 = a literal).  For the cases of roundcases.feed_cases(), "feed": the same per row of feed_rows() -- the calls with Z_NO_FLUSH give the stream of
"out" (checked here), the sync-flush and the full-flush rows streams of their own."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refzlib as R, roundcases as RC  # noqa: E402


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


def rows_of(c, feeds):
    row = {"data": [len(c.data), h16(c.data)], "out": {}, "claims": {}}
    for cfg in c.cfgs:
        z = R.deflate_calls(c.data, RC.level_of(cfg), (), wbits=-15)
        row["out"][cfg] = [len(z), h16(z)]
        row["claims"][cfg] = [[p, 0, 1] if t == RC.LIT else [p, t[0], t[1]] for p, t in c.claims[cfg]]
    if c.name in feeds:
        row["feed"] = {}
        for tag, calls, _ in RC.feed_rows(c):
            row["feed"][tag] = {}
            for cfg in c.cfgs:
                z = R.deflate_calls(c.data, RC.level_of(cfg), calls, wbits=-15)
                assert calls[0][1] != RC.Z_NO_FLUSH or [len(z), h16(z)] == row["out"][cfg], (c.name, tag, cfg)
                row["feed"][tag][cfg] = [len(z), h16(z)]
    return row


if __name__ == "__main__":
    feeds = {c.name for c in RC.feed_cases()}
    rows = {c.name: rows_of(c, feeds) for c in RC.catalogue()}
    with open(os.path.join(ROOT, "tests", "golden", "round_kat.json"), "w") as f:
        json.dump({"reference": R.version(), "cases": rows}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote round_kat.json:", len(rows), "cases")
