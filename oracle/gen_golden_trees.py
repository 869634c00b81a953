#!/usr/bin/env python3
"""Golden vectors for Huffman tree construction off the beaten path, produced by the compiled reference:  python oracle/gen_golden_trees.py
->  tests/golden/tree_kat.json

The inputs are oracle/treecases.py (regenerated, not stored: a row pins its input by length and sha256).  One row per case and level:

  chunk_len / chunk_sha   the reference's chunk function (refzlib.deflate_chunk_raw: a fresh raw stream per 65536 bytes, Z_FULL_FLUSH behind every chunk
                          but the last, Z_FINISH on the last) -- what the engine's chunk mode writes
  cont_len / cont_sha     ONE raw stream of the reference over the whole input (refzlib.deflate_calls, what compress2() does)
  primes                  overflow rows only: the one raw stream behind deflatePrime(bits, value), bits 0..7: the repaired block at every bit phase
  hex                     the whole continuous stream, for the twelve smallest overflow rows (to diff a failure by hand)
  btypes, counters        from the CPU restatement (oracle_py.tree_counters), whose bytes are checked against the reference's right here: the block types
                          and how often each tree kind (literal, distance, bit-length) went through gen_bitlen's repair (trees.c:525-566)

"summary" counts, over the btype family, the blocks of each type and the blocks that sat on static_lenb == opt_lenb / stored_len + 4 == opt_lenb.
The generator refuses to write a fixture in which an overflow row is not repaired, a control row is, or one of the summary counts is zero.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle_py as O, refzlib as R, treecases as T  # noqa: E402

PRIME_VALUES = [0, 1, 2, 5, 9, 0x15, 0x2A, 0x55]  # deflatePrime(bits, PRIME_VALUES[bits])
OUT = os.path.join(ROOT, "tests", "golden", "tree_kat.json")


def sha(b):
    return hashlib.sha256(b).hexdigest()[:24]


def ref_chunks(data, level, strategy):
    n = max(1, (len(data) + R.CHUNK - 1) // R.CHUNK)
    return b"".join(R.deflate_chunk_raw(data[k * R.CHUNK:(k + 1) * R.CHUNK], level, k + 1 == n, strategy=strategy) for k in range(n))


def ref_primed(data, level, strategy, bits, value):
    L = R.lib()
    L.deflatePrime.argtypes = [C.POINTER(R.ZStream), C.c_int, C.c_int]
    s = R.ZStream()
    assert L.deflateInit2_(C.byref(s), level, 8, -15, 8, strategy, b"1.2.3", C.sizeof(R.ZStream)) == 0
    assert L.deflatePrime(C.byref(s), bits, value) == 0
    cap = len(data) + (len(data) >> 3) + 1024
    out = C.create_string_buffer(cap)
    inb = C.create_string_buffer(data, max(len(data), 1))
    s.next_in = C.addressof(inb); s.avail_in = len(data); s.next_out = C.addressof(out); s.avail_out = cap
    assert L.deflate(C.byref(s), R.Z_FINISH) == 1 and s.avail_in == 0
    z = out.raw[: s.total_out]
    L.deflateEnd(C.byref(s))
    return z


def oracle_chunks(data, level, strategy):
    """The restatement's chunk-mode bytes and the block types of every chunk."""
    n = max(1, (len(data) + R.CHUNK - 1) // R.CHUNK)
    parts, btypes = [], []
    for k in range(n):
        z, info, _ = O.deflate_chunk(data[k * R.CHUNK:(k + 1) * R.CHUNK], level, k + 1 == n, want_tokens=True, strategy=strategy)
        parts.append(z)
        btypes += [info.btype[i] for i in range(min(info.nblocks, 8))]
    return b"".join(parts), btypes


def row_of(c, level, reference=True):
    """The fixture row of one case and level; reference=False: from the restatement alone (tests/test_trees_cpu.py compares the two)."""
    O.tree_counters_reset()
    cont = O.deflate_cont(c.data, level, (), c.strategy)
    k = O.tree_counters()
    chunk, btypes = oracle_chunks(c.data, level, c.strategy)
    if reference:
        rc, rk = R.deflate_calls(c.data, level, (), -15, c.strategy), ref_chunks(c.data, level, c.strategy)
        if rc != cont or rk != chunk:
            raise SystemExit("%s level %d: the restatement differs from the reference" % (c.name, level))
    row = dict(name=c.name, family=c.family, strategy=c.strategy, level=level, n=len(c.data), input_sha=sha(c.data), chunk_len=len(chunk), chunk_sha=sha(chunk),
               cont_len=len(cont), cont_sha=sha(cont), btypes=btypes, repairs=k["repairs"], overflow=k["overflow"], longest=k["longest"], blocks=k["blocks"],
               tie_static=k["tie_static"], tie_stored=k["tie_stored"])
    if c.family in ("lit", "dist", "both", "control") and reference:
        row["primes"] = []
        for bits in range(8):
            z = ref_primed(c.data, level, c.strategy, bits, PRIME_VALUES[bits])
            row["primes"].append(dict(bits=bits, value=PRIME_VALUES[bits], len=len(z), sha=sha(z)))
    return row


def check_rows(rows):
    """The condition the fixture stands on; returns the summary of the btype family."""
    want = {"lit": (1, 0), "dist": (0, 1), "both": (1, 1)}
    for r in rows:
        if r["family"] in want:
            for kind in (0, 1):
                assert r["repairs"][kind] >= want[r["family"]][kind], "%s level %d: tree kind %d is not repaired" % (r["name"], r["level"], kind)
        if r["family"] == "control":
            assert r["repairs"][:2] == [0, 0] and r["longest"][0] == 15, "%s level %d: the control must reach 15 bits unrepaired" % (r["name"], r["level"])
    bt = [r for r in rows if r["family"] == "btype"]
    summary = dict(stored=sum(r["blocks"][0] for r in bt), static=sum(r["blocks"][1] for r in bt), dynamic=sum(r["blocks"][2] for r in bt),
                   tie_static=sum(r["tie_static"] for r in bt), tie_stored=sum(r["tie_stored"] for r in bt))
    assert all(v > 0 for v in summary.values()), summary
    return summary


def main():
    rows, data = [], {}
    for c in T.all_cases():
        data[c.name] = c
        for level in c.levels:
            rows.append(row_of(c, level))
    summary = check_rows(rows)
    small = sorted((r for r in rows if r["family"] in ("lit", "dist", "both", "control")), key=lambda r: (r["cont_len"], r["name"], r["level"]))[:12]
    for r in small:
        r["hex"] = O.deflate_cont(data[r["name"]].data, r["level"], (), r["strategy"]).hex()
    with open(OUT, "w") as f:
        f.write('{"summary": %s,\n"rows": [\n' % json.dumps(summary, sort_keys=True))
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in rows))
        f.write("\n]}\n")
    print("wrote tree_kat.json: %d rows, %d bytes, btype family %r" % (len(rows), os.path.getsize(OUT), summary))


if __name__ == "__main__":
    main()
