"""Sizing pass and packed decode with long items: zgpu_inflate_batch_sizes_device and zgpu_inflate_batch_packed_device, device-resident, zlib items of the
synthetic Silesia-mix at level 6 (compressed by zgpu_deflate_streams_host).  Rows: 256 x 1 MiB and 16 x 64 MiB (every item long: sized in pieces),
4,096 x 96 KiB (items below the threshold of 128 KiB once compressed) and 16,384 x 4 KiB (the call's whole input may hold long items, none is): the last
two must not move.  Every row is timed three ways -- the feature on, ZGPU_BATCH_PIECES_SIZES_MIN_BYTES=0 (the sizing pass's pieces off, the decode half of
the packed call as it is), and (--parent-lib PATH) another build of the engine, the parent commit's, whose sizing pass gives every item to one wave and
whose decode half has its pieces -- each in a fresh child process, the three alternating over `--passes` passes in this one run; within a process the two
rows without long items come first (ORDER).  A figure is the median (min .. max) of `reps` timed windows of at least 0.5 s behind a warm-up
call, a host clock around calls that end in a device synchronise; the spread of a variant is min .. max over all its windows of all passes.  The sizes
are compared with the corpus's and the packed call's bytes with the corpus in every child.
Usage: python scripts/batch_sizes_long_rate.py [--parent-lib PATH] [--passes N] [--out PATH]   (default: profiles/r13_batch_sizes_long_table.txt)"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.batch_long_rate import ROWS, corpus, prepare, timed  # noqa: E402  (the same rows, corpus and clock as the decode's table)

CALLS = ("sizes", "packed")
ORDER = (3, 2, 0, 1)  # the rows without long items are timed first: behind the long rows, whose length differs twentyfold between the variants, the chip is in another state
KNOBS = ("ZGPU_BATCH_PIECES_MIN_BYTES", "ZGPU_BATCH_PIECES_SIZES_MIN_BYTES", "ZGPU_BATCH_PIECES_SIZES_ROUND_SLOTS", "ZGPU_BATCH_PIECES_ROUND_BYTES", "ZAMD_GPU_LIB")


def child(tmp):
    """times every row and both calls with the library and the environment it was started with; one JSON line"""
    import torch
    import zlib_amd
    from zlib_amd import gpu
    eng = zlib_amd.Engine(0)
    dev = torch.device("cuda", 0)
    d_corpus = corpus(eng, dev)
    out = {}
    for r in ORDER:
        name, n, s = ROWS[r]
        z, offs = np.load(os.path.join(tmp, "z%d.npy" % r)), np.load(os.path.join(tmp, "o%d.npy" % r))
        d_z, d_zoff = torch.tensor(z, device=dev), torch.tensor(offs.view(np.int64), device=dev)
        d_ooff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_out = torch.zeros(n * s, dtype=torch.uint8, device=dev)
        d_items = torch.zeros(n * C.sizeof(gpu.InflateItem), dtype=torch.uint8, device=dev)

        def sizes():
            assert eng.inflate_batch_sizes_device(d_z.data_ptr(), int(offs[-1]), d_zoff.data_ptr(), n, d_items.data_ptr(), wrap="zlib") == 0

        def packed():
            rc, total, failed = eng.inflate_batch_packed_device(d_z.data_ptr(), int(offs[-1]), d_zoff.data_ptr(), n, d_out.data_ptr(), n * s, d_ooff.data_ptr(), d_items.data_ptr(), wrap="zlib")
            assert (rc, total, failed) == (0, n * s, 0)
        for cname, call in zip(CALLS, (sizes, packed)):
            before_s, before_d = eng.batch_size_piece_counts(), eng.batch_piece_counts()
            d_items.zero_()
            call()
            after_s, after_d = eng.batch_size_piece_counts(), eng.batch_piece_counts()
            raw = d_items.cpu().numpy().tobytes()
            for k in (0, n // 2, n - 1):
                it = gpu.InflateItem.from_buffer_copy(raw, k * C.sizeof(gpu.InflateItem))
                assert (it.code, it.out_bytes, it.in_used) == (0, s, int(offs[k + 1] - offs[k])), (name, cname, k, it.code, it.out_bytes, it.in_used)
            if cname == "packed":
                assert torch.equal(d_out, d_corpus[: n * s]), "%s: the packed decode differs from the corpus" % name
            out["%s / %s" % (name, cname)] = {"ts": timed(call), "zbytes": int(offs[-1]), "sized": [after_s[0] - before_s[0], after_s[1] - before_s[1]],
                                             "decoded": [after_d[0] - before_d[0], after_d[1] - before_d[1]]}
        del d_z, d_zoff, d_ooff, d_out, d_items
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1])
    out_path, parent_lib, passes = os.path.join(ROOT, "profiles", "r13_batch_sizes_long_table.txt"), None, 2
    while args:
        a = args.pop(0)
        if a == "--out":
            out_path = args.pop(0)
        elif a == "--parent-lib":
            parent_lib = os.path.abspath(args.pop(0))
        elif a == "--passes":
            passes = int(args.pop(0))
    variants = [("feature on", {}), ("ZGPU_BATCH_PIECES_SIZES_MIN_BYTES=0", {"ZGPU_BATCH_PIECES_SIZES_MIN_BYTES": "0"})]
    if parent_lib:
        variants.append(("parent commit", {"ZAMD_GPU_LIB": parent_lib}))
    got = {v[0]: {} for v in variants}
    with tempfile.TemporaryDirectory() as tmp:
        prepare(tmp)
        print("prepared", file=sys.stderr, flush=True)
        for _ in range(passes):
            for vname, env in variants:
                e = dict(os.environ)
                for k in KNOBS:
                    e.pop(k, None)
                e.update(env)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], env=e, capture_output=True, text=True, timeout=900)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.exit("%s failed:\n%s" % (vname, p.stderr[-3000:]))
                print("timed:", vname, file=sys.stderr, flush=True)
                for row, rec in json.loads(line[0][7:]).items():
                    acc = got[vname].setdefault(row, {"ts": [], "zbytes": rec["zbytes"], "sized": rec["sized"], "decoded": rec["decoded"]})
                    acc["ts"] += rec["ts"]
    lines = ["# sizing pass (zgpu_inflate_batch_sizes_device) and packed decode (zgpu_inflate_batch_packed_device), zlib items of the Silesia-mix at level 6, device-resident",
             "# median (min .. max) per call over %d passes x 5 timed windows of at least 0.5 s behind a warm-up call, the variants alternating in fresh processes;" % passes,
             "# GiB/s of decoded bytes; min .. max is the run-to-run spread of the variant's own timing; sized / decoded: long items (in pieces, fell back) of the",
             "# sizing pass and of the decode half; `inside`: the variant's median lies inside the parent's min .. max"]
    if not parent_lib:
        lines.append("# parent commit: not measured (no --parent-lib)")
    for name, n, s in ROWS:
        for cname in CALLS:
            key = "%s / %s" % (name, cname)
            lines.append("# %s: %d items, %d bytes compressed, %d decoded" % (key, n, got[variants[0][0]][key]["zbytes"], n * s))
            par = got["parent commit"][key]["ts"] if parent_lib else None
            for vname, _ in variants:
                rec = got[vname][key]
                med = statistics.median(rec["ts"])
                note = ""
                if par and vname != "parent commit":
                    note = "   inside" if min(par) <= med <= max(par) else "   %+.1f %% of the parent's median" % ((med / statistics.median(par) - 1) * 100)
                lines.append("%-36s %10.3f ms (%10.3f .. %10.3f) %8.2f GiB/s   sized %d, %d  decoded %d, %d%s" % (vname, med * 1e3, min(rec["ts"]) * 1e3, max(rec["ts"]) * 1e3,
                                                                                                                n * s / med / 2 ** 30, rec["sized"][0], rec["sized"][1], rec["decoded"][0],
                                                                                                                rec["decoded"][1], note))
            if par:
                on = got["feature on"][key]["ts"]
                lines.append("parent / feature on = %.2f   (parent's spread: %.1f %% of its median)" % (statistics.median(par) / statistics.median(on),
                                                                                                       (max(par) - min(par)) / statistics.median(par) * 100))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
