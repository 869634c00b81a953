"""Blocking batch integrity test with long items: zgpu_inflate_batch_verify_device, device-resident, zlib items of the synthetic Silesia-mix at level 6
(compressed by zgpu_deflate_streams_host) -- the rows, the corpus and the clock of scripts/batch_long_rate.py.  Rows: 256 x 1 MiB and 16 x 64 MiB (every item
long: verified in pieces), 4,096 x 96 KiB (items that are below the threshold of 128 KiB once compressed) and 16,384 x 4 KiB (the call's whole input may hold
long items, none is): the last two must not move.
Every row is timed three ways -- the feature on with its threshold at the shared 128 KiB (ZGPU_BATCH_PIECES_VERIFY_MIN_BYTES=131072: the table this script
wrote moved the default of that knob up to 20,000,000, and the rows stay the ones that decided it), ZGPU_BATCH_PIECES_VERIFY_MIN_BYTES=0, and (--parent-lib PATH) another build of the engine, the parent
commit's -- and, the feature on, under the round-slot caps 512 and 2048 beside the default 1024; each variant in a fresh child process, the variants
alternating over `--passes` passes in this one run.  A figure is the median (min .. max) of `reps` timed windows of at least 0.5 s behind a warm-up call, a host
clock around calls that end in a device synchronise; the spread of a variant is min .. max over all its windows of all passes.  Every child compares the
records with the truth: every item good, its size the corpus item's, its Adler-32 Python zlib's of the corpus bytes.
Peak device memory beside the input (the method of scripts/batch_verify_rate.py): what a fresh engine allocates to serve the call once -- free device memory
before the engine was made minus free device memory after the call -- plus the records the caller brings.
Usage: python scripts/batch_verify_long_rate.py [--parent-lib PATH] [--passes N] [--out PATH]   (default: profiles/r14_batch_verify_long_table.txt)"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from batch_long_rate import ROWS, corpus, prepare, timed  # noqa: E402  (the same rows, corpus and clock)

VK, SLOTK = "ZGPU_BATCH_PIECES_VERIFY_MIN_BYTES", "ZGPU_BATCH_PIECES_VERIFY_ROUND_SLOTS"


def child(tmp):
    """times every row with the library and the environment it was started with; one JSON line"""
    import torch
    import zlib_amd
    from zlib_amd import gpu
    eng = zlib_amd.Engine(0)
    dev = torch.device("cuda", 0)
    d_corpus = corpus(eng, dev)
    host = d_corpus.cpu().numpy()
    del d_corpus
    isz = C.sizeof(gpu.InflateItem)
    out = {}
    # (the two rows without long items are timed first, as profiles/r13_batch_sizes_long_table.txt found it matters: behind 16 x 64 MiB the chip has just run
    # calls of very different lengths in the different variants)
    for r, (name, n, s) in sorted(enumerate(ROWS), key=lambda t: t[0] < 2):
        z, offs = np.load(os.path.join(tmp, "z%d.npy" % r)), np.load(os.path.join(tmp, "o%d.npy" % r))
        d_z, d_zoff = torch.tensor(z, device=dev), torch.tensor(offs.view(np.int64), device=dev)
        d_items = torch.empty(n * isz, dtype=torch.uint8, device=dev)
        zbytes = int(offs[-1])

        def call(e=eng):
            assert e.inflate_batch_verify_device(d_z.data_ptr(), zbytes, d_zoff.data_ptr(), n, d_items.data_ptr(), wrap="zlib", checks=0) == 0
        # what a fresh engine allocates for the call
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        fresh = zlib_amd.Engine(0)
        call(fresh)
        torch.cuda.synchronize()
        mem = max(free0 - torch.cuda.mem_get_info(0)[0], 0) + n * isz
        fresh.close()
        counts = getattr(eng, "batch_verify_piece_counts", lambda: (0, 0))
        before = counts()
        call()
        after = counts()
        raw = d_items.cpu().numpy().tobytes()
        step = max(1, n // 64)  # (Python's Adler-32 of 1 GiB is a second: every item's size and verdict, every 64th or so item's check value)
        for k in range(n):
            it = gpu.InflateItem.from_buffer_copy(raw, k * isz)
            assert (it.code, it.out_bytes, it.in_used) == (0, s, int(offs[k + 1] - offs[k])), "%s: item %d" % (name, k)
            if k % step == 0:
                assert it.adler32 == zlib.adler32(host[k * s: (k + 1) * s]), "%s: the Adler-32 of item %d" % (name, k)
        out[name] = {"ts": timed(call), "zbytes": zbytes, "in_pieces": after[0] - before[0], "fell_back": after[1] - before[1], "mem": mem}
        del d_z, d_zoff, d_items
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1])
    out_path, parent_lib, passes = os.path.join(ROOT, "profiles", "r14_batch_verify_long_table.txt"), None, 2
    while args:
        a = args.pop(0)
        if a == "--out":
            out_path = args.pop(0)
        elif a == "--parent-lib":
            parent_lib = os.path.abspath(args.pop(0))
        elif a == "--passes":
            passes = int(args.pop(0))
    variants = [("feature on", {VK: "131072"}), (VK + "=0", {VK: "0"})]
    if parent_lib:
        variants.append(("parent commit", {"ZAMD_GPU_LIB": parent_lib}))
    variants += [("round slots 512", {VK: "131072", SLOTK: "512"}), ("round slots 2048", {VK: "131072", SLOTK: "2048"})]
    got = {v[0]: {} for v in variants}
    with tempfile.TemporaryDirectory() as tmp:
        prepare(tmp)
        for _ in range(passes):
            for vname, env in variants:
                e = dict(os.environ)
                for k in ("ZGPU_BATCH_PIECES_MIN_BYTES", VK, SLOTK, "ZGPU_BATCH_PIECES_NO_SCRATCH", "ZAMD_GPU_LIB"):
                    e.pop(k, None)
                e.update(env)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], env=e, capture_output=True, text=True, timeout=900)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.exit("%s failed:\n%s" % (vname, p.stderr[-3000:]))
                print("timed:", vname, file=sys.stderr, flush=True)
                for row, rec in json.loads(line[0][7:]).items():
                    acc = got[vname].setdefault(row, {"ts": [], "zbytes": rec["zbytes"], "in_pieces": rec["in_pieces"], "fell_back": rec["fell_back"], "mem": rec["mem"]})
                    acc["ts"] += rec["ts"]
                    acc["mem"] = max(acc["mem"], rec["mem"])
    lines = ["# blocking batch integrity test (zgpu_inflate_batch_verify_device), zlib items of the Silesia-mix at level 6, device-resident, checks = what the wrapper needs (Adler-32)",
             "# median (min .. max) per call over %d passes x 5 timed windows of at least 0.5 s behind a warm-up call, the variants alternating in fresh processes;" % passes,
             "# GiB/s of decoded bytes; min .. max is the run-to-run spread of the variant's own timing; mem: peak device memory beside the input, what a fresh engine",
             "# allocates to serve the call once plus the caller's records"]
    if not parent_lib:
        lines.append("# parent commit: not measured (no --parent-lib)")
    for name, n, s in ROWS:
        any_rec = got[variants[0][0]][name]
        lines.append("# %s: %d items, %d bytes compressed, %d decoded" % (name, n, any_rec["zbytes"], n * s))
        for vname, _ in variants:
            rec = got[vname][name]
            med = statistics.median(rec["ts"])
            lines.append("%-36s %10.3f ms (%10.3f .. %10.3f) %8.2f GiB/s   in pieces %d, fell back %d   mem %d bytes (%.3f x input)" % (
                vname, med * 1e3, min(rec["ts"]) * 1e3, max(rec["ts"]) * 1e3, n * s / med / 2 ** 30, rec["in_pieces"], rec["fell_back"], rec["mem"], rec["mem"] / rec["zbytes"]))
        if parent_lib:
            on, par = got["feature on"][name]["ts"], got["parent commit"][name]["ts"]
            inside = min(par) <= statistics.median(on) <= max(par)
            lines.append("parent / feature on = %.2f   (parent's spread: %.1f %% of its median; the feature's median lies %s the parent's min .. max)" % (
                statistics.median(par) / statistics.median(on), (max(par) - min(par)) / statistics.median(par) * 100, "inside" if inside else "OUTSIDE"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
