"""Blocking batch inflate with long items: zgpu_inflate_batch_device into given offsets, device-resident, zlib items of the synthetic Silesia-mix at level 6
(compressed by zgpu_deflate_streams_host).  Rows: 256 x 1 MiB and 16 x 64 MiB (every item long: decoded in pieces), 4,096 x 96 KiB (items that are below
the threshold of 128 KiB once compressed) and 16,384 x 4 KiB (the call's whole input may hold long items, none is): the last two must not move.
Every row is timed three ways -- the feature on, ZGPU_BATCH_PIECES_MIN_BYTES=0, and (--parent-lib PATH) another build of the engine, the parent commit's --
each in a fresh child process, the three alternating over `--passes` passes in this one run.  A figure is the median (min .. max) of `reps` timed windows of
at least 0.5 s behind a warm-up call, a host clock around calls that end in a device synchronise; the spread of a variant is min .. max over all its windows
of all passes.  Decoded bytes are compared with the corpus in every child.
Usage: python scripts/batch_long_rate.py [--parent-lib PATH] [--passes N] [--out PATH]   (default: profiles/r12_batch_long_table.txt)"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = (("256 x 1 MiB", 256, 1 << 20), ("16 x 64 MiB", 16, 64 << 20), ("4096 x 96 KiB", 4096, 96 << 10), ("16384 x 4 KiB", 16384, 4096))
TOTAL = 1 << 30


def timed(fn, reps=5, window=0.5):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    inner = max(1, min(500, int(window / max(time.perf_counter() - t0, 1e-6)) + 1))
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    return ts


def corpus(eng, dev):
    import torch
    d = torch.empty(TOTAL, dtype=torch.uint8, device=dev)
    eng.corpus_fill_device(0, 1, 0, TOTAL >> 16, d.data_ptr())
    torch.cuda.synchronize()
    return d


def prepare(tmp):
    """the compressed batches, made once: row r -> tmp/z{r}.npy (the streams back to back) and tmp/o{r}.npy (n + 1 offsets)"""
    import torch
    import zlib_amd
    eng = zlib_amd.Engine(0)
    host = corpus(eng, torch.device("cuda", 0)).cpu().numpy()
    for r, (_, n, s) in enumerate(ROWS):
        streams = eng.deflate_streams_host([host[k * s: (k + 1) * s] for k in range(n)], 6, wrap="zlib")
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(z) for z in streams])
        np.save(os.path.join(tmp, "z%d.npy" % r), np.frombuffer(b"".join(streams), dtype=np.uint8))
        np.save(os.path.join(tmp, "o%d.npy" % r), offs)
    eng.close()


def child(tmp):
    """times every row with the library and the environment it was started with; one JSON line"""
    import torch
    import zlib_amd
    from zlib_amd import gpu
    eng = zlib_amd.Engine(0)
    dev = torch.device("cuda", 0)
    d_corpus = corpus(eng, dev)
    out = {}
    for r, (name, n, s) in enumerate(ROWS):
        z, offs = np.load(os.path.join(tmp, "z%d.npy" % r)), np.load(os.path.join(tmp, "o%d.npy" % r))
        d_z, d_zoff = torch.tensor(z, device=dev), torch.tensor(offs.view(np.int64), device=dev)
        d_true = torch.tensor(np.arange(n + 1, dtype=np.int64) * s, device=dev)
        d_out = torch.zeros(n * s, dtype=torch.uint8, device=dev)
        d_items = torch.empty(n * C.sizeof(gpu.InflateItem), dtype=torch.uint8, device=dev)
        counts = getattr(eng, "batch_piece_counts", lambda: (0, 0))
        before = counts()

        def call():
            assert eng.inflate_batch_device(d_z.data_ptr(), int(offs[-1]), d_zoff.data_ptr(), n, d_out.data_ptr(), n * s, d_true.data_ptr(), d_items.data_ptr(), wrap="zlib") == 0
        call()
        after = counts()
        assert torch.equal(d_out, d_corpus[: n * s]), "%s: the batch decode differs from the corpus" % name
        out[name] = {"ts": timed(call), "zbytes": int(offs[-1]), "in_pieces": after[0] - before[0], "fell_back": after[1] - before[1]}
        del d_z, d_zoff, d_true, d_out, d_items
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1])
    out_path, parent_lib, passes = os.path.join(ROOT, "profiles", "r12_batch_long_table.txt"), None, 2
    while args:
        a = args.pop(0)
        if a == "--out":
            out_path = args.pop(0)
        elif a == "--parent-lib":
            parent_lib = os.path.abspath(args.pop(0))
        elif a == "--passes":
            passes = int(args.pop(0))
    variants = [("feature on", {}), ("ZGPU_BATCH_PIECES_MIN_BYTES=0", {"ZGPU_BATCH_PIECES_MIN_BYTES": "0"})]
    if parent_lib:
        variants.append(("parent commit", {"ZAMD_GPU_LIB": parent_lib}))
    got = {v[0]: {} for v in variants}
    with tempfile.TemporaryDirectory() as tmp:
        prepare(tmp)
        for _ in range(passes):
            for vname, env in variants:
                e = dict(os.environ)
                for k in ("ZGPU_BATCH_PIECES_MIN_BYTES", "ZGPU_BATCH_PIECES_ROUND_BYTES", "ZAMD_GPU_LIB"):
                    e.pop(k, None)
                e.update(env)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], env=e, capture_output=True, text=True, timeout=900)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.exit("%s failed:\n%s" % (vname, p.stderr[-3000:]))
                print("timed:", vname, file=sys.stderr, flush=True)
                for row, rec in json.loads(line[0][7:]).items():
                    acc = got[vname].setdefault(row, {"ts": [], "zbytes": rec["zbytes"], "in_pieces": rec["in_pieces"], "fell_back": rec["fell_back"]})
                    acc["ts"] += rec["ts"]
    lines = ["# blocking batch inflate into given offsets (zgpu_inflate_batch_device), zlib items of the Silesia-mix at level 6, device-resident",
             "# median (min .. max) per call over %d passes x 5 timed windows of at least 0.5 s behind a warm-up call, the variants alternating in fresh processes;" % passes,
             "# GiB/s of decoded bytes; min .. max is the run-to-run spread of the variant's own timing"]
    if not parent_lib:
        lines.append("# parent commit: not measured (no --parent-lib)")
    for name, n, s in ROWS:
        any_rec = got[variants[0][0]][name]
        lines.append("# %s: %d items, %d bytes compressed, %d decoded" % (name, n, any_rec["zbytes"], n * s))
        for vname, _ in variants:
            rec = got[vname][name]
            med = statistics.median(rec["ts"])
            lines.append("%-32s %10.3f ms (%10.3f .. %10.3f) %8.2f GiB/s   in pieces %d, fell back %d" % (vname, med * 1e3, min(rec["ts"]) * 1e3, max(rec["ts"]) * 1e3, n * s / med / 2 ** 30,
                                                                                                      rec["in_pieces"], rec["fell_back"]))
        if parent_lib:
            on, par = got["feature on"][name]["ts"], got["parent commit"][name]["ts"]
            lines.append("parent / feature on = %.2f   (parent's spread: %.1f %% of its median)" % (statistics.median(par) / statistics.median(on),
                                                                                                   (max(par) - min(par)) / statistics.median(par) * 100))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
