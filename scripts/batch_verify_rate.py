"""The batch integrity test (zgpu_inflate_batch_verify_*) against the two calls that exist beside it, per shape, device-resident and from host buffers:
  (v) the verify call: every item decoded inside its workgroup, check values folded there, trailers compared, no destination
  (s) the sizing call: sizes and verdicts of the deflate data, no check value, no trailer compared
  (p) the packed decode with the same `checks`: sizing pass, layout, decode into memory, checksum kernels, trailers compared
Shapes: those of profiles/r06_batch_sizes_table.txt -- 16 384 zlib items of 4 KiB of the synthetic Silesia-mix (made by zgpu_deflate_segments_device) and
256 items of 1 MiB of it (made by Python's zlib).  The three calls are timed in turn, round after round, in this one process: a figure is the median of
`reps` rounds behind a warm-up call each, a host clock around calls that end in a device synchronise (short calls looped); rates count decoded bytes.
Peak device memory: what a fresh engine allocates for the call (free device memory before the engine was made minus the lowest seen after the call; the
engine's buffers only grow; the figure is rounded as the device allocator rounds its allocations) plus the buffers the caller must bring, the input and its
offsets left out.
Usage: python scripts/batch_verify_rate.py [level] [--out PATH]   (default: profiles/r07_batch_verify_table.txt)"""
import ctypes as C
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHECKS = 0  # what the wrapper needs: Adler-32 for zlib items, in (v) and in (p)


def alternating(fns, reps=7, window=0.1):
    """{name: (median, min, max) seconds per call}: a warm-up call each, then `reps` rounds in which every call gets a timed window in turn"""
    import torch
    inner = {}
    for name, fn in fns:
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        inner[name] = max(1, min(200, int(window / max(time.perf_counter() - t0, 1e-6)) + 1))
    ts = {name: [] for name, _ in fns}
    for _ in range(reps):
        for name, fn in fns:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner[name]):
                fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) / inner[name])
    return {name: (statistics.median(t), min(t), max(t)) for name, t in ts.items()}


def engine_bytes(call):
    """device bytes a fresh engine allocates to serve `call` once"""
    import torch
    import zlib_amd
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    eng = zlib_amd.Engine(0)
    call(eng)
    torch.cuda.synchronize()
    used = free0 - torch.cuda.mem_get_info(0)[0]
    eng.close()
    return max(used, 0)


def shape(eng, dev, name, d_z, zbytes, d_zoff, n, s, lines):
    import torch
    from zlib_amd import gpu
    total = n * s
    isz = C.sizeof(gpu.InflateItem)
    d_items = torch.empty(n * isz, dtype=torch.uint8, device=dev)
    d_out = torch.empty(total, dtype=torch.uint8, device=dev)
    d_ooff = torch.empty(n + 1, dtype=torch.int64, device=dev)

    def records(t=None):
        raw = (d_items.cpu().numpy() if t is None else t).tobytes()
        return [gpu.InflateItem.from_buffer_copy(raw, k * isz) for k in range(n)]

    def verify(e=eng):
        assert e.inflate_batch_verify_device(d_z.data_ptr(), zbytes, d_zoff.data_ptr(), n, d_items.data_ptr(), wrap="zlib", checks=CHECKS) == 0

    def sizes(e=eng):
        assert e.inflate_batch_sizes_device(d_z.data_ptr(), zbytes, d_zoff.data_ptr(), n, d_items.data_ptr(), wrap="zlib") == 0

    def packed(e=eng):
        rc, tot, failed = e.inflate_batch_packed_device(d_z.data_ptr(), zbytes, d_zoff.data_ptr(), n, d_out.data_ptr(), total, d_ooff.data_ptr(), d_items.data_ptr(), wrap="zlib",
                                                        checks=CHECKS)
        assert (rc, tot, failed) == (0, total, 0), (rc, tot, failed)
    packed()
    want = [(r.code, r.msg, r.out_bytes, r.in_used, r.adler32, r.crc32) for r in records()]
    verify()
    assert [(r.code, r.msg, r.out_bytes, r.in_used, r.adler32, r.crc32) for r in records()] == want and all(w[0] == 0 and w[2] == s for w in want), "verify and decode disagree"
    t = alternating([("v", verify), ("s", sizes), ("p", packed)])
    mem_v, mem_p = engine_bytes(verify), engine_bytes(packed) + total + 8 * (n + 1)

    # the same from host buffers
    h_z, h_zoff = d_z[:zbytes].cpu().numpy(), d_zoff.cpu().numpy().astype(np.uint64)
    h_items = (gpu.InflateItem * n)()
    h_out, h_ooff = np.empty(total + 1, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
    failed, tot = C.c_uint64(0), C.c_uint64(0)

    def h_verify():
        assert eng.L.zgpu_inflate_batch_verify_host(eng.h, h_z.ctypes.data, zbytes, h_zoff.ctypes.data, n, gpu.WRAP_ZLIB, CHECKS, h_items, C.byref(failed)) == 0 and failed.value == 0

    def h_sizes():
        assert eng.L.zgpu_inflate_batch_sizes_host(eng.h, h_z.ctypes.data, zbytes, h_zoff.ctypes.data, n, gpu.WRAP_ZLIB, h_items, C.byref(failed)) == 0 and failed.value == 0

    def h_packed():
        assert eng.L.zgpu_inflate_batch_packed_host(eng.h, h_z.ctypes.data, zbytes, h_zoff.ctypes.data, n, gpu.WRAP_ZLIB, CHECKS, 1, h_out.ctypes.data, total, h_ooff.ctypes.data, h_items,
                                                    C.byref(tot), C.byref(failed)) == 0 and failed.value == 0
    th = alternating([("v", h_verify), ("s", h_sizes), ("p", h_packed)])

    lines.append("# %s: %d items, %d bytes compressed, %d decoded" % (name, n, zbytes, total))
    for where, tt in (("device-resident", t), ("host buffers", th)):
        for tag, key in (("(v) verify call", "v"), ("(s) sizing call", "s"), ("(p) packed decode", "p")):
            m = tt[key]
            lines.append("%-16s %-20s %9.3f ms (%9.3f .. %9.3f) %8.2f GiB/s %8.3f us/item" % (where, tag, m[0] * 1e3, m[1] * 1e3, m[2] * 1e3, total / m[0] / 2 ** 30, m[0] / n * 1e6))
        lines.append("%-16s (v)/(s) = %.3f   (v)/(p) = %.3f" % (where, tt["v"][0] / tt["s"][0], tt["v"][0] / tt["p"][0]))
    lines.append("peak device memory beside the input, device-resident: (v) %d bytes (%.1f per item)   (p) %d bytes (%.2f x decoded)" % (mem_v, mem_v / n, mem_p, mem_p / total))


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "r07_batch_verify_table.txt")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i: i + 2]
    level = int(args[0]) if args else 6
    import torch
    import zlib_amd
    from zlib_amd import gpu
    eng = zlib_amd.Engine(0)
    dev = torch.device("cuda", 0)
    total = 256 << 20
    d_corpus = torch.empty(total, dtype=torch.uint8, device=dev)
    eng.corpus_fill_device(0, 1, 0, total >> 16, d_corpus.data_ptr())
    torch.cuda.synchronize()
    lines = ["# batch integrity test, zlib items of the Silesia-mix at level %d, checks = what the wrapper needs (Adler-32)" % level,
             "# (v), (s), (p) timed in turn, round after round: median (min .. max) per call over 7 rounds behind a warm-up call; GiB/s of decoded bytes"]

    # ---- 16 384 items of 4 KiB, compressed on the device ----
    n, s = 16384, 4096
    flags = gpu.F_FINAL | gpu.F_ZLIB_WRAP
    seg = torch.tensor(np.arange(n + 1, dtype=np.int64) * s, device=dev)
    cap = int(eng.L.zgpu_deflate_segments_bound(n, n * s, flags))
    d_z = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_zoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    p = gpu._Params(level, 0, flags, gpu.LZ_AUTO, 0, 0)
    res = gpu.DeflateResult()
    eng._check(eng.L.zgpu_deflate_segments_device(eng.h, d_corpus.data_ptr(), n * s, seg.data_ptr(), n, C.byref(p), d_z.data_ptr(), cap, d_zoff.data_ptr(), C.byref(res), None))
    shape(eng, dev, "4 KiB items", d_z, int(res.out_bytes), d_zoff, n, s, lines)
    del d_z, d_zoff, seg

    # ---- 256 items of 1 MiB, compressed by Python's zlib ----
    n, s = 256, 1 << 20
    corpus = d_corpus.cpu().numpy()
    del d_corpus
    zs = [zlib.compress(corpus[k * s:(k + 1) * s].tobytes(), level) for k in range(n)]
    zoff = np.zeros(n + 1, dtype=np.int64)
    zoff[1:] = np.cumsum([len(z) for z in zs])
    d_z = torch.tensor(np.frombuffer(b"".join(zs), dtype=np.uint8), device=dev)
    d_zoff = torch.tensor(zoff, device=dev)
    shape(eng, dev, "1 MiB items", d_z, int(zoff[-1]), d_zoff, n, s, lines)

    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
