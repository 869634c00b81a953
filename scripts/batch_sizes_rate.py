"""Batch inflate without known sizes: the sizing pass (zgpu_inflate_batch_sizes_device) and the packed decode (zgpu_inflate_batch_packed_device)
against what they replace and what they build on.  Per shape, device-resident input, offsets, output and records:
  (a) the sizing call
  (b) the only way to sizes without it: zgpu_inflate_batch_device into all-empty ranges, out_bytes of the ZGPU_BUF_ERROR records
  (c) the packed call (sizing pass, layout, decode)
  (d) the plain batch decode given the true offsets
Shapes: 16 384 zlib items of 4 KiB of the synthetic Silesia-mix (the shape of profiles/r05_batch_table.txt, made by zgpu_deflate_segments_device) and
256 items of 1 MiB of it (made by Python's zlib).  Every figure is the median of `reps` timed windows behind a warm-up call, a host clock around
calls that end in a device synchronise, all in this one process; rates count decoded bytes.
Usage: python scripts/batch_sizes_rate.py [level] [--out PATH]   (default: profiles/r06_batch_sizes_table.txt)"""
import ctypes as C
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=5, window=0.25):
    """median, min, max seconds per call: a warm-up call, then `reps` windows of as many calls as fill `window` seconds (short calls are looped)"""
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
    return statistics.median(ts), min(ts), max(ts)


def shape(eng, dev, name, d_corpus, d_z, zbytes, d_zoff, n, s, lines):
    import torch
    from zlib_amd import gpu
    total = n * s
    isz = C.sizeof(gpu.InflateItem)
    d_items = torch.empty(n * isz, dtype=torch.uint8, device=dev)
    d_out = torch.empty(total, dtype=torch.uint8, device=dev)
    d_ooff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_true = torch.tensor(np.arange(n + 1, dtype=np.int64) * s, device=dev)
    d_empty = torch.zeros(n + 1, dtype=torch.int64, device=dev)

    def records():
        raw = d_items.cpu().numpy().tobytes()
        return [gpu.InflateItem.from_buffer_copy(raw, k * isz) for k in range(n)]

    def sizes():
        assert eng.inflate_batch_sizes_device(d_z.data_ptr(), zbytes, d_zoff.data_ptr(), n, d_items.data_ptr(), wrap="zlib") == 0
    t_a = timed(sizes)
    assert all(r.code == 0 and r.out_bytes == s for r in records()), "the sizing pass is wrong"

    def empty_ranges():
        assert eng.inflate_batch_device(d_z.data_ptr(), zbytes, d_zoff.data_ptr(), n, d_out.data_ptr(), total, d_empty.data_ptr(), d_items.data_ptr(), wrap="zlib") == n
    t_b = timed(empty_ranges)
    assert all(r.code == gpu.BUF_ERROR and r.out_bytes == s for r in records()), "the decode into empty ranges gives other sizes"

    def packed():
        rc, tot, failed = eng.inflate_batch_packed_device(d_z.data_ptr(), zbytes, d_zoff.data_ptr(), n, d_out.data_ptr(), total, d_ooff.data_ptr(), d_items.data_ptr(), wrap="zlib")
        assert (rc, tot, failed) == (0, total, 0), (rc, tot, failed)
    d_out.zero_()
    t_c = timed(packed)
    assert torch.equal(d_out, d_corpus[:total]) and torch.equal(d_ooff, d_true), "the packed decode differs from the corpus"

    def plain():
        assert eng.inflate_batch_device(d_z.data_ptr(), zbytes, d_zoff.data_ptr(), n, d_out.data_ptr(), total, d_true.data_ptr(), d_items.data_ptr(), wrap="zlib") == 0
    d_out.zero_()
    t_d = timed(plain)
    assert torch.equal(d_out, d_corpus[:total]), "the batch decode differs from the corpus"

    lines.append("# %s: %d items, %d bytes compressed, %d decoded" % (name, n, zbytes, total))
    for tag, t in (("(a) sizing call", t_a), ("(b) decode into empty ranges", t_b), ("(c) packed call", t_c), ("(d) batch decode, true offsets", t_d)):
        lines.append("%-34s %9.3f ms (%9.3f .. %9.3f) %8.2f GiB/s %8.3f us/item" % (tag, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, total / t[0] / 2 ** 30, t[0] / n * 1e6))
    lines.append("(a)/(b) = %.3f   (c)/(d) = %.3f   ((a)+(d))/(c) = %.3f" % (t_a[0] / t_b[0], t_c[0] / t_d[0], (t_a[0] + t_d[0]) / t_c[0]))


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "r06_batch_sizes_table.txt")
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
    lines = ["# batch inflate without known sizes, zlib items of the Silesia-mix at level %d, device-resident" % level,
             "# median (min .. max) per call over timed windows of at least 0.25 s (short calls looped) behind a warm-up call; GiB/s of decoded bytes"]

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
    shape(eng, dev, "4 KiB items", d_corpus, d_z, int(res.out_bytes), d_zoff, n, s, lines)
    del d_z, d_zoff, seg

    # ---- 256 items of 1 MiB, compressed by Python's zlib ----
    n, s = 256, 1 << 20
    corpus = d_corpus.cpu().numpy()
    zs = [zlib.compress(corpus[k * s:(k + 1) * s].tobytes(), level) for k in range(n)]
    zoff = np.zeros(n + 1, dtype=np.int64)
    zoff[1:] = np.cumsum([len(z) for z in zs])
    d_z = torch.tensor(np.frombuffer(b"".join(zs), dtype=np.uint8), device=dev)
    d_zoff = torch.tensor(zoff, device=dev)
    shape(eng, dev, "1 MiB items", d_corpus, d_z, int(zoff[-1]), d_zoff, n, s, lines)

    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
