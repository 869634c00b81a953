"""The stream-ordered batch inflate (zgpu_inflate_batch_*_enqueue) against the blocking entry points, everything device-resident, both sides in this one run:
  (a) small batches: 200 batches of 64 zlib items of 4 KiB -- 200 blocking zgpu_inflate_batch_device calls against 200 enqueues on one stream and one
      synchronize; microseconds per batch
  (b) large batches, the shapes of profiles/r06_batch_sizes_table.txt (16 384 items of 4 KiB, 256 items of 1 MiB): one blocking decode against one enqueue
      plus synchronize, and the same for the packed decode; the ratio enqueue / blocking, and the peak device memory beside input and output
Both decoders pick their ring by ZGPU_INF_RING_KB (8 KiB unless set); (b) times every ring instantiation built -- 8, 16 and 32 KiB -- on both sides, (a)
the default.  Items: the synthetic Silesia-mix at level 6, the 4 KiB ones compressed on the device, the
1 MiB ones by Python's zlib.  A figure is the median of 7 rounds behind a warm-up, the calls of a table timed in turn, round after round; a host clock
around calls that end in a device synchronize; GiB/s of decoded bytes.
Peak device memory: blocking -- what a fresh engine allocates for the call (free device memory before the engine was made minus free memory after the
call); enqueue -- the workspace the caller brings, zgpu_inflate_batch_workspace_bytes.
Usage: python scripts/batch_enqueue_rate.py [level] [--out PATH]   (default: profiles/r08_batch_enqueue_table.txt)"""
import ctypes as C
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHECKS = 0  # what the wrapper needs: Adler-32 for zlib items
REPS = 7


def in_turn(fns, reps=REPS):
    """{name: (median, min, max) seconds}: a warm-up each, then `reps` rounds in which every function is timed once, in turn"""
    import torch
    for _, fn in fns:
        fn()
    ts = {name: [] for name, _ in fns}
    for _ in range(reps):
        for name, fn in fns:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in ts.items()}


def engine_bytes(call):
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


def with_ring(kb, fn):
    def run(*a):
        os.environ["ZGPU_INF_RING_KB"] = str(kb)
        try:
            fn(*a)
        finally:
            del os.environ["ZGPU_INF_RING_KB"]
    return run


class Shape:
    def __init__(self, eng, dev, d_z, zbytes, d_zoff, n, s):
        import torch
        from zlib_amd import gpu
        self.eng, self.d_z, self.zbytes, self.d_zoff, self.n, self.s, self.total = eng, d_z, zbytes, d_zoff, n, s, n * s
        self.isz = C.sizeof(gpu.InflateItem)
        self.d_items = torch.empty(n * self.isz, dtype=torch.uint8, device=dev)
        self.d_out = torch.empty(self.total, dtype=torch.uint8, device=dev)
        self.d_ooff = torch.tensor(np.arange(n + 1, dtype=np.int64) * s, device=dev)
        self.d_poff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        self.d_sum = torch.zeros(C.sizeof(gpu.InflateBatchSummary), dtype=torch.uint8, device=dev)
        self.ws = {job: eng.inflate_batch_workspace_bytes(job, n) for job in (gpu.JOB_DECODE, gpu.JOB_PACKED)}
        self.d_ws = torch.empty(max(self.ws.values()), dtype=torch.uint8, device=dev)

    def blocking(self, e=None):
        e = e or self.eng
        assert e.inflate_batch_device(self.d_z.data_ptr(), self.zbytes, self.d_zoff.data_ptr(), self.n, self.d_out.data_ptr(), self.total, self.d_ooff.data_ptr(), self.d_items.data_ptr(),
                                      wrap="zlib", checks=CHECKS) == 0

    def enqueue(self):
        import torch
        from zlib_amd import gpu
        self.eng.inflate_batch_enqueue(self.d_z.data_ptr(), self.zbytes, self.d_zoff.data_ptr(), self.n, self.d_out.data_ptr(), self.total, self.d_ooff.data_ptr(), self.d_items.data_ptr(),
                                       self.d_ws.data_ptr(), self.ws[gpu.JOB_DECODE], wrap="zlib", checks=CHECKS, d_summary=self.d_sum.data_ptr())
        torch.cuda.synchronize()

    def blocking_packed(self, e=None):
        e = e or self.eng
        rc, tot, failed = e.inflate_batch_packed_device(self.d_z.data_ptr(), self.zbytes, self.d_zoff.data_ptr(), self.n, self.d_out.data_ptr(), self.total, self.d_poff.data_ptr(),
                                                        self.d_items.data_ptr(), wrap="zlib", checks=CHECKS)
        assert (rc, tot, failed) == (0, self.total, 0)

    def enqueue_packed(self):
        import torch
        from zlib_amd import gpu
        self.eng.inflate_batch_packed_enqueue(self.d_z.data_ptr(), self.zbytes, self.d_zoff.data_ptr(), self.n, self.d_out.data_ptr(), self.total, self.d_poff.data_ptr(),
                                              self.d_items.data_ptr(), self.d_ws.data_ptr(), self.ws[gpu.JOB_PACKED], wrap="zlib", checks=CHECKS, d_summary=self.d_sum.data_ptr())
        torch.cuda.synchronize()

    def records(self):
        return self.d_items.cpu().numpy().tobytes()

    def check(self):
        """both sides give the same records and bytes"""
        import torch
        self.blocking()
        want, out = self.records(), self.d_out.clone()
        for fn in (self.enqueue, self.enqueue_packed):
            self.d_out.zero_()
            self.d_items.zero_()
            torch.cuda.synchronize()  # (the calls run on the engine's stream, not on torch's)
            fn()
            assert self.records() == want and bool((self.d_out == out).all()), "enqueue and blocking decode disagree"
            assert np.frombuffer(self.d_sum.cpu().numpy().tobytes(), dtype=np.uint64)[0] == 0


def large(sh, name, lines):
    from zlib_amd import gpu
    sh.check()
    rings = (8, 16, 32)
    fns = []
    for kb in rings:
        fns += [("b%d" % kb, with_ring(kb, sh.blocking)), ("e%d" % kb, with_ring(kb, sh.enqueue)), ("pb%d" % kb, with_ring(kb, sh.blocking_packed)),
                ("pe%d" % kb, with_ring(kb, sh.enqueue_packed))]
    t = in_turn(fns)
    lines.append("# (b) %s: %d items, %d bytes compressed, %d decoded" % (name, sh.n, sh.zbytes, sh.total))
    for job, b, e in (("decode", "b", "e"), ("packed", "pb", "pe")):
        for kb in rings:
            for tag, key in (("blocking", b), ("enqueue + synchronize (fused)", e)):
                m = t[key + str(kb)]
                lines.append("%s  %2d KiB ring%s  %-30s %9.3f ms (%9.3f .. %9.3f) %8.2f GiB/s" % (job, kb, " (default)" if kb == 8 else "          ", tag, m[0] * 1e3, m[1] * 1e3, m[2] * 1e3,
                                                                                              sh.total / m[0] / 2 ** 30))
        lines.append("%s  enqueue / blocking = %s" % (job, "  ".join("%.3f (%d KiB ring)" % (t[e + str(kb)][0] / t[b + str(kb)][0], kb) for kb in rings)))
    mb, mpb = engine_bytes(sh.blocking), engine_bytes(sh.blocking_packed)
    lines.append("peak device memory beside input and output: decode blocking %d bytes, enqueue %d (%.1f per item); packed blocking %d, enqueue %d (%.1f per item)" %
                 (mb, sh.ws[gpu.JOB_DECODE], sh.ws[gpu.JOB_DECODE] / sh.n, mpb, sh.ws[gpu.JOB_PACKED], sh.ws[gpu.JOB_PACKED] / sh.n))


def small(sh, lines, nbatch=200, per=64):
    """batches of `per` items cut from the 4 KiB shape: the tables are slices of the shape's tables (their entries are offsets into the whole buffers)"""
    import torch
    from zlib_amd import gpu
    eng = sh.eng
    ws = eng.inflate_batch_workspace_bytes(gpu.JOB_DECODE, per)
    args = [(sh.d_zoff.data_ptr() + 8 * per * b, sh.d_ooff.data_ptr() + 8 * per * b, sh.d_items.data_ptr() + sh.isz * per * b) for b in range(nbatch)]

    def blocking():
        for zoff, ooff, items in args:
            assert eng.inflate_batch_device(sh.d_z.data_ptr(), sh.zbytes, zoff, per, sh.d_out.data_ptr(), sh.total, ooff, items, wrap="zlib", checks=CHECKS) == 0

    def enqueue():
        for zoff, ooff, items in args:
            eng.inflate_batch_enqueue(sh.d_z.data_ptr(), sh.zbytes, zoff, per, sh.d_out.data_ptr(), sh.total, ooff, items, sh.d_ws.data_ptr(), ws, wrap="zlib", checks=CHECKS)
        torch.cuda.synchronize()
    blocking()
    want = sh.records()[: nbatch * per * sh.isz]
    sh.d_items.zero_()
    torch.cuda.synchronize()
    enqueue()
    assert sh.records()[: nbatch * per * sh.isz] == want, "enqueue and blocking decode disagree"
    t = in_turn([("b", blocking), ("e", enqueue)])
    lines.append("# (a) %d batches of %d items of %d bytes, one stream, one workspace" % (nbatch, per, sh.s))
    for tag, key in (("%d blocking calls" % nbatch, "b"), ("%d enqueues, one synchronize" % nbatch, "e")):
        m = t[key]
        lines.append("%-52s %9.3f ms (%9.3f .. %9.3f) %8.1f us/batch" % (tag, m[0] * 1e3, m[1] * 1e3, m[2] * 1e3, m[0] / nbatch * 1e6))
    lines.append("enqueue / blocking = %.3f" % (t["e"][0] / t["b"][0]))


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "r08_batch_enqueue_table.txt")
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
    lines = ["# stream-ordered batch inflate against the blocking entry points, zlib items of the Silesia-mix at level %d, device-resident, checks = Adler-32" % level,
             "# median (min .. max) over %d rounds behind a warm-up, the rows of a block timed in turn; host clock around a final synchronize" % REPS]

    n, s = 16384, 4096
    flags = gpu.F_FINAL | gpu.F_ZLIB_WRAP
    seg = torch.tensor(np.arange(n + 1, dtype=np.int64) * s, device=dev)
    cap = int(eng.L.zgpu_deflate_segments_bound(n, n * s, flags))
    d_z = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_zoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    p = gpu._Params(level, 0, flags, gpu.LZ_AUTO, 0, 0)
    res = gpu.DeflateResult()
    eng._check(eng.L.zgpu_deflate_segments_device(eng.h, d_corpus.data_ptr(), n * s, seg.data_ptr(), n, C.byref(p), d_z.data_ptr(), cap, d_zoff.data_ptr(), C.byref(res), None))
    sh = Shape(eng, dev, d_z, int(res.out_bytes), d_zoff, n, s)
    small(sh, lines)
    large(sh, "4 KiB items", lines)
    del sh, d_z, d_zoff, seg

    n, s = 256, 1 << 20
    corpus = d_corpus.cpu().numpy()
    del d_corpus
    zs = [zlib.compress(corpus[k * s:(k + 1) * s].tobytes(), level) for k in range(n)]
    zoff = np.zeros(n + 1, dtype=np.int64)
    zoff[1:] = np.cumsum([len(z) for z in zs])
    d_z = torch.tensor(np.frombuffer(b"".join(zs), dtype=np.uint8), device=dev)
    d_zoff = torch.tensor(zoff, device=dev)
    large(Shape(eng, dev, d_z, int(zoff[-1]), d_zoff, n, s), "1 MiB items", lines)

    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
