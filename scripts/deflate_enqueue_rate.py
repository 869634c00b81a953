"""The stream-ordered batch deflate (zgpu_deflate_batch_packed_enqueue) against the blocking segment call (zgpu_deflate_segments_items_device), level 6, zlib
streams, everything device-resident, both sides in this one run:
  (a) small batches: 200 batches of 64 items of 4 KiB -- 200 blocking calls against 200 enqueues back to back on one stream, one workspace, and one
      synchronize at the end; microseconds per batch
  (b) one large batch: 16 384 items of 4 KiB, and 4 096 items of 64 KiB -- the blocking call against one enqueue plus synchronize, with the default rounds
      (batch_items = 0: 4 096 items a round) and with all items in one round (batch_items = n, what the blocking call does up to 65 536 chunks)
--blocking-lib PATH: the blocking side runs through another build of the engine (the parent commit's libzamd_gpu.so) with an engine of its own; without
it through the library under test.  Items: the synthetic Silesia-mix.  A figure is the median of 7 rounds behind a warm-up, the calls of a table timed in
turn, round after round; a host clock around calls that end in a device synchronize; GiB/s of input bytes.
Measured (profiles/r09_deflate_enqueue_table.txt, blocking side: the parent commit's build), enqueue over blocking: (a) 0.84; (b) 1.14 for the 4 KiB items
in rounds of 4 096 (1.003 in one round), 1.005 for the 64 KiB items.
Usage: python scripts/deflate_enqueue_rate.py [level] [--blocking-lib PATH] [--out PATH]   (default: profiles/r09_deflate_enqueue_table.txt)"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


class Blocking:
    """zgpu_deflate_segments_items_device of the library under test, or of another build with an engine of its own"""

    def __init__(self, eng, path):
        from zlib_amd import gpu
        self.L, self.h, self.own = eng.L, eng.h, False
        if path:
            vp, u64 = C.c_void_p, C.c_uint64
            self.L = C.CDLL(path)
            self.L.zgpu_engine_create.argtypes = [C.c_int, C.POINTER(vp)]
            self.L.zgpu_engine_destroy.argtypes = [vp]
            self.L.zgpu_engine_destroy.restype = None
            self.L.zgpu_deflate_segments_items_device.argtypes = [vp, vp, u64, vp, u64, C.POINTER(gpu._Params), vp, u64, vp, C.POINTER(gpu.DeflateResult), vp, vp]
            self.h = vp()
            assert self.L.zgpu_engine_create(0, C.byref(self.h)) == 0
            self.own = True

    def call(self, d_in, in_bytes, d_seg, n, p, d_out, cap, d_ooff, d_items):
        from zlib_amd import gpu
        res = gpu.DeflateResult()
        rc = self.L.zgpu_deflate_segments_items_device(self.h, d_in, in_bytes, d_seg, n, C.byref(p), d_out, cap, d_ooff, C.byref(res), d_items, None)
        assert rc == 0, rc
        return int(res.out_bytes)

    def close(self):
        if self.own:
            self.L.zgpu_engine_destroy(self.h)


class Shape:
    """n items of s bytes of the corpus, in batches of `per`: batch b compresses into its own slice of the output"""

    def __init__(self, eng, blk, d_corpus, n, s, per, level, batch_items=0):
        import torch
        from zlib_amd import gpu
        dev = d_corpus.device
        self.eng, self.blk, self.d_in, self.n, self.s, self.per, self.level, self.batch_items = eng, blk, d_corpus, n, s, per, level, batch_items
        self.flags = gpu.F_FINAL | gpu.F_ZLIB_WRAP
        self.p = gpu._Params(level, 0, self.flags, gpu.LZ_AUTO, 0, 0)
        self.nbatch = n // per
        self.cap = int(eng.L.zgpu_deflate_segments_bound(per, per * s, self.flags))
        self.d_seg = torch.tensor(np.arange(n + 1, dtype=np.int64) * s, device=dev)
        self.d_out = torch.empty(self.nbatch * self.cap, dtype=torch.uint8, device=dev)
        self.d_ooff = torch.empty(self.nbatch * (per + 1), dtype=torch.int64, device=dev)
        self.d_bitems = torch.empty(n * C.sizeof(gpu.DeflateItem), dtype=torch.uint8, device=dev)
        self.d_eitems = torch.empty(n * C.sizeof(gpu.DeflateBatchItem), dtype=torch.uint8, device=dev)
        self.d_sum = torch.zeros(C.sizeof(gpu.DeflateBatchSummary), dtype=torch.uint8, device=dev)
        self.ws = eng.deflate_batch_workspace_bytes(per, batch_items)
        self.d_ws = torch.empty(self.ws, dtype=torch.uint8, device=dev)

    def _args(self, b):
        return (self.d_seg.data_ptr() + 8 * self.per * b, self.d_out.data_ptr() + self.cap * b, self.d_ooff.data_ptr() + 8 * (self.per + 1) * b)

    def blocking(self):
        from zlib_amd import gpu
        for b in range(self.nbatch):
            seg, out, ooff = self._args(b)
            self.blk.call(self.d_in.data_ptr(), self.n * self.s, seg, self.per, self.p, out, self.cap, ooff, self.d_bitems.data_ptr() + C.sizeof(gpu.DeflateItem) * self.per * b)

    def enqueue(self):
        import torch
        from zlib_amd import gpu
        for b in range(self.nbatch):
            seg, out, ooff = self._args(b)
            self.eng.deflate_batch_packed_enqueue(self.d_in.data_ptr(), self.n * self.s, seg, self.per, self.level, out, self.cap, ooff,
                                                  self.d_eitems.data_ptr() + C.sizeof(gpu.DeflateBatchItem) * self.per * b, self.d_ws.data_ptr(), self.ws, flags=self.flags,
                                                  batch_items=self.batch_items, d_summary=self.d_sum.data_ptr())
        torch.cuda.synchronize()

    def check(self):
        """both sides give the same bytes, offsets and records"""
        import torch
        from zlib_amd import gpu
        self.d_out.zero_()
        torch.cuda.synchronize()
        self.blocking()
        torch.cuda.synchronize()
        out, ooff = self.d_out.clone(), self.d_ooff.clone()
        brec = np.frombuffer(self.d_bitems.cpu().numpy().tobytes(), dtype=np.dtype([("out_lo", "<u8"), ("out_bytes", "<u8"), ("in_bytes", "<u4"), ("data_type", "<u4"), ("adler32", "<u4"), ("crc32", "<u4")]))
        self.d_out.zero_()
        self.d_ooff.zero_()
        torch.cuda.synchronize()
        self.enqueue()
        erec = np.frombuffer(self.d_eitems.cpu().numpy().tobytes(), dtype=np.dtype([("code", "<i4"), ("data_type", "<u4"), ("out_lo", "<u8"), ("out_bytes", "<u8"), ("in_bytes", "<u4"),
                                                                                   ("adler32", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")]))
        assert bool((self.d_out == out).all()) and bool((self.d_ooff == ooff).all()), "enqueue and blocking call disagree"
        assert (erec["code"] == 0).all() and all((erec[f] == brec[f]).all() for f in ("out_lo", "out_bytes", "in_bytes", "data_type", "adler32", "crc32"))
        assert np.frombuffer(self.d_sum.cpu().numpy().tobytes(), dtype=np.uint64)[0] == 0
        return int(self.d_ooff[self.per].item()) if self.nbatch == 1 else None


def row(lines, tag, m, nbytes, nbatch=1):
    per = "%8.1f us/batch" % (m[0] / nbatch * 1e6) if nbatch > 1 else "%8.2f GiB/s" % (nbytes / m[0] / 2 ** 30)
    lines.append("%-58s %9.3f ms (%9.3f .. %9.3f) %s" % (tag, m[0] * 1e3, m[1] * 1e3, m[2] * 1e3, per))


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "r09_deflate_enqueue_table.txt")
    blocking_lib = None
    for opt in ("--out", "--blocking-lib"):
        if opt in args:
            i = args.index(opt)
            if opt == "--out":
                out_path = args[i + 1]
            else:
                blocking_lib = args[i + 1]
            del args[i: i + 2]
    level = int(args[0]) if args else 6
    import torch
    import zlib_amd
    eng = zlib_amd.Engine(0)
    blk = Blocking(eng, blocking_lib)
    dev = torch.device("cuda", 0)
    total = 256 << 20
    d_corpus = torch.empty(total, dtype=torch.uint8, device=dev)
    eng.corpus_fill_device(0, 1, 0, total >> 16, d_corpus.data_ptr())
    torch.cuda.synchronize()
    lines = ["# stream-ordered batch deflate (packed entry) against the blocking segment call, zlib streams of the Silesia-mix at level %d, device-resident" % level,
             "# blocking side: %s" % ("another build of the engine (--blocking-lib), an engine of its own" if blocking_lib else "the library under test"),
             "# median (min .. max) over %d rounds behind a warm-up, the rows of a block timed in turn; host clock around a final synchronize" % REPS]

    sh = Shape(eng, blk, d_corpus, 200 * 64, 4096, 64, level)
    sh.check()
    t = in_turn([("b", sh.blocking), ("e", sh.enqueue)])
    lines.append("# (a) %d batches of %d items of %d bytes, one stream, one workspace of %d bytes" % (sh.nbatch, sh.per, sh.s, sh.ws))
    row(lines, "%d blocking calls" % sh.nbatch, t["b"], 0, sh.nbatch)
    row(lines, "%d enqueues, one synchronize" % sh.nbatch, t["e"], 0, sh.nbatch)
    lines.append("enqueue / blocking = %.3f" % (t["e"][0] / t["b"][0]))
    del sh

    for n, s in ((16384, 4096), (4096, 65536)):
        shapes = [("rounds of 4096 (batch_items = 0)", Shape(eng, blk, d_corpus, n, s, n, level))]
        one_ws = eng.deflate_batch_workspace_bytes(n, n)
        if n > 4096 and torch.cuda.mem_get_info(0)[0] > one_ws + (8 << 30):
            shapes.append(("one round (batch_items = n)", Shape(eng, blk, d_corpus, n, s, n, level, batch_items=n)))
        zbytes = [sh.check() for _, sh in shapes][0]
        t = in_turn([("b", shapes[0][1].blocking)] + [("e%d" % i, sh.enqueue) for i, (_, sh) in enumerate(shapes)])
        lines.append("# (b) one batch of %d items of %d bytes: %d bytes in, %d out" % (n, s, n * s, zbytes))
        row(lines, "blocking call", t["b"], n * s)
        for i, (name, sh) in enumerate(shapes):
            row(lines, "enqueue + synchronize, %s" % name, t["e%d" % i], n * s)
            lines.append("enqueue / blocking = %.3f (%s; workspace %d bytes)" % (t["e%d" % i][0] / t["b"][0], name, sh.ws))
        del shapes, sh

    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    blk.close()
    eng.close()


if __name__ == "__main__":
    main()
