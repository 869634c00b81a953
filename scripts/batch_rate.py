"""Many small independent streams: one batch call (zgpu_deflate_segments_* with the zlib wrapper, zgpu_inflate_batch_*) against a loop of one call per
item (compress2-style zgpu_deflate_host, zgpu_inflate_stream_host) over a sample of the items.  The items are slices of 1, 4, 16 and 64 KiB of the
synthetic Silesia-mix (zgpu_corpus_fill_device).  Device: input, offsets and output resident in HBM; host: from and to host buffers.  Rates count
the decoded (uncompressed) bytes.  Usage: python scripts/batch_rate.py [MiB of corpus] [level]  (profiles/r05_batch_table.txt)"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zlib_amd  # noqa: E402
from zlib_amd import gpu  # noqa: E402


def best(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    mib = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    level = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    eng = zlib_amd.Engine(0)
    dev = torch.device("cuda", 0)
    total = mib << 20
    d_corpus = torch.empty(total, dtype=torch.uint8, device=dev)
    eng.corpus_fill_device(0, 1, 0, total >> 16, d_corpus.data_ptr())
    torch.cuda.synchronize()
    corpus = d_corpus.cpu().numpy().tobytes()
    flags = gpu.F_FINAL | gpu.F_ZLIB_WRAP
    print("# batch of n independent zlib streams, Silesia-mix, level %d, %d MiB in all; GiB/s of decoded bytes, us per item" % (level, mib))
    print("# %-6s %7s | %-27s | %-27s | %-27s | %-27s | %-19s | %-19s" % ("item", "n", "encode batch, device", "encode batch, host", "decode batch, device",
                                                                         "decode batch, host", "encode loop (1/item)", "decode loop (1/item)"))
    for kib in (1, 4, 16, 64):
        s = kib << 10
        n = total // s
        items = [corpus[i * s:(i + 1) * s] for i in range(n)]
        # ---- encode, device-resident ----
        seg = torch.tensor(np.arange(n + 1, dtype=np.int64) * s, device=dev)
        cap = int(eng.L.zgpu_deflate_segments_bound(n, total, flags))
        d_z = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_zoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        p = gpu._Params(level, 0, flags, gpu.LZ_AUTO, 0, 0)
        res = gpu.DeflateResult()

        def enc_dev():
            eng._check(eng.L.zgpu_deflate_segments_device(eng.h, d_corpus.data_ptr(), total, seg.data_ptr(), n, C.byref(p), d_z.data_ptr(), cap,
                                                          d_zoff.data_ptr(), C.byref(res), None))
        t_ed = best(enc_dev)
        zbytes = res.out_bytes
        # ---- encode, host buffers (the C entry alone: arrays prepared in front) ----
        h_in = np.frombuffer(corpus, dtype=np.uint8)
        h_seg = np.arange(n + 1, dtype=np.uint64) * s
        h_z = np.empty(cap, dtype=np.uint8)
        h_zoff = np.zeros(n + 1, dtype=np.uint64)

        def enc_host():
            eng._check(eng.L.zgpu_deflate_segments_host(eng.h, h_in.ctypes.data, h_seg.ctypes.data, n, C.byref(p), h_z.ctypes.data, cap,
                                                        h_zoff.ctypes.data, C.byref(res)))
        t_eh = best(enc_host, reps=2)
        zs = [h_z[int(h_zoff[i]): int(h_zoff[i + 1])].tobytes() for i in range(n)]
        # ---- decode, device-resident: the encoder's output as it lies ----
        d_out = torch.empty(total, dtype=torch.uint8, device=dev)
        d_items = torch.empty(n * C.sizeof(gpu.InflateItem), dtype=torch.uint8, device=dev)

        def dec_dev():
            f = eng.inflate_batch_device(d_z.data_ptr(), zbytes, d_zoff.data_ptr(), n, d_out.data_ptr(), total, seg.data_ptr(), d_items.data_ptr(), wrap="zlib")
            assert f == 0
        t_dd = best(dec_dev)
        assert torch.equal(d_out, d_corpus), "device batch decode differs from the corpus"
        # ---- decode, host buffers ----
        h_out = np.empty(total, dtype=np.uint8)
        h_items = (gpu.InflateItem * n)()
        failed = C.c_uint64(0)

        def dec_host():
            eng._check(eng.L.zgpu_inflate_batch_host(eng.h, h_z.ctypes.data, int(h_zoff[n]), h_zoff.ctypes.data, n, gpu.WRAP_ZLIB, 0, h_out.ctypes.data,
                                                     total, h_seg.ctypes.data, h_items, C.byref(failed)))
            assert failed.value == 0
        t_dh = best(dec_host, reps=2)
        assert h_out.tobytes() == corpus, "host batch decode differs from the corpus"
        # ---- one call per item, over a sample ----
        k = min(n, 64)
        sample = list(range(0, n, max(1, n // k)))[:k]
        t0 = time.perf_counter()
        for i in sample:
            eng.deflate_host(items[i], level)
        t_el = (time.perf_counter() - t0) / len(sample)
        t0 = time.perf_counter()
        for i in sample:
            eng.inflate_stream_host(zs[i][2:-4], s)
        t_dl = (time.perf_counter() - t0) / len(sample)
        g = lambda t: total / t / 2 ** 30  # noqa: E731
        us = lambda t: t / n * 1e6  # noqa: E731
        print("%-4s KiB %7d | %7.2f GiB/s %7.2f us/item | %7.2f GiB/s %7.2f us/item | %7.2f GiB/s %7.2f us/item | %7.2f GiB/s %7.2f us/item | %8.4f GiB/s %7.0f us | %8.4f GiB/s %7.0f us" % (
            kib, n, g(t_ed), us(t_ed), g(t_eh), us(t_eh), g(t_dd), us(t_dd), g(t_dh), us(t_dh), s / t_el / 2 ** 30, t_el * 1e6, s / t_dl / 2 ** 30, t_dl * 1e6))
        sys.stdout.flush()
    eng.close()


if __name__ == "__main__":
    main()
