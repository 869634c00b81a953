"""ZIP archives in batches: zamd_zip_add_batch / zamd_unzip_read_batch (include/zamd_zip_batch.h) against the member-by-member loop over the same
members -- zamd_zip_add / zamd_unzip_read of the same build, in the same run -- and the batch checksum call on the same item sets.
Two archives of 16 MiB of the synthetic log-text corpus (zgpu_corpus_fill_device kind 1) at one level: 4 096 members of 4 KiB, 256 members of 64 KiB.
Every figure is the median (min .. max) of `reps` timed calls behind a warm-up call of each kind, batch and loop alternating; a host clock around
calls that return when the archive is closed (write) or every member's bytes are in the caller's buffers (read); archives in a temporary directory.
Usage: python scripts/zip_rate.py [level] [--out PATH] [--reps N]     (default: level 6, profiles/r05_zip_table.txt, 5)"""
import ctypes as C
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED5117  # the corpus seed of the other rate scripts
sys.path.insert(0, ROOT)


def bind(so):
    L = C.CDLL(so)
    L.zamd_zip_open.restype = C.c_void_p
    L.zamd_zip_open.argtypes = [C.c_char_p]
    L.zamd_zip_add.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_ulong, C.c_int, C.c_ulong, C.c_char_p]
    L.zamd_zip_add_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_ulong), C.c_int, C.POINTER(C.c_ulong),
                                     C.POINTER(C.c_char_p)]
    L.zamd_zip_close.argtypes = [C.c_void_p, C.c_char_p]
    L.zamd_unzip_open.restype = C.c_void_p
    L.zamd_unzip_open.argtypes = [C.c_char_p]
    L.zamd_unzip_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_ulong]
    L.zamd_unzip_read.restype = C.c_long
    L.zamd_unzip_read_batch.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_ulong), C.POINTER(C.c_long)]
    L.zamd_unzip_close.argtypes = [C.c_void_p]
    return L


def alternate(fns, reps):
    """{name: (median, min, max) seconds}: one warm-up call of each, then `reps` rounds that call each once, in turn"""
    for fn in fns.values():
        fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def main():
    args = sys.argv[1:]
    opt = {}
    for name in ("--out", "--reps"):
        if name in args:
            i = args.index(name)
            opt[name] = args[i + 1]
            del args[i: i + 2]
    level = int(args[0]) if args else 6
    reps = int(opt.get("--reps", 5))
    out_path = opt.get("--out", os.path.join(ROOT, "profiles", "r05_zip_table.txt"))
    import torch
    import zlib_amd
    from zlib_amd import gpu
    eng = zlib_amd.Engine(0)
    L = bind(os.path.join(ROOT, "zlib_amd", "libzamd_z.so"))
    dev = torch.device("cuda", 0)
    total = 16 << 20
    d_corpus = torch.empty(total, dtype=torch.uint8, device=dev)
    eng.corpus_fill_device(1, SEED, 0, total >> 16, d_corpus.data_ptr())
    torch.cuda.synchronize()
    corpus = d_corpus.cpu().numpy()
    lines = ["# ZIP archives of 16 MiB of log-text at level %d: the batch calls against the member-by-member loop (zamd_zip_add / zamd_unzip_read) of the same build" % level,
             "# median (min .. max) of %d timed calls behind a warm-up call of each kind, batch and loop alternating; host clock, archive files in a temporary directory" % reps]
    with tempfile.TemporaryDirectory() as tmp:
        for n, size in ((4096, 4096), (256, 65536)):
            base = corpus.ctypes.data
            names = (C.c_char_p * n)(*[b"log/%05d.txt" % k for k in range(n)])
            data = (C.c_void_p * n)(*[base + k * size for k in range(n)])
            lens = (C.c_ulong * n)(*[size] * n)
            dates = (C.c_ulong * n)(*[0x32F26459] * n)
            pb, pl = os.path.join(tmp, "batch.zip").encode(), os.path.join(tmp, "loop.zip").encode()

            def write_batch():
                z = L.zamd_zip_open(pb)
                assert L.zamd_zip_add_batch(z, n, names, data, lens, level, dates, None) == 0 and L.zamd_zip_close(z, None) == 0

            def write_loop():
                z = L.zamd_zip_open(pl)
                for k in range(n):
                    assert L.zamd_zip_add(z, names[k], data[k], size, level, dates[k], None) == 0
                assert L.zamd_zip_close(z, None) == 0
            tw = alternate({"batch": write_batch, "loop": write_loop}, reps)
            arc = open(pb, "rb").read()
            assert arc == open(pl, "rb").read(), "the two writers' archives differ"

            got = np.zeros(total, dtype=np.uint8)
            outs = (C.c_void_p * n)(*[got.ctypes.data + k * size for k in range(n)])
            res = (C.c_long * n)()

            def read_batch():
                u = L.zamd_unzip_open(pb)
                assert L.zamd_unzip_read_batch(u, None, n, outs, lens, res) == 0
                L.zamd_unzip_close(u)

            def read_loop():
                u = L.zamd_unzip_open(pb)
                for k in range(n):
                    assert L.zamd_unzip_read(u, k, outs[k], size) == size
                L.zamd_unzip_close(u)
            for name, fn in (("batch", read_batch), ("loop", read_loop)):  # (each checked on a cleared buffer, then timed in turn)
                got[:] = 0
                fn()
                assert got.tobytes() == corpus.tobytes(), "%s read differs from the corpus" % name
            tr = alternate({"batch": read_batch, "loop": read_loop}, reps)

            # the checksum call on the same items: host arrays, and device-resident
            offs = np.arange(n + 1, dtype=np.uint64) * size
            items = (gpu.CheckItem * n)()

            def check_host():
                eng.checksum_batch_host(corpus, offs, 3, items=items)
            d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
            d_items = torch.zeros((n, 2), dtype=torch.int32, device=dev)

            def check_dev():
                for _ in range(20):
                    eng.checksum_batch_device(d_corpus.data_ptr(), total, d_offs.data_ptr(), n, d_items.data_ptr(), 3)
            tc = alternate({"host": check_host, "device": check_dev}, reps)
            tc["device"] = tuple(t / 20 for t in tc["device"])
            assert items[n - 1].crc32 == zlib.crc32(corpus[total - size:].tobytes()) and items[0].adler32 == zlib.adler32(corpus[:size].tobytes())
            assert d_items.cpu().numpy().view(np.uint32).tolist() == [[it.adler32, it.crc32] for it in items]

            lines.append("## %d members of %d bytes: archive %d bytes (ratio %.3f)" % (n, size, len(arc), total / len(arc)))
            fmt = "%-34s %10.3f ms (%10.3f .. %10.3f) %9.2f us/member"
            for what, t in (("write", tw), ("read", tr)):
                for k in ("batch", "loop"):
                    lines.append(fmt % ("%s, %s" % (what, "one batch call" if k == "batch" else "member by member"), t[k][0] * 1e3, t[k][1] * 1e3, t[k][2] * 1e3, t[k][0] / n * 1e6))
                lines.append("%s: the loop takes %.2f times the batch call's time" % (what, t["loop"][0] / t["batch"][0]))
            for k, label in (("host", "checksums (Adler-32 + CRC-32), host arrays"), ("device", "checksums, device-resident, per call of 20")):
                lines.append("%-44s %10.3f ms (%10.3f .. %10.3f) %9.3f GiB/s" % (label, tc[k][0] * 1e3, tc[k][1] * 1e3, tc[k][2] * 1e3, total / tc[k][0] / 2 ** 30))
    lines.append("# checksums, device-resident: a timed sample is 20 blocking calls in a row, each with its plan round trip to the host; the figure is the sample / 20")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
