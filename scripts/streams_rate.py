"""Batch compress of items over 64 KiB: one zgpu_deflate_streams_* call (a) against the same build's one-by-one loop over the same items -- one continuous
stream per call, zgpu_deflate_device / zgpu_deflate_host with ZGPU_F_CONTINUOUS, which is what served such items before -- (b), and against ONE continuous
stream of the same total size (c), the rate the same kernels reach when they are full.  Level 6, zlib wrapper, the synthetic silesia-mix corpus
(zgpu_corpus_fill_device kind 0); three item sets: 256 items of 1 MiB, 4,096 items of 96 KiB, 16 items of 64 MiB; each device-resident and from host buffers.
Every figure is the median (min .. max) of `reps` timed calls behind a warm-up call of each kind, the kinds alternating; a host clock around calls that
return when the result is known.  The streams of (a) are compared with those of (b) before anything is timed.
Usage: python scripts/streams_rate.py [level] [--out PATH] [--reps N] [--sets 0,1,2]     (default: level 6, profiles/r10_streams_table.txt, 3, all sets)"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED5117  # the corpus seed of the other rate scripts
sys.path.insert(0, ROOT)
SETS = ((256, 1 << 20), (4096, 96 << 10), (16, 64 << 20))


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
    for name in ("--out", "--reps", "--sets"):
        if name in args:
            i = args.index(name)
            opt[name] = args[i + 1]
            del args[i: i + 2]
    level = int(args[0]) if args else 6
    reps = int(opt.get("--reps", 3))
    sets = [SETS[int(x)] for x in opt.get("--sets", "0,1,2").split(",")]
    out_path = opt.get("--out", os.path.join(ROOT, "profiles", "r10_streams_table.txt"))
    import torch
    import zlib_amd
    from zlib_amd import gpu
    eng = zlib_amd.Engine(0)
    L = eng.L
    dev = torch.device("cuda", 0)
    flags = gpu.F_FINAL | gpu.F_ZLIB_WRAP
    one_flags = flags | gpu.F_CONTINUOUS
    lines = ["# batch compress of items over 64 KiB at level %d, zlib wrapper, silesia-mix: (a) one zgpu_deflate_streams_* call, (b) the same build's loop of one continuous" % level,
             "# stream per call over the same items, (c) ONE continuous stream of the same total size.  median (min .. max) of %d timed calls behind a warm-up of each kind," % reps,
             "# the kinds alternating; host clock around blocking calls; GiB/s of input"]
    for n, size in sets:
        total = n * size
        d_in = torch.empty(total, dtype=torch.uint8, device=dev)
        eng.corpus_fill_device(0, SEED, 0, total >> 16, d_in.data_ptr())
        torch.cuda.synchronize()
        offs = np.arange(n + 1, dtype=np.uint64) * size
        oo, rooms = eng.deflate_streams_layout(offs, flags)
        d_io = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_oo = torch.from_numpy(oo.view(np.int64)).to(dev)
        d_out = torch.empty(rooms, dtype=torch.uint8, device=dev)
        d_items = torch.zeros(n * C.sizeof(gpu.DeflateBatchItem), dtype=torch.uint8, device=dev)
        one_cap = int(L.zgpu_deflate_cont_bound(size)) + 32
        d_one = torch.empty(one_cap, dtype=torch.uint8, device=dev)
        all_cap = int(L.zgpu_deflate_cont_bound(total)) + 32
        d_all = torch.empty(all_cap, dtype=torch.uint8, device=dev)
        state = {}

        def dev_streams():
            state["a"] = eng.deflate_streams_device(d_in.data_ptr(), total, d_io.data_ptr(), n, level, d_out.data_ptr(), rooms, d_oo.data_ptr(), d_items.data_ptr(), flags=flags)

        def dev_loop():
            nb = 0
            for k in range(n):
                nb += eng.deflate_device(d_in.data_ptr() + k * size, size, level, d_one.data_ptr(), one_cap, flags=one_flags).out_bytes
            state["b"] = nb

        def dev_one():
            state["c"] = eng.deflate_device(d_in.data_ptr(), total, level, d_all.data_ptr(), all_cap, flags=one_flags).out_bytes

        # the same bytes: every item's stream of (a) against the loop's, before anything is timed
        dev_streams()
        recs = np.frombuffer(d_items.cpu().numpy().tobytes(), dtype=np.dtype([("code", "<i4"), ("data_type", "<u4"), ("out_lo", "<u8"), ("out_bytes", "<u8"), ("in_bytes", "<u4"),
                                                                                ("adler32", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")]))
        assert state["a"].reserved == 0 and (recs["code"] == 0).all()
        for k in sorted({0, 1, n // 2, n - 1}):
            r = eng.deflate_device(d_in.data_ptr() + k * size, size, level, d_one.data_ptr(), one_cap, flags=one_flags)
            torch.cuda.synchronize()
            lo = int(recs["out_lo"][k])
            assert int(recs["out_bytes"][k]) == r.out_bytes and torch.equal(d_out[lo: lo + r.out_bytes], d_one[: r.out_bytes]), "item %d: the batch's stream differs from the one-call stream" % k
        td = alternate({"a": dev_streams, "b": dev_loop, "c": dev_one}, reps)
        assert state["a"].out_bytes == state["b"]

        # host buffers
        h_in = d_in.cpu().numpy()
        h_out = np.empty(rooms, dtype=np.uint8)
        h_oo = np.zeros(n + 1, dtype=np.uint64)
        h_items = (gpu.DeflateBatchItem * n)()
        p = gpu._Params(level, 0, flags, gpu.LZ_AUTO, 0, 0)
        res = gpu.DeflateResult()

        def host_streams():
            eng._check(L.zgpu_deflate_streams_host(eng.h, h_in.ctypes.data, offs.ctypes.data, n, C.byref(p), h_out.ctypes.data, rooms, h_oo.ctypes.data, h_items, C.byref(res)))

        def host_loop():
            for k in range(n):
                eng.deflate_host(h_in[k * size: (k + 1) * size], level, flags=one_flags)

        def host_one():
            eng.deflate_host(h_in, level, flags=one_flags)
        th = alternate({"a": host_streams, "b": host_loop, "c": host_one}, reps)
        assert int(h_oo[n]) == state["a"].out_bytes

        lines.append("## %d items of %d bytes (%d MiB in all, %d tiles): streams %d bytes (ratio %.3f), one stream %d bytes" % (n, size, total >> 20, state["a"].nchunks, state["a"].out_bytes,
                                                                                                                              total / state["a"].out_bytes, state["c"]))
        fmt = "%-58s %10.3f ms (%10.3f .. %10.3f) %8.3f GiB/s %10.2f us/item"
        names = {"a": "(a) one streams call", "b": "(b) one continuous stream per item, in a loop", "c": "(c) ONE continuous stream of all the bytes"}
        for where, t in (("device-resident", td), ("host buffers", th)):
            for k in ("a", "b", "c"):
                lines.append(fmt % ("%s, %s" % (where, names[k]), t[k][0] * 1e3, t[k][1] * 1e3, t[k][2] * 1e3, total / t[k][0] / 2 ** 30, t[k][0] / n * 1e6))
            lines.append("%s: (b) takes %.2f times the time of (a); (a) takes %.2f times the time of (c)" % (where, t["b"][0] / t["a"][0], t["a"][0] / t["c"][0]))
        # where the time of (a) goes: the engine's stage times of one more call
        eng.profile(True)
        dev_streams()
        pr = eng.profile_read()
        eng.profile(False)
        lines.append("device-resident (a), stages of one call, ms (launches): " + ", ".join("%s %.2f (%d)" % (k, v[0], v[1]) for k, v in pr.items() if v[1]))
        del d_in, d_out, d_one, d_all, h_in, h_out
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
