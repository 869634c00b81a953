"""Stream-ordered batch compress of items of any length: zgpu_deflate_streams_enqueue + one synchronize (e) against the blocking zgpu_deflate_streams_device of
the same build over the same items (b), in the same run.  Level 6, zlib wrapper, the synthetic silesia-mix corpus (zgpu_corpus_fill_device kind 0),
device-resident; the three item sets of scripts/streams_rate.py -- 256 items of 1 MiB, 4,096 items of 96 KiB, 16 items of 64 MiB -- and 200 calls of 16 items of
256 KiB back to back on one stream (the enqueue calls with one synchronize behind the last, the blocking calls one after the other).  Every figure is the
median (min .. max) of `reps` timed runs behind a warm-up of each kind, the kinds alternating; a host clock around calls that have returned AND been waited
for.  The streams and records of (e) are compared with those of (b) before anything is timed.
Usage: python scripts/streams_enqueue_rate.py [level] [--out PATH] [--reps N] [--sets 0,1,2,3] [--batch-tiles T]
       (default: level 6, profiles/r11_streams_enqueue_table.txt, 3, all sets, 0 = the default round)"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED5117  # the corpus seed of the other rate scripts
sys.path.insert(0, ROOT)
SETS = ((256, 1 << 20, 1), (4096, 96 << 10, 1), (16, 64 << 20, 1), (16, 256 << 10, 200))  # items, bytes an item, calls back to back
REC = np.dtype([("code", "<i4"), ("data_type", "<u4"), ("out_lo", "<u8"), ("out_bytes", "<u8"), ("in_bytes", "<u4"), ("adler32", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])


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
    for name in ("--out", "--reps", "--sets", "--batch-tiles"):
        if name in args:
            i = args.index(name)
            opt[name] = args[i + 1]
            del args[i: i + 2]
    level = int(args[0]) if args else 6
    reps = int(opt.get("--reps", 3))
    sets = [SETS[int(x)] for x in opt.get("--sets", "0,1,2,3").split(",")]
    batch_tiles = int(opt.get("--batch-tiles", 0))
    out_path = opt.get("--out", os.path.join(ROOT, "profiles", "r11_streams_enqueue_table.txt"))
    import torch
    import zlib_amd
    from zlib_amd import gpu
    eng = zlib_amd.Engine(0)
    dev = torch.device("cuda", 0)
    flags = gpu.F_FINAL | gpu.F_ZLIB_WRAP
    lines = ["# stream-ordered batch compress of items of any length at level %d, zlib wrapper, silesia-mix, device-resident: (e) zgpu_deflate_streams_enqueue + one" % level,
             "# synchronize, (b) the blocking zgpu_deflate_streams_device over the same items.  median (min .. max) of %d timed runs behind a warm-up of each kind, the kinds" % reps,
             "# alternating; host clock; GiB/s of input.  batch_tiles = %d (0: the default round of 2,048 tiles)" % batch_tiles]
    for n, size, calls in sets:
        total = n * size
        d_in = torch.empty(total, dtype=torch.uint8, device=dev)
        eng.corpus_fill_device(0, SEED, 0, total >> 16, d_in.data_ptr())
        offs = np.arange(n + 1, dtype=np.uint64) * size
        oo, rooms = eng.deflate_streams_layout(offs, flags)
        d_io = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_oo = torch.from_numpy(oo.view(np.int64)).to(dev)
        d_out = torch.empty(rooms, dtype=torch.uint8, device=dev)
        d_out_b = torch.empty(rooms, dtype=torch.uint8, device=dev)
        d_items = torch.zeros(n * REC.itemsize, dtype=torch.uint8, device=dev)
        d_items_b = torch.zeros(n * REC.itemsize, dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(C.sizeof(gpu.DeflateBatchSummary), dtype=torch.uint8, device=dev)
        ws_bytes = eng.deflate_streams_workspace_bytes(n, total, batch_tiles)
        d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        assert d_ws.data_ptr() % 256 == 0
        torch.cuda.synchronize()
        state = {}

        def enqueue():
            for _ in range(calls):
                eng.deflate_streams_enqueue(d_in.data_ptr(), total, d_io.data_ptr(), n, level, d_out.data_ptr(), rooms, d_oo.data_ptr(), d_items.data_ptr(), d_ws.data_ptr(), ws_bytes,
                                            flags=flags, batch_tiles=batch_tiles, d_summary=d_sum.data_ptr())
            torch.cuda.synchronize()

        def blocking():
            for _ in range(calls):
                state["b"] = eng.deflate_streams_device(d_in.data_ptr(), total, d_io.data_ptr(), n, level, d_out_b.data_ptr(), rooms, d_oo.data_ptr(), d_items_b.data_ptr(), flags=flags)

        # the same bytes and records, before anything is timed
        enqueue()
        blocking()
        torch.cuda.synchronize()
        ra = np.frombuffer(d_items.cpu().numpy().tobytes(), dtype=REC)
        rb = np.frombuffer(d_items_b.cpu().numpy().tobytes(), dtype=REC)
        assert (ra == rb).all() and (ra["code"] == 0).all(), "the records differ from the blocking call's"
        for k in sorted({0, 1, n // 2, n - 1}):
            lo, nb = int(ra["out_lo"][k]), int(ra["out_bytes"][k])
            assert torch.equal(d_out[lo: lo + nb], d_out_b[lo: lo + nb]), "item %d: the stream differs from the blocking call's" % k
        summary = np.frombuffer(d_sum.cpu().numpy().tobytes(), dtype=np.uint64)
        assert int(summary[0]) == 0 and int(summary[3]) == state["b"].out_bytes
        t = alternate({"e": enqueue, "b": blocking}, reps)
        lines.append("## %d call%s of %d items of %d bytes (%d MiB a call, %d tiles, laid out for %d): streams %d bytes (ratio %.3f); workspace %d bytes (%.1f MiB)"
                     % (calls, "" if calls == 1 else "s back to back", n, size, total >> 20, state["b"].nchunks, total // 32512 + n, state["b"].out_bytes, total / state["b"].out_bytes,
                        ws_bytes, ws_bytes / 2 ** 20))
        fmt = "%-48s %10.3f ms (%10.3f .. %10.3f) %8.3f GiB/s %10.2f us/item"
        for k, name in (("e", "(e) enqueue + one synchronize"), ("b", "(b) blocking zgpu_deflate_streams_device")):
            lines.append(fmt % (name, t[k][0] * 1e3, t[k][1] * 1e3, t[k][2] * 1e3, calls * total / t[k][0] / 2 ** 30, t[k][0] / (n * calls) * 1e6))
        spread = max((t[k][2] - t[k][1]) / t[k][0] for k in ("e", "b"))
        ratio = t["e"][0] / t["b"][0]
        lines.append("(e) takes %.3f times the time of (b); run-to-run spread (max - min over the median, the larger of the two) %.3f%s"
                     % (ratio, spread, "; (e) is SLOWER than (b) by more than the spread" if ratio > 1 + spread else ""))
        # where the blocking call's time goes, for comparison: the engine's stage times of one more call
        eng.profile(True)
        eng.deflate_streams_device(d_in.data_ptr(), total, d_io.data_ptr(), n, level, d_out_b.data_ptr(), rooms, d_oo.data_ptr(), d_items_b.data_ptr(), flags=flags)
        pr = eng.profile_read()
        eng.profile(False)
        lines.append("(b), stages of one call, ms (launches): " + ", ".join("%s %.2f (%d)" % (k, v[0], v[1]) for k, v in pr.items() if v[1]))
        del d_in, d_out, d_out_b, d_ws
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
