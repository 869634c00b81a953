"""Debug helper (GPU box): how full walk_kernel<1>'s per-window game logs get, from a -DZGPU_WALK_STATS build (ZAMD_GPU_LIB=build/variants/wstats.so).
Prints the games logged per chunk, the fullest window's log (capacity 8192) and how many chunks took which form of the tail (zgpu_lz_walk.hip) for the corpus,
for each input of tests/test_gpu_walk_log.py and for the inputs of tests/test_gpu_walk_tail.py that are built for one form or the other."""
import ctypes
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zlib_amd  # noqa: E402
from zlib_amd import gpu  # noqa: E402
from oracle import corpus_py as CP  # noqa: E402
import test_gpu_walk_log as T  # noqa: E402

e = zlib_amd.Engine(0)
f = e.L.zgpu_debug_walk_log_stats
f.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
out = (ctypes.c_ulonglong * 6)()


def measure(label, run, nchunks):
    f(out, 1)
    run()
    f(out, 0)
    print("%-28s games per chunk %8.0f   fullest log %5d of 8192 (%.0f%%)   tail: %d whole-chunk, %d windowed (over capacity), %d windowed (threading did not hold); %d with two games at one position (must be 0)"
          % (label, out[0] / nchunks, out[1], 100.0 * out[1] / 8192, out[2], out[3], out[4], out[5]))


for kind, name in ((CP.KIND_SILESIA, "silesia-mix"), (CP.KIND_LOGTEXT, "log-text")):
    data = CP.chunks(kind, 0, 256)
    for lvl in (4, 6, 9):
        measure("%s L%d, 256 chunks" % (name, lvl), lambda: e.deflate_host(data, lvl, flags=gpu.F_FINAL), 256)
for cfg, (lvl, strategy, tune) in T.CONFIGS.items():
    for name in ("len-65536", "straddle", "zeros", "period2", "period5", "run-then-rand", "debruijn", "rand"):
        e.set_tuning(tune)
        measure("%s %s" % (cfg, name), lambda: e.deflate_segments_host([T.INPUTS[name]], lvl, flags=gpu.F_FINAL, strategy=strategy), 1)
        e.set_tuning(None)
import test_gpu_walk_tail as TT  # noqa: E402
for cfg, (lvl, strategy) in TT.CONFIGS.items():
    for name in ("no-meeting", "debruijn-empty", "zeros-65536", "text-65536", "mix-65536", "count-1-1023", "count-1024-1025"):
        measure("%s %s" % (cfg, name), lambda: e.deflate_segments_host([TT.inputs()[0][name]], lvl, flags=gpu.F_FINAL, strategy=strategy), 1)
e.close()
