"""Debug helper (GPU box): per-phase clock of the parallel parse from a -DZGPU_P2_TIME build (ZAMD_GPU_LIB=build/variants/p2time.so).
Without arguments: parse2_kernel (ZGPU_LZ=sorted).  `p2_time.py fused [level]`: the tail behind a chunk's walkers in walk_kernel<1> (the default path), and the
workgroup's time in front of it (staging, walkers, barrier) -- together a chunk's residency in its workgroup slot.  That tail has two forms (zgpu_lz_walk.hip): the
stages of the whole-chunk form (zgpu_lz_tail.h) and of the windowed form are printed apart, each per chunk that went through it, with the share of the chunks
that took each and of those whose whole-chunk threading did not hold.  ZGPU_WALK_TAIL_CAP=0 sends every chunk through the windowed form."""
import ctypes
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import zlib_amd
from zlib_amd import gpu

fused = len(sys.argv) > 1 and sys.argv[1] == "fused"
lvl = int(sys.argv[2]) if len(sys.argv) > 2 else 6
e = zlib_amd.Engine(0)
n = 16384
src = torch.empty(n * 65536, dtype=torch.uint8, device="cuda")
e.corpus_fill_device(0, 0x5EED5117, 0, n, src.data_ptr())
cap = e.L.zgpu_deflate_bound(n * 65536, 65536)
dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
f = e.L.zgpu_debug_p2_fused_time if fused else e.L.zgpu_debug_p2_time
f.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
out = (ctypes.c_ulonglong * 8)()
g, tl = None, (ctypes.c_ulonglong * 12)()
if fused and hasattr(e.L, "zgpu_debug_p2_tail_time"):  # (a build with the whole-chunk tail)
    g = e.L.zgpu_debug_p2_tail_time
    g.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
e.deflate_device(src.data_ptr(), n * 65536, lvl, dst.data_ptr(), cap, flags=gpu.F_FINAL)
f(out, 1)
if g:
    g(tl, 1)
e.deflate_device(src.data_ptr(), n * 65536, lvl, dst.data_ptr(), cap, flags=gpu.F_FINAL)
torch.cuda.synchronize()
f(out, 0)
names = ["1 has", "A1 successors", "A2 path", "B matches", "C indices", "D tokens", "3 cuts"]
tail_names = ["1 has", "2 numbers", "3 successors", "4 blocks", "5 thread", "6 meet", "B matches", "C indices", "D tokens", "3 cuts"]


def show(title, names, t, chunks):
    tot = sum(t)
    print("%s: %d chunks" % (title, chunks))
    for nm, v in zip(names, t):
        print("  %-14s %8.1f us/chunk  %5.1f%%" % (nm, v / max(chunks, 1) / 100.0, 100.0 * v / max(tot, 1)))  # wall_clock64: 100 MHz
    print("  total %.1f us/chunk" % (tot / max(chunks, 1) / 100.0))
    return tot


if not fused:
    show("parse2_kernel", names, [int(out[i]) for i in range(7)], n)
else:
    whole, failed, t_whole = 0, 0, 0
    if g:
        g(tl, 0)
        whole, failed = int(tl[10]), int(tl[11])
        t_whole = show("whole-chunk tail", tail_names, [int(tl[i]) for i in range(10)], whole)
    windowed = n - whole + failed
    t_win = show("windowed tail", names, [int(out[i]) for i in range(7)], windowed)
    print("chunks: %d whole-chunk (%d of them fell back: the threading did not hold), %d windowed for their games" % (whole, failed, n - whole))
    front, tot = int(out[7]), t_whole + t_win
    print("the tail, both forms: %.1f us/chunk" % (tot / n / 100.0))
    print("in front of the tail (staging, walkers, barrier) %.1f us/chunk; the tail is %.1f%% of a chunk's residency" % (front / n / 100.0, 100.0 * tot / (tot + front)))
