"""Debug helper (GPU box): per-phase clock of the parallel parse from a -DZGPU_P2_TIME build (ZAMD_GPU_LIB=build/variants/p2time.so).
Without arguments: parse2_kernel (ZGPU_LZ=sorted).  `p2_time.py fused [level]`: the tail behind a chunk's walkers in walk_kernel<1> (the default path), and the
workgroup's time in front of it (staging, walkers, barrier) -- together a chunk's residency in its workgroup slot."""
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
e.deflate_device(src.data_ptr(), n * 65536, lvl, dst.data_ptr(), cap, flags=gpu.F_FINAL)
f(out, 1)
e.deflate_device(src.data_ptr(), n * 65536, lvl, dst.data_ptr(), cap, flags=gpu.F_FINAL)
torch.cuda.synchronize()
f(out, 0)
names = ["1 has", "A1 successors", "A2 path", "B matches", "C indices", "D tokens", "3 cuts"]
tot = sum(int(out[i]) for i in range(7))
for i, nm in enumerate(names):
    print("%-14s %8.1f us/chunk  %5.1f%%" % (nm, int(out[i]) / n / 100.0, 100.0 * int(out[i]) / tot))  # wall_clock64: 100 MHz
print("total %.1f us/chunk" % (tot / n / 100.0))
if fused:
    front = int(out[7])
    print("in front of the tail (staging, walkers, barrier) %.1f us/chunk; the tail is %.1f%% of a chunk's residency" % (front / n / 100.0, 100.0 * tot / (tot + front)))
