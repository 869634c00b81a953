"""Debug helper (GPU box): where a wave of sort4_kernel spends its cycles, from a -DZGPU_SORT_TIME build (scripts/build_variant.sh stime -DZGPU_SORT_TIME;
ZAMD_GPU_LIB=build/variants/stime.so python scripts/sort_time.py [waves per workgroup])."""
import ctypes
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import zlib_amd
from zlib_amd import gpu

waves = int(sys.argv[1]) if len(sys.argv) > 1 else 16  # sort4_kernel has 16 waves a workgroup
e = zlib_amd.Engine(0)
n = 16384
src = torch.empty(n * 65536, dtype=torch.uint8, device="cuda")
e.corpus_fill_device(0, 0x5EED5117, 0, n, src.data_ptr())
cap = e.L.zgpu_deflate_bound(n * 65536, 65536)
dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
f = e.L.zgpu_debug_sort_time
f.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
out = (ctypes.c_ulonglong * 9)()
e.deflate_device(src.data_ptr(), n * 65536, 6, dst.data_ptr(), cap, flags=gpu.F_FINAL)
f(out, 1)
e.deflate_device(src.data_ptr(), n * 65536, 6, dst.data_ptr(), cap, flags=gpu.F_FINAL)
torch.cuda.synchronize()
f(out, 0)
names = ["setup (zeroing)", "pass A (rest)", "pass A: token wait", "pass B + Adler", "pass C0", "heads out", "pass C1 + V", "pass A: atomics"]
tot = sum(int(out[i]) for i in range(8))
for i, nm in enumerate(names):
    print("%-20s %9.0f cycles per wave and chunk  %5.1f%%" % (nm, int(out[i]) / n / waves, 100.0 * int(out[i]) / tot))
print("total %.0f cycles per wave and chunk (%d waves a workgroup)" % (tot / n / waves, waves))
print("most workgroups on one CU at a time: %d" % int(out[8]))
