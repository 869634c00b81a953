"""BGZF (blocked gzip): all blocks of a file in one call -- zgpu_bgzf_deflate_*, zgpu_bgzf_inflate_* -- against the same file decoded member by member
through the host library's inflate() with windowBits 31.  The file is the synthetic Silesia-mix (zgpu_corpus_fill_device) cut every 65 280 bytes.
Device: input and output resident in HBM; host: from and to host buffers.  The block finder (zgpu_bgzf_index_device) is timed alone as well: its
share of the device-resident decode is stated.  Every figure is the median of `reps` calls behind a warm-up call, a host clock around calls that end
in a device synchronise; rates count decoded bytes.
The member-by-member loop runs in a child process of its own.
Usage: python scripts/bgzf_rate.py [MiB of corpus] [level] [--zlib-so PATH] [--out PATH] [--big-mib N]
  --zlib-so  the libzamd_z.so the member-by-member loop runs through (default: this tree's; give a build of the parent commit to measure there)
  --out      where the table goes (default: profiles/r06_bgzf_table.txt)
  --big-mib  size of a second, device-resident file on which the finder and the decode are timed again (default 1024; 0: none)"""
import ctypes as C
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED5117  # the corpus seed of the other rate scripts
sys.path.insert(0, ROOT)


def timed(fn, reps=5, window=0.25):
    """median, min, max seconds per call: a warm-up call, then `reps` windows of as many calls as fill `window` seconds (short calls are looped)"""
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    inner = max(1, min(500, int(window / max(time.perf_counter() - t0, 1e-6)) + 1))
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    return statistics.median(ts), min(ts), max(ts)


class ZStream(C.Structure):
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_uint), ("total_in", C.c_ulong), ("next_out", C.c_void_p), ("avail_out", C.c_uint),
                ("total_out", C.c_ulong), ("msg", C.c_char_p), ("state", C.c_void_p), ("zalloc", C.c_void_p), ("zfree", C.c_void_p),
                ("opaque", C.c_void_p), ("data_type", C.c_int), ("adler", C.c_ulong), ("reserved", C.c_ulong)]


def member_loop(L, f, starts, out):
    """inflateInit2(31) once, then inflate(Z_FINISH) + inflateReset per member, each fed exactly its own bytes; returns the decoded size"""
    s = ZStream()
    assert L.inflateInit2_(C.byref(s), 31, b"1.2.3", C.sizeof(ZStream)) == 0
    base_in, base_out, at = f.ctypes.data, out.ctypes.data, 0
    for k in range(len(starts) - 1):
        s.next_in, s.avail_in = base_in + starts[k], starts[k + 1] - starts[k]
        s.next_out, s.avail_out = base_out + at, 65536
        rc = L.inflate(C.byref(s), 4)
        assert rc == 1, (k, rc)
        at += 65536 - s.avail_out
        L.inflateReset(C.byref(s))
    L.inflateEnd(C.byref(s))
    return at


def members_only(path, so, out_bytes):
    """a process of its own (only `so` and the engine next to it are loaded): one warm-up pass and two timed ones over the file at `path`;
    prints the times, the decoded size and its CRC-32"""
    f = np.fromfile(path, dtype=np.uint8)
    starts, pos = [], 0
    while pos < f.size:  # (this script's own files: BSIZE sits at byte 16 of every block)
        starts.append(pos)
        pos += struct.unpack_from("<H", f, pos + 16)[0] + 1
    starts.append(pos)
    L = C.CDLL(so)
    P = C.POINTER(ZStream)
    L.inflateInit2_.argtypes = [P, C.c_int, C.c_char_p, C.c_int]
    L.inflate.argtypes = [P, C.c_int]
    L.inflateReset.argtypes = [P]
    L.inflateEnd.argtypes = [P]
    out = np.zeros(out_bytes, dtype=np.uint8)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        n = member_loop(L, f, starts, out)  # (inflate() returns when the member's bytes are in `out`)
        ts.append(time.perf_counter() - t0)
    ts = sorted(ts[1:])
    print("MEMBERS %.6f %.6f %.6f %d %d" % (statistics.median(ts), ts[0], ts[-1], n, zlib.crc32(out.tobytes())))


def main():
    args = sys.argv[1:]
    opt = {}
    for name in ("--zlib-so", "--out", "--members-only", "--out-bytes", "--big-mib"):
        if name in args:
            i = args.index(name)
            opt[name] = args[i + 1]
            del args[i: i + 2]
    mib = int(args[0]) if args else 64
    level = int(args[1]) if len(args) > 1 else 6
    zlib_so = opt.get("--zlib-so", os.path.join(ROOT, "zlib_amd", "libzamd_z.so"))
    out_path = opt.get("--out", os.path.join(ROOT, "profiles", "r06_bgzf_table.txt"))
    if "--members-only" in opt:
        return members_only(opt["--members-only"], zlib_so, int(opt["--out-bytes"]))
    import torch
    import zlib_amd
    from zlib_amd import gpu
    eng = zlib_amd.Engine(0)
    dev = torch.device("cuda", 0)
    total = mib << 20
    d_corpus = torch.empty(total, dtype=torch.uint8, device=dev)
    eng.corpus_fill_device(0, SEED, 0, total >> 16, d_corpus.data_ptr())
    torch.cuda.synchronize()
    h_corpus = d_corpus.cpu().numpy()
    nblocks = (total + gpu.BGZF_BLOCK - 1) // gpu.BGZF_BLOCK
    cap = int(eng.L.zgpu_bgzf_bound(total, 0))
    rows = []
    gib = lambda t: total / t / 2 ** 30  # noqa: E731

    # ---- encode ----
    d_f = torch.empty(cap, dtype=torch.uint8, device=dev)
    res = gpu.DeflateResult()

    def enc_dev():
        eng._check(eng.L.zgpu_bgzf_deflate_device(eng.h, d_corpus.data_ptr(), total, level, 0, 0, d_f.data_ptr(), cap, None, C.byref(res), None))
    t = timed(enc_dev)
    fbytes = int(res.out_bytes)
    rows.append(("encode, device-resident", t))
    h_f = np.empty(cap, dtype=np.uint8)

    def enc_host():
        eng._check(eng.L.zgpu_bgzf_deflate_host(eng.h, h_corpus.ctypes.data, total, level, 0, 0, h_f.ctypes.data, cap, None, C.byref(res)))
    rows.append(("encode, host buffers", timed(enc_host, reps=3)))
    assert int(res.out_bytes) == fbytes and h_f[:fbytes].tobytes() == d_f[:fbytes].cpu().numpy().tobytes()

    # ---- the finder alone, then the whole decode ----
    d_io = torch.empty(nblocks + 2, dtype=torch.int64, device=dev)
    d_oo = torch.empty(nblocks + 2, dtype=torch.int64, device=dev)

    def find():
        rc, n, ub, eof = eng.bgzf_index_device(d_f.data_ptr(), fbytes, d_io.data_ptr(), d_oo.data_ptr(), nblocks + 1)
        assert (rc, n, ub, eof) == (0, nblocks + 1, total, 1), (rc, n, ub, eof)
    t_find = timed(find)
    d_out = torch.empty(total, dtype=torch.uint8, device=dev)
    ires = gpu.InflateResult()

    def dec_dev():
        rc = eng.L.zgpu_bgzf_inflate_device(eng.h, d_f.data_ptr(), fbytes, d_out.data_ptr(), total, None, C.byref(ires), None)
        assert rc == 0 and ires.out_bytes == total
    t_dd = timed(dec_dev)
    assert torch.equal(d_out, d_corpus), "device decode differs from the corpus"
    h_out = np.empty(total, dtype=np.uint8)

    def dec_host():
        rc = eng.L.zgpu_bgzf_inflate_host(eng.h, h_f.ctypes.data, fbytes, h_out.ctypes.data, total, None, C.byref(ires))
        assert rc == 0 and ires.out_bytes == total
    t_dh = timed(dec_host, reps=3)
    assert h_out.tobytes() == h_corpus.tobytes(), "host decode differs from the corpus"
    rows += [("block finder alone, device-resident", t_find), ("decode, device-resident (finder included)", t_dd), ("decode, host buffers (finder included)", t_dh)]

    # ---- member by member through inflate(), in a process of its own ----
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "file.bgzf")
        h_f[:fbytes].tofile(path)
        line = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--members-only", path, "--zlib-so", zlib_so, "--out-bytes", str(total)], timeout=600).decode()
    w = [ln for ln in line.splitlines() if ln.startswith("MEMBERS ")][0].split()
    assert int(w[4]) == total and int(w[5]) == zlib.crc32(h_corpus.tobytes()), "the member-by-member decode differs from the corpus"
    t_loop = (float(w[1]), float(w[2]), float(w[3]))
    rows.append(("inflate() windowBits 31, member by member", t_loop))

    # ---- the finder on a large file: its one-workgroup scans walk a count per 4096 bytes of file ----
    big = int(opt.get("--big-mib", 1024))
    big_line = None
    if big:
        del d_out, d_f
        btotal = big << 20
        d_big = torch.empty(btotal, dtype=torch.uint8, device=dev)
        eng.corpus_fill_device(0, SEED, 0, btotal >> 16, d_big.data_ptr())
        bcap = int(eng.L.zgpu_bgzf_bound(btotal, 0))
        d_bf = torch.empty(bcap, dtype=torch.uint8, device=dev)
        eng._check(eng.L.zgpu_bgzf_deflate_device(eng.h, d_big.data_ptr(), btotal, level, 0, 0, d_bf.data_ptr(), bcap, None, C.byref(res), None))
        bbytes, bn = int(res.out_bytes), (btotal + gpu.BGZF_BLOCK - 1) // gpu.BGZF_BLOCK + 1
        d_bio = torch.empty(bn + 1, dtype=torch.int64, device=dev)
        d_boo = torch.empty(bn + 1, dtype=torch.int64, device=dev)

        def find_big():
            rc, n, ub, eof = eng.bgzf_index_device(d_bf.data_ptr(), bbytes, d_bio.data_ptr(), d_boo.data_ptr(), bn)
            assert (rc, n, ub, eof) == (0, bn, btotal, 1), (rc, n, ub, eof)
        tb_find = timed(find_big)
        d_bout = torch.empty(btotal, dtype=torch.uint8, device=dev)

        def dec_big():
            rc = eng.L.zgpu_bgzf_inflate_device(eng.h, d_bf.data_ptr(), bbytes, d_bout.data_ptr(), btotal, None, C.byref(ires), None)
            assert rc == 0 and ires.out_bytes == btotal
        tb_dec = timed(dec_big)
        assert torch.equal(d_bout, d_big), "device decode of the large file differs from the corpus"
        big_line = "%d MiB (%d blocks, %d bytes of file): block finder alone %.3f ms (%.3f .. %.3f), decode device-resident %.3f ms (%.3f .. %.3f) = %.2f GiB/s, finder's share %.1f %%" % (
            big, bn, bbytes, tb_find[0] * 1e3, tb_find[1] * 1e3, tb_find[2] * 1e3, tb_dec[0] * 1e3, tb_dec[1] * 1e3, tb_dec[2] * 1e3, btotal / tb_dec[0] / 2 ** 30, 100 * tb_find[0] / tb_dec[0])

    lines = ["# BGZF: %d MiB of Silesia-mix at level %d as %d blocks of 65280 bytes + the end block, %d bytes (ratio %.3f)" % (mib, level, nblocks, fbytes, total / fbytes),
             "# median (min .. max) per call over timed windows of at least 0.25 s (short calls looped) behind a warm-up call; GiB/s of decoded bytes",
             "# the member-by-member loop ran through %s" % os.path.relpath(zlib_so, ROOT)]
    for name, (med, lo, hi) in rows:
        lines.append("%-44s %9.3f ms (%9.3f .. %9.3f) %8.3f GiB/s %8.2f us/block" % (name, med * 1e3, lo * 1e3, hi * 1e3, gib(med), med / (nblocks + 1) * 1e6))
    lines.append("finder's share of the device-resident decode: %.1f %%; of the decode from host buffers: %.1f %%" % (100 * t_find[0] / t_dd[0], 100 * t_find[0] / t_dh[0]))
    lines.append("decode from host buffers against the member-by-member loop: %.1f times" % (t_loop[0] / t_dh[0]))
    if big_line:
        lines.append(big_line)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
