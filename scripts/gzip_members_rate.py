"""Multi-member gzip: all members of a file in one call -- zgpu_gzip_inflate_host / _device -- against the same file decoded member by member through
the host library's inflate() with windowBits 31, the same build in the same run.  The file is the synthetic log-text corpus
(zgpu_corpus_fill_device kind 1) cut into members of 4 KiB and of 64 KiB, each a gzip member of the wrapped segment path (ZGPU_F_FINAL |
ZGPU_F_GZIP_WRAP).  A second file per size has one false candidate planted -- a stored member whose payload holds a gzip signature, with a
plausible word in front of it -- so that the call takes its second decode; the table says what that costs.
Device: input and output resident in HBM; host: from and to host buffers.  Every figure is the median of 5 timed windows behind a warm-up call, a host
clock around calls that end in a device synchronise; rates count decoded bytes.  The member-by-member loop runs in a child process of its own.
Usage: python scripts/gzip_members_rate.py [MiB of corpus] [level] [--out PATH]
  --out  where the table goes (default: profiles/r06_gzip_members_table.txt)"""
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


def members_only(path, so, out_bytes):
    """a process of its own: inflateInit2(31) once, then inflate(Z_FINISH) + inflateReset per member, the way a reader without a member table goes
    (the next member begins where the last one's input ended).  One warm-up pass and five timed ones; prints the times, the decoded size, its CRC-32
    and the number of members"""
    f = np.fromfile(path, dtype=np.uint8)
    L = C.CDLL(so)
    P = C.POINTER(ZStream)
    L.inflateInit2_.argtypes = [P, C.c_int, C.c_char_p, C.c_int]
    L.inflate.argtypes = [P, C.c_int]
    L.inflateReset.argtypes = [P]
    L.inflateEnd.argtypes = [P]
    out = np.zeros(out_bytes + 1, dtype=np.uint8)
    ts, n, members = [], 0, 0
    for _ in range(6):
        t0 = time.perf_counter()
        s = ZStream()
        assert L.inflateInit2_(C.byref(s), 31, b"1.2.3", C.sizeof(ZStream)) == 0
        pos, n, members = 0, 0, 0
        while pos < f.size:
            take = min(f.size - pos, 1 << 20)
            s.next_in, s.avail_in = f.ctypes.data + pos, take
            s.next_out, s.avail_out = out.ctypes.data + n, min(out_bytes + 1 - n, 1 << 30)
            room = s.avail_out
            rc = L.inflate(C.byref(s), 4)
            assert rc == 1, (members, rc)
            pos += take - s.avail_in
            n += room - s.avail_out
            members += 1
            L.inflateReset(C.byref(s))
        L.inflateEnd(C.byref(s))
        ts.append(time.perf_counter() - t0)
    ts = sorted(ts[1:])
    print("MEMBERS %.6f %.6f %.6f %d %d %d" % (statistics.median(ts), ts[0], ts[-1], n, zlib.crc32(out[:n].tobytes()), members))


def stored_member(payload):
    c = zlib.compressobj(0, zlib.DEFLATED, 31)
    return c.compress(payload) + c.flush()


def main():
    args = sys.argv[1:]
    opt = {}
    for name in ("--out", "--members-only", "--out-bytes"):
        if name in args:
            i = args.index(name)
            opt[name] = args[i + 1]
            del args[i: i + 2]
    mib = int(args[0]) if args else 64
    level = int(args[1]) if len(args) > 1 else 6
    zlib_so = os.path.join(ROOT, "zlib_amd", "libzamd_z.so")
    out_path = opt.get("--out", os.path.join(ROOT, "profiles", "r06_gzip_members_table.txt"))
    if "--members-only" in opt:
        return members_only(opt["--members-only"], zlib_so, int(opt["--out-bytes"]))
    import torch
    import zlib_amd
    from zlib_amd import gpu
    eng = zlib_amd.Engine(0)
    dev = torch.device("cuda", 0)
    total = mib << 20
    d_corpus = torch.empty(total, dtype=torch.uint8, device=dev)
    eng.corpus_fill_device(1, SEED, 0, total >> 16, d_corpus.data_ptr())
    torch.cuda.synchronize()
    h_corpus = d_corpus.cpu().numpy()
    lines = ["# multi-member gzip: %d MiB of log-text at level %d, every member a gzip member of its own; all members in one call against inflate() member by member" % (mib, level),
             "# median (min .. max) per call over 5 timed windows of at least 0.25 s (short calls looped) behind a warm-up call; GiB/s of decoded bytes",
             "# \"planted\": the same file with one stored member in front whose payload holds a false member header: the call decodes the members twice"]
    decoy_payload = b"A" * 96 + struct.pack("<I", 50) + b"\x1f\x8b\x08\x00" + b"B" * 60
    decoy = stored_member(decoy_payload)
    for size in (4096, 65536):
        n = total // size
        # ---- the file: the wrapped segment path, segment k = corpus[k * size, (k + 1) * size) ----
        flags = gpu.F_FINAL | gpu.F_GZIP_WRAP
        cap = int(eng.L.zgpu_deflate_segments_bound(n, total, flags))
        h_f = np.empty(cap + len(decoy), dtype=np.uint8)
        offs = (np.arange(n + 1, dtype=np.uint64) * size)
        ooffs = np.zeros(n + 1, dtype=np.uint64)
        p = gpu._Params(level, 0, flags, gpu.LZ_AUTO, 0, 0)
        dres = gpu.DeflateResult()
        eng._check(eng.L.zgpu_deflate_segments_host(eng.h, h_corpus.ctypes.data, offs.ctypes.data, n, C.byref(p), h_f.ctypes.data, cap, ooffs.ctypes.data, C.byref(dres)))
        fbytes = int(dres.out_bytes)
        plain = h_f[:fbytes].copy()
        planted = np.concatenate([np.frombuffer(decoy, dtype=np.uint8), plain])
        rows, passes = [], []
        for label, h_file, extra in (("", plain, b""), (", planted", planted, decoy_payload)):
            want_bytes = total + len(extra)
            nmem = n + (1 if extra else 0)
            d_file = torch.tensor(h_file, device=dev)
            d_out = torch.empty(want_bytes + 1, dtype=torch.uint8, device=dev)
            h_out = np.empty(want_bytes + 1, dtype=np.uint8)
            ires, nm = gpu.InflateResult(), C.c_uint64(0)
            before = eng.gzip_members_count()

            def dec_dev():
                rc = eng.L.zgpu_gzip_inflate_device(eng.h, d_file.data_ptr(), h_file.size, d_out.data_ptr(), want_bytes, None, None, None, 0, C.byref(nm), C.byref(ires), None)
                assert rc == 0 and ires.out_bytes == want_bytes and nm.value == nmem, (rc, ires.out_bytes, nm.value)

            def dec_host():
                rc = eng.L.zgpu_gzip_inflate_host(eng.h, h_file.ctypes.data, h_file.size, h_out.ctypes.data, want_bytes, None, None, None, 0, C.byref(nm), C.byref(ires))
                assert rc == 0 and ires.out_bytes == want_bytes and nm.value == nmem, (rc, ires.out_bytes, nm.value)
            t_dd = timed(dec_dev)
            assert torch.equal(d_out[len(extra): want_bytes], d_corpus), "device decode differs from the corpus"
            t_dh = timed(dec_host)
            assert h_out[len(extra): want_bytes].tobytes() == h_corpus.tobytes() and h_out[: len(extra)].tobytes() == extra, "host decode differs from the corpus"
            after = eng.gzip_members_count()
            one, two = after[0] - before[0], after[1] - before[1]
            passes.append("%s: %d calls decoded once, %d twice" % ("planted" if extra else "plain", one, two))
            rows += [("device-resident" + label, t_dd), ("host buffers" + label, t_dh)]
            if not extra:
                with tempfile.TemporaryDirectory() as tmp:
                    path = os.path.join(tmp, "file.gz")
                    h_file.tofile(path)
                    line = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--members-only", path, "--out-bytes", str(total)], timeout=900).decode()
                w = [ln for ln in line.splitlines() if ln.startswith("MEMBERS ")][0].split()
                assert int(w[4]) == total and int(w[5]) == zlib.crc32(h_corpus.tobytes()) and int(w[6]) == n, "the member-by-member decode differs from the corpus"
                t_loop = (float(w[1]), float(w[2]), float(w[3]))
            del d_file, d_out
        rows.append(("inflate() windowBits 31, member by member", t_loop))
        lines.append("%d members of %d bytes, %d bytes of file (ratio %.3f); %s" % (n, size, fbytes, total / fbytes, "; ".join(passes)))
        for name, (med, lo, hi) in rows:
            lines.append("  %-44s %10.3f ms (%10.3f .. %10.3f) %8.3f GiB/s %9.3f us/member" % (name, med * 1e3, lo * 1e3, hi * 1e3, total / med / 2 ** 30, med / n * 1e6))
        lines.append("  one call from host buffers against the member-by-member loop: %.1f times; the second decode costs %.2f times the one-pass call device-resident, %.2f times from host buffers"
                     % (t_loop[0] / rows[1][1][0], rows[2][1][0] / rows[0][1][0], rows[3][1][0] / rows[1][1][0]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    eng.close()


if __name__ == "__main__":
    main()
