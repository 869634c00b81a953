"""ctypes binding of libzamd_gpu.so (C ABI: include/zamd_gpu.h).  Plumbing only."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

F_FINAL, F_ZLIB_WRAP, F_POS0, F_POS0_ALL, F_GZIP_WRAP, F_CRC32, F_CONTINUOUS, F_BGZF_WRAP = 1, 2, 4, 8, 16, 32, 64, 128
BGZF_BLOCK = 65280  # what zgpu_bgzf_deflate_* cuts its input into by default (and at most)
CONT_MORE, CONT_FLUSH, CONT_FINISH = 0, 1, 2  # zgpu_deflate_cont_host modes
WHOLE_STREAM = 0xFFFFFFFF  # inflate chunk_size: the one segment is a complete stream of any size
LZ_AUTO, LZ_SERIAL, LZ_PARALLEL, LZ_SORTED, LZ_WALK, LZ_FAST, LZ_FASTWIN = 0, 1, 2, 3, 4, 5, 6
CHECK_ADLER32, CHECK_CRC32 = 1, 2  # zgpu_inflate_set_checks
WRAP_RAW, WRAP_ZLIB, WRAP_GZIP, WRAP_AUTO = 0, 1, 2, 3  # zgpu_inflate_batch_*
_WRAPS = {"raw": WRAP_RAW, "zlib": WRAP_ZLIB, "gzip": WRAP_GZIP, "auto": WRAP_AUTO}
JOB_DECODE, JOB_SIZES, JOB_VERIFY, JOB_PACKED = 0, 1, 2, 3  # zgpu_inflate_batch_workspace_bytes
BUF_ERROR = -5  # ZGPU_BUF_ERROR: what a packed batch decode answers when its output is too small
STAGES = ["chain", "match", "parse", "lz_serial", "huffman", "stitch", "inflate"]
CHUNK = 65536


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("zgpu error %d: %s" % (code, msg))
        self.code = code


class _Params(C.Structure):
    _fields_ = [("level", C.c_int32), ("chunk_size", C.c_uint32), ("flags", C.c_uint32), ("lz_impl", C.c_int32),
                ("strategy", C.c_int32), ("prime", C.c_uint32)]


class DeflateResult(C.Structure):
    _fields_ = [("out_bytes", C.c_uint64), ("nchunks", C.c_uint64), ("adler32", C.c_uint32), ("data_type", C.c_uint32),
                ("ntokens", C.c_uint64), ("crc32", C.c_uint32), ("reserved", C.c_uint32)]


class ContState(C.Structure):
    """zgpu_cont_state: where a continuous stream stands between two feeds (stream positions)."""
    _fields_ = [("abs0", C.c_uint64), ("entry", C.c_uint64), ("block_start", C.c_uint64), ("carry_ntok", C.c_uint32), ("bit_count", C.c_uint32),
                ("bit_value", C.c_uint32), ("data_type", C.c_uint32), ("first_block", C.c_uint32), ("last_eob", C.c_uint32)]


class InflateResult(C.Structure):
    _fields_ = [("out_bytes", C.c_uint64), ("adler32", C.c_uint32), ("first_bad_chunk", C.c_int32),
                ("error_code", C.c_int32), ("error_msg", C.c_uint32), ("crc32", C.c_uint32), ("in_used_bits", C.c_uint32),
                ("in_used", C.c_uint64), ("stream_end", C.c_uint32), ("incomplete", C.c_uint32)]


class InflateItem(C.Structure):
    """zgpu_inflate_item: the verdict of one item of a batch inflate."""
    _fields_ = [("code", C.c_int32), ("msg", C.c_uint32), ("out_bytes", C.c_uint64), ("in_used", C.c_uint64), ("adler32", C.c_uint32), ("crc32", C.c_uint32)]


class InflateBatchSummary(C.Structure):
    """zgpu_inflate_batch_summary: what a stream-ordered batch inflate call (zgpu_inflate_batch_*_enqueue) leaves in device memory besides the records."""
    _fields_ = [("nfailed", C.c_uint64), ("nbad_offsets", C.c_uint64), ("total", C.c_uint64), ("overflow", C.c_uint32), ("reserved", C.c_uint32)]


class DeflateItem(C.Structure):
    """zgpu_deflate_item: one segment of zgpu_deflate_segments_items_*."""
    _fields_ = [("out_lo", C.c_uint64), ("out_bytes", C.c_uint64), ("in_bytes", C.c_uint32), ("data_type", C.c_uint32), ("adler32", C.c_uint32), ("crc32", C.c_uint32)]


class DeflateBatchItem(C.Structure):
    """zgpu_deflate_batch_item: the record of one item of a stream-ordered batch deflate call (zgpu_deflate_batch_*_enqueue)."""
    _fields_ = [("code", C.c_int32), ("data_type", C.c_uint32), ("out_lo", C.c_uint64), ("out_bytes", C.c_uint64), ("in_bytes", C.c_uint32), ("adler32", C.c_uint32),
                ("crc32", C.c_uint32), ("reserved", C.c_uint32)]


class DeflateBatchSummary(C.Structure):
    """zgpu_deflate_batch_summary: what a stream-ordered batch deflate call leaves in device memory besides the records."""
    _fields_ = [("nfailed", C.c_uint64), ("nbad_offsets", C.c_uint64), ("ntoo_long", C.c_uint64), ("total", C.c_uint64), ("overflow", C.c_uint32), ("sort_fault", C.c_uint32)]


class CheckItem(C.Structure):
    """zgpu_check_item: the checksums of one item of zgpu_checksum_batch_*."""
    _fields_ = [("adler32", C.c_uint32), ("crc32", C.c_uint32)]


def library_path():
    # ZAMD_GPU_LIB: load another build of the engine (A/B measurements of kernel variants)
    return os.environ.get("ZAMD_GPU_LIB") or os.path.join(_HERE, "libzamd_gpu.so")


def load_library():
    """Load the HIP engine.  Fails loudly when it has not been built (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process.  The torch wheel bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's);
    # whichever is mapped first serves both, so when torch is installed it must come first -- loading the system
    # runtime first and torch's afterwards leaves two runtimes in the process and torch then sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        raise ImportError("%s is missing: build it with `make -C zlib_amd/csrc` (or __graft_entry__.build())" % path)
    L = C.CDLL(path)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.zgpu_device_count.restype = C.c_int
    L.zgpu_engine_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.zgpu_engine_destroy.argtypes = [vp]
    L.zgpu_engine_destroy.restype = None
    L.zgpu_engine_error.argtypes = [vp]
    L.zgpu_engine_error.restype = C.c_char_p
    L.zgpu_version.restype = C.c_char_p
    L.zgpu_deflate_bound.argtypes = [u64, u32]
    L.zgpu_deflate_bound.restype = u64
    L.zgpu_deflate_bound_geometry.argtypes = [u64, u32, C.c_int, C.c_int]
    L.zgpu_deflate_bound_geometry.restype = u64
    L.zgpu_deflate_set_geometry.argtypes = [vp, C.c_int, C.c_int]
    L.zgpu_deflate_set_tuning.argtypes = [vp, C.c_int, u32, u32, u32, u32]
    L.zgpu_deflate_device.argtypes = [vp, vp, u64, C.POINTER(_Params), vp, u64, vp, C.POINTER(DeflateResult), vp]
    L.zgpu_deflate_host.argtypes = [vp, vp, u64, C.POINTER(_Params), vp, u64, vp, C.POINTER(DeflateResult)]
    L.zgpu_deflate_cont_bound.argtypes = [u64]
    L.zgpu_deflate_cont_bound.restype = u64
    L.zgpu_deflate_cont_host.argtypes = [vp, vp, u64, vp, u64, u64, C.POINTER(_Params), C.c_int, C.POINTER(ContState), vp, vp, vp, u32, vp, u64, C.POINTER(DeflateResult)]
    L.zgpu_deflate_segments_host.argtypes = [vp, vp, vp, u64, C.POINTER(_Params), vp, u64, vp, C.POINTER(DeflateResult)]
    L.zgpu_deflate_segments_device.argtypes = [vp, vp, u64, vp, u64, C.POINTER(_Params), vp, u64, vp, C.POINTER(DeflateResult), vp]
    L.zgpu_deflate_segments_items_host.argtypes = [vp, vp, vp, u64, C.POINTER(_Params), vp, u64, vp, C.POINTER(DeflateResult), vp]
    L.zgpu_deflate_segments_items_device.argtypes = [vp, vp, u64, vp, u64, C.POINTER(_Params), vp, u64, vp, C.POINTER(DeflateResult), vp, vp]
    L.zgpu_deflate_batch_workspace_bytes.argtypes = [u64, u32]
    L.zgpu_deflate_batch_workspace_bytes.restype = u64
    L.zgpu_deflate_batch_enqueue.argtypes = [vp, vp, u64, vp, u64, C.POINTER(_Params), vp, u64, vp, vp, vp, vp, u64, u32, vp]
    L.zgpu_deflate_batch_packed_enqueue.argtypes = [vp, vp, u64, vp, u64, C.POINTER(_Params), vp, u64, vp, vp, vp, vp, u64, u32, vp]
    L.zgpu_deflate_streams_bound.argtypes = [u64, u32]
    L.zgpu_deflate_streams_bound.restype = u64
    L.zgpu_deflate_streams_layout.argtypes = [vp, u64, u32, vp, C.POINTER(u64)]
    L.zgpu_deflate_streams_device.argtypes = [vp, vp, u64, vp, u64, C.POINTER(_Params), vp, u64, vp, vp, C.POINTER(DeflateResult), vp]
    L.zgpu_deflate_streams_host.argtypes = [vp, vp, vp, u64, C.POINTER(_Params), vp, u64, vp, vp, C.POINTER(DeflateResult)]
    L.zgpu_deflate_streams_workspace_bytes.argtypes = [u64, u64, u32]
    L.zgpu_deflate_streams_workspace_bytes.restype = u64
    L.zgpu_deflate_streams_rooms_bound.argtypes = [u64, u64, u32]
    L.zgpu_deflate_streams_rooms_bound.restype = u64
    L.zgpu_deflate_streams_layout_enqueue.argtypes = [vp, vp, u64, u64, u32, vp, vp]
    L.zgpu_deflate_streams_enqueue.argtypes = [vp, vp, u64, vp, u64, C.POINTER(_Params), vp, u64, vp, vp, vp, vp, u64, u32, vp]
    L.zgpu_engine_set_exact_sort.argtypes = [vp, C.c_int]
    L.zgpu_debug_sort_fallback.argtypes = [vp]
    L.zgpu_checksum_batch_host.argtypes = [vp, vp, u64, vp, u64, u32, vp]
    L.zgpu_checksum_batch_device.argtypes = [vp, vp, u64, vp, u64, u32, vp, vp]
    L.zgpu_inflate_device.argtypes = [vp, vp, u64, vp, u64, u32, vp, u64, C.POINTER(InflateResult), vp]
    L.zgpu_inflate_host.argtypes = [vp, vp, u64, vp, u64, u32, vp, u64, C.POINTER(InflateResult)]
    L.zgpu_deflate_segments_bound.argtypes = [u64, u64, u32]
    L.zgpu_deflate_segments_bound.restype = u64
    L.zgpu_inflate_batch_device.argtypes = [vp, vp, u64, vp, u64, C.c_int, u32, vp, u64, vp, vp, C.POINTER(u64), vp]
    L.zgpu_inflate_batch_host.argtypes = [vp, vp, u64, vp, u64, C.c_int, u32, vp, u64, vp, vp, C.POINTER(u64)]
    L.zgpu_inflate_batch_sizes_device.argtypes = [vp, vp, u64, vp, u64, C.c_int, vp, C.POINTER(u64), vp]
    L.zgpu_inflate_batch_sizes_host.argtypes = [vp, vp, u64, vp, u64, C.c_int, vp, C.POINTER(u64)]
    L.zgpu_inflate_batch_packed_device.argtypes = [vp, vp, u64, vp, u64, C.c_int, u32, u32, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(u64), vp]
    L.zgpu_inflate_batch_packed_host.argtypes = [vp, vp, u64, vp, u64, C.c_int, u32, u32, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(u64)]
    L.zgpu_inflate_batch_verify_device.argtypes = [vp, vp, u64, vp, u64, C.c_int, u32, vp, C.POINTER(u64), vp]
    L.zgpu_inflate_batch_verify_host.argtypes = [vp, vp, u64, vp, u64, C.c_int, u32, vp, C.POINTER(u64)]
    L.zgpu_inflate_batch_workspace_bytes.argtypes = [C.c_int, u64]
    L.zgpu_inflate_batch_workspace_bytes.restype = u64
    L.zgpu_inflate_batch_enqueue.argtypes = [vp, vp, u64, vp, u64, C.c_int, u32, vp, u64, vp, vp, vp, vp, u64, vp]
    L.zgpu_inflate_batch_sizes_enqueue.argtypes = [vp, vp, u64, vp, u64, C.c_int, vp, vp, vp, u64, vp]
    L.zgpu_inflate_batch_verify_enqueue.argtypes = [vp, vp, u64, vp, u64, C.c_int, u32, vp, vp, vp, u64, vp]
    L.zgpu_inflate_batch_packed_enqueue.argtypes = [vp, vp, u64, vp, u64, C.c_int, u32, u32, vp, u64, vp, vp, vp, vp, u64, vp]
    L.zgpu_bgzf_verify_device.argtypes = [vp, vp, u64, vp, C.POINTER(InflateResult), vp]
    L.zgpu_bgzf_verify_host.argtypes = [vp, vp, u64, vp, C.POINTER(InflateResult)]
    L.zgpu_bgzf_bound.argtypes = [u64, u32]
    L.zgpu_bgzf_bound.restype = u64
    L.zgpu_bgzf_deflate_device.argtypes = [vp, vp, u64, C.c_int, C.c_int, u32, vp, u64, vp, C.POINTER(DeflateResult), vp]
    L.zgpu_bgzf_deflate_host.argtypes = [vp, vp, u64, C.c_int, C.c_int, u32, vp, u64, vp, C.POINTER(DeflateResult)]
    L.zgpu_bgzf_index_device.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u32), vp]
    L.zgpu_bgzf_inflate_device.argtypes = [vp, vp, u64, vp, u64, vp, C.POINTER(InflateResult), vp]
    L.zgpu_bgzf_inflate_host.argtypes = [vp, vp, u64, vp, u64, vp, C.POINTER(InflateResult)]
    L.zgpu_gzip_inflate_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(InflateResult), vp]
    L.zgpu_gzip_inflate_host.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(InflateResult)]
    L.zgpu_gzip_members_count.argtypes = [C.c_int]
    L.zgpu_gzip_members_count.restype = u64
    L.zgpu_inflate_find_chunks_host.argtypes = [vp, vp, u64, u32, vp, u64, C.POINTER(u64)]
    L.zgpu_inflate_stream_host2.argtypes = [vp, vp, u64, u32, vp, u64, C.POINTER(InflateResult)]
    L.zgpu_inflate_stream_host3.argtypes = [vp, vp, u64, u32, u32, vp, u64, C.POINTER(InflateResult)]
    L.zgpu_comm_unique_id.argtypes = [vp]
    L.zgpu_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.zgpu_comm_destroy.argtypes = [vp]
    L.zgpu_comm_destroy.restype = None
    L.zgpu_comm_error.restype = C.c_char_p
    L.zgpu_gather_layout.argtypes = [C.c_int, vp, vp, C.POINTER(u64)]
    L.zgpu_gather_layout.restype = None
    L.zgpu_deflate_gather_sizes.argtypes = [vp, u64, u32, u64, vp, C.POINTER(u64), vp]
    L.zgpu_deflate_gather.argtypes = [vp, vp, vp, C.c_int, vp, u64, C.POINTER(u32), vp]
    L.zgpu_inflate_spec_count.argtypes = [C.c_int]
    L.zgpu_inflate_spec_count.restype = u64
    L.zgpu_inflate_message.argtypes = [u32]
    L.zgpu_inflate_message.restype = C.c_char_p
    L.zgpu_adler32_device.argtypes = [vp, vp, u64, C.POINTER(u32), vp]
    L.zgpu_crc32_device.argtypes = [vp, vp, u64, C.POINTER(u32), vp]
    L.zgpu_deflate_dict_chunk_host.argtypes = [vp, vp, u32, u32, vp, vp, u64, vp]
    L.zgpu_inflate_set_dictionary.argtypes = [vp, vp, u32]
    L.zgpu_inflate_set_checks.argtypes = [vp, u32]
    L.zgpu_profile_enable.argtypes = [vp, C.c_int]
    L.zgpu_profile_enable.restype = None
    L.zgpu_profile_reset.argtypes = [vp]
    L.zgpu_profile_reset.restype = None
    L.zgpu_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(u64)]
    L.zgpu_stage_name.argtypes = [C.c_int]
    L.zgpu_stage_name.restype = C.c_char_p
    L.zgpu_deflate_fast_count.argtypes = [vp, C.c_int]
    L.zgpu_deflate_fast_count.restype = u64
    L.zgpu_corpus_fill_device.argtypes = [vp, u32, u64, u64, u64, vp, vp]
    _lib = L
    return L


class Engine:
    """One engine per process and GPU (one process per GPU is the deployment model)."""

    def __init__(self, device=0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.zgpu_engine_create(device, C.byref(h))
        if rc != 0:
            raise EngineError(rc, "cannot create engine on device %d (%d visible)" % (device, self.L.zgpu_device_count()))
        self.h = h

    def close(self):
        if self.h:
            self.L.zgpu_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.L.zgpu_engine_error(self.h).decode())

    def inflate_set_dictionary(self, dictionary):
        d = bytes(dictionary) if dictionary else b""
        self._check(self.L.zgpu_inflate_set_dictionary(self.h, d if d else None, len(d)))

    def inflate_set_checks(self, mask):
        """Which checks of the decoded bytes the inflate calls that follow compute: CHECK_ADLER32 | CHECK_CRC32 (default both)."""
        self._check(self.L.zgpu_inflate_set_checks(self.h, mask))

    def deflate_dict_chunk_host(self, dictionary, chunk, level, final, strategy=0, flags=0):
        """One chunk behind a preset dictionary (its last 32506 bytes count); returns the raw deflate stream of `chunk`."""
        import numpy as np
        d = bytes(dictionary)[-32506:]
        buf = np.frombuffer(d + bytes(chunk) + b"\0", dtype=np.uint8)
        n = len(d) + len(chunk)
        cap = self.L.zgpu_deflate_bound(n, CHUNK)
        out = np.empty(cap, dtype=np.uint8)
        p = _Params(level, CHUNK, flags | (F_FINAL if final else 0), LZ_AUTO, strategy, 0)
        res = DeflateResult()
        self._check(self.L.zgpu_deflate_dict_chunk_host(self.h, buf.ctypes.data, n, len(d), C.byref(p), out.ctypes.data, cap, C.byref(res)))
        self.last = res
        return out[: res.out_bytes].tobytes()

    # ---- deflate ----
    def deflate_host(self, data, level, flags=F_FINAL | F_ZLIB_WRAP, chunk_size=CHUNK, lz_impl=LZ_AUTO, want_offsets=False, strategy=0, prime=(0, 0)):
        """data: bytes-like or numpy uint8 array.  Returns bytes (and the chunk offsets when asked)."""
        import numpy as np
        arr = np.frombuffer(data, dtype=np.uint8) if not hasattr(data, "ctypes") else data
        n = int(arr.size)
        cap = self.L.zgpu_deflate_bound_geometry(n, chunk_size, *getattr(self, "geometry", (15, 8)))
        if flags & F_CONTINUOUS:
            cap = self.L.zgpu_deflate_cont_bound(n) + 32
        out = np.empty(cap, dtype=np.uint8)
        nchunks = max(1, (n + chunk_size - 1) // chunk_size)
        offs = np.zeros(nchunks + 1, dtype=np.uint64)
        p = _Params(level, chunk_size, flags, lz_impl, strategy, (prime[0] << 16) | (prime[1] & 0xffff))  # prime = (nbits, value): deflatePrime
        res = DeflateResult()
        src = arr.ctypes.data if n else None
        self._check(self.L.zgpu_deflate_host(self.h, src, n, C.byref(p), out.ctypes.data, cap,
                                             offs.ctypes.data if want_offsets else None, C.byref(res)))
        self.last = res
        z = out[: res.out_bytes].tobytes()
        return (z, offs) if want_offsets else z

    def cont_new(self):
        """State of a fresh continuous stream (no dictionary) + its token carry."""
        import numpy as np
        cs = ContState(0, 0, 0, 0, 0, 0, 2, 1, 8)
        return cs, (np.zeros(16384, dtype=np.uint32), np.zeros(1040, dtype=np.uint32))  # the block's tokens so far; which history positions are in the chains (levels 1-3)

    def deflate_cont_host(self, buf, check_from, level, mode, cs, carry, strategy=0, flags=0, excl=(), split=None):
        """One feed of a continuous stream (zgpu_deflate_cont_host): buf = the history the parse can still reach + the unparsed bytes, buf[0] at stream
        position cs.abs0 (handed over as two pieces cut at `split`, default: all of it as history-less input).  Returns the whole bytes the feed
        wrote; cs and carry move on.  self.last has the checksums of buf[check_from:]."""
        import numpy as np
        arr = np.frombuffer(bytes(buf) + b"\0", dtype=np.uint8)
        n = int(arr.size) - 1
        split = 0 if split is None else min(max(split, 0), n)
        cap = self.L.zgpu_deflate_cont_bound(n) + 64
        out = np.empty(cap, dtype=np.uint8)
        p = _Params(level, 0, flags, LZ_AUTO, strategy, 0)
        res = DeflateResult()
        ex = np.ascontiguousarray(list(excl) + [0], dtype=np.uint64)
        self._check(self.L.zgpu_deflate_cont_host(self.h, arr.ctypes.data, split, arr.ctypes.data + split, n - split, check_from, C.byref(p), mode, C.byref(cs), carry[0].ctypes.data,
                                                  carry[1].ctypes.data, ex.ctypes.data, len(excl), out.ctypes.data, cap, C.byref(res)))
        self.last = res
        return out[: res.out_bytes].tobytes()

    def set_geometry(self, window_bits=15, mem_level=8):
        """deflateInit2's windowBits (9..15) and memLevel (1..9) for the deflate calls that follow; 15 / 8 is the default."""
        self._check(self.L.zgpu_deflate_set_geometry(self.h, window_bits, mem_level))
        self.geometry = (window_bits, mem_level)

    FAST_COUNTS = ("rounds", "tile_parses", "same_entry", "stopped_early", "different_token", "reach_to_end", "windows_to_diff", "windows_of_diff")

    def fast_round_counts(self):
        """Levels 1-3, one continuous stream: what the rounds of the tile parse did since the engine was made (zgpu_deflate_fast_count), as a dict.  Rounds and
        tile parses always count; the other six only over calls made while ZGPU_FAST_STATS is set in the environment."""
        return {k: int(self.L.zgpu_deflate_fast_count(self.h, i)) for i, k in enumerate(self.FAST_COUNTS)}

    def set_tuning(self, tune=None):
        """deflateTune for the deflate calls that follow: tune = (good_length, max_lazy, nice_length, max_chain) instead of the level's row; None: the level's row again."""
        g, l, n, c = tune if tune else (0, 0, 0, 0)
        self._check(self.L.zgpu_deflate_set_tuning(self.h, 1 if tune else 0, g, l, n, c))

    def deflate_segments_host(self, buffers, level, flags=0, lz_impl=LZ_AUTO, want_items=False, strategy=0):
        """Batch of independent buffers (each <= 65536 bytes) -> list of raw-deflate segments, one launch.  want_items: also the per-segment
        records (zgpu_deflate_segments_items_host) as a list of (out_lo, out_bytes, in_bytes, data_type, adler32, crc32)."""
        import numpy as np
        sizes = [len(b) for b in buffers]
        offs = np.zeros(len(buffers) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(sizes)
        blob = np.frombuffer(b"".join(buffers) + b"\0", dtype=np.uint8)
        cap = int(offs[-1]) + 40 * len(buffers) + 64
        if getattr(self, "geometry", (15, 8)) != (15, 8):
            cap = int(offs[-1]) + len(buffers) * (12288 + 5 * 520)
        out = np.empty(cap, dtype=np.uint8)
        ooffs = np.zeros(len(buffers) + 1, dtype=np.uint64)
        p = _Params(level, 0, flags, lz_impl, strategy, 0)
        res = DeflateResult()
        if want_items:
            cap += 26 * len(buffers)  # (room for any wrapper)
            out = np.empty(cap, dtype=np.uint8)
            items = (DeflateItem * max(len(buffers), 1))()
            self._check(self.L.zgpu_deflate_segments_items_host(self.h, blob.ctypes.data, offs.ctypes.data, len(buffers), C.byref(p),
                                                                out.ctypes.data, cap, ooffs.ctypes.data, C.byref(res), items))
        else:
            self._check(self.L.zgpu_deflate_segments_host(self.h, blob.ctypes.data, offs.ctypes.data, len(buffers), C.byref(p),
                                                          out.ctypes.data, cap, ooffs.ctypes.data, C.byref(res)))
        self.last = res
        raw = out[: res.out_bytes].tobytes()
        segs = [raw[int(ooffs[i]): int(ooffs[i + 1])] for i in range(len(buffers))]
        if want_items:
            return segs, [(it.out_lo, it.out_bytes, it.in_bytes, it.data_type, it.adler32, it.crc32) for it in items[: len(buffers)]]
        return segs

    def checksum_batch_host(self, data, offsets, checks=CHECK_ADLER32 | CHECK_CRC32, items=None):
        """Adler-32 / CRC-32 of the items data[offsets[k]:offsets[k+1]] in one call (zgpu_checksum_batch_host): a list of (adler32, crc32).
        data: bytes-like, or a numpy uint8 array (used in place).  items: a CheckItem array to fill -- it is left as it was when the call fails,
        and is itself what is returned (no list is built)."""
        import numpy as np
        arr = data if hasattr(data, "ctypes") else np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)[:-1]
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offs) - 1
        given = items is not None
        if not given:
            items = (CheckItem * max(n, 1))()
        self._check(self.L.zgpu_checksum_batch_host(self.h, arr.ctypes.data if arr.size else None, arr.size, offs.ctypes.data, n, checks, items))
        return items if given else [(items[k].adler32, items[k].crc32) for k in range(n)]

    def checksum_batch_device(self, d_in, in_bytes, d_offsets, n, d_items, checks=CHECK_ADLER32 | CHECK_CRC32, stream=None):
        """Device pointers as ints: d_offsets holds n + 1 uint64, d_items n records of 8 bytes (zgpu_check_item).  Blocks until they are written."""
        self._check(self.L.zgpu_checksum_batch_device(self.h, d_in, in_bytes, d_offsets, n, checks, d_items, stream))

    def deflate_batch_host(self, buffers, level, wrap="zlib", strategy=0):
        """Batch of independent buffers (each <= 65536 bytes) -> one complete stream per buffer, one launch: wrap "zlib" (what compress2()
        of the buffer emits), "gzip" (a gzip member as deflate() with windowBits 31 writes it) or "raw" (windowBits -15)."""
        import numpy as np
        flags = F_FINAL | {"raw": 0, "zlib": F_ZLIB_WRAP, "gzip": F_GZIP_WRAP}[wrap]
        sizes = [len(b) for b in buffers]
        offs = np.zeros(len(buffers) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(sizes)
        blob = np.frombuffer(b"".join(bytes(b) for b in buffers) + b"\0", dtype=np.uint8)
        cap = int(self.L.zgpu_deflate_segments_bound(len(buffers), int(offs[-1]), flags))
        out = np.empty(cap, dtype=np.uint8)
        ooffs = np.zeros(len(buffers) + 1, dtype=np.uint64)
        p = _Params(level, 0, flags, LZ_AUTO, strategy, 0)
        res = DeflateResult()
        self._check(self.L.zgpu_deflate_segments_host(self.h, blob.ctypes.data, offs.ctypes.data, len(buffers), C.byref(p),
                                                      out.ctypes.data, cap, ooffs.ctypes.data, C.byref(res)))
        self.last = res
        raw = out[: res.out_bytes].tobytes()
        return [raw[int(ooffs[i]): int(ooffs[i + 1])] for i in range(len(buffers))]

    def deflate_streams_host(self, items, level, wrap="zlib", strategy=0, flags=0, want_items=False):
        """Batch of independent buffers of ANY length -> one complete stream per buffer (zgpu_deflate_streams_host): the bytes compress2() /
        deflate(Z_FINISH) of the reference gives for that buffer alone, the tiles of all buffers sharing the launches.  Levels 4..9.  wrap as for
        deflate_batch_host; flags: further ZGPU_F_* bits (F_CRC32).  want_items: also the records, a list of DeflateBatchItem."""
        import numpy as np
        flags = flags | F_FINAL | {"raw": 0, "zlib": F_ZLIB_WRAP, "gzip": F_GZIP_WRAP}[wrap]
        n = len(items)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(b) for b in items])
        blob = np.frombuffer(b"".join(bytes(b) for b in items) + b"\0", dtype=np.uint8)
        ooffs = np.zeros(n + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        self._check(self.L.zgpu_deflate_streams_layout(offs.ctypes.data, n, flags, ooffs.ctypes.data, C.byref(total)))
        cap = int(total.value)
        out = np.empty(cap + 1, dtype=np.uint8)
        recs = (DeflateBatchItem * max(n, 1))()
        p = _Params(level, 0, flags, LZ_AUTO, strategy, 0)
        res = DeflateResult()
        self._check(self.L.zgpu_deflate_streams_host(self.h, blob.ctypes.data, offs.ctypes.data, n, C.byref(p), out.ctypes.data, cap, ooffs.ctypes.data, recs, C.byref(res)))
        self.last = res
        raw = out[: int(ooffs[n])].tobytes()
        streams = [raw[int(ooffs[i]): int(ooffs[i + 1])] for i in range(n)]
        return (streams, list(recs[:n])) if want_items else streams

    def deflate_streams_layout(self, in_offsets, flags):
        """Rooms that always suffice, from the sizes alone (zgpu_deflate_streams_layout): (out_offsets as a numpy uint64 array, total)."""
        import numpy as np
        offs = np.ascontiguousarray(in_offsets, dtype=np.uint64)
        n = len(offs) - 1
        ooffs = np.zeros(n + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        self._check(self.L.zgpu_deflate_streams_layout(offs.ctypes.data, n, flags, ooffs.ctypes.data, C.byref(total)))
        return ooffs, int(total.value)

    def deflate_streams_device(self, d_in, in_bytes, d_in_offsets, n, level, d_out, out_cap, d_out_offsets, d_items, flags=F_FINAL, strategy=0, stream=None, lz_impl=LZ_AUTO):
        """Device pointers as ints: d_in_offsets / d_out_offsets hold n + 1 uint64 (every room starts at a multiple of 4), d_items room for n
        DeflateBatchItem.  Blocks until the records are written; returns the DeflateResult (reserved = records that are not ZGPU_OK)."""
        p = _Params(level, 0, flags, lz_impl, strategy, 0)
        res = DeflateResult()
        self._check(self.L.zgpu_deflate_streams_device(self.h, d_in, in_bytes, d_in_offsets, n, C.byref(p), d_out, out_cap, d_out_offsets, d_items, C.byref(res), stream))
        self.last = res
        return res

    def inflate_batch_host(self, streams, out_caps, wrap="zlib", checks=0):
        """Batch of independent streams, one call (zgpu_inflate_batch_host).  out_caps: the room of each item (an int: the same for all).
        Returns one (code, msg, data, in_used, adler32, crc32) per item; data is the decoded bytes (b"" unless code is 0)."""
        import numpy as np
        n = len(streams)
        caps = [int(out_caps)] * n if isinstance(out_caps, int) else [int(c) for c in out_caps]
        ioffs = np.zeros(n + 1, dtype=np.uint64)
        ioffs[1:] = np.cumsum([len(s) for s in streams])
        ooffs = np.zeros(n + 1, dtype=np.uint64)
        ooffs[1:] = np.cumsum(caps)
        blob = np.frombuffer(b"".join(bytes(s) for s in streams) + b"\0", dtype=np.uint8)
        out = np.zeros(int(ooffs[-1]) + 1, dtype=np.uint8)
        items = (InflateItem * max(n, 1))()
        failed = C.c_uint64(0)
        self._check(self.L.zgpu_inflate_batch_host(self.h, blob.ctypes.data, int(ioffs[-1]), ioffs.ctypes.data, n, _WRAPS[wrap], checks,
                                                   out.ctypes.data, int(ooffs[-1]), ooffs.ctypes.data, items, C.byref(failed)))
        self.last_failed = failed.value
        res = []
        for k in range(n):
            it = items[k]
            data = out[int(ooffs[k]): int(ooffs[k]) + it.out_bytes].tobytes() if it.code == 0 else b""
            res.append((it.code, self.L.zgpu_inflate_message(it.msg).decode(), data, it.in_used, it.adler32, it.crc32))
        return res

    def inflate_batch_device(self, d_in, in_bytes, d_in_offsets, n, d_out, out_cap, d_out_offsets, d_items, wrap="zlib", checks=0, stream=None):
        """Device pointers as ints (e.g. torch.Tensor.data_ptr()): in_offsets / out_offsets hold n + 1 uint64 each, d_items n records of 32 bytes
        (zgpu_inflate_item).  Blocks until the records are written; returns the number of items that failed."""
        failed = C.c_uint64(0)
        self._check(self.L.zgpu_inflate_batch_device(self.h, d_in, in_bytes, d_in_offsets, n, _WRAPS[wrap] if isinstance(wrap, str) else wrap, checks,
                                                     d_out, out_cap, d_out_offsets, d_items, C.byref(failed), stream))
        return failed.value

    # ---- batch inflate without known sizes ----
    @staticmethod
    def _pack_streams(streams):
        import numpy as np
        ioffs = np.zeros(len(streams) + 1, dtype=np.uint64)
        ioffs[1:] = np.cumsum([len(s) for s in streams])
        return np.frombuffer(b"".join(bytes(s) for s in streams) + b"\0", dtype=np.uint8), ioffs

    def inflate_batch_sizes_host(self, streams, wrap="zlib"):
        """The sizing pass (zgpu_inflate_batch_sizes_host): what every item decodes to, nothing decoded into memory and no trailer checked.
        Returns one (code, msg, out_bytes, in_used) per item."""
        n = len(streams)
        blob, ioffs = self._pack_streams(streams)
        items = (InflateItem * max(n, 1))()
        failed = C.c_uint64(0)
        self._check(self.L.zgpu_inflate_batch_sizes_host(self.h, blob.ctypes.data, int(ioffs[-1]), ioffs.ctypes.data, n, _WRAPS[wrap], items, C.byref(failed)))
        self.last_failed = failed.value
        return [(items[k].code, self.L.zgpu_inflate_message(items[k].msg).decode(), items[k].out_bytes, items[k].in_used) for k in range(n)]

    def inflate_batch_packed_host(self, streams, wrap="zlib", checks=0, align=1):
        """Sizing pass, layout and decode in one call (zgpu_inflate_batch_packed_host); the output buffer is made here, as large as the items need
        (a second call once the first has said how much that is).  Returns (list of bytes, records): records as inflate_batch_host gives them without
        the data; self.last_offsets holds the n + 1 offsets of the layout."""
        import numpy as np
        n = len(streams)
        blob, ioffs = self._pack_streams(streams)
        items = (InflateItem * max(n, 1))()
        ooffs = np.zeros(n + 1, dtype=np.uint64)
        failed, total = C.c_uint64(0), C.c_uint64(0)
        cap = 4 * int(ioffs[-1]) + 4096
        for _ in range(2):
            out = np.zeros(cap + 1, dtype=np.uint8)
            rc = self.L.zgpu_inflate_batch_packed_host(self.h, blob.ctypes.data, int(ioffs[-1]), ioffs.ctypes.data, n, _WRAPS[wrap], checks, align,
                                                       out.ctypes.data, cap, ooffs.ctypes.data, items, C.byref(total), C.byref(failed))
            if rc != BUF_ERROR:
                break
            cap = total.value
        self._check(rc)
        self.last_failed, self.last_offsets = failed.value, [int(o) for o in ooffs]
        datas, recs = [], []
        for k in range(n):
            it = items[k]
            datas.append(out[int(ooffs[k]): int(ooffs[k]) + it.out_bytes].tobytes() if it.code == 0 else b"")
            recs.append((it.code, self.L.zgpu_inflate_message(it.msg).decode(), it.out_bytes, it.in_used, it.adler32, it.crc32))
        return datas, recs

    def inflate_batch_sizes_device(self, d_in, in_bytes, d_in_offsets, n, d_items, wrap="zlib", stream=None):
        """Device pointers as ints, as inflate_batch_device takes them.  Blocks until the records are written; returns the number of items that failed."""
        failed = C.c_uint64(0)
        self._check(self.L.zgpu_inflate_batch_sizes_device(self.h, d_in, in_bytes, d_in_offsets, n, _WRAPS[wrap] if isinstance(wrap, str) else wrap, d_items,
                                                           C.byref(failed), stream))
        return failed.value

    def inflate_batch_packed_device(self, d_in, in_bytes, d_in_offsets, n, d_out, out_cap, d_out_offsets, d_items, wrap="zlib", checks=0, align=1, stream=None):
        """d_out_offsets receives n + 1 uint64.  Returns (code, total, failed): code is 0, or BUF_ERROR when total > out_cap (the offsets and the sizing
        records are written, nothing is decoded)."""
        failed, total = C.c_uint64(0), C.c_uint64(0)
        rc = self.L.zgpu_inflate_batch_packed_device(self.h, d_in, in_bytes, d_in_offsets, n, _WRAPS[wrap] if isinstance(wrap, str) else wrap, checks, align,
                                                     d_out, out_cap, d_out_offsets, d_items, C.byref(total), C.byref(failed), stream)
        if rc != BUF_ERROR:
            self._check(rc)
        return rc, total.value, failed.value

    # ---- batch integrity test ----
    def inflate_batch_verify_host(self, streams, wrap="zlib", checks=0):
        """The integrity test (zgpu_inflate_batch_verify_host): every item decoded in full and its trailer compared, nothing decoded into memory.
        Returns one (code, msg, out_bytes, in_used, adler32, crc32) per item: what inflate_batch_host says of it given room of exactly its size."""
        n = len(streams)
        blob, ioffs = self._pack_streams(streams)
        items = (InflateItem * max(n, 1))()
        failed = C.c_uint64(0)
        self._check(self.L.zgpu_inflate_batch_verify_host(self.h, blob.ctypes.data, int(ioffs[-1]), ioffs.ctypes.data, n, _WRAPS[wrap], checks, items, C.byref(failed)))
        self.last_failed = failed.value
        return [(items[k].code, self.L.zgpu_inflate_message(items[k].msg).decode(), items[k].out_bytes, items[k].in_used, items[k].adler32, items[k].crc32) for k in range(n)]

    def inflate_batch_verify_device(self, d_in, in_bytes, d_in_offsets, n, d_items, wrap="zlib", checks=0, stream=None):
        """Device pointers as ints, as inflate_batch_sizes_device takes them.  Blocks until the records are written; returns the number of items that failed."""
        failed = C.c_uint64(0)
        self._check(self.L.zgpu_inflate_batch_verify_device(self.h, d_in, in_bytes, d_in_offsets, n, _WRAPS[wrap] if isinstance(wrap, str) else wrap, checks, d_items,
                                                            C.byref(failed), stream))
        self.last_failed = failed.value
        return failed.value

    # ---- stream-ordered batch inflate ----
    def inflate_batch_workspace_bytes(self, job, n):
        """Bytes of caller-owned device workspace a zgpu_inflate_batch_*_enqueue call of `job` (JOB_*) needs for n items; it grows with n only."""
        return int(self.L.zgpu_inflate_batch_workspace_bytes(job, n))

    def inflate_batch_enqueue(self, d_in, in_bytes, d_in_offsets, n, d_out, out_cap, d_out_offsets, d_items, d_ws, ws_bytes, wrap="zlib", checks=0, d_summary=None, stream=None):
        """Device pointers as ints, as inflate_batch_device takes them; d_ws: 256-byte aligned workspace, d_summary: room for an InflateBatchSummary or None.
        Enqueues the decode on `stream` (an int; None: the engine's) and returns: nothing is read back, the results are there when the stream gets there."""
        self._check(self.L.zgpu_inflate_batch_enqueue(self.h, d_in, in_bytes, d_in_offsets, n, _WRAPS[wrap] if isinstance(wrap, str) else wrap, checks, d_out, out_cap, d_out_offsets,
                                                      d_items, d_summary, d_ws, ws_bytes, stream))

    def inflate_batch_sizes_enqueue(self, d_in, in_bytes, d_in_offsets, n, d_items, d_ws, ws_bytes, wrap="zlib", d_summary=None, stream=None):
        """The sizing pass, enqueued (see inflate_batch_enqueue)."""
        self._check(self.L.zgpu_inflate_batch_sizes_enqueue(self.h, d_in, in_bytes, d_in_offsets, n, _WRAPS[wrap] if isinstance(wrap, str) else wrap, d_items, d_summary, d_ws, ws_bytes,
                                                            stream))

    def inflate_batch_verify_enqueue(self, d_in, in_bytes, d_in_offsets, n, d_items, d_ws, ws_bytes, wrap="zlib", checks=0, d_summary=None, stream=None):
        """The integrity test, enqueued (see inflate_batch_enqueue)."""
        self._check(self.L.zgpu_inflate_batch_verify_enqueue(self.h, d_in, in_bytes, d_in_offsets, n, _WRAPS[wrap] if isinstance(wrap, str) else wrap, checks, d_items, d_summary, d_ws,
                                                             ws_bytes, stream))

    def inflate_batch_packed_enqueue(self, d_in, in_bytes, d_in_offsets, n, d_out, out_cap, d_out_offsets, d_items, d_ws, ws_bytes, wrap="zlib", checks=0, align=1, d_summary=None,
                                     stream=None):
        """The packed decode, enqueued: d_out_offsets receives n + 1 uint64; whether the layout fit out_cap is the summary's `overflow` (see inflate_batch_enqueue)."""
        self._check(self.L.zgpu_inflate_batch_packed_enqueue(self.h, d_in, in_bytes, d_in_offsets, n, _WRAPS[wrap] if isinstance(wrap, str) else wrap, checks, align, d_out, out_cap,
                                                             d_out_offsets, d_items, d_summary, d_ws, ws_bytes, stream))

    # ---- stream-ordered batch deflate ----
    def deflate_batch_workspace_bytes(self, n, batch_items=0):
        """Bytes of caller-owned device workspace a zgpu_deflate_batch_*_enqueue call needs for n items in rounds of batch_items (0: min(n, 4096))."""
        return int(self.L.zgpu_deflate_batch_workspace_bytes(n, batch_items))

    def deflate_batch_enqueue(self, d_in, in_bytes, d_in_offsets, n, level, d_out, out_cap, d_out_offsets, d_items, d_ws, ws_bytes, flags=F_FINAL, strategy=0, batch_items=0,
                              d_summary=None, stream=None, lz_impl=LZ_AUTO, prime=0):
        """Device pointers as ints.  Item k = d_in[io[k], io[k+1]) becomes a stream of its own in its range d_out[oo[k], oo[k+1]) (d_out_offsets: n + 1 uint64, read);
        d_items: room for n DeflateBatchItem, d_ws: 256-byte aligned workspace, d_summary: room for a DeflateBatchSummary or None.  Enqueues on `stream` (an int;
        None: the engine's) and returns: nothing is read back, the results are there when the stream gets there."""
        p = _Params(level, 0, flags, lz_impl, strategy, prime)
        self._check(self.L.zgpu_deflate_batch_enqueue(self.h, d_in, in_bytes, d_in_offsets, n, C.byref(p), d_out, out_cap, d_out_offsets, d_items, d_summary, d_ws, ws_bytes,
                                                      batch_items, stream))

    def deflate_batch_packed_enqueue(self, d_in, in_bytes, d_in_offsets, n, level, d_out, out_cap, d_out_offsets, d_items, d_ws, ws_bytes, flags=F_FINAL, strategy=0, batch_items=0,
                                     d_summary=None, stream=None, lz_impl=LZ_AUTO, prime=0):
        """The same with the streams back to back in item order: d_out_offsets receives n + 1 uint64; whether they fit out_cap is the summary's `overflow`."""
        p = _Params(level, 0, flags, lz_impl, strategy, prime)
        self._check(self.L.zgpu_deflate_batch_packed_enqueue(self.h, d_in, in_bytes, d_in_offsets, n, C.byref(p), d_out, out_cap, d_out_offsets, d_items, d_summary, d_ws,
                                                             ws_bytes, batch_items, stream))

    # ---- stream-ordered batch compress of items of any length ----
    def deflate_streams_workspace_bytes(self, n, in_bytes, batch_tiles=0):
        """Bytes of caller-owned device workspace a zgpu_deflate_streams_enqueue call needs: a function of n, in_bytes and batch_tiles (0: 2048 tiles a round) alone."""
        return int(self.L.zgpu_deflate_streams_workspace_bytes(n, in_bytes, batch_tiles))

    def deflate_streams_rooms_bound(self, n, in_bytes, flags):
        """An out_cap that holds the rooms of every table of n items that runs forward and ends inside in_bytes (closed form, no table needed)."""
        return int(self.L.zgpu_deflate_streams_rooms_bound(n, in_bytes, flags))

    def deflate_streams_layout_enqueue(self, d_in_offsets, n, in_bytes, flags, d_out_offsets, stream=None):
        """Enqueues the rooms' table: d_out_offsets receives n + 1 uint64, what deflate_streams_layout gives a good table; a bad entry gets a room of 0."""
        self._check(self.L.zgpu_deflate_streams_layout_enqueue(self.h, d_in_offsets, n, in_bytes, flags, d_out_offsets, stream))

    def deflate_streams_enqueue(self, d_in, in_bytes, d_in_offsets, n, level, d_out, out_cap, d_out_offsets, d_items, d_ws, ws_bytes, flags=F_FINAL, strategy=0, batch_tiles=0,
                                d_summary=None, stream=None, lz_impl=LZ_AUTO, prime=0):
        """Device pointers as ints.  Item k = d_in[io[k], io[k+1]), of any length, becomes the stream deflate_streams_device gives it, in its room d_out[oo[k], oo[k+1]);
        d_items: room for n DeflateBatchItem, d_ws: 256-byte aligned workspace of deflate_streams_workspace_bytes(n, in_bytes, batch_tiles), d_summary: room for a
        DeflateBatchSummary or None.  Enqueues on `stream` (an int; None: the engine's) and returns: nothing is read back."""
        p = _Params(level, 0, flags, lz_impl, strategy, prime)
        self._check(self.L.zgpu_deflate_streams_enqueue(self.h, d_in, in_bytes, d_in_offsets, n, C.byref(p), d_out, out_cap, d_out_offsets, d_items, d_summary, d_ws, ws_bytes,
                                                        batch_tiles, stream))

    def set_exact_sort(self, on):
        """on: the engine's calls sort with the ballot-ranked sort (what a caller does after a batch's summary said sort_fault); off: the fast sort again."""
        self._check(self.L.zgpu_engine_set_exact_sort(self.h, 1 if on else 0))

    # ---- BGZF (blocked gzip) ----
    def bgzf_deflate_host(self, data, level=6, block_size=0, strategy=0, want_offsets=False):
        """data -> a BGZF file (zgpu_bgzf_deflate_host); with want_offsets also where every block begins, where the end block begins, the length."""
        import numpy as np
        arr = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
        n = int(arr.size) - 1
        cap = int(self.L.zgpu_bgzf_bound(n, block_size))
        out = np.empty(cap, dtype=np.uint8)
        bs = block_size or BGZF_BLOCK
        offs = np.zeros((n + bs - 1) // bs + 2, dtype=np.uint64)
        res = DeflateResult()
        self._check(self.L.zgpu_bgzf_deflate_host(self.h, arr.ctypes.data, n, level, strategy, block_size, out.ctypes.data, cap, offs.ctypes.data, C.byref(res)))
        self.last = res
        z = out[: res.out_bytes].tobytes()
        return (z, offs) if want_offsets else z

    def bgzf_inflate_host(self, data, out_cap=None):
        """A BGZF file -> (rc, bytes, items): rc the call's code (0, -3 when the chain or a block is bad, -5 when out_cap is too small), items one
        (code, msg, out_bytes, in_used) per block; self.last_inflate has out_bytes (the size needed) and the first failing block."""
        import numpy as np
        arr = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
        n = int(arr.size) - 1
        items = (InflateItem * max(n // 28, 1))()  # (no block is shorter than 28 bytes)
        res = InflateResult()
        cap = out_cap
        if cap is None:  # ask for the size first: a call with no room says what is needed
            cap = 0
            if self.L.zgpu_bgzf_inflate_host(self.h, arr.ctypes.data, n, None, 0, items, C.byref(res)) == -5:
                cap = res.out_bytes
        out = np.zeros(cap + 1, dtype=np.uint8)
        rc = self.L.zgpu_bgzf_inflate_host(self.h, arr.ctypes.data, n, out.ctypes.data, cap, items, C.byref(res))
        self.last_inflate = res
        if rc not in (0, -3, -5):
            self._check(rc)
        return rc, out[: res.out_bytes].tobytes() if rc in (0, -3) else b"", items

    def bgzf_verify_host(self, data):
        """Test a BGZF file without decoding it into memory (zgpu_bgzf_verify_host) -> (rc, items): rc 0 or -3, items as bgzf_inflate_host gives them;
        self.last_inflate has out_bytes and the first failing block."""
        import numpy as np
        arr = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
        n = int(arr.size) - 1
        items = (InflateItem * max(n // 28, 1))()
        res = InflateResult()
        rc = self.L.zgpu_bgzf_verify_host(self.h, arr.ctypes.data, n, items, C.byref(res))
        self.last_inflate = res
        if rc not in (0, -3):
            self._check(rc)
        return rc, items

    def bgzf_verify_device(self, d_in, in_bytes, d_items=None, stream=None):
        """Returns (rc, InflateResult)."""
        res = InflateResult()
        rc = self.L.zgpu_bgzf_verify_device(self.h, d_in, in_bytes, d_items, C.byref(res), stream)
        if rc not in (0, -3):
            self._check(rc)
        return rc, res

    def bgzf_index_device(self, d_in, in_bytes, d_in_offsets, d_out_offsets, cap_blocks, stream=None):
        """Device pointers as ints; the tables hold cap_blocks + 1 uint64 each.  Returns (rc, nblocks, out_bytes, ends_with_eof_block)."""
        n, total, eof = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        rc = self.L.zgpu_bgzf_index_device(self.h, d_in, in_bytes, d_in_offsets, d_out_offsets, cap_blocks, C.byref(n), C.byref(total), C.byref(eof), stream)
        if rc not in (0, -3, -5):
            self._check(rc)
        return rc, n.value, total.value, eof.value

    def bgzf_inflate_device(self, d_in, in_bytes, d_out, out_cap, d_items=None, stream=None):
        """Returns (rc, InflateResult)."""
        res = InflateResult()
        rc = self.L.zgpu_bgzf_inflate_device(self.h, d_in, in_bytes, d_out, out_cap, d_items, C.byref(res), stream)
        if rc not in (0, -3, -5):
            self._check(rc)
        return rc, res

    def bgzf_deflate_device(self, d_in, n, level, d_out, out_cap, block_size=0, strategy=0, d_offsets=None, stream=None):
        res = DeflateResult()
        self._check(self.L.zgpu_bgzf_deflate_device(self.h, d_in, n, level, strategy, block_size, d_out, out_cap, d_offsets, C.byref(res), stream))
        return res

    # ---- multi-member gzip ----
    def gzip_inflate_host(self, data, out_cap=None, cap_members=None):
        """A multi-member gzip file -> (rc, bytes, in_offsets, out_offsets, items): rc the call's code (0, -3 when a member failed, -5 when out_cap or
        cap_members is too small), the tables of the good members (zgpu_gzip_inflate_host), bytes what was delivered.  self.last_inflate has out_bytes
        (-5: the size needed), in_used and the first failing member; self.last_members the number of good members."""
        import numpy as np
        arr = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
        n = int(arr.size) - 1
        cm = n // 20 if cap_members is None else cap_members  # (no member is shorter than 20 bytes)
        items = (InflateItem * (cm + 1))()
        ioffs = np.zeros(cm + 1, dtype=np.uint64)
        ooffs = np.zeros(cm + 1, dtype=np.uint64)
        res, nm = InflateResult(), C.c_uint64(0)
        cap = out_cap
        if cap is None:  # ask for the size first: a call with no room says what is needed
            cap = 0
            if self.L.zgpu_gzip_inflate_host(self.h, arr.ctypes.data, n, None, 0, None, None, None, 0, C.byref(nm), C.byref(res)) == -5:
                cap = res.out_bytes
        out = np.zeros(cap + 1, dtype=np.uint8)
        rc = self.L.zgpu_gzip_inflate_host(self.h, arr.ctypes.data, n, out.ctypes.data, cap, ioffs.ctypes.data, ooffs.ctypes.data, items, cm, C.byref(nm), C.byref(res))
        self.last_inflate, self.last_members = res, nm.value
        if rc not in (0, -3, -5):
            self._check(rc)
        k = nm.value if rc in (0, -3) and nm.value <= cm else 0
        return rc, out[: res.out_bytes].tobytes() if rc in (0, -3) else b"", [int(x) for x in ioffs[: k + 1]], [int(x) for x in ooffs[: k + 1]], items

    def gzip_inflate_device(self, d_in, in_bytes, d_out, out_cap, d_in_offsets=None, d_out_offsets=None, d_items=None, cap_members=0, stream=None):
        """Device pointers as ints; the offset tables hold cap_members + 1 uint64 each, d_items cap_members records.  Returns (rc, nmembers, InflateResult)."""
        res, nm = InflateResult(), C.c_uint64(0)
        rc = self.L.zgpu_gzip_inflate_device(self.h, d_in, in_bytes, d_out, out_cap, d_in_offsets, d_out_offsets, d_items, cap_members, C.byref(nm), C.byref(res), stream)
        if rc not in (0, -3, -5):
            self._check(rc)
        return rc, nm.value, res

    def gzip_members_count(self):
        """(calls that decoded every member once, calls that needed the second decode) since the library was loaded"""
        return int(self.L.zgpu_gzip_members_count(0)), int(self.L.zgpu_gzip_members_count(1))

    def deflate_device(self, d_in, n, level, d_out, out_cap, flags=F_FINAL | F_ZLIB_WRAP, chunk_size=CHUNK, lz_impl=LZ_AUTO,
                       d_offsets=None, stream=None):
        """d_in / d_out / d_offsets: device pointers as ints (e.g. torch.Tensor.data_ptr())."""
        p = _Params(level, chunk_size, flags, lz_impl)
        res = DeflateResult()
        self._check(self.L.zgpu_deflate_device(self.h, d_in, n, C.byref(p), d_out, out_cap, d_offsets, C.byref(res), stream))
        return res

    # ---- inflate ----
    def inflate_host(self, data, offsets, chunk_size=CHUNK, out_len=None):
        import numpy as np
        arr = np.frombuffer(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        nchunks = len(offs) - 1
        cap = nchunks * chunk_size if out_len is None else out_len
        out = np.empty(max(cap, 1), dtype=np.uint8)
        res = InflateResult()
        rc = self.L.zgpu_inflate_host(self.h, arr.ctypes.data, arr.size, offs.ctypes.data, nchunks, chunk_size, out.ctypes.data, cap,
                                      C.byref(res))
        self.last_inflate = res
        if rc != 0:
            msg = self.L.zgpu_inflate_message(res.error_msg).decode() if rc == -3 else self.L.zgpu_engine_error(self.h).decode()
            raise EngineError(rc, msg)
        return out[: res.out_bytes].tobytes()

    def inflate_stream_host(self, body, out_cap, flags=0, out=None):
        """A raw deflate body without a side table (zgpu_inflate_stream_host2): split at its flush markers if it has them, in pieces at
        block starts found by search if it is long enough, by one workgroup otherwise.  Returns the bytes; self.last_inflate has the rest."""
        import numpy as np
        arr = np.frombuffer(body, dtype=np.uint8)
        given = out is not None
        if not given:
            out = np.empty(max(out_cap, 1), dtype=np.uint8)
        res = InflateResult()
        rc = self.L.zgpu_inflate_stream_host2(self.h, arr.ctypes.data, arr.size, flags, out.ctypes.data, out_cap, C.byref(res))
        self.last_inflate = res
        if rc != 0:
            msg = self.L.zgpu_inflate_message(res.error_msg).decode() if rc == -3 else self.L.zgpu_engine_error(self.h).decode()
            raise EngineError(rc, msg)
        return out[: res.out_bytes] if given else out[: res.out_bytes].tobytes()

    def spec_counts(self):
        return int(self.L.zgpu_inflate_spec_count(0)), int(self.L.zgpu_inflate_spec_count(1))

    def batch_piece_counts(self):
        """(long items of blocking batch decodes that were decoded in pieces, long items that fell back to the one-workgroup decoder), since the library was loaded"""
        return int(self.L.zgpu_inflate_spec_count(2)), int(self.L.zgpu_inflate_spec_count(3))

    def batch_size_piece_counts(self):
        """(long items of sizing passes -- the sizes call, the sizing half of the packed call -- that were sized in pieces, long items of a sizing pass that
        fell back to the one-wave sizing kernel), since the library was loaded.  batch_piece_counts() goes on counting the decode alone."""
        return int(self.L.zgpu_inflate_spec_count(4)), int(self.L.zgpu_inflate_spec_count(5))

    def batch_verify_piece_counts(self):
        """(long items of blocking integrity tests -- inflate_batch_verify_host / _device and what stands on them -- that were verified in pieces, long items of
        an integrity test that fell back to the one-workgroup verifier), since the library was loaded.  The decode's and the sizing pass's counters do not move
        in a verify call."""
        return int(self.L.zgpu_inflate_spec_count(6)), int(self.L.zgpu_inflate_spec_count(7))

    def inflate_device(self, d_in, n, d_offsets, nchunks, d_out, out_cap, chunk_size=CHUNK, stream=None):
        res = InflateResult()
        rc = self.L.zgpu_inflate_device(self.h, d_in, n, d_offsets, nchunks, chunk_size, d_out, out_cap, C.byref(res), stream)
        if rc != 0:
            msg = self.L.zgpu_inflate_message(res.error_msg).decode() if rc == -3 else self.L.zgpu_engine_error(self.h).decode()
            raise EngineError(rc, msg)
        return res

    def find_chunks_host(self, body, chunk_size=CHUNK, max_chunks=None):
        import numpy as np
        arr = np.frombuffer(body, dtype=np.uint8)
        max_chunks = max_chunks or (arr.size // 5 + 2)
        offs = np.zeros(max_chunks + 1, dtype=np.uint64)
        n = C.c_uint64(0)
        self._check(self.L.zgpu_inflate_find_chunks_host(self.h, arr.ctypes.data, arr.size, chunk_size, offs.ctypes.data, max_chunks,
                                                         C.byref(n)))
        return offs[: n.value + 1]

    # ---- misc ----
    def adler32_device(self, d_in, n, stream=None):
        a = C.c_uint32(0)
        self._check(self.L.zgpu_adler32_device(self.h, d_in, n, C.byref(a), stream))
        return a.value

    def crc32_device(self, d_in, n, stream=None):
        a = C.c_uint32(0)
        self._check(self.L.zgpu_crc32_device(self.h, d_in, n, C.byref(a), stream))
        return a.value

    def corpus_fill_device(self, kind, seed, first_chunk, nchunks, d_out, stream=None):
        self._check(self.L.zgpu_corpus_fill_device(self.h, kind, seed, first_chunk, nchunks, d_out, stream))

    def profile(self, on=True):
        self.L.zgpu_profile_enable(self.h, int(on))
        self.L.zgpu_profile_reset(self.h)

    def profile_read(self):
        out = {}
        for i, name in enumerate(STAGES):
            ms, n = C.c_double(0), C.c_uint64(0)
            self.L.zgpu_profile_get(self.h, i, C.byref(ms), C.byref(n))
            out[name] = (ms.value, n.value)
        return out


def gather_layout(table):
    """table: world rows of (body bytes, Adler-32, input bytes).  Returns (offsets[world + 1], total): where every rank's body starts in the gathered
    stream, where the trailer goes, the stream's length -- the C library's arithmetic (zgpu_gather_layout), which the RCCL gather itself uses."""
    import numpy as np
    L = load_library()
    t = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 3)
    offs = np.zeros(len(t) + 1, dtype=np.uint64)
    total = C.c_uint64(0)
    L.zgpu_gather_layout(len(t), t.ctypes.data, offs.ctypes.data, C.byref(total))
    return [int(x) for x in offs], int(total.value)


class Comm:
    """The RCCL communicator of the C library (include/zamd_gpu.h zgpu_comm_*): one per process and GPU.  `exchange_id` hands rank 0's 128-byte id
    to the other ranks -- any channel will do; bench.py uses the torch.distributed group it has for its barrier."""

    def __init__(self, device, world, rank, exchange_id):
        import numpy as np
        self.L = load_library()
        self.world, self.rank = world, rank
        ident = np.zeros(128, dtype=np.uint8)
        rc0 = self.L.zgpu_comm_unique_id(ident.ctypes.data) if rank == 0 else 0
        if rc0 != 0:
            ident[:] = 0
        ident = np.frombuffer(exchange_id(ident.tobytes()), dtype=np.uint8).copy()  # (also when rank 0 has no id: the others must not wait for it)
        if rc0 != 0 or not ident.any():
            raise EngineError(rc0 or -2, self.L.zgpu_comm_error().decode() if rank == 0 else "rank 0 could not make an RCCL id")
        h = C.c_void_p()
        rc = self.L.zgpu_comm_create(device, world, rank, ident.ctypes.data, C.byref(h))
        if rc != 0:
            raise EngineError(rc, self.L.zgpu_comm_error().decode())
        self.h = h

    def sizes(self, body_bytes, adler, in_bytes, stream=None):
        import numpy as np
        table = np.zeros(self.world * 3, dtype=np.uint64)
        total = C.c_uint64(0)
        rc = self.L.zgpu_deflate_gather_sizes(self.h, body_bytes, adler, in_bytes, table.ctypes.data, C.byref(total), stream)
        if rc != 0:
            raise EngineError(rc, self.L.zgpu_comm_error().decode())
        return table, int(total.value)

    def gather(self, d_body, table, level, d_out=None, out_cap=0, stream=None):
        adler = C.c_uint32(0)
        rc = self.L.zgpu_deflate_gather(self.h, d_body, table.ctypes.data, level, d_out, out_cap, C.byref(adler), stream)
        if rc != 0:
            raise EngineError(rc, self.L.zgpu_comm_error().decode())
        return int(adler.value)

    def close(self):
        if self.h:
            self.L.zgpu_comm_destroy(self.h)
            self.h = None
