// zgpu_inflate_batch.hip -- batch of independent streams (zgpu_inflate_batch_*): item k = in[in_off[k], in_off[k+1]) -> out[out_off[k], out_off[k+1]), every
// item a stream of its own with its own verdict.  The header kernel reads each item's wrapper (qcsrc/inflate.c:589-760), the decoder (zgpu_inflate.hip) runs
// in BATCH mode (one workgroup per item, straight into the item's range), the decoded bytes are checked in 64 KiB pieces by adler_kernel / crc_kernel, and
// the finish kernel (zgpu_stitch.hip) joins the pieces of each item and compares its trailer.  Items of 128 KiB of deflate data or more are decoded in
// pieces instead (zgpu_inflate_batch_pieces.hip), blocking decode only, and rejoin the chain at the merge kernel.  The sizing pass and the integrity test (further down) run
// the same header kernel and the decoder in its SIZES / VERIFY mode: neither has a destination, the second still has its trailers compared.  The blocking
// sizing pass has its long items counted in pieces, the sizing form of the same file's piece path, behind its read-back (batch_sizes_long); the blocking
// integrity test has them checked in pieces, the verify form, behind its read-back (batch_pieces_verify_run).
// The stream-ordered calls (zgpu_inflate_batch_*_enqueue, at the end) put the same chains on the caller's stream with the caller's workspace in place of
// the engine's scratch and read nothing back; their decode runs the decoder in its FOLD mode, which checks the bytes while it stores them.
#include "zgpu_common.h"
#include "zgpu_engine.h"
#include "zgpu_inflate_batch_plan.h"
#include "zgpu_inflate_pieces_plan.h"
#include "../../include/zamd_gpu.h"
#include <cstring>
#include <vector>

namespace zgpu {
__device__ inline uint32_t crc_bytes(uint32_t c, const uint8_t *p, uint64_t n) // crc32() of the reference (crc32.c:219), bit by bit: headers are short
{
    c = ~c;
    for (uint64_t i = 0; i < n; i++) {
        c ^= p[i];
#pragma unroll
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1;
    }
    return ~c;
}

// one lane per item: the wrapper in front of the deflate data (HEAD .. HCRC / DICTID of inflate(), inflate.c:589-760, windowBits -15 / 15 / 31 / 47).
// bad[0] |= 1: an offsets table that runs backwards or leaves its buffer (a bad argument of the call; such an item is made empty here).
// Item k reads in[in_lo[k], in_hi[k]) and owns out[out_lo[k], out_hi[k]): four tables, so that a caller whose items overlap (zgpu_gzip.hip) can say
// so; an offsets table of n + 1 entries is (off, off + 1).
// pl (the blocking decode with long items in pieces, zgpu_inflate_batch_pieces.hip): an item whose header is fine and whose body -- what lies behind the
// header, trailer included -- is long (pieces_long) leaves the segment table for the list of long items: its entry is made empty, so the one-workgroup
// decoder's launch over the table does nothing for it, and its record there is overwritten by the piece path.  The list's order is that of the
// atomic counter, not the items': nothing depends on it.  A list that is full (max_long = in_bytes / min_bytes: only items that overlap pass it) keeps
// the rest where they are.
__global__ void __launch_bounds__(256) batch_header_kernel(const uint8_t *__restrict__ in, uint64_t in_bytes, const uint64_t *in_lo, const uint64_t *in_hi, uint64_t n,
                                                           uint32_t wrap, uint64_t out_cap, const uint64_t *out_lo, const uint64_t *out_hi, uint64_t *seg,
                                                           BatchItemState *items, uint32_t *bad, PiecesList pl = PiecesList{})
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint64_t lo = in_lo[k], hi = in_hi[k], ol = out_lo[k], oh = out_hi[k];
    if (lo > hi || hi > in_bytes || ol > oh || oh > out_cap) { atomicOr(bad, 1u); lo = hi = 0; ol = oh = 0; }
    const uint8_t *p = in + lo;
    const uint64_t len = hi - lo;
    uint32_t kind = wrap, msg = kMsgNone;
    int32_t code = ZGPU_OK;
    uint64_t pos = 0;
    if (wrap == kWrapAuto) kind = (len >= 2 && p[0] == 0x1f && p[1] == 0x8b) ? kWrapGzip : kWrapZlib;
    auto fail = [&](uint32_t m) { if (code == ZGPU_OK) { code = ZGPU_DATA_ERROR; msg = m; } };
    if (kind == kWrapZlib) {
        if (len < 2) fail(kMsgTruncated);
        else if (((uint32_t)p[0] << 8 | p[1]) % 31) fail(kMsgHeaderCheck);
        else if ((p[0] & 15u) != 8) fail(kMsgMethod);
        else if ((p[0] >> 4) + 8 > 15) fail(kMsgWindow);
        else if (p[1] & 0x20) { if (len < 6) fail(kMsgTruncated); else code = 2; } // FDICT: the dictionary's Adler-32 follows, inflate() returns Z_NEED_DICT
        pos = 2;
    } else if (kind == kWrapGzip) {
        if (len < 2) fail(kMsgTruncated);
        else if (p[0] != 0x1f || p[1] != 0x8b) fail(kMsgHeaderCheck);
        else if (len < 10) fail(kMsgTruncated);
        else if (p[2] != 8) fail(kMsgMethod);
        else if (p[3] & 0xe0) fail(kMsgHeaderFlags);
        else {
            const uint32_t flg = p[3];
            pos = 10;
            if (flg & 4) { // FEXTRA
                if (pos + 2 > len) fail(kMsgTruncated);
                else { pos += 2 + (p[pos] | (uint32_t)p[pos + 1] << 8); if (pos > len) fail(kMsgTruncated); }
            }
            for (uint32_t f = 8; f <= 16 && code == ZGPU_OK; f <<= 1) // FNAME, FCOMMENT: zero-terminated
                if (flg & f) { while (pos < len && p[pos]) pos++; if (pos >= len) fail(kMsgTruncated); else pos++; }
            if ((flg & 2) && code == ZGPU_OK) { // FHCRC: the low 16 bits of the CRC-32 of the header in front of it
                if (pos + 2 > len) fail(kMsgTruncated);
                else if ((crc_bytes(0, p, pos) & 0xffffu) != (p[pos] | (uint32_t)p[pos + 1] << 8)) fail(kMsgHeaderCrc);
                pos += 2;
            }
        }
    }
    if (code != ZGPU_OK) pos = 0;
    const uint64_t body = code == ZGPU_OK ? lo + pos : 0, end = code == ZGPU_OK ? hi : 0; // (an item whose header failed decodes as an empty segment)
    seg[4 * k] = body; seg[4 * k + 1] = end; seg[4 * k + 2] = ol; seg[4 * k + 3] = oh;
    BatchItemState s{};
    s.in_lo = lo; s.in_hi = hi; s.body_lo = lo + pos; s.out_lo = ol; s.kind = kind; s.code = code; s.msg = msg;
    items[k] = s;
    if (pl.min_bytes && code == ZGPU_OK && pieces_long(hi - body, pl.min_bytes)) {
        const unsigned long long j = atomicAdd(&pl.hdr[kHdrLong], 1ull);
        if (j >= pl.max_long) { atomicAdd(&pl.hdr[kHdrLong], ~0ull); return; } // (no room in the list: the count goes back, the item stays with the one-workgroup decoder)
        const PiecesGeom g = pieces_geom(hi - body);
        PieceItem it{};
        it.body_lo = body; it.in_hi = hi; it.out_lo = ol; it.out_hi = oh; it.k = (uint32_t)k; it.ntargets = g.ntargets; it.piece_cap = g.piece_cap;
        pl.items[j] = it;
        seg[4 * k] = 0; seg[4 * k + 1] = 0; seg[4 * k + 2] = 0; seg[4 * k + 3] = 0;
        atomicAdd(&pl.hdr[kHdrTargets], (unsigned long long)g.ntargets); atomicAdd(&pl.hdr[kHdrSlots], (unsigned long long)g.piece_cap); atomicAdd(&pl.hdr[kHdrRoom], (unsigned long long)(oh - ol));
    }
}

// the decoder's verdict behind the header's; how many 64 KiB pieces of output the item's checks read
__global__ void __launch_bounds__(256) batch_merge_kernel(const InfStatus *__restrict__ status, uint64_t n, uint32_t any_check, BatchItemState *items)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    BatchItemState s = items[k];
    if (s.code == ZGPU_OK) {
        const InfStatus t = status[k];
        s.code = t.code; s.msg = t.code == ZGPU_DATA_ERROR ? t.msg : 0u; s.out_bytes = t.out_bytes; s.used = t.used & 0x7fffffffu;
    }
    s.npieces = (s.code == ZGPU_OK && any_check) ? (uint32_t)(((uint64_t)s.out_bytes + kChunkMax - 1) / kChunkMax) : 0u;
    items[k].code = s.code; items[k].msg = s.msg; items[k].out_bytes = s.out_bytes; items[k].used = s.used; items[k].npieces = s.npieces;
}

// one workgroup: piece0 = exclusive scan of npieces; total[0] = all pieces
__global__ void __launch_bounds__(1024) batch_piece_scan_kernel(BatchItemState *items, uint64_t n, unsigned long long *total)
{
    __shared__ unsigned long long part[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n + 1023) / 1024, a = tid * per < n ? tid * per : n, z = (tid + 1) * per < n ? (tid + 1) * per : n;
    unsigned long long sum = 0;
    for (uint64_t i = a; i < z; i++) sum += items[i].npieces;
    part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    unsigned long long o = part[tid] - sum;
    for (uint64_t i = a; i < z; i++) { items[i].piece0 = o; o += items[i].npieces; }
    if (tid == 1023) total[0] = part[1023];
}

// the piece table: item k owns boundaries [piece0 + k, piece0 + k + npieces] (its pieces, then the gap up to the next item's range, which no
// launch reads); map lists the pieces themselves, in item order
__global__ void __launch_bounds__(256) batch_piece_fill_kernel(const BatchItemState *__restrict__ items, uint64_t n, uint64_t *tab, uint32_t *map)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const BatchItemState s = items[k];
    const uint64_t base = s.piece0 + k;
    for (uint32_t i = 0; i < s.npieces; i++) { tab[base + i] = s.out_lo + (uint64_t)i * kChunkMax; map[s.piece0 + i] = (uint32_t)(base + i); }
    tab[base + s.npieces] = s.out_lo + s.out_bytes;
}

// The scratch of a batch call, one allocation (the engine's inf_status).  The sizing pass has the prefix; the decode adds the pieces of the output its
// checks read.  A packed call runs one behind the other over the same items: the decode takes the scratch over, its prefix lies where the sizing pass's lay.
// The integrity test has the prefix and, right behind it, one checksum record per item (no piece table: its pieces never leave the workgroup).
struct BatchScratch {
    uint64_t *seg; BatchItemState *items; InfStatus *status;
    unsigned long long *cnt; // 256 bytes: [0] pieces (a packed call: the layout's total), [1] failed items, [2] bad offsets
    uint64_t *tab; uint32_t *map; ChunkMeta *meta; // decode only: the piece boundaries, the piece list, the pieces' checksums (verify: meta alone, the items' checksums)
    uint8_t *long_items;                           // decode with long items in pieces only: the scratch of zgpu_inflate_batch_pieces.hip
};
enum BatchScratchKind { kScratchSizes, kScratchDecode, kScratchVerify };
static int batch_scratch(zgpu_engine *e, uint64_t n, BatchScratchKind kind, uint64_t max_pieces, BatchScratch *s, size_t long_bytes = 0)
{
    Carve at;
    const bool decode = kind == kScratchDecode;
    const size_t o_seg = at(n * 32), o_items = at(n * sizeof(BatchItemState)), o_status = at(n * sizeof(InfStatus)), o_cnt = at(256);
    size_t o_tab = 0, o_map = 0, o_meta = 0;
    if (decode) { o_tab = at((max_pieces + n + 1) * 8); o_map = at(max_pieces * 4); o_meta = at(max_pieces * sizeof(ChunkMeta)); }
    if (kind == kScratchVerify) o_meta = at(n * sizeof(ChunkMeta));
    const size_t o_long = long_bytes ? at(long_bytes) : 0;
    if (e->inf_status.reserve(e, at.off)) return ZGPU_MEM_ERROR;
    uint8_t *scr = e->inf_status;
    *s = BatchScratch{};
    s->seg = reinterpret_cast<uint64_t *>(scr + o_seg); s->items = reinterpret_cast<BatchItemState *>(scr + o_items);
    s->status = reinterpret_cast<InfStatus *>(scr + o_status); s->cnt = reinterpret_cast<unsigned long long *>(scr + o_cnt);
    if (decode) { s->tab = reinterpret_cast<uint64_t *>(scr + o_tab); s->map = reinterpret_cast<uint32_t *>(scr + o_map); }
    if (kind != kScratchSizes) s->meta = reinterpret_cast<ChunkMeta *>(scr + o_meta);
    if (long_bytes) s->long_items = scr + o_long;
    return ZGPU_OK;
}

int inflate_batch_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, uint32_t checks,
                      uint8_t *d_out, uint64_t out_cap, const uint64_t *d_out_off, zgpu_inflate_item *d_items, uint64_t *nfailed, hipStream_t st)
{
    return inflate_batch_run_ranges(e, d_in, in_bytes, d_in_off, d_in_off ? d_in_off + 1 : nullptr, n, wrap, checks, d_out, out_cap, d_out_off,
                                    d_out_off ? d_out_off + 1 : nullptr, d_items, nfailed, nullptr, st);
}

// The same with every item's input end and output end given on their own (device tables of n entries each): items may overlap in the input.
// *states (optional): the items' BatchItemState records in the engine's scratch, good until the next inflate call -- `used` and `out_bytes` of an
// item whose range was too small (ZGPU_BUF_ERROR) are there.
// Long items (a deflate body of ZGPU_BATCH_PIECES_MIN_BYTES or more, 128 KiB unless set; 0: none) are decoded in pieces by zgpu_inflate_batch_pieces.hip,
// the pieces of all of them in shared launches; the short ones, and the long ones that fall back, by the one-workgroup decoder as ever.  A call whose
// whole input is shorter than the threshold is launch for launch what it was.  no_pieces: the caller's items overlap in the input (the trial decode of
// zgpu_gzip.hip, most of whose candidates are no members at all): every item to the one-workgroup decoder.
int inflate_batch_run_ranges(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_lo, const uint64_t *d_in_hi, uint64_t n, int wrap, uint32_t checks,
                             uint8_t *d_out, uint64_t out_cap, const uint64_t *d_out_lo, const uint64_t *d_out_hi, zgpu_inflate_item *d_items, uint64_t *nfailed,
                             const BatchItemState **states, hipStream_t st, bool no_pieces)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (nfailed) *nfailed = 0;
    if (states) *states = nullptr;
    if (wrap < (int)kWrapRaw || wrap > (int)kWrapAuto || (checks & ~3u) || (n && (!d_in_lo || !d_in_hi || !d_out_lo || !d_out_hi || !d_items)) || (n && in_bytes && !d_in) ||
        (n && out_cap && !d_out) || n >= (1ull << 32))
        return fail(e, ZGPU_STREAM_ERROR, "bad inflate batch arguments");
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    // the check each item's wrapper needs is always computed (AUTO: both), the others when asked for
    const uint32_t do_adler = (checks & 1u) || wrap == (int)kWrapZlib || wrap == (int)kWrapAuto;
    const uint32_t do_crc = (checks & 2u) || wrap == (int)kWrapGzip || wrap == (int)kWrapAuto;
    // long items in pieces: only a call whose input can hold one (the block finder reads the input in 16-byte vectors: an input that is not aligned goes the old way)
    const BatchPiecesKnobs kn = batch_pieces_knobs();
    const bool pieces = !no_pieces && kn.min_bytes && in_bytes >= kn.min_bytes && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
    const uint64_t max_long = pieces ? (in_bytes / kn.min_bytes < n ? in_bytes / kn.min_bytes : n) : 0;
    BatchScratch s;
    if (int rc = batch_scratch(e, n, kScratchDecode, (out_cap >> 16) + n, &s, pieces ? batch_pieces_scratch_bytes(max_long) : 0)) return rc;
    ZGPU_HIP_CHECK(hipMemsetAsync(s.cnt, 0, 256, st));
    const uint32_t ngrid = (uint32_t)((n + 255) / 256);
    unsigned long long *d_hl = s.cnt + 8; // the piece path's eight counters: zeroed with the call's, fetched with them
    const PiecesList pl = pieces ? PiecesList{d_hl, batch_pieces_items(s.long_items), kn.min_bytes, max_long} : PiecesList{};
    hipLaunchKernelGGL(batch_header_kernel, dim3(ngrid), dim3(256), 0, st, d_in, in_bytes, d_in_lo, d_in_hi, n, (uint32_t)wrap, out_cap, d_out_lo, d_out_hi, s.seg, s.items,
                       reinterpret_cast<uint32_t *>(s.cnt + 2), pl);
    const int ring_kb = inflate_ring_kb(); // (items go straight to their place: the small rings serve them as they serve chunks)
    hipEvent_t ev{};
    prof_span_begin(e, st, &ev);
    for (uint64_t c0 = 0; c0 < n; c0 += 65536) {
        const uint32_t nb = (uint32_t)(n - c0 < 65536 ? n - c0 : 65536);
        launch_inflate_decode(kInfBatch, ring_kb, InfLaunch{d_in, in_bytes, s.seg, c0, nb, d_out, out_cap, s.status + c0}, SpecArgs{}, st);
    }
    prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev);
    unsigned long long h[16] = {};
    const unsigned long long *hl = h + 8;
    // The call's one round trip before the checks.  With long items possible it also fetches their number (the header kernel has counted them: a call that
    // has none pays 104 bytes more of this copy and nothing else); when there are some, the piece path runs now, the long items' records replace
    // the empty ones the decoder's launch left, and the merge, the piece table and the round trip are taken again.
    for (int pass = 0; pass < 2; pass++) {
        hipLaunchKernelGGL(batch_merge_kernel, dim3(ngrid), dim3(256), 0, st, s.status, n, do_adler | do_crc, s.items);
        hipLaunchKernelGGL(batch_piece_scan_kernel, dim3(1), dim3(1024), 0, st, s.items, n, s.cnt);
        hipLaunchKernelGGL(batch_piece_fill_kernel, dim3(ngrid), dim3(256), 0, st, s.items, n, s.tab, s.map);
        ZGPU_HIP_CHECK(hipGetLastError());
        ZGPU_HIP_CHECK(hipMemcpyAsync(h, s.cnt, (pieces && pass == 0) ? sizeof h : 3 * sizeof h[0], hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        if (h[2] || pass == 1 || !pieces || hl[kHdrLong] == 0) break;
        prof_span_begin(e, st, &ev);
        const int prc = batch_pieces_run(e, d_in, in_bytes, d_out, out_cap, max_long, s.long_items, d_hl, hl, s.items, s.status, kn.round_bytes, ring_kb, st);
        prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev);
        if (prc) return prc;
    }
    if (h[2]) { collect_spans(e); return fail(e, ZGPU_STREAM_ERROR, "inflate batch offsets out of range"); }
    if (h[0]) {
        ChunkGeom g{}; g.in = d_out; g.in_bytes = out_cap; g.seg_off = s.tab; g.chunk0 = 0; g.final_chunk = ~0ull; g.chunk_size = kChunkMax;
        g.nchunks = (uint32_t)h[0]; g.chunk_map = s.map;
        if (do_adler) launch_adler(g, s.meta, st);
        if (do_crc) launch_crc(g, s.meta, st);
    }
    launch_batch_finish(s.items, n, s.meta, d_in, do_adler, do_crc, d_items, s.cnt + 1, st);
    ZGPU_HIP_CHECK(hipGetLastError());
    ZGPU_HIP_CHECK(hipMemcpyAsync(h, s.cnt, 3 * sizeof h[0], hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    collect_spans(e);
    if (nfailed) *nfailed = h[1];
    if (states) *states = s.items;
    return ZGPU_OK;
}

// ---- sizing pass and packed decode (zgpu_inflate_batch_sizes_* / zgpu_inflate_batch_packed_*) ----
// the record of a sizes call: the header's verdict, behind it the sizing kernel's, behind that the one thing batch_finish_kernel says without having
// seen the decoded bytes -- an item whose trailer does not fit behind its final block is truncated
__global__ void __launch_bounds__(256) batch_sizes_finish_kernel(const BatchItemState *__restrict__ items, const InfStatus *__restrict__ status, uint64_t n,
                                                                 zgpu_inflate_item *out, unsigned long long *nfailed)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const BatchItemState s = items[k];
    zgpu_inflate_item r{};
    r.code = s.code; r.msg = s.msg; r.adler32 = 1; r.crc32 = 0;
    if (s.code == ZGPU_OK) {
        const InfStatus t = status[k];
        r.code = t.code; r.msg = t.code == ZGPU_DATA_ERROR ? t.msg : 0u;
        if (t.code == ZGPU_OK) {
            const uint64_t end = s.body_lo + (t.used & 0x7fffffffu), tl = s.kind == kWrapZlib ? 4 : s.kind == kWrapGzip ? 8 : 0;
            if (end + tl > s.in_hi) { r.code = ZGPU_DATA_ERROR; r.msg = kMsgTruncated; }
            else { r.out_bytes = t.out_bytes; r.in_used = end + tl - s.in_lo; }
        }
    }
    out[k] = r;
    if (r.code != ZGPU_OK) atomicAdd(nfailed, 1ull);
}

// one workgroup (the pattern of batch_piece_scan_kernel): lo[k] = the sizes in front of item k, each start rounded up to `align` (a power of two; starts
// that are all multiples of it: an exclusive scan of the rounded sizes), hi[k] = lo[k] + size[k], lo[n] = total[0] = the end of the last item.  An item
// whose sizing failed has size 0.
__global__ void __launch_bounds__(1024) batch_layout_kernel(const zgpu_inflate_item *__restrict__ items, uint64_t n, uint64_t align, uint64_t *lo, uint64_t *hi,
                                                            unsigned long long *total)
{
    __shared__ unsigned long long part[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n + 1023) / 1024, a = tid * per < n ? tid * per : n, z = (tid + 1) * per < n ? (tid + 1) * per : n;
    auto size_of = [&](uint64_t i) { return items[i].code == ZGPU_OK ? items[i].out_bytes : 0ull; };
    unsigned long long sum = 0;
    for (uint64_t i = a; i < z; i++) sum += (size_of(i) + align - 1) & ~(align - 1);
    part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    unsigned long long o = part[tid] - sum;
    for (uint64_t i = a; i < z; i++) {
        const uint64_t sz = size_of(i);
        lo[i] = o; hi[i] = o + sz;
        if (i + 1 == n) { lo[n] = o + sz; total[0] = o + sz; }
        o += (sz + align - 1) & ~(align - 1);
    }
}

// behind the decode of a packed call: an item that was sized takes the decoder's record, one whose sizing failed keeps the sizing pass's
__global__ void __launch_bounds__(256) batch_packed_merge_kernel(const zgpu_inflate_item *__restrict__ decoded, uint64_t n, zgpu_inflate_item *items, unsigned long long *nfailed)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (items[k].code == ZGPU_OK) items[k] = decoded[k];
    if (items[k].code != ZGPU_OK) atomicAdd(nfailed, 1ull);
}

// The sizing pass over items in[d_in_off[k], d_in_off[k + 1]): records into d_items.  The counters stay in the engine's scratch (c->s.cnt: [1] failed
// items, [2] bad offsets, [8..15] the long items' eight) and nothing is read back here: the caller's one read-back fetches them (batch_sizes_readback).
// Long items (a deflate body of ZGPU_BATCH_PIECES_SIZES_MIN_BYTES or more; not set: ZGPU_BATCH_PIECES_MIN_BYTES, 128 KiB; 0: none) leave the segment table for
// the list, as in inflate_batch_run_ranges, and the one-wave launch skips them: batch_sizes_long, behind the caller's read-back, counts them in pieces.
struct SizesCall { BatchScratch s; bool pieces; uint64_t max_long, round_slots; };
static int inflate_batch_sizes_launch(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, zgpu_inflate_item *d_items, SizesCall *c,
                                      hipStream_t st)
{
    // long items in pieces: only a call whose input can hold one (the block finder reads the input in 16-byte vectors: an input that is not aligned goes the old way)
    const BatchPiecesSizesKnobs kn = batch_pieces_sizes_knobs();
    c->pieces = kn.min_bytes && in_bytes >= kn.min_bytes && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
    c->max_long = c->pieces ? (in_bytes / kn.min_bytes < n ? in_bytes / kn.min_bytes : n) : 0;
    c->round_slots = kn.round_slots;
    BatchScratch &s = c->s;
    if (int rc = batch_scratch(e, n, kScratchSizes, 0, &s, c->pieces ? batch_pieces_scratch_bytes(c->max_long) : 0)) return rc;
    ZGPU_HIP_CHECK(hipMemsetAsync(s.cnt, 0, 256, st));
    const uint32_t ngrid = (uint32_t)((n + 255) / 256);
    const PiecesList pl = c->pieces ? PiecesList{s.cnt + 8, batch_pieces_items(s.long_items), kn.min_bytes, c->max_long} : PiecesList{};
    // (there is no destination: the header kernel is given the input tables a second time in its place, so that its range check passes what the first passes)
    hipLaunchKernelGGL(batch_header_kernel, dim3(ngrid), dim3(256), 0, st, d_in, in_bytes, d_in_off, d_in_off + 1, n, (uint32_t)wrap, in_bytes, d_in_off, d_in_off + 1, s.seg, s.items,
                       reinterpret_cast<uint32_t *>(s.cnt + 2), pl);
    hipEvent_t ev{};
    prof_span_begin(e, st, &ev);
    for (uint64_t c0 = 0; c0 < n; c0 += 65536) {
        const uint32_t nb = (uint32_t)(n - c0 < 65536 ? n - c0 : 65536);
        launch_inflate_decode(kInfSizes, kInfNoRing, InfLaunch{d_in, in_bytes, s.seg, c0, nb, nullptr, 0, s.status + c0}, SpecArgs{}, st);
    }
    prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev);
    hipLaunchKernelGGL(batch_sizes_finish_kernel, dim3(ngrid), dim3(256), 0, st, s.items, s.status, n, d_items, s.cnt + 1);
    ZGPU_HIP_CHECK(hipGetLastError());
    return ZGPU_OK;
}

// the caller's one read-back: h[0..2] as ever, and -- only where a long item was possible -- the long items' counters behind them, h[8..15] (104 bytes
// more of the same copy: all a call without long items pays)
static int batch_sizes_readback(zgpu_engine *e, const SizesCall &c, unsigned long long (&h)[16], hipStream_t st)
{
    ZGPU_HIP_CHECK(hipMemcpyAsync(h, c.s.cnt, c.pieces ? sizeof h : 3 * sizeof h[0], hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    return ZGPU_OK;
}

// Behind the read-back: *again = false and nothing is enqueued when the call has no long items (or its offsets are bad).  Otherwise the long items are
// counted in pieces (batch_pieces_sizes_run), their records replace the empty ones the one-wave launch left, and the finish kernel runs again over all
// items with the failed counter cleared first -- the first pass has counted the long items' empty records --; the caller takes its layout and its
// read-back again.
static int batch_sizes_long(zgpu_engine *e, const SizesCall &c, const unsigned long long (&h)[16], const uint8_t *d_in, uint64_t in_bytes, uint64_t n, zgpu_inflate_item *d_items,
                            bool *again, hipStream_t st)
{
    *again = false;
    if (!c.pieces || h[2] || h[8 + kHdrLong] == 0) return ZGPU_OK;
    hipEvent_t ev{};
    prof_span_begin(e, st, &ev);
    const int rc = batch_pieces_sizes_run(e, d_in, in_bytes, c.max_long, c.s.long_items, c.s.cnt + 8, h + 8, c.s.items, c.s.status, c.round_slots, st);
    prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev);
    if (rc) return rc;
    ZGPU_HIP_CHECK(hipMemsetAsync(c.s.cnt + 1, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(batch_sizes_finish_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, c.s.items, c.s.status, n, d_items, c.s.cnt + 1);
    ZGPU_HIP_CHECK(hipGetLastError());
    *again = true;
    return ZGPU_OK;
}

static int batch_sizes_args(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, const void *d_items)
{
    if (wrap < (int)kWrapRaw || wrap > (int)kWrapAuto || (n && (!d_in_off || !d_items)) || (n && in_bytes && !d_in) || n >= (1ull << 32))
        return fail(e, ZGPU_STREAM_ERROR, "bad inflate batch arguments");
    return ZGPU_OK;
}

int inflate_batch_sizes_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, zgpu_inflate_item *d_items, uint64_t *nfailed,
                            hipStream_t st)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (nfailed) *nfailed = 0;
    if (int rc = batch_sizes_args(e, d_in, in_bytes, d_in_off, n, wrap, d_items)) return rc;
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    unsigned long long h[16] = {};
    SizesCall c{};
    bool again = false;
    if (int rc = inflate_batch_sizes_launch(e, d_in, in_bytes, d_in_off, n, wrap, d_items, &c, st)) return rc;
    if (int rc = batch_sizes_readback(e, c, h, st)) return rc;
    if (int rc = batch_sizes_long(e, c, h, d_in, in_bytes, n, d_items, &again, st)) return rc;
    if (again) { if (int rc = batch_sizes_readback(e, c, h, st)) return rc; }
    collect_spans(e);
    if (h[2]) return fail(e, ZGPU_STREAM_ERROR, "inflate batch offsets out of range");
    if (nfailed) *nfailed = h[1];
    return ZGPU_OK;
}

// ---- integrity test (zgpu_inflate_batch_verify_*) ----
// the verifying decoder's verdict behind the header's, as batch_merge_kernel puts the decoder's there.  The item's check values arrive whole (meta[k]):
// for the finish kernel the item is ONE piece of all its bytes -- joining that onto the start values (1, 0 and 0) gives it back as it is -- or none
__global__ void __launch_bounds__(256) batch_verify_merge_kernel(const InfStatus *__restrict__ status, uint64_t n, uint32_t any_check, BatchItemState *items)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    BatchItemState s = items[k];
    if (s.code == ZGPU_OK) {
        const InfStatus t = status[k];
        s.code = t.code; s.msg = t.code == ZGPU_DATA_ERROR ? t.msg : 0u; s.out_bytes = t.out_bytes; s.used = t.used & 0x7fffffffu;
    }
    s.npieces = (s.code == ZGPU_OK && any_check && s.out_bytes) ? 1u : 0u;
    items[k].code = s.code; items[k].msg = s.msg; items[k].out_bytes = s.out_bytes; items[k].used = s.used; items[k].npieces = s.npieces; items[k].piece0 = k;
}

// header kernel, the verifying decoder in rounds of 65,536 items, the finish kernel of the batch decoder (the trailer is compared by the very code that
// compares it there), one read-back.  No destination, no piece table, no checksum kernels.  *states: as inflate_batch_run_ranges
// Long items: classified by the header kernel, checked in pieces behind the read-back (zgpu_inflate_batch_pieces.hip, the verify form), then merge and finish again.
// zgpu_inflate_batch_verify_enqueue does not have this: no host sees its items' sizes.
int inflate_batch_verify_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, uint32_t checks, zgpu_inflate_item *d_items,
                             uint64_t *nfailed, const BatchItemState **states, hipStream_t st)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (nfailed) *nfailed = 0;
    if (states) *states = nullptr;
    if (checks & ~3u) return fail(e, ZGPU_STREAM_ERROR, "bad inflate batch arguments");
    if (int rc = batch_sizes_args(e, d_in, in_bytes, d_in_off, n, wrap, d_items)) return rc;
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    // the check each item's wrapper needs is always computed (AUTO: both), the others when asked for
    const uint32_t do_adler = (checks & 1u) || wrap == (int)kWrapZlib || wrap == (int)kWrapAuto;
    const uint32_t do_crc = (checks & 2u) || wrap == (int)kWrapGzip || wrap == (int)kWrapAuto;
    // long items in pieces (a deflate body of ZGPU_BATCH_PIECES_VERIFY_MIN_BYTES or more; not set: ZGPU_BATCH_PIECES_MIN_BYTES where set, else 20,000,000; 0: none): only a call whose
    // input can hold one (the block finder reads the input in 16-byte vectors: an input that is not aligned goes the old way).  They leave the segment table
    // for the list, as in inflate_batch_run_ranges, and the verifier's launch skips them: batch_pieces_verify_run, behind the read-back, checks them in pieces.
    const BatchPiecesVerifyKnobs kn = batch_pieces_verify_knobs();
    const bool pieces = kn.min_bytes && in_bytes >= kn.min_bytes && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
    const uint64_t max_long = pieces ? (in_bytes / kn.min_bytes < n ? in_bytes / kn.min_bytes : n) : 0;
    BatchScratch s;
    if (int rc = batch_scratch(e, n, kScratchVerify, 0, &s, pieces ? batch_pieces_verify_scratch_bytes(max_long) : 0)) return rc;
    ZGPU_HIP_CHECK(hipMemsetAsync(s.cnt, 0, 256, st));
    const uint32_t ngrid = (uint32_t)((n + 255) / 256);
    const PiecesList pl = pieces ? PiecesList{s.cnt + 8, batch_pieces_items(s.long_items), kn.min_bytes, max_long} : PiecesList{};
    // (no destination: the input tables stand in for it, as in the sizing pass)
    hipLaunchKernelGGL(batch_header_kernel, dim3(ngrid), dim3(256), 0, st, d_in, in_bytes, d_in_off, d_in_off + 1, n, (uint32_t)wrap, in_bytes, d_in_off, d_in_off + 1, s.seg, s.items,
                       reinterpret_cast<uint32_t *>(s.cnt + 2), pl);
    hipEvent_t ev{};
    prof_span_begin(e, st, &ev);
    for (uint64_t c0 = 0; c0 < n; c0 += 65536) {
        const uint32_t nb = (uint32_t)(n - c0 < 65536 ? n - c0 : 65536);
        InfLaunch a{d_in, in_bytes, s.seg, c0, nb, nullptr, (uint64_t)(do_adler | (do_crc << 1)), s.status + c0};
        a.meta = s.meta + c0;
        launch_inflate_decode(kInfVerify, kInfNoRing, a, SpecArgs{}, st);
    }
    prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev);
    hipLaunchKernelGGL(batch_verify_merge_kernel, dim3(ngrid), dim3(256), 0, st, s.status, n, do_adler | do_crc, s.items);
    launch_batch_finish(s.items, n, s.meta, d_in, do_adler, do_crc, d_items, s.cnt + 1, st);
    ZGPU_HIP_CHECK(hipGetLastError());
    // The call's one read-back.  With long items possible it also fetches their counters (104 bytes more of this copy: all a call without long items pays);
    // when there are some, the piece path runs now, the long items' records and check values replace the empty ones the verifier's launch left, and the merge,
    // the finish kernel -- the failed counter cleared first: the first pass has counted the long items' empty records -- and the read-back are taken again.
    unsigned long long h[16] = {};
    ZGPU_HIP_CHECK(hipMemcpyAsync(h, s.cnt, pieces ? sizeof h : 3 * sizeof h[0], hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (pieces && !h[2] && h[8 + kHdrLong] != 0) {
        prof_span_begin(e, st, &ev);
        const int prc = batch_pieces_verify_run(e, d_in, in_bytes, do_adler | (do_crc << 1), max_long, s.long_items, s.cnt + 8, h + 8, s.items, s.status, s.meta, kn.round_slots, st);
        prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev);
        if (prc) return prc;
        ZGPU_HIP_CHECK(hipMemsetAsync(s.cnt + 1, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(batch_verify_merge_kernel, dim3(ngrid), dim3(256), 0, st, s.status, n, do_adler | do_crc, s.items);
        launch_batch_finish(s.items, n, s.meta, d_in, do_adler, do_crc, d_items, s.cnt + 1, st);
        ZGPU_HIP_CHECK(hipGetLastError());
        ZGPU_HIP_CHECK(hipMemcpyAsync(h, s.cnt, 3 * sizeof h[0], hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    }
    collect_spans(e);
    if (h[2]) return fail(e, ZGPU_STREAM_ERROR, "inflate batch offsets out of range");
    if (nfailed) *nfailed = h[1];
    if (states) *states = s.items;
    return ZGPU_OK;
}

// sizing pass, layout, decode.  ZGPU_BUF_ERROR (*total > out_cap): d_out_offsets, *total and the sizing records stand, nothing is decoded.
// stage_out (the host entry): the destination is the engine's output staging buffer, made large enough once the total is known -- d_out is not used
int inflate_batch_packed_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, uint32_t checks, uint32_t align,
                             uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, zgpu_inflate_item *d_items, uint64_t *total, uint64_t *nfailed, hipStream_t st, bool stage_out)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (nfailed) *nfailed = 0;
    if (align == 0 || align > 256 || (align & (align - 1)) || (checks & ~3u) || !total || (n && !d_out_off) || (n && out_cap && !d_out && !stage_out))
        return fail(e, ZGPU_STREAM_ERROR, "bad inflate batch arguments");
    if (int rc = batch_sizes_args(e, d_in, in_bytes, d_in_off, n, wrap, d_items)) return rc;
    *total = 0;
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    if (e->pk_hi.reserve(e, n + 1) || e->pk_items.reserve(e, n)) return ZGPU_MEM_ERROR;
    unsigned long long h[16] = {};
    SizesCall c{};
    if (int rc = inflate_batch_sizes_launch(e, d_in, in_bytes, d_in_off, n, wrap, d_items, &c, st)) return rc;
    for (int pass = 0; pass < 2; pass++) { // (the second pass: a call with long items, their records in place)
        hipLaunchKernelGGL(batch_layout_kernel, dim3(1), dim3(1024), 0, st, d_items, n, (uint64_t)align, d_out_off, e->pk_hi.p, c.s.cnt);
        ZGPU_HIP_CHECK(hipGetLastError());
        if (int rc = batch_sizes_readback(e, c, h, st)) return rc;
        bool again = false;
        if (pass == 0) { if (int rc = batch_sizes_long(e, c, h, d_in, in_bytes, n, d_items, &again, st)) return rc; }
        if (!again) break;
    }
    collect_spans(e);
    if (h[2]) return fail(e, ZGPU_STREAM_ERROR, "inflate batch offsets out of range");
    *total = h[0];
    if (nfailed) *nfailed = h[1];
    if (h[0] > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    if (stage_out) {
        if (int rc = ensure_stage(e, 0, h[0])) return rc;
        d_out = e->stage_out; out_cap = h[0];
    }
    // (the decode takes the engine's scratch over: the layout lives in the caller's table and pk_hi, the decoder's records go to pk_items)
    if (int rc = inflate_batch_run_ranges(e, d_in, in_bytes, d_in_off, d_in_off + 1, n, wrap, checks, d_out, out_cap, d_out_off, e->pk_hi.p, e->pk_items.p, nullptr, nullptr, st)) return rc;
    unsigned long long *fin = reinterpret_cast<unsigned long long *>(e->pk_hi.p + n);
    ZGPU_HIP_CHECK(hipMemsetAsync(fin, 0, sizeof *fin, st));
    hipLaunchKernelGGL(batch_packed_merge_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, e->pk_items.p, n, d_items, fin);
    ZGPU_HIP_CHECK(hipGetLastError());
    ZGPU_HIP_CHECK(hipMemcpyAsync(h, fin, sizeof h[0], hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (nfailed) *nfailed = h[0];
    return ZGPU_OK;
}

// ---- stream-ordered calls (zgpu_inflate_batch_*_enqueue) ----
// A call is hipMemsetAsync and kernel launches on one stream, in one chain, and returns: no synchronize, no allocation, no copy to or from the host, no
// event, no second stream, no profiling span, and no device memory of the engine's -- the scratch is the caller's workspace, laid out by
// zgpu_inflate_batch_plan.h.  What the blocking calls learn from a read-back is decided on the device instead: offsets that run backwards or leave their
// buffer fail their item, not the call; a packed call's total > out_cap empties the decode stage's items; the counts go to the caller's summary.
static_assert(sizeof(BatchItemState) == kWsStateBytes && sizeof(InfStatus) == kWsStatusBytes && sizeof(ChunkMeta) == kWsMetaBytes &&
              sizeof(zgpu_inflate_item) == kWsItemBytes && 4 * sizeof(uint64_t) == kWsSegBytes, "zgpu_inflate_batch_plan.h states the record sizes as numbers");
static_assert(ZGPU_BATCH_JOB_DECODE == kBatchJobDecode && ZGPU_BATCH_JOB_SIZES == kBatchJobSizes && ZGPU_BATCH_JOB_VERIFY == kBatchJobVerify &&
              ZGPU_BATCH_JOB_PACKED == kBatchJobPacked, "the jobs of the public header are the plan's");

// behind the header kernel, which has made such an item empty (it reads and writes nothing): the item's own verdict, ZGPU_STREAM_ERROR with no message.
// The merge kernels leave a verdict that is not ZGPU_OK alone and the finish kernels report it with sizes 0, adler32 = 1, crc32 = 0.
__global__ void __launch_bounds__(256) batch_bad_offsets_kernel(uint64_t in_bytes, const uint64_t *in_lo, const uint64_t *in_hi, uint64_t n, uint64_t out_cap, const uint64_t *out_lo,
                                                                const uint64_t *out_hi, BatchItemState *items, unsigned long long *nbad)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t lo = in_lo[k], hi = in_hi[k], ol = out_lo[k], oh = out_hi[k];
    if (lo > hi || hi > in_bytes || ol > oh || oh > out_cap) { items[k].code = ZGPU_STREAM_ERROR; items[k].msg = 0; atomicAdd(nbad, 1ull); } // (batch_header_kernel's test)
}

// a packed call whose layout does not fit the destination: the decode stage's items are made empty before the decoder sees them, so that it writes nothing
__global__ void __launch_bounds__(256) batch_packed_gate_kernel(const unsigned long long *total, uint64_t out_cap, uint64_t n, uint64_t *seg)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n || total[0] <= out_cap) return;
    seg[4 * k] = 0; seg[4 * k + 1] = 0; seg[4 * k + 2] = 0; seg[4 * k + 3] = 0;
}

// batch_packed_merge_kernel with the overflow decided here: a layout that did not fit leaves every sizing record as it is
__global__ void __launch_bounds__(256) batch_packed_merge_gated_kernel(const zgpu_inflate_item *__restrict__ decoded, uint64_t n, const unsigned long long *total, uint64_t out_cap,
                                                                       zgpu_inflate_item *items, unsigned long long *nfailed)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (total[0] <= out_cap && items[k].code == ZGPU_OK) items[k] = decoded[k];
    if (items[k].code != ZGPU_OK) atomicAdd(nfailed, 1ull);
}

__global__ void batch_summary_kernel(const unsigned long long *cnt, uint32_t failed_at, uint32_t packed, uint64_t out_cap, zgpu_inflate_batch_summary *s)
{
    const bool over = packed && cnt[kCntTotal] > out_cap; // (the merge has counted the sizing records' failures then)
    s->nfailed = cnt[failed_at]; s->nbad_offsets = cnt[kCntBadOffsets]; s->total = packed ? cnt[kCntTotal] : 0;
    s->overflow = over ? 1u : 0u; s->reserved = 0;
}

struct BatchWs { BatchScratch s; uint64_t *hi; zgpu_inflate_item *items2; };

// what every enqueue call checks before it enqueues anything, and the workspace carved up.  *st: the stream of the call.  n == 0 needs no workspace
static int batch_enqueue_begin(zgpu_engine *e, int job, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, uint32_t checks, const void *d_items,
                               void *d_ws, uint64_t ws_bytes, void *hip_stream, BatchWs *w, hipStream_t *st)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (wrap < (int)kWrapRaw || wrap > (int)kWrapAuto || (checks & ~3u) || n >= kWsMaxItems || (n && (!d_in_off || !d_items)) || (n && in_bytes && !d_in))
        return fail(e, ZGPU_STREAM_ERROR, "bad inflate batch arguments");
    *st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    *w = BatchWs{};
    if (n == 0) return ZGPU_OK;
    const BatchWsPlan p = inflate_batch_ws_plan(job, n);
    if (!d_ws || (reinterpret_cast<uintptr_t>(d_ws) & (kWsAlign - 1)) || p.total == 0 || ws_bytes < p.total) return fail(e, ZGPU_STREAM_ERROR, "inflate batch workspace: null, not 256-byte aligned or too small");
    uint8_t *b = static_cast<uint8_t *>(d_ws);
    w->s.seg = reinterpret_cast<uint64_t *>(b + p.seg.off); w->s.items = reinterpret_cast<BatchItemState *>(b + p.states.off);
    w->s.status = reinterpret_cast<InfStatus *>(b + p.status.off); w->s.cnt = reinterpret_cast<unsigned long long *>(b + p.cnt.off);
    if (p.meta.bytes) w->s.meta = reinterpret_cast<ChunkMeta *>(b + p.meta.off);
    if (p.hi.bytes) w->hi = reinterpret_cast<uint64_t *>(b + p.hi.off);
    if (p.items2.bytes) w->items2 = reinterpret_cast<zgpu_inflate_item *>(b + p.items2.off);
    int cur = -1; // (the engine supplies the device; a thread that is on it already -- a stream capture, say -- is left alone)
    ZGPU_HIP_CHECK(hipGetDevice(&cur));
    if (cur != e->device) ZGPU_HIP_CHECK(hipSetDevice(e->device));
    return ZGPU_OK;
}

static uint32_t batch_grid(uint64_t n) { return (uint32_t)((n + 255) / 256); }

static int batch_enqueue_summary(zgpu_engine *e, const BatchWs &w, uint64_t n, uint32_t failed_at, bool packed, uint64_t out_cap, zgpu_inflate_batch_summary *d_summary, hipStream_t st)
{
    if (d_summary && n) hipLaunchKernelGGL(batch_summary_kernel, dim3(1), dim3(1), 0, st, w.s.cnt, failed_at, packed ? 1u : 0u, out_cap, d_summary);
    ZGPU_HIP_CHECK(hipGetLastError());
    return ZGPU_OK;
}

// header kernel, the items with bad offsets marked (mark_bad: a packed call's decode stage leaves that to its sizing stage), the gate of a packed call,
// the fused decoder in rounds of 65,536 items, the merge of the integrity test (an item is ONE piece of all its bytes, folded already), the finish kernel
static void enqueue_fused_decode(const BatchScratch &s, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *in_lo, const uint64_t *in_hi, uint64_t n, int wrap, uint32_t checks,
                                 uint8_t *d_out, uint64_t out_cap, const uint64_t *out_lo, const uint64_t *out_hi, zgpu_inflate_item *d_items, unsigned long long *nfailed, bool mark_bad,
                                 const unsigned long long *gate_total, hipStream_t st)
{
    const uint32_t do_adler = (checks & 1u) || wrap == (int)kWrapZlib || wrap == (int)kWrapAuto;
    const uint32_t do_crc = (checks & 2u) || wrap == (int)kWrapGzip || wrap == (int)kWrapAuto;
    const uint32_t ngrid = batch_grid(n);
    const int ring_kb = inflate_ring_kb(); // (the ring the blocking decode would pick: the small rings serve items as they serve chunks)
    hipLaunchKernelGGL(batch_header_kernel, dim3(ngrid), dim3(256), 0, st, d_in, in_bytes, in_lo, in_hi, n, (uint32_t)wrap, out_cap, out_lo, out_hi, s.seg, s.items,
                       reinterpret_cast<uint32_t *>(s.cnt + kCntHeaderFlag));
    if (mark_bad) hipLaunchKernelGGL(batch_bad_offsets_kernel, dim3(ngrid), dim3(256), 0, st, in_bytes, in_lo, in_hi, n, out_cap, out_lo, out_hi, s.items, s.cnt + kCntBadOffsets);
    if (gate_total) hipLaunchKernelGGL(batch_packed_gate_kernel, dim3(ngrid), dim3(256), 0, st, gate_total, out_cap, n, s.seg);
    for (uint64_t c0 = 0; c0 < n; c0 += 65536) {
        const uint32_t nb = (uint32_t)(n - c0 < 65536 ? n - c0 : 65536);
        InfLaunch a{d_in, in_bytes, s.seg, c0, nb, d_out, out_cap, s.status + c0};
        a.meta = s.meta + c0; a.checks = do_adler | (do_crc << 1);
        launch_inflate_decode(kInfBatchFold, ring_kb, a, SpecArgs{}, st);
    }
    hipLaunchKernelGGL(batch_verify_merge_kernel, dim3(ngrid), dim3(256), 0, st, s.status, n, do_adler | do_crc, s.items);
    launch_batch_finish(s.items, n, s.meta, d_in, do_adler, do_crc, d_items, nfailed, st);
}

// the sizing pass's chain (inflate_batch_sizes_launch) with the workspace in place of the scratch
static void enqueue_sizes(const BatchScratch &s, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, zgpu_inflate_item *d_items, hipStream_t st)
{
    const uint32_t ngrid = batch_grid(n);
    hipLaunchKernelGGL(batch_header_kernel, dim3(ngrid), dim3(256), 0, st, d_in, in_bytes, d_in_off, d_in_off + 1, n, (uint32_t)wrap, in_bytes, d_in_off, d_in_off + 1, s.seg, s.items,
                       reinterpret_cast<uint32_t *>(s.cnt + kCntHeaderFlag));
    hipLaunchKernelGGL(batch_bad_offsets_kernel, dim3(ngrid), dim3(256), 0, st, in_bytes, d_in_off, d_in_off + 1, n, in_bytes, d_in_off, d_in_off + 1, s.items, s.cnt + kCntBadOffsets);
    for (uint64_t c0 = 0; c0 < n; c0 += 65536) {
        const uint32_t nb = (uint32_t)(n - c0 < 65536 ? n - c0 : 65536);
        launch_inflate_decode(kInfSizes, kInfNoRing, InfLaunch{d_in, in_bytes, s.seg, c0, nb, nullptr, 0, s.status + c0}, SpecArgs{}, st);
    }
    hipLaunchKernelGGL(batch_sizes_finish_kernel, dim3(ngrid), dim3(256), 0, st, s.items, s.status, n, d_items, s.cnt + kCntFailed);
}
} // namespace zgpu

using namespace zgpu;

// host arrays: the input and its offsets table staged in the engine's input buffer, the records and a second table behind them -- a packed call's
// layout, or (out_offsets) the caller's output table, checked like the first and uploaded; out_bytes: the room the output staging buffer needs
static int batch_stage_input(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *in_offsets, uint64_t n, uint64_t out_bytes, uint64_t **d_in_off, uint64_t **d_out_off,
                             zgpu_inflate_item **d_items, const uint64_t *out_offsets = nullptr, uint64_t out_cap = 0)
{
    for (uint64_t k = 0; k < n; k++)
        if (in_offsets[k] > in_offsets[k + 1] || in_offsets[k + 1] > in_bytes || (out_offsets && (out_offsets[k] > out_offsets[k + 1] || out_offsets[k + 1] > out_cap)))
            return fail(e, ZGPU_STREAM_ERROR, "inflate batch offsets out of range");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const uint64_t tab_bytes = (n + 1) * sizeof(uint64_t), tab_room = (tab_bytes + 255) & ~255ull, o_tab = (in_bytes + 255) & ~255ull, o_items = o_tab + 2 * tab_room;
    if (int rc = ensure_stage(e, o_items + n * sizeof(zgpu_inflate_item), out_bytes)) return rc;
    uint8_t *sin = e->stage_in;
    *d_in_off = reinterpret_cast<uint64_t *>(sin + o_tab); *d_out_off = reinterpret_cast<uint64_t *>(sin + o_tab + tab_room);
    *d_items = reinterpret_cast<zgpu_inflate_item *>(sin + o_items);
    if (in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(sin, in, in_bytes, hipMemcpyHostToDevice, e->stream));
    ZGPU_HIP_CHECK(hipMemcpyAsync(*d_in_off, in_offsets, tab_bytes, hipMemcpyHostToDevice, e->stream));
    if (out_offsets) ZGPU_HIP_CHECK(hipMemcpyAsync(*d_out_off, out_offsets, tab_bytes, hipMemcpyHostToDevice, e->stream));
    return ZGPU_OK;
}

// Bytes [lo, hi) of the output staging buffer to the caller's buffer `o`, only those of the items that succeeded (the others' bytes, any room an item
// did not fill and the gaps of an alignment stay as the caller left them).  dense: there is nothing to leave out, the range goes in one copy
static int batch_copy_back(zgpu_engine *e, bool dense, uint64_t lo, uint64_t hi, const uint64_t *out_offsets, const zgpu_inflate_item *items, uint64_t n, uint8_t *o)
{
    if (dense) {
        if (hi > lo) ZGPU_HIP_CHECK(hipMemcpy(o + lo, e->stage_out.p + lo, hi - lo, hipMemcpyDeviceToHost));
        return ZGPU_OK;
    }
    std::vector<uint8_t> tmp(hi - lo);
    if (hi > lo) ZGPU_HIP_CHECK(hipMemcpy(tmp.data(), e->stage_out.p + lo, hi - lo, hipMemcpyDeviceToHost));
    for (uint64_t k = 0; k < n; k++)
        if (items[k].code == ZGPU_OK && items[k].out_bytes) memcpy(o + out_offsets[k], tmp.data() + (out_offsets[k] - lo), items[k].out_bytes);
    return ZGPU_OK;
}

extern "C" {
#pragma GCC visibility push(default)
int zgpu_inflate_batch_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap, uint32_t checks,
                              void *d_out, uint64_t out_cap, const uint64_t *d_out_offsets, zgpu_inflate_item *d_items, uint64_t *nfailed, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    return inflate_batch_run(e, static_cast<const uint8_t *>(d_in), in_bytes, d_in_offsets, n, wrap, checks, static_cast<uint8_t *>(d_out), out_cap,
                             d_out_offsets, d_items, nfailed, st);
}

// host arrays: input, both offset tables and the records staged in the engine's buffers; the decoded range comes back in one copy and each item
// that succeeded is placed from there
int zgpu_inflate_batch_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *in_offsets, uint64_t n, int wrap, uint32_t checks,
                            void *out, uint64_t out_cap, const uint64_t *out_offsets, zgpu_inflate_item *items, uint64_t *nfailed)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (nfailed) *nfailed = 0;
    if (n && (!in_offsets || !out_offsets || !items || (in_bytes && !in) || (out_cap && !out))) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    if (n == 0) return ZGPU_OK;
    const uint64_t lo = out_offsets[0], hi = out_offsets[n];
    uint64_t *d_in_off, *d_out_off;
    zgpu_inflate_item *d_items;
    if (int rc = batch_stage_input(e, in, in_bytes, in_offsets, n, hi, &d_in_off, &d_out_off, &d_items, out_offsets, out_cap)) return rc;
    hipStream_t st = e->stream;
    if (int rc = inflate_batch_run(e, e->stage_in, in_bytes, d_in_off, n, wrap, checks, e->stage_out, hi, d_out_off, d_items, nfailed, st)) return rc;
    ZGPU_HIP_CHECK(hipMemcpyAsync(items, d_items, n * sizeof(zgpu_inflate_item), hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    bool all = true; // every item succeeded and filled its room exactly: the range goes straight to the caller
    for (uint64_t k = 0; k < n && all; k++) all = items[k].code == ZGPU_OK && items[k].out_bytes == out_offsets[k + 1] - out_offsets[k];
    return batch_copy_back(e, all, lo, hi, out_offsets, items, n, static_cast<uint8_t *>(out));
}

int zgpu_inflate_batch_sizes_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap, zgpu_inflate_item *d_items,
                                    uint64_t *nfailed, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    return inflate_batch_sizes_run(e, static_cast<const uint8_t *>(d_in), in_bytes, d_in_offsets, n, wrap, d_items, nfailed, st);
}

int zgpu_inflate_batch_packed_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap, uint32_t checks, uint32_t align,
                                     void *d_out, uint64_t out_cap, uint64_t *d_out_offsets, zgpu_inflate_item *d_items, uint64_t *total, uint64_t *nfailed, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    return inflate_batch_packed_run(e, static_cast<const uint8_t *>(d_in), in_bytes, d_in_offsets, n, wrap, checks, align, static_cast<uint8_t *>(d_out), out_cap, d_out_offsets,
                                    d_items, total, nfailed, st, false);
}

int zgpu_inflate_batch_sizes_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *in_offsets, uint64_t n, int wrap, zgpu_inflate_item *items, uint64_t *nfailed)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (nfailed) *nfailed = 0;
    if (int rc = batch_sizes_args(e, in, in_bytes, in_offsets, n, wrap, items)) return rc;
    if (n == 0) return ZGPU_OK;
    uint64_t *d_in_off, *d_out_off;
    zgpu_inflate_item *d_items;
    if (int rc = batch_stage_input(e, in, in_bytes, in_offsets, n, 0, &d_in_off, &d_out_off, &d_items)) return rc;
    if (int rc = inflate_batch_sizes_run(e, e->stage_in, in_bytes, d_in_off, n, wrap, d_items, nfailed, e->stream)) return rc;
    ZGPU_HIP_CHECK(hipMemcpy(items, d_items, n * sizeof(zgpu_inflate_item), hipMemcpyDeviceToHost));
    return ZGPU_OK;
}

int zgpu_inflate_batch_verify_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap, uint32_t checks,
                                     zgpu_inflate_item *d_items, uint64_t *nfailed, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    return inflate_batch_verify_run(e, static_cast<const uint8_t *>(d_in), in_bytes, d_in_offsets, n, wrap, checks, d_items, nfailed, nullptr, st);
}

int zgpu_inflate_batch_verify_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *in_offsets, uint64_t n, int wrap, uint32_t checks,
                                   zgpu_inflate_item *items, uint64_t *nfailed)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (nfailed) *nfailed = 0;
    if (checks & ~3u) return fail(e, ZGPU_STREAM_ERROR, "bad inflate batch arguments");
    if (int rc = batch_sizes_args(e, in, in_bytes, in_offsets, n, wrap, items)) return rc;
    if (n == 0) return ZGPU_OK;
    uint64_t *d_in_off, *d_out_off;
    zgpu_inflate_item *d_items;
    if (int rc = batch_stage_input(e, in, in_bytes, in_offsets, n, 0, &d_in_off, &d_out_off, &d_items)) return rc;
    if (int rc = inflate_batch_verify_run(e, e->stage_in, in_bytes, d_in_off, n, wrap, checks, d_items, nfailed, nullptr, e->stream)) return rc;
    ZGPU_HIP_CHECK(hipMemcpy(items, d_items, n * sizeof(zgpu_inflate_item), hipMemcpyDeviceToHost));
    return ZGPU_OK;
}

int zgpu_inflate_batch_packed_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *in_offsets, uint64_t n, int wrap, uint32_t checks, uint32_t align,
                                   void *out, uint64_t out_cap, uint64_t *out_offsets, zgpu_inflate_item *items, uint64_t *total, uint64_t *nfailed)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (nfailed) *nfailed = 0;
    if (align == 0 || align > 256 || (align & (align - 1)) || (checks & ~3u) || !total || (n && !out_offsets) || (n && out_cap && !out))
        return fail(e, ZGPU_STREAM_ERROR, "bad inflate batch arguments");
    if (int rc = batch_sizes_args(e, in, in_bytes, in_offsets, n, wrap, items)) return rc;
    *total = 0;
    if (n == 0) return ZGPU_OK;
    uint64_t *d_in_off, *d_out_off;
    zgpu_inflate_item *d_items;
    if (int rc = batch_stage_input(e, in, in_bytes, in_offsets, n, 0, &d_in_off, &d_out_off, &d_items)) return rc;
    const int rc = inflate_batch_packed_run(e, e->stage_in, in_bytes, d_in_off, n, wrap, checks, align, nullptr, out_cap, d_out_off, d_items, total, nfailed, e->stream, true);
    if (rc != ZGPU_OK && rc != ZGPU_BUF_ERROR) return rc;
    ZGPU_HIP_CHECK(hipMemcpy(items, d_items, n * sizeof(zgpu_inflate_item), hipMemcpyDeviceToHost));
    ZGPU_HIP_CHECK(hipMemcpy(out_offsets, d_out_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (rc == ZGPU_BUF_ERROR) return rc;
    bool dense = align == 1; // every item succeeded and no alignment leaves gaps between them
    for (uint64_t k = 0; k < n && dense; k++) dense = items[k].code == ZGPU_OK;
    return batch_copy_back(e, dense, 0, *total, out_offsets, items, n, static_cast<uint8_t *>(out));
}

// ---- the stream-ordered entry points (include/zamd_gpu.h) ----
uint64_t zgpu_inflate_batch_workspace_bytes(int job, uint64_t n) { return inflate_batch_ws_bytes(job, n); }

int zgpu_inflate_batch_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap, uint32_t checks, void *d_out, uint64_t out_cap,
                               const uint64_t *d_out_offsets, zgpu_inflate_item *d_items, zgpu_inflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes, void *hip_stream)
{
    BatchWs w;
    hipStream_t st;
    if (e && n && (!d_out_offsets || (out_cap && !d_out))) return fail(e, ZGPU_STREAM_ERROR, "bad inflate batch arguments");
    if (int rc = batch_enqueue_begin(e, kBatchJobDecode, d_in, in_bytes, d_in_offsets, n, wrap, checks, d_items, d_ws, ws_bytes, hip_stream, &w, &st)) return rc;
    if (d_summary) ZGPU_HIP_CHECK(hipMemsetAsync(d_summary, 0, sizeof *d_summary, st));
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipMemsetAsync(w.s.cnt, 0, kWsCntBytes, st));
    enqueue_fused_decode(w.s, static_cast<const uint8_t *>(d_in), in_bytes, d_in_offsets, d_in_offsets + 1, n, wrap, checks, static_cast<uint8_t *>(d_out), out_cap, d_out_offsets,
                         d_out_offsets + 1, d_items, w.s.cnt + kCntFailed, true, nullptr, st);
    return batch_enqueue_summary(e, w, n, kCntFailed, false, 0, d_summary, st);
}

int zgpu_inflate_batch_sizes_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap, zgpu_inflate_item *d_items,
                                     zgpu_inflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes, void *hip_stream)
{
    BatchWs w;
    hipStream_t st;
    if (int rc = batch_enqueue_begin(e, kBatchJobSizes, d_in, in_bytes, d_in_offsets, n, wrap, 0, d_items, d_ws, ws_bytes, hip_stream, &w, &st)) return rc;
    if (d_summary) ZGPU_HIP_CHECK(hipMemsetAsync(d_summary, 0, sizeof *d_summary, st));
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipMemsetAsync(w.s.cnt, 0, kWsCntBytes, st));
    enqueue_sizes(w.s, static_cast<const uint8_t *>(d_in), in_bytes, d_in_offsets, n, wrap, d_items, st);
    return batch_enqueue_summary(e, w, n, kCntFailed, false, 0, d_summary, st);
}

// the integrity test's chain (inflate_batch_verify_run) with the workspace in place of the scratch
int zgpu_inflate_batch_verify_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap, uint32_t checks, zgpu_inflate_item *d_items,
                                      zgpu_inflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes, void *hip_stream)
{
    BatchWs w;
    hipStream_t st;
    if (int rc = batch_enqueue_begin(e, kBatchJobVerify, d_in, in_bytes, d_in_offsets, n, wrap, checks, d_items, d_ws, ws_bytes, hip_stream, &w, &st)) return rc;
    if (d_summary) ZGPU_HIP_CHECK(hipMemsetAsync(d_summary, 0, sizeof *d_summary, st));
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipMemsetAsync(w.s.cnt, 0, kWsCntBytes, st));
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    const BatchScratch &s = w.s;
    const uint32_t do_adler = (checks & 1u) || wrap == (int)kWrapZlib || wrap == (int)kWrapAuto;
    const uint32_t do_crc = (checks & 2u) || wrap == (int)kWrapGzip || wrap == (int)kWrapAuto;
    const uint32_t ngrid = batch_grid(n);
    hipLaunchKernelGGL(batch_header_kernel, dim3(ngrid), dim3(256), 0, st, in, in_bytes, d_in_offsets, d_in_offsets + 1, n, (uint32_t)wrap, in_bytes, d_in_offsets, d_in_offsets + 1, s.seg,
                       s.items, reinterpret_cast<uint32_t *>(s.cnt + kCntHeaderFlag));
    hipLaunchKernelGGL(batch_bad_offsets_kernel, dim3(ngrid), dim3(256), 0, st, in_bytes, d_in_offsets, d_in_offsets + 1, n, in_bytes, d_in_offsets, d_in_offsets + 1, s.items,
                       s.cnt + kCntBadOffsets);
    for (uint64_t c0 = 0; c0 < n; c0 += 65536) {
        const uint32_t nb = (uint32_t)(n - c0 < 65536 ? n - c0 : 65536);
        InfLaunch a{in, in_bytes, s.seg, c0, nb, nullptr, (uint64_t)(do_adler | (do_crc << 1)), s.status + c0};
        a.meta = s.meta + c0;
        launch_inflate_decode(kInfVerify, kInfNoRing, a, SpecArgs{}, st);
    }
    hipLaunchKernelGGL(batch_verify_merge_kernel, dim3(ngrid), dim3(256), 0, st, s.status, n, do_adler | do_crc, s.items);
    launch_batch_finish(s.items, n, s.meta, in, do_adler, do_crc, d_items, s.cnt + kCntFailed, st);
    return batch_enqueue_summary(e, w, n, kCntFailed, false, 0, d_summary, st);
}

// sizing pass, layout, fused decode into that layout, merge: one chain.  Whether the layout fits out_cap is decided where the total is, on the device
int zgpu_inflate_batch_packed_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap, uint32_t checks, uint32_t align, void *d_out,
                                      uint64_t out_cap, uint64_t *d_out_offsets, zgpu_inflate_item *d_items, zgpu_inflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes,
                                      void *hip_stream)
{
    BatchWs w;
    hipStream_t st;
    if (e && (align == 0 || align > 256 || (align & (align - 1)) || (n && !d_out_offsets) || (n && out_cap && !d_out))) return fail(e, ZGPU_STREAM_ERROR, "bad inflate batch arguments");
    if (int rc = batch_enqueue_begin(e, kBatchJobPacked, d_in, in_bytes, d_in_offsets, n, wrap, checks, d_items, d_ws, ws_bytes, hip_stream, &w, &st)) return rc;
    if (d_summary) ZGPU_HIP_CHECK(hipMemsetAsync(d_summary, 0, sizeof *d_summary, st));
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipMemsetAsync(w.s.cnt, 0, kWsCntBytes, st));
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    enqueue_sizes(w.s, in, in_bytes, d_in_offsets, n, wrap, d_items, st);
    hipLaunchKernelGGL(batch_layout_kernel, dim3(1), dim3(1024), 0, st, d_items, n, (uint64_t)align, d_out_offsets, w.hi, w.s.cnt + kCntTotal);
    // (the decode stage takes seg, the states and the status over; its records go to the second set until the merge)
    enqueue_fused_decode(w.s, in, in_bytes, d_in_offsets, d_in_offsets + 1, n, wrap, checks, static_cast<uint8_t *>(d_out), out_cap, d_out_offsets, w.hi, w.items2,
                         w.s.cnt + kCntDecodeFailed, false, w.s.cnt + kCntTotal, st);
    hipLaunchKernelGGL(batch_packed_merge_gated_kernel, dim3(batch_grid(n)), dim3(256), 0, st, w.items2, n, w.s.cnt + kCntTotal, out_cap, d_items, w.s.cnt + kCntMerged);
    return batch_enqueue_summary(e, w, n, kCntMerged, true, out_cap, d_summary, st);
}
#pragma GCC visibility pop
}
