// zgpu_deflate_batch.hip -- stream-ordered batch deflate (zgpu_deflate_batch_*_enqueue, include/zamd_gpu.h): many independent items of at most 64 KiB that
// sit in device memory, each compressed to a stream of its own on the CALLER's stream.  A call is kernel launches in one chain and
// returns: no synchronize, no allocation, no copy to or from the host, no event, no profiling span, and no device memory of the engine's -- the scratch is
// the caller's workspace, laid out by zgpu_deflate_batch_plan.h.  The kernels that make the streams are the segment call's own (launch_lz_sorted,
// launch_huffman, launch_adler, launch_crc, on regions of that workspace); what the blocking call (deflate_device, zgpu_deflate.hip) learns from a
// read-back is decided on the device here:
//   the caller's table    dbatch_check_kernel judges every entry -- an item whose offsets run backwards, leave the input or are too far apart fails alone --
//                         and lays the served items of a round out back to back; dbatch_gather_kernel copies them into the workspace's staging buffer, so
//                         that the chunk kernels read a monotone segment table, as they always have (ChunkGeom and chunk_span are untouched)
//   where a stream goes   dbatch_scan_kernel (packed entry: back to back, the running total carried from round to round in the workspace) or the caller's
//                         ranges; dbatch_place_kernel compares the stream with its room, copies the slot, writes header and trailer and the record
//   the sort's self-check dbatch_finish_kernel, the call's last launch, reads the fault word: raised, every record becomes ZGPU_ERRNO; it writes the summary
#include "zgpu_engine.h"
#include "zgpu_deflate_plan.h"
#include "zgpu_deflate_batch_plan.h"

namespace zgpu {

static_assert(kDwsTokenBytes == kChunkMax * sizeof(uint32_t) && kDwsSlotBytes == kSlotStride && kDwsMetaBytes == sizeof(ChunkMeta),
              "zgpu_deflate_batch_plan.h states what a round's item costs as numbers");
static_assert(sizeof(zgpu_deflate_batch_item) == 40 && sizeof(zgpu_deflate_batch_summary) == 40, "the records of include/zamd_gpu.h");
static_assert(kDwsStageBytes == kChunkMax && kDwsLoBytes == sizeof(uint64_t) && kDwsPreBytes == sizeof(uint64_t), "the staging buffer and its tables");
static_assert(kDwsCntBytes / 8 == 32, "dbatch_head_kernel clears the counters with lanes 0..31");
static_assert(kSlotStride % 4 == 0, "dbatch_place_kernel reads the slots as words");

constexpr uint32_t kItemServed = 0, kItemFailed = 1;

// ---- the head of the chain: the counters, the sort's fault word and the summary start from zero.  A kernel, not hipMemsetAsync.  What was seen with three
// memsets here (256 bytes of counters, 4 of the fault word, 40 of the summary) in a call captured with torch.cuda.graph: the first replay was right; from
// the second replay on the counters held a repeating 16-byte pattern and the summary's first 24 bytes the same bytes, while eager calls were always
// right.  The pattern was the argument block of the kernel launched between the replays -- a fill of the destination with 0xA5: its byte, its element
// count 0x1a1d4 and its pointer -- in three fresh processes, and it followed whichever fill came last.  The cause inside the runtime is not known; the
// inflate enqueue calls (zgpu_inflate_batch.hip) still clear with hipMemsetAsync and their test replays once, so they are not known to be clear of it ----
__global__ void __launch_bounds__(64) dbatch_head_kernel(unsigned long long *cnt, uint32_t *fault, zgpu_deflate_batch_summary *summary)
{
    const uint32_t tid = threadIdx.x;
    if (cnt && tid < kDwsCntBytes / 8) cnt[tid] = 0;
    if (fault && tid == 32) fault[0] = 0;
    if (summary && tid == 33) *summary = zgpu_deflate_batch_summary{};
}

// ---- the table check: one workgroup for the round that begins at item c0, its items dealt to the lanes in runs.  An item whose
// offsets run backwards, leave the input or lie further apart than an item may be long fails alone; ranges entry (not packed): so does one whose range runs
// backwards or leaves out_cap.  t[] gets the round's layout in the staging buffer: the exclusive sum of the served items' lengths, and the round's end ----
__global__ void __launch_bounds__(1024) dbatch_check_kernel(const uint64_t *__restrict__ in_off, uint64_t n, uint64_t in_bytes, uint32_t limit, const uint64_t *__restrict__ out_off,
                                                            uint64_t out_cap, uint32_t packed, uint64_t c0, uint32_t nb, uint64_t *__restrict__ lo_out, uint64_t *__restrict__ t,
                                                            uint32_t *__restrict__ state, unsigned long long *cnt)
{
    __shared__ uint64_t part[1024];
    const uint32_t tid = threadIdx.x, per = (nb + 1023) / 1024;
    const uint32_t a = (uint64_t)tid * per < nb ? tid * per : nb, z = (uint64_t)(tid + 1) * per < nb ? (tid + 1) * per : nb;
    uint64_t sum = 0;
    uint32_t nbad = 0, nlong = 0;
    for (uint32_t i = a; i < z; i++) {
        const uint64_t k = c0 + i, lo = in_off[k], hi = in_off[k + 1];
        bool bad = hi < lo || hi > in_bytes;
        const bool too_long = !bad && hi - lo > limit;
        if (!packed) { const uint64_t oa = out_off[k], oz = out_off[k + 1]; bad = bad || oz < oa || oz > out_cap; }
        const bool failed = bad || too_long;
        lo_out[i] = failed ? 0 : lo;
        state[i] = failed ? kItemFailed : kItemServed;
        sum += failed ? 0 : hi - lo;
        nbad += bad ? 1u : 0u; nlong += !bad && too_long ? 1u : 0u;
    }
    part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    uint64_t o = part[tid] - sum;
    for (uint32_t i = a; i < z; i++) { const uint64_t k = c0 + i; t[i] = o; o += state[i] == kItemServed ? in_off[k + 1] - in_off[k] : 0; }
    if (tid == 0) t[nb] = part[1023];
    if (nbad) atomicAdd(cnt + kDcntBadOffsets, (unsigned long long)nbad);
    if (nlong) atomicAdd(cnt + kDcntTooLong, (unsigned long long)nlong);
}

// ---- the round's served items gathered into the staging buffer, back to back: t[c] is where item c begins there.  The chunk kernels then see one monotone
// segment table, the form they have always read.  One workgroup per item; 4-byte stores aligned at the destination, the source read as it lies ----
struct __attribute__((packed, aligned(1))) GatherWord { uint32_t v; };
__global__ void __launch_bounds__(256) dbatch_gather_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ lo_tab, const uint32_t *__restrict__ state,
                                                            const uint64_t *__restrict__ t, uint32_t nb, uint8_t *__restrict__ stage)
{
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    if (c >= nb || state[c] != kItemServed) return;
    const uint64_t off = t[c];
    const uint32_t n = (uint32_t)(t[c + 1] - off); // (at most kChunkMax: the check kernel has seen to it)
    const uint8_t *src = in + lo_tab[c];
    uint8_t *dst = stage + off;
    uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
    if (head > n) head = n;
    if (tid < head) dst[tid] = src[tid];
    const uint32_t nwords = (n - head) >> 2;
    uint32_t *d32 = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t j = tid; j < nwords; j += 256) d32[j] = reinterpret_cast<const GatherWord *>(src + head + 4 * (size_t)j)->v; // (inside [0, n): nothing behind the item is read)
    const uint32_t done = head + (nwords << 2);
    if (tid < n - done) dst[done + tid] = src[done + tid];
}

// ---- packed entry: where every stream of the round begins.  One workgroup; an exclusive scan of the streams' sizes, wrapper counted in, failed items
// counting nothing, on top of the total the rounds before have left in the workspace (the carry RunState::out_total is for the blocking call) ----
__global__ void __launch_bounds__(1024) dbatch_scan_kernel(const ChunkMeta *__restrict__ meta, const uint32_t *__restrict__ state, uint64_t c0, uint32_t nb, uint32_t frame,
                                                           uint64_t *__restrict__ out_off, unsigned long long *cnt)
{
    __shared__ uint64_t part[1024];
    const uint32_t tid = threadIdx.x, per = (nb + 1023) / 1024;
    const uint32_t a = (uint64_t)tid * per < nb ? tid * per : nb, z = (uint64_t)(tid + 1) * per < nb ? (tid + 1) * per : nb;
    uint64_t sum = 0;
    for (uint32_t i = a; i < z; i++) sum += state[i] == kItemServed ? meta[i].out_bytes + frame : 0u;
    part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const uint64_t base = cnt[kDcntTotal];
    uint64_t o = base + part[tid] - sum;
    for (uint32_t i = a; i < z; i++) { out_off[c0 + i] = o; o += state[i] == kItemServed ? meta[i].out_bytes + frame : 0u; }
    __syncthreads(); // (every lane has read the total before lane 0 moves it on)
    if (tid == 0) { const uint64_t acc = base + part[1023]; cnt[kDcntTotal] = acc; out_off[c0 + nb] = acc; }
}

// ---- placement: one workgroup per item of the round.  The stream is the slot's bytes between the header and the trailer frame_kernel writes (zgpu_stitch.hip);
// it goes to out[off, off + need) when that lies inside the item's room -- the caller's range, or out_cap for the packed entry -- with stitch_kernel's copy,
// 4-byte aligned at the destination.  Lane 0 writes the record ----
__global__ void __launch_bounds__(256) dbatch_place_kernel(const uint8_t *__restrict__ slots, const ChunkMeta *__restrict__ meta, const uint32_t *__restrict__ state,
                                                           const uint64_t *__restrict__ t, const uint64_t *__restrict__ out_off, uint64_t c0,
                                                           uint32_t nb, uint8_t *out, uint64_t out_cap, uint32_t packed, uint32_t with_crc, FrameHead h, uint32_t tail,
                                                           zgpu_deflate_batch_item *items, unsigned long long *cnt)
{
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    if (c >= nb) return;
    const uint64_t k = c0 + c;
    if (state[c] != kItemServed) { // it has read nothing and occupies no output
        if (tid == 0) {
            zgpu_deflate_batch_item r{};
            r.code = ZGPU_STREAM_ERROR; r.data_type = 2; r.out_lo = packed ? out_off[k] : 0; r.adler32 = 1;
            items[k] = r;
            atomicAdd(cnt + kDcntFailed, 1ull);
        }
        return;
    }
    const ChunkMeta m = meta[c];
    const uint32_t n = m.out_bytes, need = h.n + n + tail;
    const uint64_t off = out_off[k];
    const bool fits = packed ? off + need <= out_cap : need <= out_off[k + 1] - off; // (the check kernel has kept the range inside out_cap)
    if (tid == 0) {
        zgpu_deflate_batch_item r{};
        r.code = fits ? ZGPU_OK : ZGPU_BUF_ERROR; r.data_type = m.data_type; r.out_lo = off; r.out_bytes = need;
        r.in_bytes = (uint32_t)(t[c + 1] - t[c]); r.adler32 = m.adler_a | (m.adler_b << 16); r.crc32 = with_crc ? m.crc : 0u;
        items[k] = r;
        if (!fits) atomicAdd(cnt + kDcntFailed, 1ull);
    }
    if (!fits) return;
    const uint8_t *src = slots + (size_t)c * kSlotStride;
    uint8_t *dst = out + off + h.n;
    uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
    if (head > n) head = n;
    if (tid < head) dst[tid] = src[tid];
    const uint32_t nwords = (n - head) >> 2;
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
    uint32_t *d32 = reinterpret_cast<uint32_t *>(dst + head);
    const uint32_t sh = head & 3, w0 = head >> 2;
    for (uint32_t j = tid; j < nwords; j += 256) {
        const uint32_t a = s32[w0 + j], b = s32[w0 + j + 1]; // (a slot has slack behind the longest stream: the word behind is the slot's)
        d32[j] = __builtin_amdgcn_alignbyte(b, a, sh);
    }
    const uint32_t done = head + (nwords << 2);
    if (tid < n - done) dst[done + tid] = src[done + tid];
    // header and trailer, a byte a lane (frame_kernel's bytes): BSIZE of a BGZF block is its total length - 1, at most 65328 for 65280 bytes of input
    uint8_t *d = out + off;
    if (tid < h.n) {
        uint8_t v = h.b[tid];
        if (h.bgzf && tid + 2 >= h.n) { const uint32_t bsize = need - 1; v = (uint8_t)(tid + 2 == h.n ? bsize : bsize >> 8); }
        d[tid] = v;
    }
    if (tid >= 64 && tid < 64 + tail) {
        const uint32_t i = tid - 64;
        uint8_t v;
        if (h.gzip) { const uint32_t isz = (uint32_t)(t[c + 1] - t[c]); v = (uint8_t)((i < 4 ? m.crc : isz) >> (8 * (i & 3))); }
        else { const uint32_t adler = m.adler_a | (m.adler_b << 16); v = (uint8_t)(adler >> (24 - 8 * i)); }
        d[h.n + n + i] = v;
    }
}

// ---- the call's last launch: the sort's self-check and the summary.  A raised fault word (sort4_kernel, zgpu_lz_sort.hip: the LDS did not serve an
// atomic's lanes in lane order) means that no stream of the call can be trusted: every record gets ZGPU_ERRNO.  The host cannot redo the call, it has
// returned long ago; the caller sets the engine to the exact sort (zgpu_engine_set_exact_sort) and enqueues again ----
__global__ void __launch_bounds__(256) dbatch_finish_kernel(const uint32_t *__restrict__ fault, uint64_t n, uint32_t packed, uint64_t out_cap, const unsigned long long *__restrict__ cnt,
                                                            zgpu_deflate_batch_item *items, zgpu_deflate_batch_summary *summary)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool raised = fault[0] != 0;
    if (raised && k < n) items[k].code = ZGPU_ERRNO;
    if (k == 0 && summary) {
        zgpu_deflate_batch_summary s{};
        s.nfailed = raised ? n : cnt[kDcntFailed]; s.nbad_offsets = cnt[kDcntBadOffsets]; s.ntoo_long = cnt[kDcntTooLong];
        s.total = packed ? cnt[kDcntTotal] : 0; s.overflow = packed && cnt[kDcntTotal] > out_cap ? 1u : 0u; s.sort_fault = raised ? 1u : 0u;
        *summary = s;
    }
}

// the workspace of a call carved up
struct DeflateBatchWs {
    unsigned long long *cnt; uint64_t *lo, *pre; uint32_t *state; uint8_t *stage; uint8_t *sorted; uint32_t *tokens; uint8_t *slots; ChunkMeta *meta;
    uint32_t round;
};

// What a call needs to know of its parameters, or why the chain does not serve them
struct DeflateBatchCfg { LevelCfg cfg; int impl; bool with_crc; FrameHead fh; uint32_t tail, limit; };
static const char *batch_params(const zgpu_engine *e, const zgpu_deflate_params *p, DeflateBatchCfg *bc)
{
    constexpr uint32_t kServed = ZGPU_F_FINAL | ZGPU_F_ZLIB_WRAP | ZGPU_F_GZIP_WRAP | ZGPU_F_CRC32 | ZGPU_F_BGZF_WRAP;
    if (p->level < 1 || p->level > 9) return "deflate batch: level must be 1..9";
    if (!(p->flags & ZGPU_F_FINAL)) return "deflate batch: every item is a stream of its own, ZGPU_F_FINAL is required";
    if (p->flags & ~kServed) return "deflate batch: ZGPU_F_POS0 / ZGPU_F_POS0_ALL / ZGPU_F_CONTINUOUS are not served";
    const uint32_t wrappers = (p->flags & ZGPU_F_ZLIB_WRAP ? 1 : 0) + (p->flags & ZGPU_F_GZIP_WRAP ? 1 : 0) + (p->flags & ZGPU_F_BGZF_WRAP ? 1 : 0);
    if (wrappers > 1) return "deflate batch: one wrapper at a time";
    if (p->prime) return "deflate batch: prime is not served";
    if (p->lz_impl != ZGPU_LZ_AUTO) return "deflate batch: lz_impl must be ZGPU_LZ_AUTO";
    if (p->strategy < 0 || p->strategy > (int)kFixed) return "strategy must be 0..4";
    if (p->strategy == (int)kHuffmanOnly || p->strategy == (int)kRle) return "deflate batch: Z_HUFFMAN_ONLY and Z_RLE are not served (the blocking segment call serves them)";
    if (e->geo_w != 15 || e->geo_m != 8) return "deflate batch: the default geometry only (windowBits 15, memLevel 8)";
    bc->cfg = level_cfg_for(e, p->level, p->strategy);
    if (bc->cfg.slow) {
        if (const char *why = records_refuse(bc->cfg, ZGPU_LZ_WALK)) return why;
        bc->impl = ZGPU_LZ_WALK;
    } else {
        if (!lz_fastwin_serves(bc->cfg)) return "deflate batch: levels 1-3 with their own parameters only (ZGPU_LZ_FASTWIN does not serve this deflateTune row)";
        if (const char *why = fast_refuse(bc->cfg)) return why;
        bc->impl = ZGPU_LZ_FASTWIN;
    }
    const bool wrap = p->flags & ZGPU_F_ZLIB_WRAP, bgzf = p->flags & ZGPU_F_BGZF_WRAP, gz = (p->flags & ZGPU_F_GZIP_WRAP) || bgzf;
    bc->with_crc = gz || (p->flags & ZGPU_F_CRC32);
    bc->fh = frame_head(p->level, p->strategy, wrap, gz, bgzf);
    bc->tail = gz ? 8u : wrap ? 4u : 0u;
    bc->limit = bgzf ? kBgzfBlockMax : kChunkMax;
    return nullptr;
}

static int deflate_batch_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, const zgpu_deflate_params *p, void *d_out, uint64_t out_cap,
                                 uint64_t *d_out_off, bool packed, zgpu_deflate_batch_item *d_items, zgpu_deflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes,
                                 uint32_t batch_items, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    // everything the host can judge, before anything is enqueued
    if (!p || n >= kDwsMaxItems || (n && (!d_in_off || !d_items || !d_out_off)) || (n && in_bytes && !d_in) || (n && out_cap && !d_out))
        return fail(e, ZGPU_STREAM_ERROR, "bad deflate batch arguments");
    DeflateBatchCfg bc{};
    if (const char *why = batch_params(e, p, &bc)) return fail(e, ZGPU_STREAM_ERROR, why);
    const hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    DeflateBatchWs w{};
    if (n) {
        const DeflateWsPlan pl = deflate_batch_ws_plan(n, batch_items);
        if (!d_ws || (reinterpret_cast<uintptr_t>(d_ws) & (kDwsAlign - 1)) || pl.total == 0 || ws_bytes < pl.total)
            return fail(e, ZGPU_STREAM_ERROR, "deflate batch workspace: null, not 256-byte aligned or too small");
        uint8_t *b = static_cast<uint8_t *>(d_ws);
        w.cnt = reinterpret_cast<unsigned long long *>(b + pl.cnt.off); w.lo = reinterpret_cast<uint64_t *>(b + pl.lo.off); w.pre = reinterpret_cast<uint64_t *>(b + pl.pre.off); w.stage = b + pl.stage.off;
        w.state = reinterpret_cast<uint32_t *>(b + pl.state.off); w.sorted = b + pl.sorted.off; w.tokens = reinterpret_cast<uint32_t *>(b + pl.tokens.off);
        w.slots = b + pl.slots.off; w.meta = reinterpret_cast<ChunkMeta *>(b + pl.meta.off); w.round = (uint32_t)pl.round;
    }
    int cur = -1; // (the engine supplies the device; a thread that is on it already -- a stream capture, say -- is left alone)
    ZGPU_HIP_CHECK(hipGetDevice(&cur));
    if (cur != e->device) ZGPU_HIP_CHECK(hipSetDevice(e->device));
    if (n == 0) { // at most the summary is written
        if (d_summary) hipLaunchKernelGGL(dbatch_head_kernel, dim3(1), dim3(64), 0, st, static_cast<unsigned long long *>(nullptr), static_cast<uint32_t *>(nullptr), d_summary);
        ZGPU_HIP_CHECK(hipGetLastError());
        return ZGPU_OK;
    }
    // the head of the chain: counters, fault word and summary cleared
    uint32_t *const fault = lz_sorted_fault_word(w.sorted);
    hipLaunchKernelGGL(dbatch_head_kernel, dim3(1), dim3(64), 0, st, w.cnt, fault, d_summary);
    const uint32_t ngrid = (uint32_t)((n + 255) / 256);
    ChunkGeom g{}; // the chunk kernels' view of a round: the staging buffer under a monotone table, chunk c = item c0 + c
    g.in = w.stage; g.in_bytes = (uint64_t)w.round * kDwsStageBytes; g.chunk_size = kChunkMax;
    g.final_chunk = ~0ull; g.all_final = 1; g.block_tokens = kBlockTokens; g.slot_stride = kSlotStride;
    const uint32_t frame = bc.fh.n + bc.tail;
    // the rounds, one behind the other in the same regions
    for (uint64_t c0 = 0; c0 < n; c0 += w.round) {
        const uint32_t nb = (uint32_t)(n - c0 < w.round ? n - c0 : w.round);
        const uint64_t *const t = w.pre; // the round's nb + 1 entries
        g.seg_off = t; g.chunk0 = 0; g.nchunks = nb;
        hipLaunchKernelGGL(dbatch_check_kernel, dim3(1), dim3(1024), 0, st, d_in_off, n, in_bytes, bc.limit, d_out_off, out_cap, packed ? 1u : 0u, c0, nb, w.lo, w.pre, w.state, w.cnt);
        hipLaunchKernelGGL(dbatch_gather_kernel, dim3(nb), dim3(256), 0, st, static_cast<const uint8_t *>(d_in), w.lo, w.state, t, nb, w.stage);
        const bool adler_done = launch_lz_sorted(g, bc.cfg, w.sorted, w.tokens, w.meta, st, nullptr, e->exact_sort, bc.impl); // (no engine: no stage timer, no event)
        launch_huffman(g, w.tokens, w.meta, w.slots, st, bc.cfg.strategy == kFixed);
        if (!adler_done) launch_adler(g, w.meta, st);
        if (bc.with_crc) launch_crc(g, w.meta, st);
        if (packed) hipLaunchKernelGGL(dbatch_scan_kernel, dim3(1), dim3(1024), 0, st, w.meta, w.state, c0, nb, frame, d_out_off, w.cnt);
        hipLaunchKernelGGL(dbatch_place_kernel, dim3(nb), dim3(256), 0, st, w.slots, w.meta, w.state, t, d_out_off, c0, nb, static_cast<uint8_t *>(d_out), out_cap,
                           packed ? 1u : 0u, bc.with_crc ? 1u : 0u, bc.fh, bc.tail, d_items, w.cnt);
    }
    hipLaunchKernelGGL(dbatch_finish_kernel, dim3(ngrid), dim3(256), 0, st, fault, n, packed ? 1u : 0u, out_cap, w.cnt, d_items, d_summary);
    ZGPU_HIP_CHECK(hipGetLastError());
    return ZGPU_OK;
}

} // namespace zgpu

using namespace zgpu;

extern "C" {
#pragma GCC visibility push(default)

uint64_t zgpu_deflate_batch_workspace_bytes(uint64_t n, uint32_t batch_items) { return deflate_batch_ws_bytes(n, batch_items); }

int zgpu_deflate_batch_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, const zgpu_deflate_params *p, void *d_out,
                               uint64_t out_cap, const uint64_t *d_out_offsets, zgpu_deflate_batch_item *d_items, zgpu_deflate_batch_summary *d_summary, void *d_ws,
                               uint64_t ws_bytes, uint32_t batch_items, void *hip_stream)
{
    // (the ranges are read only: the one routine takes the table as the packed entry's, which it writes)
    return deflate_batch_enqueue(e, d_in, in_bytes, d_in_offsets, n, p, d_out, out_cap, const_cast<uint64_t *>(d_out_offsets), false, d_items, d_summary, d_ws, ws_bytes, batch_items,
                                 hip_stream);
}

int zgpu_deflate_batch_packed_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, const zgpu_deflate_params *p, void *d_out,
                                      uint64_t out_cap, uint64_t *d_out_offsets, zgpu_deflate_batch_item *d_items, zgpu_deflate_batch_summary *d_summary, void *d_ws,
                                      uint64_t ws_bytes, uint32_t batch_items, void *hip_stream)
{
    return deflate_batch_enqueue(e, d_in, in_bytes, d_in_offsets, n, p, d_out, out_cap, d_out_offsets, true, d_items, d_summary, d_ws, ws_bytes, batch_items, hip_stream);
}

int zgpu_engine_set_exact_sort(zgpu_engine *e, int on)
{
    if (!e) return ZGPU_STREAM_ERROR;
    e->exact_sort = on != 0; // (the field deflate_device sets when a blocking call's self-check fails; zgpu_debug_sort_fallback reports it)
    return ZGPU_OK;
}

#pragma GCC visibility pop
} // extern "C"
