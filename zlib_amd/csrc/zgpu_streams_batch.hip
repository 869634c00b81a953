// zgpu_streams_batch.hip -- the plan of the stream-ordered batch compress of items of any length, made on the DEVICE (zgpu_deflate_streams_enqueue.hip is the
// host side, zgpu_deflate_streams_plan.h has the arithmetic, which these kernels call lane by lane and the CPU model calls in loops).  The blocking call reads
// its tables and plans on the host (streams_run, zgpu_deflate_streams.hip); a stream-ordered call may not, so here are
//   senq_clear_kernel    the head of the chain: counters, the sort's fault word and the summary start from zero
//   senq_scan_kernel     every table entry judged (state[k]), tile0[0..n] = the tiles in front of every item, piece0[0..n] = the checksum pieces likewise
//   senq_rows_kernel     the TileRow of every tile of the padded list (rows behind the real tiles: streams_pad_row)
//   senq_round_kernel    per round of tiles: its parts (StreamsRoundPart) and their number, the real tiles, the block slots in use
//   streams_pad_kernel   per round: a padding row's exit row (all 0) and its record (no tokens), which the kernels that leave at their top do not write
//   senq_layout_kernel   zgpu_deflate_streams_layout_enqueue: the rooms of a table on the device
//   senq_summary_kernel  the call's last launch: the sort's self-check and the summary
// No kernel waits for another workgroup; the scans are one workgroup each, looped (a call has up to 2^32 items, a round up to 32,768 tiles).
#include "zgpu_common.h"
#include "zgpu_engine.h"
#include "zgpu_deflate_streams_plan.h"
#include "zgpu_deflate_batch_plan.h"

namespace zgpu {

static_assert(sizeof(TileRow) == 32 && sizeof(ContState) == 64 && sizeof(ContBlk) == 56 && sizeof(StreamsRoundPart) == 32 && sizeof(zgpu_check_item) == 8,
              "senq_ws_plan's comment states what a tile and an item cost");
static_assert(kSenqSortedChunk == kDwsSortedChunk && kSenqSortedOnce == kDwsSortedHeader + kDwsSortedSlack, "the sorted buckets' workspace (zgpu_lz_sorted.h asserts the other header's numbers)");

// A kernel, not hipMemsetAsync: the comment above dbatch_head_kernel (zgpu_deflate_batch.hip) records what memsets did in a replayed graph
__global__ void __launch_bounds__(64) senq_clear_kernel(unsigned long long *cnt, uint32_t *fault, zgpu_deflate_batch_summary *summary)
{
    const uint32_t tid = threadIdx.x;
    if (cnt && tid < 32) cnt[tid] = 0;
    if (fault && tid == 32) fault[0] = 0;
    if (summary && tid == 33) *summary = zgpu_deflate_batch_summary{};
}

// exclusive scan of one value a lane over the workgroup's 1024 lanes; *total: the sum.  Every lane calls it
__device__ inline uint64_t scan1024(uint64_t *part, uint32_t tid, uint64_t v, uint64_t *total)
{
    __syncthreads(); // (part may still be read from the scan before)
    part[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    *total = part[1023];
    return part[tid] - v;
}

// one workgroup, its items dealt to the lanes in runs: senq_tile_scan (zgpu_deflate_streams_plan.h) with a scan in place of the running sums
__global__ void __launch_bounds__(1024) senq_scan_kernel(const uint64_t *__restrict__ in_off, const uint64_t *__restrict__ oo, uint64_t n, uint64_t in_bytes, uint64_t out_cap,
                                                         uint32_t *__restrict__ state, uint64_t *__restrict__ tile0, uint64_t *__restrict__ piece0, unsigned long long *cnt)
{
    __shared__ uint64_t part[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n + 1023) / 1024, a = tid * per < n ? tid * per : n, z = (tid + 1) * per < n ? (tid + 1) * per : n, m = senq_ntiles_max(n, in_bytes);
    // the tiles asked for, as if every item with good offsets were served
    uint64_t sum = 0, total;
    for (uint64_t k = a; k < z; k++) sum += senq_item_tiles(senq_item_state(in_off[k], in_off[k + 1], in_bytes, oo[k], oo[k + 1], out_cap), in_off[k], in_off[k + 1]);
    uint64_t asked = scan1024(part, tid, sum, &total);
    // the states; the tiles and pieces of the served
    uint64_t nt_sum = 0, pc_sum = 0;
    uint32_t nbad = 0, nlong = 0;
    for (uint64_t k = a; k < z; k++) {
        uint32_t s = senq_item_state(in_off[k], in_off[k + 1], in_bytes, oo[k], oo[k + 1], out_cap);
        const uint64_t nt = senq_item_tiles(s, in_off[k], in_off[k + 1]);
        asked += nt;
        if (!senq_item_fits(nt, asked, m)) s = kSenqBad;
        state[k] = s;
        if (s == kSenqServed) { nt_sum += nt; pc_sum += senq_item_pieces(in_off[k + 1] - in_off[k]); }
        nbad += s == kSenqBad ? 1u : 0u; nlong += s == kSenqTooLong ? 1u : 0u;
    }
    uint64_t ntiles, npieces;
    uint64_t at = scan1024(part, tid, nt_sum, &ntiles), pc = scan1024(part, tid, pc_sum, &npieces);
    for (uint64_t k = a; k < z; k++) {
        tile0[k] = at; piece0[k] = pc;
        if (state[k] == kSenqServed) { const uint64_t L = in_off[k + 1] - in_off[k]; at += streams_ntiles(L); pc += senq_item_pieces(L); }
    }
    if (tid == 0) { tile0[n] = ntiles; piece0[n] = npieces; }
    if (nbad) atomicAdd(cnt + kScntBadOffsets, (unsigned long long)nbad);
    if (nlong) atomicAdd(cnt + kScntTooLong, (unsigned long long)nlong);
}

// a lane per tile of the padded list
__global__ void __launch_bounds__(256) senq_rows_kernel(const uint64_t *__restrict__ in_off, const uint64_t *__restrict__ tile0, uint64_t n, uint64_t nrows, TileRow *__restrict__ rows)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < nrows) rows[t] = senq_tile_row(in_off, tile0, n, t);
}

// one workgroup: the round [t0, t0 + batch) of the padded list.  streams_round_plan with a scan in place of the running sums: a part begins at a tile
__global__ void __launch_bounds__(1024) senq_round_kernel(const uint64_t *__restrict__ tile0, uint64_t n, uint64_t t0, uint32_t batch, StreamsRoundPart *__restrict__ parts,
                                                          StreamsRound *__restrict__ round)
{
    __shared__ uint64_t part[1024];
    const uint32_t tid = threadIdx.x, nreal = streams_round_real(tile0[n], t0, batch), per = (nreal + 1023) / 1024;
    const uint32_t a = tid * per < nreal ? tid * per : nreal, z = (tid + 1) * per < nreal ? (tid + 1) * per : nreal;
    uint64_t tj = 0, blk = 0; // tokens | parts << 32 (a round's tokens stay below 2^32: kSenqMaxBatch), block slots
    StreamsRoundPart p;
    for (uint32_t c = a; c < z; c++)
        if (streams_part_at(tile0, n, t0, nreal, c, &p)) { tj += streams_tok_cap(p.nt) + (1ull << 32); blk += p.nblk_cap; }
    uint64_t tj_all, blk_all;
    uint64_t tj0 = scan1024(part, tid, tj, &tj_all), b0 = scan1024(part, tid, blk, &blk_all);
    for (uint32_t c = a; c < z; c++)
        if (streams_part_at(tile0, n, t0, nreal, c, &p)) {
            p.toff = (uint32_t)tj0; p.j = (uint32_t)(tj0 >> 32); p.boff = (uint32_t)b0;
            parts[p.j] = p;
            tj0 += streams_tok_cap(p.nt) + (1ull << 32); b0 += p.nblk_cap;
        }
    if (tid == 0) *round = StreamsRound{(uint32_t)(tj_all >> 32), nreal, (uint32_t)blk_all, (uint32_t)tj_all};
}

// a workgroup per tile of the round: what sort, walkers and parse leave unwritten for a padding row -- a defined exit row (the chain of entries runs over
// padded tiles too) and a record without tokens
__global__ void __launch_bounds__(256) streams_pad_kernel(const TileRow *__restrict__ rows, uint16_t *__restrict__ exits, ChunkMeta *__restrict__ meta)
{
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    if (!streams_row_is_pad(rows[c])) return;
    uint32_t *ex = reinterpret_cast<uint32_t *>(exits + (size_t)c * kTileExitStride); // (kTileExitStride is even and a row 4-byte aligned)
    for (uint32_t i = tid; i < kTileExitStride / 2; i += 256) ex[i] = 0;
    if (tid == 0) meta[c] = ChunkMeta{};
}

// zgpu_deflate_streams_layout_enqueue: oo[k] = the exclusive sum of the entries' rooms (senq_room), oo[n] the total
__global__ void __launch_bounds__(1024) senq_layout_kernel(const uint64_t *__restrict__ in_off, uint64_t n, uint64_t in_bytes, uint32_t flags, uint64_t *__restrict__ oo)
{
    __shared__ uint64_t part[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n + 1023) / 1024, a = tid * per < n ? tid * per : n, z = (tid + 1) * per < n ? (tid + 1) * per : n;
    uint64_t sum = 0, total;
    for (uint64_t k = a; k < z; k++) sum += senq_room(in_off[k], in_off[k + 1], in_bytes, flags);
    uint64_t at = scan1024(part, tid, sum, &total);
    for (uint64_t k = a; k < z; k++) { oo[k] = at; at += senq_room(in_off[k], in_off[k + 1], in_bytes, flags); }
    if (tid == 0) oo[n] = total;
}

// the call's last launch.  A raised fault word (sort4_kernel's self-check) means that no stream of the call can be trusted: every record gets ZGPU_ERRNO; the
// caller sets the engine to the exact sort and enqueues again (dbatch_finish_kernel, zgpu_deflate_batch.hip, has the same contract)
__global__ void __launch_bounds__(256) senq_summary_kernel(const uint32_t *__restrict__ fault, uint64_t n, const unsigned long long *__restrict__ cnt, zgpu_deflate_batch_item *items,
                                                           zgpu_deflate_batch_summary *summary)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool raised = fault[0] != 0;
    if (raised && k < n) items[k].code = ZGPU_ERRNO;
    if (k == 0 && summary) {
        zgpu_deflate_batch_summary s{};
        s.nfailed = raised ? n : cnt[kScntFailed]; s.nbad_offsets = cnt[kScntBadOffsets]; s.ntoo_long = cnt[kScntTooLong];
        s.total = cnt[kScntTotal]; s.overflow = 0; s.sort_fault = raised ? 1u : 0u;
        *summary = s;
    }
}

void launch_senq_clear(unsigned long long *cnt, uint32_t *fault, zgpu_deflate_batch_summary *summary, hipStream_t s)
{
    hipLaunchKernelGGL(senq_clear_kernel, dim3(1), dim3(64), 0, s, cnt, fault, summary);
}
void launch_senq_scan(const uint64_t *in_off, const uint64_t *oo, uint64_t n, uint64_t in_bytes, uint64_t out_cap, uint32_t *state, uint64_t *tile0, uint64_t *piece0,
                      unsigned long long *cnt, hipStream_t s)
{
    hipLaunchKernelGGL(senq_scan_kernel, dim3(1), dim3(1024), 0, s, in_off, oo, n, in_bytes, out_cap, state, tile0, piece0, cnt);
}
void launch_senq_rows(const uint64_t *in_off, const uint64_t *tile0, uint64_t n, uint64_t nrows, TileRow *rows, hipStream_t s)
{
    if (nrows) hipLaunchKernelGGL(senq_rows_kernel, dim3((uint32_t)((nrows + 255) / 256)), dim3(256), 0, s, in_off, tile0, n, nrows, rows);
}
void launch_senq_round(const uint64_t *tile0, uint64_t n, uint64_t t0, uint32_t batch, const TileRow *rows, StreamsRoundPart *parts, StreamsRound *round, uint16_t *exits, ChunkMeta *meta,
                       hipStream_t s)
{
    hipLaunchKernelGGL(senq_round_kernel, dim3(1), dim3(1024), 0, s, tile0, n, t0, batch, parts, round);
    hipLaunchKernelGGL(streams_pad_kernel, dim3(batch), dim3(256), 0, s, rows, exits, meta);
}
void launch_senq_layout(const uint64_t *in_off, uint64_t n, uint64_t in_bytes, uint32_t flags, uint64_t *oo, hipStream_t s)
{
    hipLaunchKernelGGL(senq_layout_kernel, dim3(1), dim3(1024), 0, s, in_off, n, in_bytes, flags, oo);
}
void launch_senq_summary(const uint32_t *fault, uint64_t n, const unsigned long long *cnt, zgpu_deflate_batch_item *items, zgpu_deflate_batch_summary *summary, hipStream_t s)
{
    hipLaunchKernelGGL(senq_summary_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, fault, n, cnt, items, summary);
}

} // namespace zgpu
