// zgpu_cont.hip -- ONE continuous deflate stream of any size on the device: what plain compress2() / deflate(Z_NO_FLUSH ... Z_FINISH) of the reference emits
// (round 4).  The reference slides a 32 KiB window through the whole input (qcsrc/deflate.c:1266-1358), its matches cross every 64 KiB
// boundary (deflate.c:1027-1168), its lazy parse is one serial chain (deflate.c:1554-1674), blocks are cut every 16383 tokens counted from the start of the
// stream (h/deflate.h:313), a block may be stored only while its first byte is still in the window (deflate.c:1364-1367) and blocks follow each other bit
// by bit (trees.c:217-229).  None of that splits into independent 64 KiB chunks; all of it splits into TILES plus four small serial chains:
//
//   tile i   = the 64 KiB of input that start at 32512 * i: it parses its local positions [h0, h1) = [32512, 65024) with the 32512 bytes in front as
//              history (MAX_DIST = 32506) and 512 bytes behind for the lazy game and the lookahead of its last positions (tests/tools/cont_tile_model.c
//              is this decomposition on the CPU, byte-identical with the reference's loop).  sort4_kernel (zgpu_lz_sort.hip) and walk_kernel<2> (zgpu_lz_walk.hip) work
//              on a tile as they work on a chunk; every quantity the reference keeps in window coordinates is a function of the absolute position here.
//   chain 1  where the parse ENTERS each tile: a tile's walkers start from every possible entry (513 of them), tile_exits() turns their games into the
//              tile's exit as a function of its entry, and the entries are the composition of those functions along the tiles: chain_*_kernel, groups of
//              256 tiles composed side by side, one short serial chain over the groups.
//   chain 2  which tokens make a BLOCK: a prefix sum of the tiles' token counts; the tokens are copied into one array (cont_compact_kernel), block b is
//              tokens [16383 b, 16383 (b + 1)) of it, and the tile that holds a block's last token says where the block ends in the input.
//   chain 3  where each block STARTS in the output, a bit position: a block's size depends on the phase it starts at only when it is stored (the padding
//              in front of LEN), so the scan runs over functions of the phase (cont_bitscan_kernel).  huffman_kernel<true> codes every block from bit 0 of
//              a slot of its own; cont_stitch_kernel shifts it into place (stored blocks: straight from the input).
//   chain 4  from one batch of tiles to the next, and from one feed of a stream to the next: ContState + the tokens of the block that is still filling.
#include "zgpu_common.h"
#include "zgpu_engine.h"
#include "../../include/zamd_gpu.h"
#include "zgpu_deflate_streams_plan.h"

namespace zgpu {

// ------------------------------------------------------------------------------------------------- chain 1: entries
constexpr uint32_t kChainGroup = 256;

__global__ void __launch_bounds__(576) chain_compose_kernel(const uint16_t *__restrict__ exits, uint32_t ntiles, uint16_t *__restrict__ comp)
{
    const uint32_t g = blockIdx.x, k = threadIdx.x, t0 = g * kChainGroup, t1 = t0 + kChainGroup < ntiles ? t0 + kChainGroup : ntiles;
    uint32_t v = k < kTileEntries ? k : 0;
    for (uint32_t t = t0; t < t1; t++) v = exits[(size_t)t * kTileExitStride + v];
    if (k < kTileExitStride) comp[(size_t)g * kTileExitStride + k] = (uint16_t)v;
}
__global__ void __launch_bounds__(64) chain_serial_kernel(const uint16_t *__restrict__ comp, uint32_t ngroups, uint16_t *__restrict__ gentry, const uint16_t *__restrict__ first)
{
    if (threadIdx.x != 0) return;
    uint32_t v = *first;
    for (uint32_t g = 0; g < ngroups; g++) { gentry[g] = (uint16_t)v; if (g + 1 < ngroups) v = comp[(size_t)g * kTileExitStride + v]; }
}
// entry[t] for the tiles of the launch; entry[ntiles] = the entry of the tile behind them (the next batch's first, or where the feed's parse ends)
__global__ void __launch_bounds__(64) chain_apply_kernel(const uint16_t *__restrict__ exits, uint32_t ntiles, const uint16_t *__restrict__ gentry, uint16_t *__restrict__ entry)
{
    if (threadIdx.x != 0) return;
    const uint32_t g = blockIdx.x, t0 = g * kChainGroup, t1 = t0 + kChainGroup < ntiles ? t0 + kChainGroup : ntiles;
    uint32_t v = gentry[g];
    for (uint32_t t = t0; t < t1; t++) { entry[t] = (uint16_t)v; v = exits[(size_t)t * kTileExitStride + v]; }
    if (t1 == ntiles) entry[ntiles] = (uint16_t)v;
}

// ------------------------------------------------------------------------------------------------- chain 2: tokens -> blocks
// exclusive scan of the tiles' token counts behind the carried tokens (which become the front of the compact array)
// (the bodies of the block layer's kernels are functions of the per-stream arguments: the kernels below call them with the host's arguments, the batched
// kernels at the end of the file with arguments read from a part of a round.  NT: lanes of the workgroup, 1024 in the one-stream kernels)
template <uint32_t NT>
__device__ __forceinline__ void cont_tokscan_body(const ChunkMeta *__restrict__ tmeta, uint32_t ntiles, ContState *st, uint32_t *__restrict__ tokoff,
                                                  const uint32_t *__restrict__ carry, uint32_t *__restrict__ T)
{
    __shared__ uint32_t part[NT];
    const uint32_t tid = threadIdx.x, per = (ntiles + NT - 1) / NT;
    const uint32_t a = tid * per < ntiles ? tid * per : ntiles, z = (tid + 1) * per < ntiles ? (tid + 1) * per : ntiles;
    uint32_t sum = 0;
    for (uint32_t i = a; i < z; i++) sum += tmeta[i].ntok;
    part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < NT; d <<= 1) {
        const uint32_t add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const uint32_t cn = st->carry_n;
    uint32_t o = cn + part[tid] - sum;
    for (uint32_t i = a; i < z; i++) { tokoff[i] = o; o += tmeta[i].ntok; }
    for (uint32_t j = tid; j < cn; j += NT) T[j] = carry[j];
    if (tid == NT - 1) { tokoff[ntiles] = cn + part[NT - 1]; st->total = cn + part[NT - 1]; }
}
__global__ void __launch_bounds__(1024) cont_tokscan_kernel(const ChunkMeta *__restrict__ tmeta, uint32_t ntiles, ContState *st, uint32_t *__restrict__ tokoff,
                                                            const uint32_t *__restrict__ carry, uint32_t *__restrict__ T)
{
    cont_tokscan_body<1024>(tmeta, ntiles, st, tokoff, carry, T);
}

// a tile's tokens to their place in the compact array; for every block whose LAST token lies in this tile: where the block ends, how long that token is
constexpr uint32_t kMaxCuts = 6; // ceil(65536 / 16383) + 1
__global__ void __launch_bounds__(256) cont_compact_kernel(ChunkGeom g, TileGeom tg, const uint32_t *__restrict__ tokens, const ChunkMeta *__restrict__ tmeta,
                                                           const uint32_t *__restrict__ tokoff, uint32_t *__restrict__ T, ContBlk *__restrict__ blk)
{
    const uint32_t c = blockIdx.x;
#include "zgpu_cont_compact_body.inc"
}

// slides of the reference's window that have happened when its loop stands at stream position ptop (deflate.c:1293: strstart >= wsize + MAX_DIST inside
// fill_window, which is called while lookahead < MIN_LOOKAHEAD): slide k at the first loop top >= 32768 (k - 1) + 65275 -- or one position earlier when
// that position, sp, lies in the last 261 bytes in front of a segment's end (less than MIN_LOOKAHEAD left: fill_window is called at every loop top there).
__host__ __device__ inline uint64_t cont_slides(uint64_t ptop, uint64_t sp)
{
    return (ptop >= 65275u ? (ptop - 65275u) / 32768u + 1u : 0u) + (ptop == sp ? 1u : 0u);
}
// (sp for a segment that ends at stream position n: cont_special, zgpu_deflate_plan.h)

// the batch's blocks.  seg_end: the stream position the segment ends at when this batch reaches it (the block that is filling is closed there), ~0: more follows
// b: the block slot of the stream; true: it holds a block of this batch
__device__ __forceinline__ bool cont_table_body(uint32_t b, ContBlk *__restrict__ blk, ContState *st, const uint32_t *__restrict__ T, uint64_t seg_end, uint32_t final_block,
                                                uint64_t sp, uint32_t nblk_cap, uint32_t slow)
{
    const uint32_t total = st->total;
    uint32_t nblk = total / kBlockTokens;
    if (seg_end != ~0ull) {
        // deflate_slow tallies the last byte's pending literal BEHIND its loop without looking at "buffer full" (deflate.c:1660-1665): when that literal fills the
        // block, the full block is the segment's last; any other token that fills a block is followed by one more (possibly empty) block at the flush
        // (deflate_fast has no such literal: its last token is tallied inside the loop, deflate.c:1524-1541)
        const bool full_last = slow && total != 0 && total % kBlockTokens == 0 && (T[total - 1] >> 8) == 0;
        if (!full_last) nblk++;
    }
    if (nblk > nblk_cap) nblk = nblk_cap; // (cannot happen: the capacity is computed from the positions of the batch)
    if (b == 0) st->nblk = nblk;
    if (b >= nblk) return false;
    ContBlk &k = blk[b];
    k.tok0 = b * kBlockTokens;
    const bool complete = (uint64_t)(b + 1) * kBlockTokens <= total;
    k.nt = complete ? kBlockTokens : total - k.tok0;
    if (!complete) { k.end_pos = seg_end; k.last_len = 1; }          // the flush at the segment's end: the loop stands at the end itself
    else if (seg_end != ~0ull && b + 1 == nblk) k.last_len = 1;       // (the full last block: flushed behind the loop as well; its end_pos IS seg_end)
    k.start_pos = b == 0 ? st->block_start : blk[b - 1].end_pos;
    k.eof = final_block && b + 1 == nblk;
    k.first = st->first_block && b == 0;
    // where the loop stood when the block was flushed: deflate_slow emits a token one iteration late (the match of position m while it stands at m + 1,
    // deflate.c:1617-1640; a literal likewise, :1644-1656), deflate_fast in the iteration of the token's own position (:1499-1541); at a segment's end both
    // flush behind the loop, which stands at the end then (last_len is 1 there and end_pos the end: the slow formula)
    const uint64_t ptop = k.end_pos - k.last_len + ((slow || !complete) ? 1 : 0);
    k.nostore = k.start_pos < 32768u * cont_slides(ptop, sp);
    k.nbits = 0; k.btype = 0; k.stored_len = 0; k.eob_len = 8;
    return true;
}
__global__ void __launch_bounds__(256) cont_table_kernel(ContBlk *__restrict__ blk, ContState *st, const uint32_t *__restrict__ T, uint64_t seg_end, uint32_t final_block,
                                                         uint64_t sp, uint32_t nblk_cap, uint32_t slow)
{
    cont_table_body(blockIdx.x * 256 + threadIdx.x, blk, st, T, seg_end, final_block, sp, nblk_cap, slow);
}

// ------------------------------------------------------------------------------------------------- chain 3: bit positions
__device__ inline uint64_t blk_advance(uint64_t pos, const ContBlk &k)
{
    return k.btype ? pos + k.nbits : ((pos + 3 + 7) & ~7ull) + 32 + 8ull * k.stored_len; // trees.c:867-879: 3 header bits, bi_windup, LEN, NLEN, the bytes
}
template <uint32_t NT>
__device__ __forceinline__ void cont_bitscan_body(const ContBlk *__restrict__ blk, ContState *st, uint64_t *__restrict__ pos, uint64_t out_cap_bits)
{
    __shared__ uint32_t adv[NT][8];
    __shared__ uint64_t segpos[NT + 1];
    const uint32_t tid = threadIdx.x, nblk = st->nblk, per = (nblk + NT - 1) / NT;
    const uint32_t a = tid * per < nblk ? tid * per : nblk, z = (tid + 1) * per < nblk ? (tid + 1) * per : nblk;
    for (uint32_t ph = 0; ph < 8; ph++) {
        uint64_t p = ph;
        for (uint32_t i = a; i < z; i++) p = blk_advance(p, blk[i]);
        adv[tid][ph] = (uint32_t)(p - ph);
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t p = st->out_bits;
        for (uint32_t s = 0; s < NT; s++) { segpos[s] = p; p += adv[s][p & 7]; }
        segpos[NT] = p;
        st->out_bits = p;
        pos[nblk] = p;
        if (p > out_cap_bits) st->overflow = 1;
    }
    __syncthreads();
    uint64_t p = segpos[tid];
    for (uint32_t i = a; i < z; i++) { pos[i] = p; p = blk_advance(p, blk[i]); }
}
__global__ void __launch_bounds__(1024) cont_bitscan_kernel(const ContBlk *__restrict__ blk, ContState *st, uint64_t *__restrict__ pos, uint64_t out_cap_bits)
{
    cont_bitscan_body<1024>(blk, st, pos, out_cap_bits);
}

// A word of the output belongs to one block alone when all its 32 bits do: such words are stored.  A word that holds a block boundary is ORed into by
// every block that has bits in it, and is cleared here first -- except the word the batch starts in when earlier bits (the batch before, the stream's
// header, the bits a flush left over) are in it already.
__device__ inline bool word_is_inner(uint64_t w, uint64_t D, uint64_t E) { return 32 * w >= D && 32 * w + 32 <= E; }
__device__ __forceinline__ void cont_edges_body(uint32_t b, const ContState *st, const uint64_t *__restrict__ pos, uint32_t *__restrict__ out, uint64_t out_words)
{
    const uint32_t nblk = st->nblk;
    if (b >= nblk) return;
    const uint64_t D = pos[b], E = pos[b + 1];
    if (E == D) return;
    const uint64_t wf = D >> 5, wl = (E - 1) >> 5, keep = (pos[0] & 31) ? pos[0] >> 5 : ~0ull; // the word the batch starts in, when it is not empty
    if (!word_is_inner(wf, D, E) && wf != keep && wf < out_words) out[wf] = 0;
    if (wl != wf && !word_is_inner(wl, D, E) && wl < out_words) out[wl] = 0;
}
__global__ void __launch_bounds__(256) cont_edges_kernel(const ContState *st, const uint64_t *__restrict__ pos, uint32_t *__restrict__ out, uint64_t out_words)
{
    cont_edges_body(blockIdx.x * 256 + threadIdx.x, st, pos, out, out_words);
}
__global__ void __launch_bounds__(256) cont_stitch_kernel(const ContBlk *__restrict__ blk, const ContState *st, const uint64_t *__restrict__ pos, const uint8_t *__restrict__ slots,
                                                          uint32_t slot_stride, const uint8_t *__restrict__ in, uint64_t abs0, uint32_t *__restrict__ out, uint64_t out_words)
{
    const uint32_t b = blockIdx.x;
#include "zgpu_cont_stitch_body.inc"
}

// ------------------------------------------------------------------------------------------------- chain 4: to the next batch
// the tokens behind the last emitted block wait in the carry buffer; the state moves on.  seg_end as in cont_table_kernel.
template <uint32_t NT>
__device__ __forceinline__ void cont_carry_body(const ContBlk *__restrict__ blk, ContState *st, const uint32_t *__restrict__ T, uint32_t *__restrict__ carry, uint64_t seg_end)
{
    const uint32_t tid = threadIdx.x, nblk = st->nblk, total = st->total, old_carry = st->carry_n;
    const uint32_t used = seg_end != ~0ull ? total : nblk * kBlockTokens, rem = total - used;
    for (uint32_t j = tid; j < rem; j += NT) carry[j] = T[used + j];
    __syncthreads();
    if (tid == 0) {
        st->ntokens += total - old_carry;
        st->carry_n = rem;
        if (nblk) { st->block_start = blk[nblk - 1].end_pos; st->last_eob = blk[nblk - 1].eob_len; st->first_block = 0; }
        if (seg_end != ~0ull) st->block_start = seg_end;
    }
}
__global__ void __launch_bounds__(1024) cont_carry_kernel(const ContBlk *__restrict__ blk, ContState *st, const uint32_t *__restrict__ T, uint32_t *__restrict__ carry, uint64_t seg_end)
{
    cont_carry_body<1024>(blk, st, T, carry, seg_end);
}

// ------------------------------------------------------------------------------------------------- the block layer of MANY streams, batched
// Both batch calls over many streams use this: the seven scans above as seven launches over ALL parts of a round of tiles, whatever the number of
// streams.  A part (StreamsRoundPart, zgpu_deflate_streams_plan.h) is one stream's tiles in the round; the bodies above get the arguments a one-stream
// launch would get from the host, read from the part (streams_part_args) -- part blockIdx.x for the three scans, the part found for a tile or a block
// slot for the others.  The blocking call (zgpu_deflate_streams.hip) plans the rounds on the host, uploads parts and records and launches at the exact
// extents; the stream-ordered call (zgpu_deflate_streams_enqueue.hip) has them made on the device (senq_round_kernel, zgpu_streams_batch.hip) and
// launches at the host's upper bounds, a part per tile and kSenqBlkPerTile block slots per tile.  What belongs to nobody leaves at the top, uniformly
// per workgroup where a barrier follows.
constexpr uint32_t kBatchScan = 256; // lanes of the batched scans: most parts have a handful of tiles and blocks, a lane of a long part takes a run of them

struct PartView { // a part with its stream's arguments
    StreamsRoundPart p; StreamsPartArgs a; uint64_t in_lo, out_lo, out_words;
};
__device__ __forceinline__ PartView part_view(const ContBatch &q, uint32_t j)
{
    PartView v;
    v.p = q.parts[j];
    const uint64_t k = v.p.item;
    v.in_lo = q.in_off[k];
    v.a = streams_part_args(v.p, q.in_off[k + 1] - v.in_lo, q.tile0[k], q.t0);
    v.out_lo = q.oo[k];
    v.out_words = streams_room_cap(q.oo[k + 1] - v.out_lo, q.flags) >> 2;
    return v;
}
// the last part with key <= x (x below the round's extent: there is one)
__device__ __forceinline__ uint32_t part_of_tile(const ContBatch &q, uint32_t nparts, uint32_t c)
{
    uint32_t lo = 0, hi = nparts;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (q.parts[mid].c0 <= c) lo = mid; else hi = mid; }
    return lo;
}
__device__ __forceinline__ uint32_t part_of_slot(const ContBatch &q, uint32_t nparts, uint32_t s)
{
    uint32_t lo = 0, hi = nparts;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (q.parts[mid].boff <= s) lo = mid; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(kBatchScan) cont_tokscan_batch_kernel(ContBatch q)
{
    if (blockIdx.x >= q.round->nparts) return;
    const PartView v = part_view(q, blockIdx.x);
    cont_tokscan_body<kBatchScan>(q.tmeta + v.p.c0, v.p.nt, q.st + v.p.item, q.tokoff + v.p.c0 + v.p.j, q.carry, q.T + v.p.toff);
}
__global__ void __launch_bounds__(256) cont_compact_batch_kernel(ContBatch q)
{
    const StreamsRound r = *q.round;
    if (blockIdx.x >= r.nreal) return;
    const PartView v = part_view(q, part_of_tile(q, r.nparts, blockIdx.x));
    ChunkGeom g{}; TileGeom tg{};
    g.in = q.in + v.in_lo; g.in_bytes = v.a.L; g.chunk_size = kChunkMax; g.final_chunk = ~0ull; g.block_tokens = kBlockTokens; g.slot_stride = kSlotStride;
    g.tile_w0 = 0; g.tile_stride = kTileStride; g.chunk0 = v.a.chunk0; g.nchunks = v.p.nt;
    tg.abs0 = 0; tg.e0 = 0; tg.end = v.a.L; tg.nil_pos = ~0ull; tg.abs0_nil = 1;
    tg.entry = const_cast<uint16_t *>(q.entry) + q.tile0[v.p.item];
    const uint32_t c = blockIdx.x - v.p.c0;
    const uint32_t *tokens = q.tokens + (size_t)v.p.c0 * kChunkMax;
    const ChunkMeta *tmeta = q.tmeta + v.p.c0;
    const uint32_t *tokoff = q.tokoff + v.p.c0 + v.p.j;
    uint32_t *T = q.T + v.p.toff;
    ContBlk *blk = q.blk + v.p.boff;
#include "zgpu_cont_compact_body.inc"
}
// ... and what ONE block-construction launch over all streams needs: every slot of the launch learns whose it is (blk_item: the item, ~0 for a slot behind
// its stream's last block), a block's tokens their place in the round's array
__global__ void __launch_bounds__(256) cont_table_batch_kernel(ContBatch q)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= q.nslots_max) return;
    const StreamsRound r = *q.round;
    if (s >= r.nslots) { q.blk_item[s] = 0xFFFFFFFFu; return; }
    const PartView v = part_view(q, part_of_slot(q, r.nparts, s));
    ContBlk *blk = q.blk + v.p.boff;
    const uint32_t b = s - v.p.boff;
    const bool is_block = cont_table_body(b, blk, q.st + v.p.item, q.T + v.p.toff, v.a.seg_end, v.a.final_block, v.a.sp, v.p.nblk_cap, q.slow);
    if (is_block) { blk[b].tok0 += v.p.toff; q.blk_item[s] = v.p.item; }
    else q.blk_item[s] = 0xFFFFFFFFu;
}
__global__ void __launch_bounds__(kBatchScan) cont_bitscan_batch_kernel(ContBatch q)
{
    if (blockIdx.x >= q.round->nparts) return;
    const PartView v = part_view(q, blockIdx.x);
    cont_bitscan_body<kBatchScan>(q.blk + v.p.boff, q.st + v.p.item, q.pos + v.p.boff + v.p.j, v.out_words * 32);
}
__global__ void __launch_bounds__(256) cont_edges_batch_kernel(ContBatch q)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    const StreamsRound r = *q.round;
    if (s >= r.nslots) return;
    const PartView v = part_view(q, part_of_slot(q, r.nparts, s));
    cont_edges_body(s - v.p.boff, q.st + v.p.item, q.pos + v.p.boff + v.p.j, reinterpret_cast<uint32_t *>(q.out + v.out_lo), v.out_words);
}
__global__ void __launch_bounds__(256) cont_stitch_batch_kernel(ContBatch q)
{
    const StreamsRound r = *q.round;
    if (blockIdx.x >= r.nslots) return;
    const PartView v = part_view(q, part_of_slot(q, r.nparts, blockIdx.x));
    const uint32_t b = blockIdx.x - v.p.boff;
    const ContBlk *blk = q.blk + v.p.boff;
    const ContState *st = q.st + v.p.item;
    const uint64_t *pos = q.pos + v.p.boff + v.p.j;
    const uint8_t *slots = q.slots + (size_t)v.p.boff * kSlotStride;
    const uint32_t slot_stride = kSlotStride;
    const uint8_t *in = q.in + v.in_lo;
    const uint64_t abs0 = 0, out_words = v.out_words;
    uint32_t *out = reinterpret_cast<uint32_t *>(q.out + v.out_lo);
#include "zgpu_cont_stitch_body.inc"
}
// (at most one stream is open at a round's end, the last part's: the one carry buffer serves; a stream that ends carries nothing)
__global__ void __launch_bounds__(kBatchScan) cont_carry_batch_kernel(ContBatch q)
{
    if (blockIdx.x >= q.round->nparts) return;
    const PartView v = part_view(q, blockIdx.x);
    cont_carry_body<kBatchScan>(q.blk + v.p.boff, q.st + v.p.item, q.T + v.p.toff, q.carry, v.a.seg_end);
}

// ------------------------------------------------------------------------------------------------- launches
void launch_chain(const uint16_t *exits, uint32_t ntiles, uint16_t *comp, uint16_t *gentry, uint16_t *entry, hipStream_t st)
{
    const uint32_t ngroups = (ntiles + kChainGroup - 1) / kChainGroup;
    if (ngroups > 1) hipLaunchKernelGGL(chain_compose_kernel, dim3(ngroups), dim3(576), 0, st, exits, ntiles, comp);
    hipLaunchKernelGGL(chain_serial_kernel, dim3(1), dim3(64), 0, st, comp, ngroups, gentry, entry);
    hipLaunchKernelGGL(chain_apply_kernel, dim3(ngroups), dim3(64), 0, st, exits, ntiles, gentry, entry);
}
uint32_t chain_groups(uint32_t ntiles) { return (ntiles + kChainGroup - 1) / kChainGroup; }

void launch_cont_tokens(const ChunkGeom &g, const TileGeom &tg, const uint32_t *tokens, const ChunkMeta *tmeta, ContState *st, uint32_t *tokoff, const uint32_t *carry, uint32_t *T,
                        ContBlk *blk, uint64_t seg_end, bool final_block, uint64_t sp, uint32_t nblk_cap, bool slow, hipStream_t s)
{
    hipLaunchKernelGGL(cont_tokscan_kernel, dim3(1), dim3(1024), 0, s, tmeta, g.nchunks, st, tokoff, carry, T);
    if (g.nchunks) hipLaunchKernelGGL(cont_compact_kernel, dim3(g.nchunks), dim3(256), 0, s, g, tg, tokens, tmeta, tokoff, T, blk);
    hipLaunchKernelGGL(cont_table_kernel, dim3((nblk_cap + 255) / 256), dim3(256), 0, s, blk, st, T, seg_end, final_block ? 1u : 0u, sp, nblk_cap, slow ? 1u : 0u);
}
void launch_cont_stitch(const ContBlk *blk, ContState *st, uint64_t *pos, const uint8_t *slots, uint32_t slot_stride, const uint8_t *in, uint64_t abs0, uint8_t *out, uint64_t out_cap,
                        uint32_t nblk_cap, const uint32_t *T, uint32_t *carry, uint64_t seg_end, hipStream_t s)
{
    const uint64_t out_words = out_cap >> 2;
    hipLaunchKernelGGL(cont_bitscan_kernel, dim3(1), dim3(1024), 0, s, blk, st, pos, out_words * 32);
    hipLaunchKernelGGL(cont_edges_kernel, dim3((nblk_cap + 255) / 256), dim3(256), 0, s, st, pos, reinterpret_cast<uint32_t *>(out), out_words);
    hipLaunchKernelGGL(cont_stitch_kernel, dim3(nblk_cap), dim3(256), 0, s, blk, st, pos, slots, slot_stride, in, abs0, reinterpret_cast<uint32_t *>(out), out_words);
    hipLaunchKernelGGL(cont_carry_kernel, dim3(1), dim3(1024), 0, s, blk, st, T, carry, seg_end);
}
uint64_t cont_special_pos(uint64_t n) { return cont_special(n); }

// the round's tokens into blocks, behind the parse: launches 1-3 of the seven.  nparts_max, ntiles_max: what the host knows of the round's parts and
// real tiles -- the numbers themselves (the blocking call) or bounds of them (the stream-ordered call); block slots: q.nslots_max
void launch_cont_batch_tokens(const ContBatch &q, uint32_t nparts_max, uint32_t ntiles_max, hipStream_t s)
{
    hipLaunchKernelGGL(cont_tokscan_batch_kernel, dim3(nparts_max), dim3(kBatchScan), 0, s, q);
    hipLaunchKernelGGL(cont_compact_batch_kernel, dim3(ntiles_max), dim3(256), 0, s, q);
    hipLaunchKernelGGL(cont_table_batch_kernel, dim3((q.nslots_max + 255) / 256), dim3(256), 0, s, q);
}
// ... and the coded blocks into the rooms, behind block construction: launches 4-7
void launch_cont_batch_stitch(const ContBatch &q, uint32_t nparts_max, hipStream_t s)
{
    hipLaunchKernelGGL(cont_bitscan_batch_kernel, dim3(nparts_max), dim3(kBatchScan), 0, s, q);
    hipLaunchKernelGGL(cont_edges_batch_kernel, dim3((q.nslots_max + 255) / 256), dim3(256), 0, s, q);
    hipLaunchKernelGGL(cont_stitch_batch_kernel, dim3(q.nslots_max), dim3(256), 0, s, q);
    hipLaunchKernelGGL(cont_carry_batch_kernel, dim3(nparts_max), dim3(kBatchScan), 0, s, q);
}

} // namespace zgpu
