// zgpu_deflate_streams_plan.h -- internal (not installed): what a batch compress of many independent streams decides from plain numbers.  Two calls share it.
// The BLOCKING call (zgpu_deflate_streams_device / _host, streams_run in zgpu_deflate_streams.hip) reads its tables, so the HOST decides everything in the
// first part of this header: how many tiles a stream of a given length has, the row of the per-tile table for each of them, the rooms of the output and
// their bound, where the batches of tiles end, and the round plan -- which streams a batch holds (its parts) and what they need of the block layer's
// buffers.  The stream-ordered call (second part) decides the same things with the same functions, on the device.  No HIP call, no getenv;
// tests/tools/deflate_streams_plan_model.cpp prints the same numbers on a machine without a GPU.
//
// Every stream of the call is a fresh one-feed FINISH stream (zgpu_cont.hip): stream position 0 is its first byte, the parse enters its first tile at 0,
// later tiles start every kTileStride bytes, and the parse runs up to the stream's end.  The tiles of all streams, stream after stream, form ONE list;
// a batch of tiles (a round) is a run of that list and may begin and end inside a stream.
#pragma once
#include "zgpu_deflate_plan.h"

namespace zgpu {

constexpr uint32_t kStreamsCarry = 16384; // tokens of the block that is still filling when a batch ends inside a stream (fewer than kBlockTokens + 1)

// tiles of a stream of L bytes: what plan_cont gives a fresh stream's one FINISH feed
__host__ __device__ inline uint64_t streams_ntiles(uint64_t L) { return L == 0 ? 0 : L <= kTileH1 ? 1 : (L - kTileH1 + kTileStride - 1) / kTileStride + 1; }

// the one position of a stream of n bytes whose first candidate, exactly MAX_DIST back, is NIL: cont_special (zgpu_deflate_plan.h), if it is below n; ~0: none
__host__ __device__ inline uint64_t streams_special(uint64_t n)
{
    const uint64_t sp = cont_special(n);
    return sp < n ? sp : ~0ull;
}

// tile ti of the stream in[off, off + L): the row that says of it what ChunkGeom's and TileGeom's scalars say of tile ti of a one-stream launch
__host__ __device__ inline TileRow streams_tile_row(uint64_t off, uint64_t L, uint64_t ti)
{
    TileRow r;
    const uint64_t wb = ti * kTileStride, rem = L - wb; // (ti < streams_ntiles(L): wb < L)
    r.lo = off + wb;
    r.n = (uint32_t)(rem < kChunkMax ? rem : kChunkMax); // clipped at the stream's own end: the next item's bytes are no lookahead
    r.h0 = ti == 0 ? 0u : kTileStride;
    r.h1 = (uint32_t)(rem < kTileH1 ? rem : kTileH1);
    if (r.h1 < r.h0) r.h1 = r.h0;
    r.nent = ti == 0 ? 1u : kTileEntries;
    r.base = ti == 0 ? 0u : 1u;
    const uint64_t sp = streams_special(L);
    r.nil_local = (sp != ~0ull && sp >= wb && sp - wb < kChunkMax) ? (uint32_t)(sp - wb) : ~0u;
    return r;
}

// ---- the output: a room per item ----
__host__ __device__ inline uint32_t streams_head_bytes(uint32_t flags) { return (flags & ZGPU_F_ZLIB_WRAP) ? 2u : (flags & ZGPU_F_GZIP_WRAP) ? 10u : 0u; }
__host__ __device__ inline uint32_t streams_tail_bytes(uint32_t flags) { return (flags & ZGPU_F_ZLIB_WRAP) ? 4u : (flags & ZGPU_F_GZIP_WRAP) ? 8u : 0u; }
// a room that always suffices for an item of item_bytes: the continuous stream's bound (deflateBound's arithmetic for blocks that may not be stored, a
// word per block boundary) plus the wrapper, rounded up to the rooms' alignment
__host__ __device__ inline uint64_t streams_bound(uint64_t item_bytes, uint32_t flags)
{
    const uint64_t cont = item_bytes + ((item_bytes + 7) >> 3) + ((item_bytes + 63) >> 6) + 5 * (item_bytes / 16383 + 2) + 64; // zgpu_deflate_cont_bound
    return (cont + streams_head_bytes(flags) + streams_tail_bytes(flags) + 3) & ~3ull;
}
// the rooms of n items from their sizes alone; false: the table runs backwards
inline bool streams_layout(const uint64_t *in_off, uint64_t n, uint32_t flags, uint64_t *out_off, uint64_t *total)
{
    uint64_t at = 0;
    for (uint64_t k = 0; k < n; k++) {
        if (in_off[k + 1] < in_off[k]) return false;
        out_off[k] = at;
        at += streams_bound(in_off[k + 1] - in_off[k], flags);
    }
    out_off[n] = at;
    if (total) *total = at;
    return true;
}
// what the block layer may write of a stream into a room of `room` bytes: whole words in front of the trailer; 0: the room cannot hold the smallest stream
__host__ __device__ inline uint64_t streams_room_cap(uint64_t room, uint32_t flags)
{
    const uint64_t head = streams_head_bytes(flags), tail = streams_tail_bytes(flags);
    return room >= head + tail + 8 ? (room - tail) & ~3ull : 0;
}

// ---- the tiles of all items as one list ----
// tile0[k] = tiles in front of item k (n + 1 entries); false: an item of 4 GiB or more, or a table that runs backwards
inline bool streams_tile_scan(const uint64_t *in_off, uint64_t n, uint64_t *tile0)
{
    uint64_t at = 0;
    for (uint64_t k = 0; k < n; k++) {
        if (in_off[k + 1] < in_off[k] || in_off[k + 1] - in_off[k] > 0xffffffffull) return false;
        tile0[k] = at;
        at += streams_ntiles(in_off[k + 1] - in_off[k]);
    }
    tile0[n] = at;
    return true;
}
// the item that holds tile t of the list (t < tile0[n]; items without tiles hold none)
__host__ __device__ inline uint64_t streams_item_of(const uint64_t *tile0, uint64_t n, uint64_t t)
{
    uint64_t lo = 0, hi = n; // the last k with tile0[k] <= t
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (tile0[mid] <= t) lo = mid; else hi = mid; }
    return lo;
}

// tiles of a full batch: ZGPU_CONT_BATCH_TILES, else as many as the device's memory admits, 32768 at the most (plan_cont's arithmetic; the block layer's
// buffers are counted for the worst case, every tile a stream of its own)
inline uint32_t streams_batch_tiles(uint64_t ntiles, const PlanEngine &eng, const ContKnobs &kn)
{
    uint64_t batch_max = kn.batch_tiles ? kn.batch_tiles : 32768;
    if (batch_max > 32768) batch_max = 32768; // (a batch's tokens are indexed with 32 bits: 32768 one-tile streams are 2.7e9 tokens of room)
    if (eng.free_bytes) {
        const uint64_t per_tile = eng.sorted_ws_chunk + (uint64_t)kChunkMax * 4 + kSlotStride + 2 * (uint64_t)(kTileStride + kTileSlack) * 4 + 7 * (uint64_t)kSlotStride;
        const uint64_t held = (uint64_t)eng.batch_cap * ((uint64_t)kChunkMax * 4 + kSlotStride) + (uint64_t)eng.par_cap * eng.sorted_ws_chunk;
        uint64_t fit = (eng.free_bytes + held) / 10 * 6 / per_tile;
        if (fit < 64) fit = 64;
        if (fit < batch_max) batch_max = fit;
    }
    return (uint32_t)(ntiles < batch_max ? (ntiles ? ntiles : 1) : batch_max);
}

// What a stream's tiles [a, b) of one batch need of the batch's block-layer buffers: tokens (the carried ones, the positions the tiles parse -- a stream's
// first tile twice as many --, the last game's overhang) and blocks
__host__ __device__ inline uint32_t streams_tok_cap(uint32_t nt) { return (kStreamsCarry + kTileStride * (nt + 1) + kTileSlack + 3) & ~3u; }
__host__ __device__ inline uint32_t streams_blk_cap(uint32_t nt) { return streams_tok_cap(nt) / kBlockTokens + 2; }

// A round = tiles [t0, t0 + batch) of the list, of which the first nreal exist (the blocking call's batches are all real; the stream-ordered call pads
// its list).  Its parts -- a part is the tiles of ONE stream in the round -- as the batched block layer reads them (cont_*_batch_kernel, zgpu_cont.hip)
struct StreamsRoundPart {
    uint32_t boff, toff; // where the part's blocks and tokens lie in the round's buffers (exclusive sums of the caps of the parts in front)
    uint32_t item;       // whose tiles
    uint32_t c0, nt;     // tiles [c0, c0 + nt) of the round
    uint32_t ends;       // the stream's last tile is among them
    uint32_t nblk_cap;   // streams_blk_cap(nt)
    uint32_t j;          // the part's number in the round (its pos[] and tokoff[] run one entry longer than its blocks and tiles)
};
struct StreamsRound { uint32_t nparts, nreal, nslots, ntok; }; // parts, real tiles, block slots and token room in use (sums of the parts' caps)
__host__ __device__ inline uint32_t streams_round_real(uint64_t ntiles, uint64_t t0, uint32_t batch) { return (uint32_t)(ntiles <= t0 ? 0 : ntiles - t0 < batch ? ntiles - t0 : batch); }
// does a part begin at tile c of the round (c < nreal)?  fills all but boff, toff and j
__host__ __device__ inline bool streams_part_at(const uint64_t *tile0, uint64_t n, uint64_t t0, uint32_t nreal, uint32_t c, StreamsRoundPart *p)
{
    const uint64_t t = t0 + c, k = streams_item_of(tile0, n, t);
    if (c != 0 && tile0[k] != t) return false;
    const uint64_t end = tile0[k + 1] < t0 + nreal ? tile0[k + 1] : t0 + nreal;
    p->item = (uint32_t)k; p->c0 = c; p->nt = (uint32_t)(end - t); p->ends = end == tile0[k + 1] ? 1u : 0u; p->nblk_cap = streams_blk_cap(p->nt);
    return true;
}
// the round's plan as one loop: the blocking call's, and what senq_round_kernel (zgpu_streams_batch.hip) does with a workgroup's scan over the tiles
inline StreamsRound streams_round_plan(const uint64_t *tile0, uint64_t n, uint64_t t0, uint32_t batch, StreamsRoundPart *parts)
{
    StreamsRound r{0, streams_round_real(tile0[n], t0, batch), 0, 0};
    for (uint32_t c = 0; c < r.nreal; c++) {
        StreamsRoundPart p{};
        if (!streams_part_at(tile0, n, t0, r.nreal, c, &p)) continue;
        p.boff = r.nslots; p.toff = r.ntok; p.j = r.nparts;
        parts[r.nparts++] = p;
        r.nslots += p.nblk_cap; r.ntok += streams_tok_cap(p.nt);
    }
    return r;
}
// what the batched block layer takes from a part: the stream's own geometry (its length, its end, its special position, its own number of the part's
// first tile) -- the arguments a one-stream launch of the same kernels gets from the host
struct StreamsPartArgs { uint64_t L, seg_end, sp; uint64_t chunk0; uint32_t final_block; };
__host__ __device__ inline StreamsPartArgs streams_part_args(const StreamsRoundPart &p, uint64_t L, uint64_t tile0_item, uint64_t t0)
{
    StreamsPartArgs a;
    a.L = L; a.seg_end = p.ends ? L : ~0ull; a.final_block = p.ends;
    a.sp = p.ends ? cont_special(L) : ~0ull;
    a.chunk0 = t0 + p.c0 - tile0_item;
    return a;
}

// =====================================================================================================================================================
// The stream-ordered call (zgpu_deflate_streams_enqueue, zgpu_deflate_streams_enqueue.hip): the host may not read the tables, so the DEVICE makes the
// plan above -- the kernels of zgpu_streams_batch.hip call the same functions lane by lane -- after judging every table entry itself.  The host knows n,
// in_bytes and batch_tiles only and decides what follows from them: an upper bound of the tiles, the rounds and their padding rows, a bound of the rooms,
// the workspace.  tests/tools/deflate_streams_enqueue_plan_model.cpp calls all of it in plain loops.
//
// The tile count: streams_ntiles(L) <= L / kTileStride + 1 (L <= kTileH1: one tile at most; above, ceil(L / kTileStride) - 1 <= L / kTileStride), so the
// tiles of items that do not overlap and end inside in_bytes are at most
__host__ __device__ inline uint64_t senq_ntiles_max(uint64_t n, uint64_t in_bytes) { return in_bytes / kTileStride + n; }
// The list never grows past that: items whose ranges overlap can ask for more, and an item with tiles whose last tile -- counted as if every item with
// good offsets were served -- lies behind ntiles_max fails as a bad entry.  The served items with tiles are then a run from the front of the table.
constexpr uint32_t kSenqDefaultBatch = 2048; // batch_tiles == 0: tiles of a round (about 2.2 MB of workspace each: senq_ws_plan)
constexpr uint32_t kSenqMaxBatch = 32768;    // as streams_batch_tiles: a round's tokens are indexed with 32 bits
constexpr uint32_t kSenqBlkPerTile = 7, kSenqTokPerTile = 81920; // streams_blk_cap(1), streams_tok_cap(1): a round's parts need at most this much per tile, whatever the parts are
__host__ __device__ inline uint32_t senq_batch(uint64_t n, uint64_t in_bytes, uint32_t batch_tiles)
{
    uint64_t b = batch_tiles ? batch_tiles : kSenqDefaultBatch;
    if (b > kSenqMaxBatch) b = kSenqMaxBatch;
    const uint64_t m = senq_ntiles_max(n, in_bytes);
    return (uint32_t)(m < b ? (m ? m : 1) : b);
}
__host__ __device__ inline uint64_t senq_rounds(uint64_t n, uint64_t in_bytes, uint32_t batch_tiles)
{
    const uint64_t b = senq_batch(n, in_bytes, batch_tiles);
    return (senq_ntiles_max(n, in_bytes) + b - 1) / b;
}

// an item's state: what the table says of it
constexpr uint32_t kSenqServed = 0, kSenqBad = 1, kSenqTooLong = 2;
__host__ __device__ inline uint32_t senq_item_state(uint64_t lo, uint64_t hi, uint64_t in_bytes, uint64_t oa, uint64_t oz, uint64_t out_cap)
{
    if (hi < lo || hi > in_bytes || oz < oa || oz > out_cap || (oa & 3)) return kSenqBad;
    return hi - lo > 0xffffffffull ? kSenqTooLong : kSenqServed;
}
// the tiles item k asks for
__host__ __device__ inline uint64_t senq_item_tiles(uint32_t state, uint64_t lo, uint64_t hi) { return state == kSenqServed ? streams_ntiles(hi - lo) : 0; }
// ... and whether it gets them: `end` = the tiles asked for by the items up to and including this one
__host__ __device__ inline bool senq_item_fits(uint64_t nt, uint64_t end, uint64_t ntiles_max) { return nt == 0 || end <= ntiles_max; }
// 64 KiB pieces of an item's checksums (zgpu_checksum.hip: items of at most 4096 bytes have none).  pieces <= tiles for every length, so the served items'
// pieces are at most ntiles_max too
__host__ __device__ inline uint64_t senq_item_pieces(uint64_t L) { return L <= 4096 ? 0 : (L + kChunkMax - 1) / kChunkMax; }

// The whole scan as one loop: state[k], tile0[0..n], piece0[0..n]; returns the number of tiles.  (The kernel does the same with a workgroup's scan.)
inline uint64_t senq_tile_scan(const uint64_t *in_off, const uint64_t *oo, uint64_t n, uint64_t in_bytes, uint64_t out_cap, uint32_t *state, uint64_t *tile0, uint64_t *piece0)
{
    const uint64_t m = senq_ntiles_max(n, in_bytes);
    uint64_t asked = 0, at = 0, pc = 0;
    for (uint64_t k = 0; k < n; k++) {
        uint32_t s = senq_item_state(in_off[k], in_off[k + 1], in_bytes, oo[k], oo[k + 1], out_cap);
        const uint64_t nt = senq_item_tiles(s, in_off[k], in_off[k + 1]);
        asked += nt;
        if (!senq_item_fits(nt, asked, m)) s = kSenqBad;
        state[k] = s; tile0[k] = at; piece0[k] = pc;
        if (s == kSenqServed) { at += nt; pc += senq_item_pieces(in_off[k + 1] - in_off[k]); }
    }
    tile0[n] = at; piece0[n] = pc;
    return at;
}

// A padding row: the list is laid out for ntiles_max tiles in whole rounds, and the rows behind the real tiles are tiles that parse nothing -- no bytes,
// an empty range.  Every kernel of the chain leaves at its top for such a row; its exit row is all 0 and it has no tokens (streams_pad_kernel)
__host__ __device__ inline TileRow streams_pad_row() { TileRow r; r.lo = 0; r.n = 0; r.h0 = 0; r.h1 = 0; r.nent = 1; r.base = 0; r.nil_local = ~0u; return r; }
__host__ __device__ inline bool streams_row_is_pad(const TileRow &r) { return r.n == 0; } // (a real tile has at least one byte)
// row t of the padded list
__host__ __device__ inline TileRow senq_tile_row(const uint64_t *in_off, const uint64_t *tile0, uint64_t n, uint64_t t)
{
    if (n == 0 || t >= tile0[n]) return streams_pad_row();
    const uint64_t k = streams_item_of(tile0, n, t);
    return streams_tile_row(in_off[k], in_off[k + 1] - in_off[k], t - tile0[k]);
}

// ---- rooms without the host knowing the sizes ----
// at least streams_layout's total for every table of n items that runs forward and ends inside in_bytes (a sum of floors is at most the floor of the
// sum, and the total is a multiple of 4); equal to it for one item of in_bytes
__host__ __device__ inline uint64_t senq_rooms_bound(uint64_t n, uint64_t in_bytes, uint32_t flags)
{
    const uint64_t s = in_bytes;
    return (s + ((s + 7 * n) >> 3) + ((s + 63 * n) >> 6) + 5 * (s / 16383 + 2 * n) + (64 + streams_head_bytes(flags) + streams_tail_bytes(flags) + 3) * n) & ~3ull;
}
// the room zgpu_deflate_streams_layout_enqueue gives entry k: 0 for one that runs backwards or leaves in_bytes
__host__ __device__ inline uint64_t senq_room(uint64_t lo, uint64_t hi, uint64_t in_bytes, uint32_t flags) { return hi < lo || hi > in_bytes ? 0 : streams_bound(hi - lo, flags); }

// ---- the workspace: host arithmetic on (n, in_bytes, batch_tiles) alone ----
struct SenqRegion { uint64_t off, bytes; };
enum {
    kSwCnt, kSwState, kSwTile0, kSwPiece0, kSwRows, kSwEntry, kSwSt, kSwCheck, kSwCkPart, kSwRound, kSwParts, kSwTokoff, kSwBlkItem, kSwExits, kSwComp, kSwGentry, kSwCarry,
    kSwT, kSwBlk, kSwPos, kSwSlots, kSwTokens, kSwMeta, kSwSorted, kSwRegions
};
// the counters (uint64_t each, cleared by the call's first launch); the first three are streams_finish_kernel's totals
constexpr uint32_t kScntTotal = 0, kScntTokens = 1, kScntFailed = 2, kScntBadOffsets = 3, kScntTooLong = 4;
struct SenqWsPlan {
    SenqRegion r[kSwRegions];
    uint64_t ntiles_max, rounds, total; // total 0: n >= 2^32
    uint32_t batch;
};
inline const char *senq_region_name(int i)
{
    static const char *const names[kSwRegions] = {"cnt", "state", "tile0", "piece0", "rows", "entry", "st", "check", "ckpart", "round", "parts", "tokoff", "blk_item", "exits", "comp",
                                                  "gentry", "carry", "T", "blk", "pos", "slots", "tokens", "meta", "sorted"};
    return i >= 0 && i < kSwRegions ? names[i] : "";
}
constexpr uint64_t kSenqSortedChunk = 1058832, kSenqSortedOnce = 256 + 1024; // SortedWs (zgpu_lz_sorted.h; zgpu_deflate_batch_plan.h states the same numbers)
// What a tile of a round costs: the sorted buckets 1,058,832, its tokens 262,144, the compact tokens 327,680, seven block slots 460,544, seven blocks'
// records 392 + 28 + 64, exits 1,044, meta, part and offsets 72 -- 2,110,800 bytes; what the call costs besides: 92 bytes an item (state, tile0, piece0,
// its ContState, its checksums) and 46 per tile of ntiles_max (row, entry, checksum partial)
inline SenqWsPlan senq_ws_plan(uint64_t n, uint64_t in_bytes, uint32_t batch_tiles)
{
    SenqWsPlan p{};
    if (n >= (1ull << 32)) return p;
    p.ntiles_max = senq_ntiles_max(n, in_bytes); p.batch = senq_batch(n, in_bytes, batch_tiles); p.rounds = senq_rounds(n, in_bytes, batch_tiles);
    const uint64_t b = p.batch, nt = p.rounds * b, groups = (b + 255) / 256;
    uint64_t off = 0;
    auto carve = [&](int i, uint64_t bytes) { p.r[i] = SenqRegion{off, bytes}; off = (off + bytes + 255) & ~255ull; };
    carve(kSwCnt, 256);
    carve(kSwState, n * 4);
    carve(kSwTile0, (n + 1) * 8);
    carve(kSwPiece0, (n + 1) * 8);
    carve(kSwRows, nt * sizeof(TileRow));
    carve(kSwEntry, (nt + 2) * 2);
    carve(kSwSt, n * sizeof(ContState));
    carve(kSwCheck, n * 8);
    carve(kSwCkPart, p.ntiles_max * 12);
    carve(kSwRound, 256);
    carve(kSwParts, b * sizeof(StreamsRoundPart));
    carve(kSwTokoff, (2 * b + 1) * 4);
    carve(kSwBlkItem, kSenqBlkPerTile * b * 4);
    carve(kSwExits, b * kTileExitStride * 2);
    carve(kSwComp, groups * kTileExitStride * 2);
    carve(kSwGentry, (groups + 1) * 2);
    carve(kSwCarry, (uint64_t)kStreamsCarry * 4);
    carve(kSwT, b * kSenqTokPerTile * 4);
    carve(kSwBlk, kSenqBlkPerTile * b * sizeof(ContBlk));
    carve(kSwPos, (kSenqBlkPerTile * b + b + 1) * 8);
    carve(kSwSlots, kSenqBlkPerTile * b * kSlotStride);
    carve(kSwTokens, b * kChunkMax * 4);
    carve(kSwMeta, b * sizeof(ChunkMeta));
    carve(kSwSorted, kSenqSortedOnce + b * kSenqSortedChunk);
    p.total = off;
    return p;
}

} // namespace zgpu
