// zgpu_deflate_streams_plan.h -- internal (not installed): what a batch compress of many independent streams (zgpu_deflate_streams_*,
// zgpu_deflate_streams.hip) decides from plain numbers -- how many tiles a stream of a given length has, the row of the per-tile table for each of
// them, the rooms of the output and their bound, where the batches of tiles end and which streams a batch holds.  No HIP call, no getenv;
// tests/tools/deflate_streams_plan_model.cpp prints the same numbers on a machine without a GPU.
//
// Every stream of the call is a fresh one-feed FINISH stream (zgpu_cont.hip): stream position 0 is its first byte, the parse enters its first tile at 0,
// later tiles start every kTileStride bytes, and the parse runs up to the stream's end.  The tiles of all streams, stream after stream, form ONE list;
// a batch of tiles is a run of that list and may begin and end inside a stream.
#pragma once
#include "zgpu_deflate_plan.h"

namespace zgpu {

constexpr uint32_t kStreamsCarry = 16384; // tokens of the block that is still filling when a batch ends inside a stream (fewer than kBlockTokens + 1)

// tiles of a stream of L bytes: what plan_cont gives a fresh stream's one FINISH feed
__host__ __device__ inline uint64_t streams_ntiles(uint64_t L) { return L == 0 ? 0 : L <= kTileH1 ? 1 : (L - kTileH1 + kTileStride - 1) / kTileStride + 1; }

// the one position of a stream of n bytes whose first candidate, exactly MAX_DIST back, is NIL: 32768 k + 65274 in [n - 261, n) (zgpu_cont.hip, cont_special); ~0: none
__host__ __device__ inline uint64_t streams_special(uint64_t n)
{
    if (n < 65274u) return ~0ull;
    const uint64_t sp = (n - 65274u) / 32768u * 32768u + 65274u;
    return (sp + 261u >= n && sp < n) ? sp : ~0ull;
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
inline uint64_t streams_bound(uint64_t item_bytes, uint32_t flags)
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
inline uint64_t streams_item_of(const uint64_t *tile0, uint64_t n, uint64_t t)
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
inline uint32_t streams_tok_cap(uint32_t nt) { return (kStreamsCarry + kTileStride * (nt + 1) + kTileSlack + 3) & ~3u; }
inline uint32_t streams_blk_cap(uint32_t nt) { return streams_tok_cap(nt) / kBlockTokens + 2; }

// a stream's part of a batch as the device sees it: where its blocks and tokens lie in the batch's buffers (slots boff .., tokens toff ..), whose they are
struct StreamsBlkPart { uint32_t boff, toff, item, pad; };

// One batch of the list: tiles [t0, t0 + nb); its streams are the items k0 .. with tiles in it
struct StreamsPart { uint64_t item; uint64_t a, b; bool ends; }; // tiles [a, b) of the list belong to `item`; ends: the stream's last tile is among them
// the part of item k in the batch, false: none
inline bool streams_part(const uint64_t *tile0, uint64_t k, uint64_t t0, uint32_t nb, StreamsPart *out)
{
    const uint64_t a = tile0[k] > t0 ? tile0[k] : t0, b = tile0[k + 1] < t0 + nb ? tile0[k + 1] : t0 + nb;
    if (a >= b) return false;
    out->item = k; out->a = a; out->b = b; out->ends = b == tile0[k + 1];
    return true;
}
// the block layer's needs of the batch [t0, t0 + nb): streams in it, tokens, blocks (sums of the parts' caps)
inline void streams_batch_needs(const uint64_t *tile0, uint64_t n, uint64_t t0, uint32_t nb, uint64_t *nstreams, uint64_t *ntok, uint64_t *nblk)
{
    uint64_t s = 0, t = 0, b = 0;
    StreamsPart pt;
    for (uint64_t k = streams_item_of(tile0, n, t0); k < n && tile0[k] < t0 + nb; k++)
        if (streams_part(tile0, k, t0, nb, &pt)) { s++; t += streams_tok_cap((uint32_t)(pt.b - pt.a)); b += streams_blk_cap((uint32_t)(pt.b - pt.a)); }
    *nstreams = s; *ntok = t; *nblk = b;
}

} // namespace zgpu
