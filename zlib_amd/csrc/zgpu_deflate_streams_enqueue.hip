// zgpu_deflate_streams_enqueue.hip -- host side of the STREAM-ORDERED batch compress of items of any length (zgpu_deflate_streams_enqueue and its helpers in
// include/zamd_gpu.h): what zgpu_deflate_streams_device makes, as one chain of kernel launches on the caller's stream.  No synchronize, no allocation, no
// copy to or from the host, no event, no second stream, no timing, and no device memory of the engine's: the scratch is the caller's workspace, laid out by
// senq_ws_plan (zgpu_deflate_streams_plan.h).  No kernel lives here.
//
// The blocking call (streams_run, zgpu_deflate_streams.hip) reads its tables, plans its rounds on the host and launches the same kernels at the exact
// extents.  Here the plan is made on the device; the host knows three numbers -- n, in_bytes, batch_tiles -- and sizes and launches by them alone:
//   the tiles    at most ntiles_max = in_bytes / kTileStride + n; the list is laid out for that many, in whole rounds of `batch` tiles, and the rows behind
//                the real tiles are padding rows, for which every kernel of the chain leaves at its top
//   the plan     senq_scan_kernel, senq_rows_kernel once; senq_round_kernel per round (zgpu_streams_batch.hip)
//   the LZ stage launch_lz_tiles / launch_lz_tiles_parse over the round's rows, as the blocking call's
//   the blocks   the blocking call's: seven launches per round over all of its streams (launch_cont_batch_*, zgpu_cont.hip) around ONE block-construction
//                launch -- but all at the host's upper bounds: a part per tile, kSenqBlkPerTile block slots per tile
//   checksums    checksum_batch_enqueue (zgpu_checksum.hip) at the upper bound of pieces, ntiles_max
#include "zgpu_engine.h"
#include "zgpu_deflate_streams_plan.h"

namespace zgpu {

struct SenqWs {
    unsigned long long *cnt; uint32_t *state; uint64_t *tile0, *piece0; TileRow *rows; uint16_t *entry; ContState *st; zgpu_check_item *check; void *ckpart;
    StreamsRound *round; StreamsRoundPart *parts; uint32_t *tokoff, *blk_item; uint16_t *exits, *comp, *gentry; uint32_t *carry, *T; ContBlk *blk; uint64_t *pos;
    uint8_t *slots; uint32_t *tokens; ChunkMeta *meta; uint8_t *sorted;
    SenqWs(void *d_ws, const SenqWsPlan &pl)
    {
        uint8_t *b = static_cast<uint8_t *>(d_ws);
        auto at = [&](int i) { return static_cast<void *>(b + pl.r[i].off); };
        cnt = static_cast<unsigned long long *>(at(kSwCnt)); state = static_cast<uint32_t *>(at(kSwState)); tile0 = static_cast<uint64_t *>(at(kSwTile0));
        piece0 = static_cast<uint64_t *>(at(kSwPiece0)); rows = static_cast<TileRow *>(at(kSwRows)); entry = static_cast<uint16_t *>(at(kSwEntry));
        st = static_cast<ContState *>(at(kSwSt)); check = static_cast<zgpu_check_item *>(at(kSwCheck)); ckpart = at(kSwCkPart);
        round = static_cast<StreamsRound *>(at(kSwRound)); parts = static_cast<StreamsRoundPart *>(at(kSwParts)); tokoff = static_cast<uint32_t *>(at(kSwTokoff));
        blk_item = static_cast<uint32_t *>(at(kSwBlkItem)); exits = static_cast<uint16_t *>(at(kSwExits)); comp = static_cast<uint16_t *>(at(kSwComp));
        gentry = static_cast<uint16_t *>(at(kSwGentry)); carry = static_cast<uint32_t *>(at(kSwCarry)); T = static_cast<uint32_t *>(at(kSwT));
        blk = static_cast<ContBlk *>(at(kSwBlk)); pos = static_cast<uint64_t *>(at(kSwPos)); slots = static_cast<uint8_t *>(at(kSwSlots));
        tokens = static_cast<uint32_t *>(at(kSwTokens)); meta = static_cast<ChunkMeta *>(at(kSwMeta)); sorted = static_cast<uint8_t *>(at(kSwSorted));
    }
};

// the device the engine is on, for a thread that is not on it already (a stream capture, say, is left alone)
static int on_device(zgpu_engine *e)
{
    int cur = -1;
    ZGPU_HIP_CHECK(hipGetDevice(&cur));
    if (cur != e->device) ZGPU_HIP_CHECK(hipSetDevice(e->device));
    return ZGPU_OK;
}

} // namespace zgpu

using namespace zgpu;

extern "C" {
#pragma GCC visibility push(default)

uint64_t zgpu_deflate_streams_workspace_bytes(uint64_t n, uint64_t in_bytes, uint32_t batch_tiles) { return senq_ws_plan(n, in_bytes, batch_tiles).total; }

uint64_t zgpu_deflate_streams_rooms_bound(uint64_t n, uint64_t in_bytes, uint32_t flags) { return senq_rooms_bound(n, in_bytes, flags); }

int zgpu_deflate_streams_layout_enqueue(zgpu_engine *e, const uint64_t *d_in_offsets, uint64_t n, uint64_t in_bytes, uint32_t flags, uint64_t *d_out_offsets, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!d_in_offsets || !d_out_offsets || n >= (1ull << 32)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    if (int rc = on_device(e)) return rc;
    launch_senq_layout(d_in_offsets, n, in_bytes, flags, d_out_offsets, hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream);
    ZGPU_HIP_CHECK(hipGetLastError());
    return ZGPU_OK;
}

int zgpu_deflate_streams_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, const zgpu_deflate_params *p, void *d_out, uint64_t out_cap,
                                 const uint64_t *d_out_offsets, zgpu_deflate_batch_item *d_items, zgpu_deflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes,
                                 uint32_t batch_tiles, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    // everything the host can judge, before anything is enqueued
    if (!p || n >= (1ull << 32) || (n && (!d_in_offsets || !d_out_offsets || !d_items)) || (n && in_bytes && !d_in) || (n && out_cap && !d_out))
        return fail(e, ZGPU_STREAM_ERROR, "null argument");
    if (const char *why = streams_refuse(e, p)) return fail(e, ZGPU_STREAM_ERROR, why);
    if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(e, ZGPU_STREAM_ERROR, "many streams in one call: the output must be 4-byte aligned");
    const SenqWsPlan pl = senq_ws_plan(n, in_bytes, batch_tiles);
    if (n && (!d_ws || (reinterpret_cast<uintptr_t>(d_ws) & 255) || pl.total == 0 || ws_bytes < pl.total))
        return fail(e, ZGPU_STREAM_ERROR, "many streams in one call: the workspace is null, not 256-byte aligned or too small");
    if (int rc = on_device(e)) return rc;
    const hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    if (n == 0) { // at most the summary is written
        if (d_summary) launch_senq_clear(nullptr, nullptr, d_summary, st);
        ZGPU_HIP_CHECK(hipGetLastError());
        return ZGPU_OK;
    }
    const SenqWs w(d_ws, pl);
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    uint8_t *out = static_cast<uint8_t *>(d_out);
    const LevelCfg cfg = level_cfg_for(e, p->level, p->strategy);
    const bool wrap = p->flags & ZGPU_F_ZLIB_WRAP, gz = p->flags & ZGPU_F_GZIP_WRAP, want_crc = gz || (p->flags & ZGPU_F_CRC32);
    const FrameHead fh = frame_head(p->level, p->strategy, wrap, gz);
    const uint32_t batch = pl.batch, nslots_max = kSenqBlkPerTile * batch;
    // the head of the chain, the plan of the call, every stream's state and header
    uint32_t *const fault = lz_sorted_fault_word(w.sorted);
    launch_senq_clear(w.cnt, fault, d_summary, st);
    launch_senq_scan(d_in_offsets, d_out_offsets, n, in_bytes, out_cap, w.state, w.tile0, w.piece0, w.cnt, st);
    launch_senq_rows(d_in_offsets, w.tile0, n, pl.rounds * batch, w.rows, st);
    launch_streams_head(d_in_offsets, d_out_offsets, w.state, n, fh, p->flags, w.st, out, w.entry, nullptr, st); // (the counters: cleared above)
    ChunkGeom g; TileGeom tg;
    streams_list_geom(in, in_bytes, w.exits, w.entry, &g, &tg);
    ContBatch q{};
    q.parts = w.parts; q.round = w.round; q.in_off = d_in_offsets; q.oo = d_out_offsets; q.tile0 = w.tile0; q.in = in; q.out = out; q.flags = p->flags; q.slow = cfg.slow != 0;
    q.nslots_max = nslots_max; q.st = w.st; q.entry = w.entry; q.tokens = w.tokens; q.tmeta = w.meta; q.tokoff = w.tokoff; q.carry = w.carry; q.T = w.T; q.blk = w.blk; q.pos = w.pos;
    q.slots = w.slots; q.blk_item = w.blk_item;
    // the rounds, one behind the other in the same regions: every one a full round of `batch` rows, real or padding
    for (uint64_t r = 0; r < pl.rounds; r++) {
        const uint64_t t0 = r * batch;
        g.chunk0 = t0; g.nchunks = batch; g.rows = w.rows + t0;
        q.t0 = t0;
        launch_senq_round(w.tile0, n, t0, batch, g.rows, w.parts, w.round, w.exits, w.meta, st);
        launch_lz_tiles(g, tg, cfg, w.sorted, w.meta, w.comp, w.gentry, st, nullptr, e->exact_sort); // (no engine: no stage timer, no event)
        launch_streams_entry(g.rows, batch, w.entry + t0, st);
        launch_lz_tiles_parse(g, tg, cfg, w.sorted, w.tokens, w.meta, st, nullptr);
        launch_cont_batch_tokens(q, batch, batch, st);
        launch_huffman_streams(g, w.T, nslots_max, w.blk, w.st, w.blk_item, w.slots, st, cfg.strategy == kFixed); // (g: block_tokens and slot_stride only)
        launch_cont_batch_stitch(q, batch, st);
    }
    // checksums of every served item, trailers, records; the sort's self-check and the summary
    checksum_batch_enqueue(in, d_in_offsets, w.state, w.piece0, n, pl.ntiles_max, want_crc ? 3u : 1u, w.ckpart, w.check, st);
    launch_streams_finish(d_in_offsets, d_out_offsets, w.state, n, fh, p->flags, w.st, w.check, want_crc, out, d_items, w.cnt, st);
    launch_senq_summary(fault, n, w.cnt, d_items, d_summary, st);
    ZGPU_HIP_CHECK(hipGetLastError());
    return ZGPU_OK;
}

#pragma GCC visibility pop
} // extern "C"
