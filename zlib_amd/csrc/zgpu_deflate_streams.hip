// zgpu_deflate_streams.hip -- host side of the batch compress of MANY independent streams of any length (zgpu_deflate_streams_* in include/zamd_gpu.h): item k
// becomes exactly the bytes the reference's one-call stream gives for that item alone, and the tiles of all items share the launches.
// zgpu_deflate_streams_plan.h has what the call decides from plain numbers, zgpu_streams.hip the small kernels around the streams.  No kernel lives here.
//
// A continuous stream is cut into tiles (zgpu_cont.hip); sort, walkers, the chain of entries and the token parse treat a tile as a chunk and never needed
// the tiles of a launch to belong to one stream: here they come as one list over all items, described row by row (TileRow) instead of by the one
// stream's scalars, in batches that end wherever they end -- also inside a stream.  That is ONE set of LZ launches per batch of tiles whatever the
// number of streams, and ONE set of block-layer launches (chains 2-4: tokens -> blocks -> bit positions -> carry): the batched kernels of zgpu_cont.hip,
// seven launches over all streams' parts of the batch around one block-construction launch (huffman_kernel<true, true>).  The call reads its tables,
// so the batches and their parts are planned here on the host (streams_round_plan), uploaded once, and every launch has its exact extent.  Nothing
// between the launches waits for the host.  The stream-ordered call (zgpu_deflate_streams_enqueue.hip) runs the same kernels from a plan made on the device.
#include "zgpu_engine.h"
#include "zgpu_deflate_streams_plan.h"
#include <cstdlib>
#include <vector>

namespace zgpu {

// max_parts, max_tok, max_slots: the most a batch of the call has (StreamsRound's numbers)
static int reserve_streams(zgpu_engine *e, uint64_t n, uint64_t ntiles, uint32_t batch, size_t nbatches, size_t nparts_all, uint64_t max_parts, uint64_t max_tok, uint64_t max_slots)
{
    int rc = ensure_deflate_ws(e, batch, false, 1);
    if (rc) return rc;
    const uint32_t ngroups = chain_groups(batch);
    if ((rc = e->ds_rows.reserve(e, ntiles + 1)) || (rc = e->ds_entry.reserve(e, ntiles + 2)) || (rc = e->ds_st.reserve(e, n)) || (rc = e->ds_check.reserve(e, n)) ||
        (rc = e->ds_totals.reserve(e, 4)) || (rc = e->ds_tokoff.reserve(e, (size_t)batch + max_parts + 1)) || (rc = e->ds_blk_item.reserve(e, max_slots)) ||
        (rc = e->ds_parts.reserve(e, nparts_all + 1)) || (rc = e->ds_rounds.reserve(e, nbatches + 1)) || (rc = e->ds_tile0.reserve(e, n + 1))) return rc;
    if ((rc = e->ct_exits.reserve(e, (size_t)batch * kTileExitStride)) || (rc = e->ct_comp.reserve(e, (size_t)ngroups * kTileExitStride)) || (rc = e->ct_gentry.reserve(e, (size_t)ngroups + 1)) ||
        (rc = e->ct_carry.reserve(e, kStreamsCarry)) || (rc = e->ct_T.reserve(e, max_tok)) || (rc = e->ct_blk.reserve(e, max_slots)) ||
        (rc = e->ct_pos.reserve(e, max_slots + max_parts + 1)) || (rc = e->ct_slots.reserve(e, max_slots * kSlotStride))) return rc;
    return ZGPU_OK;
}

// the ChunkGeom / TileGeom of a list of tiles that comes row by row (g.rows, g.chunk0 and g.nchunks: per batch)
void streams_list_geom(const uint8_t *d_in, uint64_t in_bytes, uint16_t *exits, uint16_t *entry, ChunkGeom *g, TileGeom *tg)
{
    *g = ChunkGeom{}; *tg = TileGeom{};
    g->in = d_in; g->in_bytes = in_bytes; g->chunk_size = kChunkMax; g->final_chunk = ~0ull; g->block_tokens = kBlockTokens; g->slot_stride = kSlotStride;
    g->tile_stride = kTileStride;
    tg->nil_pos = ~0ull; tg->exits = exits; tg->entry = entry;
}

const char *streams_refuse(const zgpu_engine *e, const zgpu_deflate_params *p)
{
    if (p->level < 4 || p->level > 9) return "many streams in one call: levels 4..9 (levels 0..3 are served one stream at a time)";
    if (p->strategy < 0 || p->strategy > (int)kFixed) return "strategy must be 0..4";
    if (!(p->flags & ZGPU_F_FINAL)) return "many streams in one call: every item is a whole stream, FINAL is required";
    if (e->geo_w != 15 || e->geo_m != 8) return "many streams in one call: the default geometry (windowBits 15, memLevel 8)";
    if (p->prime || (p->flags & (ZGPU_F_POS0 | ZGPU_F_POS0_ALL | ZGPU_F_BGZF_WRAP | ZGPU_F_CONTINUOUS))) return "many streams in one call: no prime, POS0, BGZF_WRAP or CONTINUOUS";
    if (p->lz_impl != ZGPU_LZ_AUTO) return "many streams in one call: ZGPU_LZ_AUTO only";
    if ((p->flags & ZGPU_F_ZLIB_WRAP) && (p->flags & ZGPU_F_GZIP_WRAP)) return "one wrapper at a time";
    return nullptr;
}

// The call with its input table on both sides: h_in_off is the host's copy of d_in_off (both tables checked by the caller)
static int streams_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, const uint64_t *h_in_off, uint64_t n, const zgpu_deflate_params *p, uint8_t *d_out,
                       const uint64_t *d_oo, zgpu_deflate_batch_item *d_items, zgpu_deflate_result *res, hipStream_t st)
{
    int rc;
    std::vector<uint64_t> tile0(n + 1);
    if (!streams_tile_scan(h_in_off, n, tile0.data())) return fail(e, ZGPU_STREAM_ERROR, "many streams in one call: an item of 4 GiB or more");
    const uint64_t ntiles = tile0[n];
    const LevelCfg cfg = level_cfg_for(e, p->level, p->strategy);
    ContKnobs kn;
    kn.batch_tiles = env_u32("ZGPU_CONT_BATCH_TILES", 0); kn.batch_tiles_set = getenv("ZGPU_CONT_BATCH_TILES") != nullptr; // (read per call)
    const uint32_t batch = streams_batch_tiles(ntiles, plan_engine(e, &cfg), kn);
    // the plan of every batch (round) in one loop: its record, its parts (all batches back to back), where its parts begin
    std::vector<StreamsRound> rounds;
    std::vector<StreamsRoundPart> parts;
    std::vector<size_t> part0;
    uint64_t max_parts = 1, max_tok = 1, max_slots = 1;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += batch) {
        part0.push_back(parts.size());
        parts.resize(parts.size() + batch); // (a part per tile at the most)
        const StreamsRound rd = streams_round_plan(tile0.data(), n, t0, batch, parts.data() + part0.back());
        parts.resize(part0.back() + rd.nparts);
        rounds.push_back(rd);
        if (rd.nparts > max_parts) max_parts = rd.nparts;
        if (rd.ntok > max_tok) max_tok = rd.ntok;
        if (rd.nslots > max_slots) max_slots = rd.nslots;
    }
    if ((rc = reserve_streams(e, n, ntiles, batch, rounds.size(), parts.size(), max_parts, max_tok, max_slots))) return rc;
    // the plan and the rows of all tiles to the device, in one wait
    {
        std::vector<TileRow> rows(ntiles);
        for (uint64_t k = 0; k < n; k++)
            for (uint64_t ti = 0, nt = tile0[k + 1] - tile0[k]; ti < nt; ti++) rows[tile0[k] + ti] = streams_tile_row(h_in_off[k], h_in_off[k + 1] - h_in_off[k], ti);
        if (ntiles) {
            ZGPU_HIP_CHECK(hipMemcpyAsync(e->ds_rows, rows.data(), ntiles * sizeof(TileRow), hipMemcpyHostToDevice, st));
            ZGPU_HIP_CHECK(hipMemcpyAsync(e->ds_parts, parts.data(), parts.size() * sizeof(StreamsRoundPart), hipMemcpyHostToDevice, st));
            ZGPU_HIP_CHECK(hipMemcpyAsync(e->ds_rounds, rounds.data(), rounds.size() * sizeof(StreamsRound), hipMemcpyHostToDevice, st));
        }
        ZGPU_HIP_CHECK(hipMemcpyAsync(e->ds_tile0, tile0.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st)); // (the vector goes out of scope)
    }
    const bool wrap = p->flags & ZGPU_F_ZLIB_WRAP, gz = p->flags & ZGPU_F_GZIP_WRAP, want_crc = gz || (p->flags & ZGPU_F_CRC32);
    const FrameHead fh = frame_head(p->level, p->strategy, wrap, gz);
    launch_streams_head(d_in_off, d_oo, nullptr, n, fh, p->flags, e->ds_st, d_out, e->ds_entry, e->ds_totals, st);
    const bool check_sort = !e->exact_sort;
    if (check_sort) ZGPU_HIP_CHECK(hipMemsetAsync(lz_sorted_fault_word(e->par_ws), 0, 4, st));
    ChunkGeom g; TileGeom tg;
    streams_list_geom(d_in, in_bytes, e->ct_exits, e->ds_entry, &g, &tg);
    ContBatch q{};
    q.in_off = d_in_off; q.oo = d_oo; q.tile0 = e->ds_tile0; q.in = d_in; q.out = d_out; q.flags = p->flags; q.slow = cfg.slow != 0;
    q.st = e->ds_st; q.entry = e->ds_entry; q.tokens = e->tokens; q.tmeta = e->meta; q.tokoff = e->ds_tokoff; q.carry = e->ct_carry; q.T = e->ct_T; q.blk = e->ct_blk; q.pos = e->ct_pos;
    q.slots = e->ct_slots; q.blk_item = e->ds_blk_item;
    for (size_t r = 0; r < rounds.size(); r++) {
        const uint64_t t0 = (uint64_t)r * batch;
        const StreamsRound &rd = rounds[r];
        g.chunk0 = t0; g.nchunks = rd.nreal; g.rows = e->ds_rows + t0;
        q.round = e->ds_rounds + r; q.parts = e->ds_parts + part0[r]; q.nslots_max = rd.nslots; q.t0 = t0;
        // the LZ stage: one set of launches for the batch's tiles, whatever streams they belong to
        launch_lz_tiles(g, tg, cfg, e->par_ws, e->meta, e->ct_comp, e->ct_gentry, st, e, e->exact_sort);
        launch_streams_entry(g.rows, rd.nreal, e->ds_entry + t0, st);
        launch_lz_tiles_parse(g, tg, cfg, e->par_ws, e->tokens, e->meta, st, e);
        // the block layer, no wait for the host anywhere: one set of launches over the parts of all streams of the batch, at the plan's extents
        {
            StageTimer t(e, st, ZGPU_STAGE_PARSE);
            launch_cont_batch_tokens(q, rd.nparts, rd.nreal, st);
        }
        {
            StageTimer t(e, st, ZGPU_STAGE_HUFFMAN);
            launch_huffman_streams(g, e->ct_T, rd.nslots, e->ct_blk, e->ds_st, e->ds_blk_item, e->ct_slots, st, cfg.strategy == kFixed); // (g: block_tokens and slot_stride only)
        }
        {
            StageTimer t(e, st, ZGPU_STAGE_STITCH);
            launch_cont_batch_stitch(q, rd.nparts, st);
        }
        const hipError_t he = hipGetLastError();
        if (he != hipSuccess) return fail_hip(e, he, "kernel launch", __FILE__, __LINE__);
    }
    // checksums of every item, trailers, records
    {
        StageTimer t(e, st, ZGPU_STAGE_STITCH);
        if ((rc = checksum_batch_run(e, d_in, in_bytes, d_in_off, n, want_crc ? 3u : 1u, e->ds_check, st))) return rc;
        launch_streams_finish(d_in_off, d_oo, nullptr, n, fh, p->flags, e->ds_st, e->ds_check, want_crc, d_out, d_items, e->ds_totals, st);
    }
    unsigned long long totals[3] = {0, 0, 0};
    uint32_t sort_fault = 0;
    zgpu_deflate_batch_item last{};
    ZGPU_HIP_CHECK(hipMemcpyAsync(totals, e->ds_totals, sizeof totals, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipMemcpyAsync(&last, d_items + (n - 1), sizeof last, hipMemcpyDeviceToHost, st));
    if (check_sort && ntiles) ZGPU_HIP_CHECK(hipMemcpyAsync(&sort_fault, lz_sorted_fault_word(e->par_ws), 4, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    collect_spans(e);
    if (sort_fault) { e->exact_sort = 1; return streams_run(e, d_in, in_bytes, d_in_off, h_in_off, n, p, d_out, d_oo, d_items, res, st); } // (the input is untouched: the whole call again with the exact sort)
    res->out_bytes = totals[0]; res->ntokens = totals[1]; res->reserved = (uint32_t)(totals[2] < 0xffffffffull ? totals[2] : 0xffffffffull);
    res->nchunks = ntiles; res->adler32 = last.adler32; res->crc32 = last.crc32; res->data_type = last.data_type;
    return ZGPU_OK;
}

// the tables as the host judges them before anything is launched
static const char *streams_tables_refuse(const uint64_t *in_off, const uint64_t *oo, uint64_t n, uint64_t in_bytes, uint64_t out_cap)
{
    for (uint64_t k = 0; k < n; k++) {
        if (in_off[k + 1] < in_off[k] || oo[k + 1] < oo[k]) return "many streams in one call: a table runs backwards";
        if (oo[k] & 3) return "many streams in one call: every room starts at a multiple of 4";
    }
    if (in_off[n] > in_bytes || oo[n] > out_cap || (oo[n] & 3)) return "many streams in one call: a table leaves its buffer";
    return nullptr;
}

} // namespace zgpu

using namespace zgpu;

extern "C" {
#pragma GCC visibility push(default)

uint64_t zgpu_deflate_streams_bound(uint64_t item_bytes, uint32_t flags) { return streams_bound(item_bytes, flags); }

int zgpu_deflate_streams_layout(const uint64_t *in_offsets, uint64_t n, uint32_t flags, uint64_t *out_offsets, uint64_t *total)
{
    if (!in_offsets || !out_offsets) return ZGPU_STREAM_ERROR;
    return streams_layout(in_offsets, n, flags, out_offsets, total) ? ZGPU_OK : ZGPU_STREAM_ERROR;
}

int zgpu_deflate_streams_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, const zgpu_deflate_params *p, void *d_out, uint64_t out_cap,
                                const uint64_t *d_out_offsets, zgpu_deflate_batch_item *d_items, zgpu_deflate_result *res, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!p || !res || (n && (!d_in_offsets || !d_out_offsets || !d_out || !d_items)) || (!d_in && in_bytes) || n >= (1ull << 32)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    if (const char *why = streams_refuse(e, p)) return fail(e, ZGPU_STREAM_ERROR, why);
    if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(e, ZGPU_STREAM_ERROR, "many streams in one call: the output must be 4-byte aligned");
    *res = zgpu_deflate_result{}; res->adler32 = 1; res->data_type = 2;
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    std::vector<uint64_t> in_off(n + 1), oo(n + 1); // the call is blocking: it reads its tables
    ZGPU_HIP_CHECK(hipMemcpyAsync(in_off.data(), d_in_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipMemcpyAsync(oo.data(), d_out_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (const char *why = streams_tables_refuse(in_off.data(), oo.data(), n, in_bytes, out_cap)) return fail(e, ZGPU_STREAM_ERROR, why);
    return streams_run(e, static_cast<const uint8_t *>(d_in), in_bytes, d_in_offsets, in_off.data(), n, p, static_cast<uint8_t *>(d_out), d_out_offsets, d_items, res, st);
}

int zgpu_deflate_streams_host(zgpu_engine *e, const void *in, const uint64_t *in_offsets, uint64_t n, const zgpu_deflate_params *p, void *out, uint64_t out_cap, uint64_t *out_offsets,
                              zgpu_deflate_batch_item *items, zgpu_deflate_result *res)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!p || !res || (n && (!in_offsets || !out_offsets || !items)) || n >= (1ull << 32)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    if (const char *why = streams_refuse(e, p)) return fail(e, ZGPU_STREAM_ERROR, why);
    *res = zgpu_deflate_result{}; res->adler32 = 1; res->data_type = 2;
    if (n == 0) { if (out_offsets) out_offsets[0] = 0; return ZGPU_OK; }
    if (in_offsets[0] != 0) return fail(e, ZGPU_STREAM_ERROR, "many streams in one call: the first item starts at offset 0");
    const uint64_t in_bytes = in_offsets[n];
    if ((!in && in_bytes) || (!out && out_cap)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    std::vector<uint64_t> oo(n + 1);
    uint64_t rooms = 0;
    if (!streams_layout(in_offsets, n, p->flags, oo.data(), &rooms)) return fail(e, ZGPU_STREAM_ERROR, "many streams in one call: a table runs backwards");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const hipStream_t st = e->stream;
    int rc;
    if ((rc = ensure_stage(e, in_bytes, rooms)) || (rc = e->ds_in_off.reserve(e, n + 1)) || (rc = e->ds_oo.reserve(e, n + 1)) || (rc = e->ds_po.reserve(e, n + 1)) || (rc = e->ds_items.reserve(e, n))) return rc;
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, in, in_bytes, hipMemcpyHostToDevice, st));
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->ds_in_off, in_offsets, (n + 1) * 8, hipMemcpyHostToDevice, st));
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->ds_oo, oo.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if ((rc = streams_run(e, e->stage_in, in_bytes, e->ds_in_off, in_offsets, n, p, e->stage_out, e->ds_oo, e->ds_items, res, st))) return rc;
    // the records, then the streams packed back to back on the device and home in one copy
    ZGPU_HIP_CHECK(hipMemcpyAsync(items, e->ds_items, n * sizeof(zgpu_deflate_batch_item), hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    uint64_t at = 0;
    for (uint64_t k = 0; k < n; k++) { out_offsets[k] = at; items[k].out_lo = at; at += items[k].out_bytes; }
    out_offsets[n] = at;
    if (at > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    if (at == 0) return ZGPU_OK;
    if ((rc = e->ds_packed.reserve(e, at + 16))) return rc;
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->ds_po, out_offsets, (n + 1) * 8, hipMemcpyHostToDevice, st));
    launch_streams_pack(e->stage_out, e->ds_oo, e->ds_po, n, at, e->ds_packed, st);
    ZGPU_HIP_CHECK(hipGetLastError());
    ZGPU_HIP_CHECK(hipMemcpyAsync(out, e->ds_packed, at, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    return ZGPU_OK;
}

#pragma GCC visibility pop
} // extern "C"
