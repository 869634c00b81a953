// zgpu_deflate_streams.hip -- host side of the batch compress of MANY independent streams of any length (zgpu_deflate_streams_* in include/zamd_gpu.h): item k
// becomes exactly the bytes the reference's one-call stream gives for that item alone, and the tiles of all items share the launches.
// zgpu_deflate_streams_plan.h has what the call decides from plain numbers, zgpu_streams.hip the small kernels around the streams.  No kernel lives here.
//
// A continuous stream is cut into tiles (zgpu_cont.hip); sort, walkers, the chain of entries and the token parse treat a tile as a chunk and never needed
// the tiles of a launch to belong to one stream: here they come as one list over all items, described row by row (TileRow) instead of by the one
// stream's scalars, in batches that end wherever they end -- also inside a stream.  That is ONE set of LZ launches per batch of tiles whatever the
// number of streams.  The block layer (chains 2-4: tokens -> blocks -> bit positions -> carry) is zgpu_cont.hip's as it stands, launched once per
// stream of the batch with that stream's pointers, its own ContState and a ChunkGeom / TileGeom that describe the stream alone -- but for block
// construction, which is ONE launch over the blocks of all streams of the batch (huffman_kernel<true, true>).  Nothing between those launches waits
// for the host.
#include "zgpu_engine.h"
#include "zgpu_deflate_streams_plan.h"
#include <cstdlib>
#include <vector>

namespace zgpu {

static int reserve_streams(zgpu_engine *e, uint64_t n, uint64_t ntiles, uint32_t batch, uint64_t max_streams, uint64_t max_tok, uint64_t max_blk)
{
    int rc = ensure_deflate_ws(e, batch, false, 1);
    if (rc) return rc;
    const uint32_t ngroups = chain_groups(batch);
    if ((rc = e->ds_rows.reserve(e, ntiles + 1)) || (rc = e->ds_entry.reserve(e, ntiles + 2)) || (rc = e->ds_st.reserve(e, n)) || (rc = e->ds_check.reserve(e, n)) ||
        (rc = e->ds_totals.reserve(e, 4)) || (rc = e->ds_tokoff.reserve(e, (size_t)batch + max_streams + 1))) return rc;
    if ((rc = e->ct_exits.reserve(e, (size_t)batch * kTileExitStride)) || (rc = e->ct_comp.reserve(e, (size_t)ngroups * kTileExitStride)) || (rc = e->ct_gentry.reserve(e, (size_t)ngroups + 1)) ||
        (rc = e->ct_carry.reserve(e, kStreamsCarry)) || (rc = e->ct_T.reserve(e, max_tok)) || (rc = e->ct_blk.reserve(e, max_blk)) ||
        (rc = e->ct_pos.reserve(e, max_blk + max_streams + 1)) || (rc = e->ct_slots.reserve(e, max_blk * kSlotStride))) return rc;
    return ZGPU_OK;
}

// What the batches of one call share
struct StreamsRun {
    const uint8_t *d_in; const uint64_t *in_off; // (host copy of the table)
    uint8_t *d_out; const uint64_t *oo;          // (host copy)
    const uint64_t *tile0; uint64_t n; uint32_t flags;
    LevelCfg cfg; hipStream_t st;
};

// One stream's tiles [pt.a, pt.b) of the batch that starts at tile t0, in the block layer (chains 2-4 with the stream's own state).  j: the stream's number
// within the batch; toff, boff: where its tokens and blocks lie in the batch's buffers
struct StreamBlocks {
    ChunkGeom g{}; TileGeom tg{};
    uint64_t L, seg_here; bool ends; size_t c0; uint32_t nblk_cap;
    ContState *cs; uint32_t *T; ContBlk *blk; uint8_t *slots; uint64_t *pos; uint32_t *tokoff;
    StreamBlocks(zgpu_engine *e, const StreamsRun &r, const StreamsPart &pt, uint64_t t0, uint64_t j, uint64_t toff, uint64_t boff)
    {
        const uint64_t k = pt.item;
        const uint32_t nt = (uint32_t)(pt.b - pt.a);
        L = r.in_off[k + 1] - r.in_off[k]; ends = pt.ends; seg_here = pt.ends ? L : ~0ull; c0 = (size_t)(pt.a - t0); nblk_cap = streams_blk_cap(nt);
        g.in = r.d_in + r.in_off[k]; g.in_bytes = L; g.chunk_size = kChunkMax; g.final_chunk = ~0ull; g.block_tokens = kBlockTokens; g.slot_stride = kSlotStride;
        g.tile_w0 = 0; g.tile_stride = kTileStride; g.chunk0 = pt.a - r.tile0[k]; g.nchunks = nt; // (the stream's own tile numbers: one stream's scalars say the rest)
        tg.abs0 = 0; tg.e0 = 0; tg.end = L; tg.nil_pos = ~0ull; tg.abs0_nil = 1;
        tg.entry = e->ds_entry + r.tile0[k];                                                       // entry[g.chunk0 + c] is the list's entry of that tile
        cs = e->ds_st + k; T = e->ct_T + toff; blk = e->ct_blk + boff; slots = e->ct_slots + boff * kSlotStride; pos = e->ct_pos + boff + j; tokoff = e->ds_tokoff + c0 + j;
    }
    // chain 2: the stream's tokens into its run of the batch's token array, its blocks' table
    void tokens(zgpu_engine *e, const StreamsRun &r) const
    {
        launch_cont_tokens(g, tg, e->tokens + c0 * kChunkMax, e->meta + c0, cs, tokoff, e->ct_carry, T, blk, seg_here, ends, ends ? cont_special_pos(L) : ~0ull, nblk_cap, r.cfg.slow != 0, r.st);
    }
    // chains 3 and 4: bit positions, the blocks into the stream's room, the carry
    void stitch(zgpu_engine *e, const StreamsRun &r, uint64_t k) const
    {
        launch_cont_stitch(blk, cs, pos, slots, kSlotStride, g.in, 0, r.d_out + r.oo[k], streams_room_cap(r.oo[k + 1] - r.oo[k], r.flags), nblk_cap, T, e->ct_carry, seg_here, r.st);
    }
};

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

// The call with its tables on both sides: h_in_off / h_oo are the host's copies of d_in_off / d_oo (checked by the caller)
static int streams_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, const uint64_t *h_in_off, uint64_t n, const zgpu_deflate_params *p, uint8_t *d_out,
                       const uint64_t *d_oo, const uint64_t *h_oo, zgpu_deflate_batch_item *d_items, zgpu_deflate_result *res, hipStream_t st)
{
    int rc;
    std::vector<uint64_t> tile0(n + 1);
    if (!streams_tile_scan(h_in_off, n, tile0.data())) return fail(e, ZGPU_STREAM_ERROR, "many streams in one call: an item of 4 GiB or more");
    const uint64_t ntiles = tile0[n];
    const LevelCfg cfg = level_cfg_for(e, p->level, p->strategy);
    ContKnobs kn;
    kn.batch_tiles = env_u32("ZGPU_CONT_BATCH_TILES", 0); kn.batch_tiles_set = getenv("ZGPU_CONT_BATCH_TILES") != nullptr; // (read per call)
    const uint32_t batch = streams_batch_tiles(ntiles, plan_engine(e, &cfg), kn);
    uint64_t max_streams = 1, max_tok = 1, max_blk = 1;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += batch) {
        uint64_t s, t, b;
        streams_batch_needs(tile0.data(), n, t0, (uint32_t)(ntiles - t0 < batch ? ntiles - t0 : batch), &s, &t, &b);
        if (s > max_streams) max_streams = s;
        if (t > max_tok) max_tok = t;
        if (b > max_blk) max_blk = b;
    }
    if ((rc = reserve_streams(e, n, ntiles, batch, max_streams, max_tok, max_blk))) return rc;
    // the streams' parts of every batch, as the one block-construction launch of a batch finds its streams (one copy for the whole call)
    std::vector<StreamsBlkPart> parts;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += batch) {
        const uint32_t nb = (uint32_t)(ntiles - t0 < batch ? ntiles - t0 : batch);
        uint64_t toff = 0, boff = 0;
        StreamsPart pt;
        for (uint64_t k = streams_item_of(tile0.data(), n, t0); k < n && tile0[k] < t0 + nb; k++) {
            if (!streams_part(tile0.data(), k, t0, nb, &pt)) continue;
            parts.push_back(StreamsBlkPart{(uint32_t)boff, (uint32_t)toff, (uint32_t)k, 0u});
            const uint32_t nt = (uint32_t)(pt.b - pt.a);
            toff += streams_tok_cap(nt); boff += streams_blk_cap(nt);
        }
    }
    if ((rc = e->ds_parts.reserve(e, parts.size() + 1)) || (rc = e->ds_blk_item.reserve(e, max_blk))) return rc;
    if (!parts.empty()) ZGPU_HIP_CHECK(hipMemcpyAsync(e->ds_parts, parts.data(), parts.size() * sizeof(StreamsBlkPart), hipMemcpyHostToDevice, st)); // (waited for below, with the rows)
    size_t part0 = 0;
    // the rows of all tiles
    {
        std::vector<TileRow> rows(ntiles);
        for (uint64_t k = 0; k < n; k++)
            for (uint64_t ti = 0, nt = tile0[k + 1] - tile0[k]; ti < nt; ti++) rows[tile0[k] + ti] = streams_tile_row(h_in_off[k], h_in_off[k + 1] - h_in_off[k], ti);
        if (ntiles) ZGPU_HIP_CHECK(hipMemcpyAsync(e->ds_rows, rows.data(), ntiles * sizeof(TileRow), hipMemcpyHostToDevice, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st)); // (the vector goes out of scope)
    }
    const bool wrap = p->flags & ZGPU_F_ZLIB_WRAP, gz = p->flags & ZGPU_F_GZIP_WRAP, want_crc = gz || (p->flags & ZGPU_F_CRC32);
    const FrameHead fh = frame_head(p->level, p->strategy, wrap, gz);
    launch_streams_head(d_in_off, d_oo, n, fh, p->flags, e->ds_st, d_out, e->ds_entry, e->ds_totals, st);
    const bool check_sort = !e->exact_sort;
    if (check_sort) ZGPU_HIP_CHECK(hipMemsetAsync(lz_sorted_fault_word(e->par_ws), 0, 4, st));
    StreamsRun r{d_in, h_in_off, d_out, h_oo, tile0.data(), n, p->flags, cfg, st};
    ChunkGeom g{}; TileGeom tg{};
    g.in = d_in; g.in_bytes = in_bytes; g.chunk_size = kChunkMax; g.final_chunk = ~0ull; g.block_tokens = kBlockTokens; g.slot_stride = kSlotStride;
    g.tile_stride = kTileStride; // (with g.rows: the tiles come row by row)
    tg.nil_pos = ~0ull; tg.exits = e->ct_exits; tg.entry = e->ds_entry;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += batch) {
        const uint32_t nb = (uint32_t)(ntiles - t0 < batch ? ntiles - t0 : batch);
        g.chunk0 = t0; g.nchunks = nb; g.rows = e->ds_rows + t0;
        // the LZ stage: one set of launches for the batch's tiles, whatever streams they belong to
        launch_lz_tiles(g, tg, cfg, e->par_ws, e->meta, e->ct_comp, e->ct_gentry, st, e, e->exact_sort);
        launch_streams_entry(g.rows, nb, e->ds_entry + t0, st);
        launch_lz_tiles_parse(g, tg, cfg, e->par_ws, e->tokens, e->meta, st, e);
        // the block layer, no wait for the host anywhere: every stream's tokens and block table (launches per stream), ONE block-construction launch over the
        // blocks of all streams of the batch, every stream's bits into its room (launches per stream)
        std::vector<StreamBlocks> sb;
        std::vector<uint64_t> items_of;
        uint64_t toff = 0, boff = 0;
        StreamsPart pt;
        for (uint64_t k = streams_item_of(tile0.data(), n, t0); k < n && tile0[k] < t0 + nb; k++) {
            if (!streams_part(tile0.data(), k, t0, nb, &pt)) continue;
            sb.emplace_back(e, r, pt, t0, (uint64_t)sb.size(), toff, boff);
            items_of.push_back(k);
            const uint32_t nt = (uint32_t)(pt.b - pt.a);
            toff += streams_tok_cap(nt); boff += streams_blk_cap(nt);
        }
        {
            StageTimer t(e, st, ZGPU_STAGE_PARSE);
            for (const StreamBlocks &s : sb) s.tokens(e, r);
            launch_streams_blocks(e->ds_parts + part0, (uint32_t)sb.size(), (uint32_t)boff, e->ds_st, e->ct_blk, e->ds_blk_item, st);
        }
        {
            StageTimer t(e, st, ZGPU_STAGE_HUFFMAN);
            launch_huffman_streams(sb[0].g, e->ct_T, (uint32_t)boff, e->ct_blk, e->ds_st, e->ds_blk_item, e->ct_slots, st, cfg.strategy == kFixed); // (g: block_tokens and slot_stride only)
        }
        {
            StageTimer t(e, st, ZGPU_STAGE_STITCH);
            for (size_t i = 0; i < sb.size(); i++) sb[i].stitch(e, r, items_of[i]);
        }
        part0 += sb.size();
        const hipError_t he = hipGetLastError();
        if (he != hipSuccess) return fail_hip(e, he, "kernel launch", __FILE__, __LINE__);
    }
    // checksums of every item, trailers, records
    {
        StageTimer t(e, st, ZGPU_STAGE_STITCH);
        if ((rc = checksum_batch_run(e, d_in, in_bytes, d_in_off, n, want_crc ? 3u : 1u, e->ds_check, st))) return rc;
        launch_streams_finish(d_in_off, d_oo, n, fh, p->flags, e->ds_st, e->ds_check, want_crc, d_out, d_items, e->ds_totals, st);
    }
    unsigned long long totals[3] = {0, 0, 0};
    uint32_t sort_fault = 0;
    zgpu_deflate_batch_item last{};
    ZGPU_HIP_CHECK(hipMemcpyAsync(totals, e->ds_totals, sizeof totals, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipMemcpyAsync(&last, d_items + (n - 1), sizeof last, hipMemcpyDeviceToHost, st));
    if (check_sort && ntiles) ZGPU_HIP_CHECK(hipMemcpyAsync(&sort_fault, lz_sorted_fault_word(e->par_ws), 4, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    collect_spans(e);
    if (sort_fault) { e->exact_sort = 1; return streams_run(e, d_in, in_bytes, d_in_off, h_in_off, n, p, d_out, d_oo, h_oo, d_items, res, st); } // (the input is untouched: the whole call again with the exact sort)
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
    return streams_run(e, static_cast<const uint8_t *>(d_in), in_bytes, d_in_offsets, in_off.data(), n, p, static_cast<uint8_t *>(d_out), d_out_offsets, oo.data(), d_items, res, st);
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
    if ((rc = streams_run(e, e->stage_in, in_bytes, e->ds_in_off, in_offsets, n, p, e->stage_out, e->ds_oo, oo.data(), e->ds_items, res, st))) return rc;
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
