// zgpu_deflate_cont.hip -- host side of the continuous stream (zgpu_cont.hip has the plan of the stream, zgpu_deflate_plan.h the sizes of a feed): deflate_cont,
// one feed in batches of tiles; lz_tiles_fast, the rounds of a batch at levels 1-3; the one-shot form behind ZGPU_F_CONTINUOUS and the C entry points of
// the feeds in include/zamd_gpu.h.  No kernel lives here.
#include "zgpu_engine.h"
#include "zgpu_deflate_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <algorithm>

namespace zgpu {

constexpr uint32_t kContCarry = 16384;
static int ensure_cont_ws(zgpu_engine *e, uint32_t batch_tiles, uint64_t feed_tiles)
{
    int rc;
    if ((rc = e->ct_st.reserve(e, 1))) return rc;
    if ((rc = e->ct_carry.reserve(e, kContCarry))) return rc;
    if ((rc = e->ct_carry_in.reserve(e, kContCarry))) return rc;
    if (feed_tiles + 2 > e->ct_entry.cap && (rc = e->ct_entry.reserve(e, feed_tiles + 2 + 1024))) return rc;
    const size_t ntok_cap = (size_t)kContCarry + kChunkMax + (size_t)batch_tiles * (kTileStride + kTileSlack); // tile 0 of a feed parses up to 65024 positions, the others 32512, + the last game's overhang
    const uint32_t nblk_cap = (uint32_t)(ntok_cap / kBlockTokens + 2);
    const uint32_t ngroups = chain_groups(batch_tiles);
    if ((rc = e->ct_exits.reserve(e, (size_t)batch_tiles * kTileExitStride))) return rc;
    if ((rc = e->ct_comp.reserve(e, (size_t)ngroups * kTileExitStride))) return rc;
    if ((rc = e->ct_gentry.reserve(e, (size_t)ngroups + 1))) return rc;
    if ((rc = e->ct_tokoff.reserve(e, (size_t)batch_tiles + 1))) return rc;
    if ((rc = e->ct_T.reserve(e, ntok_cap))) return rc;
    if ((rc = e->ct_blk.reserve(e, (size_t)nblk_cap))) return rc;
    if ((rc = e->ct_pos.reserve(e, (size_t)nblk_cap + 1))) return rc;
    return e->ct_slots.reserve(e, (size_t)nblk_cap * kSlotStride);
}

static int ensure_fast_ws(zgpu_engine *e, uint32_t batch_tiles)
{
    int rc;
    if ((rc = e->cf_prev.reserve(e, kInsWords + 8))) return rc;
    if ((rc = e->cf_prev2.reserve(e, kInsWords + 8))) return rc;
    if ((rc = e->cf_hist.reserve(e, kInsWords + 8))) return rc;
    if ((rc = e->cf_count.reserve(e, 4))) return rc;
    if ((rc = e->cf_exit_a.reserve(e, (size_t)batch_tiles))) return rc;
    if ((rc = e->cf_exit_b.reserve(e, (size_t)batch_tiles))) return rc;
    if ((rc = e->cf_ins0.reserve(e, (size_t)batch_tiles * kInsWords))) return rc;
    if ((rc = e->cf_ins1.reserve(e, (size_t)batch_tiles * kInsWords))) return rc;
    if ((rc = e->cf_cur.reserve(e, (size_t)batch_tiles))) return rc;
    if ((rc = e->cf_act_a.reserve(e, (size_t)batch_tiles))) return rc;
    if ((rc = e->cf_act_b.reserve(e, (size_t)batch_tiles))) return rc;
    if ((rc = e->cf_changed.reserve(e, (size_t)batch_tiles))) return rc;
    if ((rc = e->cf_list_a.reserve(e, (size_t)batch_tiles))) return rc;
    if ((rc = e->cf_list_b.reserve(e, (size_t)batch_tiles))) return rc;
    if ((rc = e->cf_kept.reserve(e, (size_t)batch_tiles))) return rc;
    if ((rc = e->cf_used.reserve(e, (size_t)batch_tiles * kInsWords))) return rc;
    return e->cf_entry_used.reserve(e, (size_t)batch_tiles);
}

static ContKnobs read_cont_knobs()
{
    ContKnobs kn;
    kn.batch_tiles = env_u32("ZGPU_CONT_BATCH_TILES", 0); kn.batch_tiles_set = getenv("ZGPU_CONT_BATCH_TILES") != nullptr;
    { const char *v = getenv("ZGPU_CONT_PIPE"); if (v && *v) kn.pipe = atoi(v); }
    kn.fast_run = env_u32("ZGPU_FAST_RUN", 0);
    kn.trace = getenv("ZGPU_FAST_TRACE") != nullptr;
    kn.stats = getenv("ZGPU_FAST_STATS") != nullptr;
    return kn;
}

// Everything of lz_tiles_fast that is there for ZGPU_FAST_TRACE (what every round did, to stderr) and ZGPU_FAST_FORCE_ROUNDS=n (debug: every tile is
// parsed again in each of the first n rounds) and ZGPU_FAST_STATS (the trace's six counters summed into the engine, zgpu_deflate_fast_count); with none set
// no member does anything
struct FastDebug {
    zgpu_engine *e; uint32_t nb; hipStream_t st;
    bool trace = false, stats = false; int force = 0;
    int init(zgpu_engine *e_, uint32_t nb_, bool trace_, bool stats_, hipStream_t st_)
    {
        e = e_; nb = nb_; st = st_; trace = trace_; stats = stats_;
        static int force_env = -1; // (read once a process)
        if (force_env < 0) { const char *v = getenv("ZGPU_FAST_FORCE_ROUNDS"); force_env = v ? atoi(v) : 0; }
        force = force_env;
        if (trace && e->cf_dbg.reserve(e, 65536 * 8)) return ZGPU_MEM_ERROR;
        if ((trace || stats) && e->cf_dstat.reserve(e, 8)) return ZGPU_MEM_ERROR;
        return ZGPU_OK;
    }
    void arm(FastTiles &ft) const // the kernel's records of a launch: eight words per tile, eight counters
    {
        ft.dbg = trace && nb <= 65536 ? static_cast<uint32_t *>(e->cf_dbg) : nullptr;
        if (trace || stats) { hipMemsetAsync(e->cf_dstat, 0, 32, st); ft.stat = e->cf_dstat; }
    }
    // ZGPU_FAST_STATS: the round's counters come back with the round's own read-back (queued in front of its synchronise) and are summed behind it.  They count
    // tiles that are parsed AGAIN: the launches of round 0 in phases (fast_round0_phases) clear them and nobody reads them, no tile has old results there
    int read_stats(uint32_t *hs) const { if (stats) ZGPU_HIP_CHECK(hipMemcpyAsync(hs, e->cf_dstat, 32, hipMemcpyDeviceToHost, st)); return ZGPU_OK; }
    void add_stats(const uint32_t *hs) const { if (stats) for (int i = 0; i < 6; i++) e->cf_stat[i] += hs[i]; }
    void phases_done(uint32_t K, size_t nheads) const { if (trace) fprintf(stderr, "fast tiles: round 0 in %u phases, %zu run heads to parse again\n", K, nheads); }
    void before_round(const FastTiles &ft) const { if (ft.dbg) hipMemsetAsync(e->cf_dbg, 0xff, (size_t)nb * 32, st); }
    void after_launch(const FastTiles &ft) const
    {
        if (!ft.dbg) return;
        std::vector<uint32_t> h((size_t)nb * 8);
        hipMemcpyAsync(h.data(), e->cf_dbg, (size_t)nb * 32, hipMemcpyDeviceToHost, st); hipStreamSynchronize(st);
        uint32_t shown = 0;
        for (uint32_t c = 0; c < nb && shown < 6; c++) if (h[c * 8] != 0xffffffffu && ++shown)
            fprintf(stderr, "   tile %u: %u words differ (%u .. %u), exit %u (was %u), entry %u, %u tokens\n", c, h[c * 8 + 1], h[c * 8 + 2], h[c * 8 + 3], h[c * 8 + 4], h[c * 8 + 5], h[c * 8 + 6], h[c * 8 + 7]);
    }
    // a forced round: all tiles but the first again (the list is 1 .. nb - 1), whatever the flip found
    int force_round(uint32_t round, uint8_t *act_next, uint32_t *list_next, uint32_t *active) const
    {
        if ((int)round >= force || nb <= 1) return ZGPU_OK;
        std::vector<uint32_t> all(nb - 1);
        for (uint32_t i = 1; i < nb; i++) all[i - 1] = i;
        ZGPU_HIP_CHECK(hipMemsetAsync(act_next + 1, 1, nb - 1, st));
        ZGPU_HIP_CHECK(hipMemcpyAsync(list_next, all.data(), (size_t)(nb - 1) * 4, hipMemcpyHostToDevice, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        *active = nb - 1;
        return ZGPU_OK;
    }
    void round_done(uint32_t round, uint32_t active) const
    {
        if (!trace) return;
        static double t_last = 0; timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); const double t_now = ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
        fprintf(stderr, "[%.2f ms since the last round's end] ", t_now - t_last); t_last = t_now;
        uint32_t hs[8] = {};
        hipMemcpy(hs, e->cf_dstat, 32, hipMemcpyDeviceToHost);
        fprintf(stderr, "fast tiles: round %u, %u of %u tiles to parse again (this round: %u entered where they had, %u stopped early, %u met a different token, %u had changes within reach to the end; first different token after %u of %u windows)\n", round, active, nb, hs[0], hs[1], hs[2], hs[3], hs[4], hs[5]);
    }
};

// What the launches of one batch's rounds share (lz_tiles_fast)
struct FastRun {
    zgpu_engine *e; const ChunkGeom &g; const TileGeom &tg; const LevelCfg &cfg; hipStream_t st;
    const uint16_t *S; const uint32_t *ir; // the batch's sorted buckets
    uint8_t *act, *act_next;               // "parse this tile", this round's and the next one's
    FastDebug dbg;
    FastTiles tiles(uint32_t round, const uint32_t *list) const
    {
        static int keep = -1; // ZGPU_FAST_KEEP=0: every active tile is parsed to its end (A/B runs)
        if (keep < 0) { const char *v = getenv("ZGPU_FAST_KEEP"); keep = v ? atoi(v) : 1; }
        FastTiles ft{};
        ft.exit_cur = e->cf_exit_a; ft.exit_new = e->cf_exit_b; ft.ins0 = ft.ins0w = e->cf_ins0; ft.ins1 = ft.ins1w = e->cf_ins1; ft.cur = e->cf_cur; ft.active = act; ft.changed = e->cf_changed;
        ft.prev0 = e->fast_prev0 != 0; ft.before = e->before_buf;
        ft.prev_ins = e->cf_prev; ft.round = round; ft.list = list; ft.low_out = e->cf_hist; // (cf_hist: free until the feed's hand-over is put together)
        if (keep) { ft.used_ins = e->cf_used; ft.entry_used = e->cf_entry_used; ft.kept = e->cf_kept; }
        dbg.arm(ft);
        return ft;
    }
    void launch(const FastTiles &ft, uint32_t ngrid) const { launch_lz_fastwin_tiles(g, tg, ft, cfg, S, ir, e->tokens, e->meta, ngrid, st); }
    void finish() const { launch_fast_finish(e->cf_cur, e->cf_exit_a, e->cf_ins0, e->cf_ins1, g.nchunks, tg.entry + g.chunk0 + g.nchunks, e->cf_prev, e->cf_prev2, g.chunk0 == 0 ? e->cf_hist : nullptr, st); }
};

// Round 0 in K > 1 phases (plan_fast_phases says why): phase p parses the tiles p, p + K, p + 2 K ..., each from where the tile in front ended.  What the rounds
// then start with is left in cf_list_a and act: the run heads behind the first -- the tile in front of each was parsed after it.  *nheads: their number
static int fast_round0_phases(const FastRun &r, uint32_t K, uint32_t *nheads)
{
    zgpu_engine *const e = r.e;
    const uint32_t nb = r.g.nchunks;
    std::vector<uint32_t> all(nb);
    uint32_t at = 0;
    std::vector<uint32_t> start(K + 1, 0);
    for (uint32_t p = 0; p < K; p++) { start[p] = at; for (uint32_t c = p; c < nb; c += K) all[at++] = c; }
    start[K] = at;
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->cf_list_b, all.data(), (size_t)nb * 4, hipMemcpyHostToDevice, r.st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(r.st)); // (the vector goes out of scope)
    for (uint32_t p = 0; p < K; p++) {
        const uint32_t cnt = start[p + 1] - start[p];
        if (!cnt) continue;
        FastTiles ft = r.tiles(0, e->cf_list_b + start[p]);
        ft.warm_mode = p == 0;
        r.launch(ft, cnt);
        launch_fast_flip_list(e->cf_cur, e->cf_exit_a, e->cf_exit_b, e->cf_list_b + start[p], cnt, r.st);
        e->cf_tile_parses += cnt;
    }
    e->cf_rounds++;
    std::vector<uint32_t> heads;
    std::vector<uint8_t> ab(nb, 0);
    for (uint32_t c = K; c < nb; c += K) { heads.push_back(c); ab[c] = 1; }
    *nheads = (uint32_t)heads.size();
    if (heads.empty()) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->cf_list_a, heads.data(), heads.size() * 4, hipMemcpyHostToDevice, r.st));
    ZGPU_HIP_CHECK(hipMemcpyAsync(r.act, ab.data(), nb, hipMemcpyHostToDevice, r.st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(r.st));
    r.dbg.phases_done(K, heads.size());
    return ZGPU_OK;
}

// levels 1-3: the tiles of one batch by rounds (zgpu_lz_fastwin.hip, fastwin_tile_kernel): until no tile's predecessor has changed
static int lz_tiles_fast(zgpu_engine *e, const ChunkGeom &g, const TileGeom &tg, const LevelCfg &cfg, const ContKnobs &kn, hipStream_t st)
{
    const uint32_t nb = g.nchunks;
    FastRun r{e, g, tg, cfg, st, nullptr, nullptr, e->cf_act_a, e->cf_act_b, {}};
    launch_sort_tiles(g, e->par_ws, e->meta, st, e, e->exact_sort, &r.S, &r.ir);
    StageTimer t(e, st, ZGPU_STAGE_MATCH);
    launch_fast_init(e->cf_cur, e->cf_act_a, e->cf_exit_a, nb, st);
    uint32_t *list = nullptr, *list_next = e->cf_list_a, ngrid = nb;
    int rc = r.dbg.init(e, nb, kn.trace, kn.stats, st);
    if (rc) return rc;
    const uint32_t K = plan_fast_phases(nb, kn.fast_run);
    if (K > 1) {
        if ((rc = fast_round0_phases(r, K, &ngrid))) return rc;
        if (ngrid == 0) { r.finish(); return ZGPU_OK; } // (one run: no tile was parsed in front of its predecessor)
        list = e->cf_list_a; list_next = e->cf_list_b;
        e->cf_tile_parses += ngrid;
    }
    for (uint32_t round = K > 1 ? 1 : 0;; round++) {
        FastTiles ft = r.tiles(round, list);
        ft.warm_mode = round == 0;
        r.dbg.before_round(ft);
        r.launch(ft, ngrid);
        r.dbg.after_launch(ft);
        launch_fast_flip(e->cf_cur, r.act, r.act_next, e->cf_changed, e->cf_exit_a, e->cf_exit_b, nb, round, e->cf_count, list_next, ft.kept, st);
        uint32_t active = 0, hs[8] = {};
        ZGPU_HIP_CHECK(hipMemcpyAsync(&active, e->cf_count, 4, hipMemcpyDeviceToHost, st));
        if ((rc = r.dbg.read_stats(hs))) return rc;
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        r.dbg.add_stats(hs);
        e->cf_rounds++; e->cf_tile_parses += round == 0 ? nb : 0;
        if ((rc = r.dbg.force_round(round, r.act_next, list_next, &active))) return rc;
        r.dbg.round_done(round, active);
        if (active == 0) break;
        e->cf_tile_parses += active;
        std::swap(r.act, r.act_next);
        list = list_next; list_next = list == e->cf_list_a ? e->cf_list_b : e->cf_list_a; ngrid = active;
    }
    r.finish();
    return ZGPU_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// One FEED of a continuous stream (zgpu_cont.hip has the plan): d_buf holds the history the parse can still reach followed by the bytes that have
// not been parsed yet, cs says where the stream stands (absolute stream positions) and receives where it stands afterwards, d_carry_in holds the
// tokens of the block that is filling (device memory, cs->carry_ntok words, not e->ct_carry); the ones the feed leaves behind are in e->ct_carry.  The output starts at bit cs->bit_count of d_out's byte 0 ... in general at bit
// `prefix_bits` of d_out: the caller has put the bytes in front (a wrapper's header) and the bits of the unfinished byte there, zero-filled to a whole word.
struct ContFeed { // one call of deflate_cont
    const uint8_t *d_buf; uint64_t buf_bytes; // history + unparsed bytes
    uint64_t check_from;                      // Adler-32 / CRC-32 of d_buf[check_from ..): the bytes this feed brought (buf_bytes: none)
    int mode;                                 // ZGPU_CONT_*
    const uint64_t *h_excl; uint32_t nexcl;   // stream positions that are not in the hash chains (in front of earlier flushes), ascending
    uint8_t *d_out; uint64_t out_cap; uint64_t prefix_bits;
    bool want_crc;
    uint32_t *h_hist; // levels 1-3: "in the hash chains", one bit per position of the history (bit j: the position 32512, or all there are, in front of cs->entry, + j); in and out; kInsWords words
    LevelCfg cfg;                // the level's parameters (level_cfg_for)
    zgpu_cont_state *cs;         // in and out
    const uint32_t *d_carry_in;
    zgpu_deflate_result *res;
    hipStream_t st;
};

// the workspaces, streams and events of a planned feed
static int reserve_cont(zgpu_engine *e, const ContPlan &pl, const ContKnobs &kn)
{
    const uint32_t batch = pl.batch;
    timespec ts0; clock_gettime(CLOCK_MONOTONIC, &ts0);
    if (kn.trace) fprintf(stderr, "continuous stream: %llu tiles, memory admits %u, batches of %u (held: %u tiles, %u chunks of tokens, %u of buckets)\n", (unsigned long long)pl.ntiles, pl.batch_fit, batch, e->ct_tiles(), e->batch_cap(), e->par_cap);
    int rc = ensure_deflate_ws(e, pl.pipe ? 2 * batch + 1 : batch, false, 1);
    if (rc) return rc;
    if ((rc = ensure_cont_ws(e, pl.pipe ? 2 * batch : batch, pl.ntiles))) return rc;
    if (kn.trace) { timespec ts1; clock_gettime(CLOCK_MONOTONIC, &ts1); fprintf(stderr, "continuous stream: workspaces in %.1f ms\n", (ts1.tv_sec - ts0.tv_sec) * 1e3 + (ts1.tv_nsec - ts0.tv_nsec) * 1e-6); }
    if (pl.pipe && !e->ct_stream) {
        ZGPU_HIP_CHECK(hipStreamCreateWithFlags(&e->ct_stream, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) { ZGPU_HIP_CHECK(hipEventCreateWithFlags(&e->ct_ev_a[i], hipEventDisableTiming)); ZGPU_HIP_CHECK(hipEventCreateWithFlags(&e->ct_ev_b[i], hipEventDisableTiming)); }
    }
    if (pl.fast_lz) return ensure_fast_ws(e, batch);
    return ZGPU_OK;
}

// levels 4-9: the positions that are not in the chains, as buffer offsets in e->ct_excl; *nexcl_dev: how many of them lie in this feed's buffer
static int upload_excl(zgpu_engine *e, const ContFeed &f, uint32_t *nexcl_dev)
{
    int rc;
    const zgpu_cont_state *cs = f.cs;
    if (f.nexcl > e->ct_excl.cap && (rc = e->ct_excl.reserve(e, (size_t)f.nexcl + 64))) return rc;
    std::vector<uint64_t> off(f.nexcl);
    uint32_t k = 0;
    for (uint32_t i = 0; i < f.nexcl; i++) if (f.h_excl[i] >= cs->abs0 && f.h_excl[i] - cs->abs0 < f.buf_bytes) off[k++] = f.h_excl[i] - cs->abs0; // (buffer offsets)
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->ct_excl, off.data(), (size_t)k * 8, hipMemcpyHostToDevice, f.st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(f.st));
    *nexcl_dev = k;
    return ZGPU_OK;
}

// What the batches of one feed share
struct ContRun {
    const ContFeed &f; const ContPlan &pl; const ContKnobs &kn;
    ChunkGeom g; TileGeom tg;
    uint8_t *ws_set[2];          // the sorted buckets' workspace of either set of per-batch buffers (pipe; else both the one)
    uint64_t seg_end, sp;        // where the segment ends (~0: not in this feed), its special position
    uint32_t nblk_cap;           // blocks the per-batch buffers have room for
    hipStream_t sb;              // where a batch's blocks are made
};

// batch kbatch of the feed, tiles [t0, t0 + nb): sort and match on the feed's stream, tokens, blocks and bits on r.sb
static int cont_batch(zgpu_engine *e, ContRun &r, uint64_t t0, uint64_t kbatch)
{
    const ContFeed &f = r.f;
    const ContPlan &pl = r.pl;
    const hipStream_t st = f.st, sb = r.sb;
    const uint32_t batch = pl.batch, nb = (uint32_t)(pl.ntiles - t0 < batch ? pl.ntiles - t0 : batch);
    const bool last_batch = t0 + nb >= pl.ntiles, ends = f.mode != ZGPU_CONT_MORE;
    const int set = pl.pipe ? (int)(kbatch & 1) : 0;
    uint32_t *const tokens = e->tokens + (size_t)set * batch * kChunkMax;
    ChunkMeta *const tmeta = e->meta + (size_t)set * batch;
    ChunkGeom &g = r.g; TileGeom &tg = r.tg;
    int rc;
    tg.exits = e->ct_exits + (size_t)set * batch * kTileExitStride;
    g.chunk0 = t0; g.nchunks = nb;
    if (pl.pipe && kbatch >= 2) ZGPU_HIP_CHECK(hipStreamWaitEvent(st, e->ct_ev_b[set], 0)); // this set's buffers: the batch before last is done with them
    if (nb && !pl.fast_lz) launch_lz_tiles(g, tg, f.cfg, r.ws_set[set], tmeta, e->ct_comp, e->ct_gentry, st, e, e->exact_sort);
    else if (nb && (rc = lz_tiles_fast(e, g, tg, f.cfg, r.kn, st))) return rc;
    if (pl.pipe) { ZGPU_HIP_CHECK(hipEventRecord(e->ct_ev_a[set], st)); ZGPU_HIP_CHECK(hipStreamWaitEvent(sb, e->ct_ev_a[set], 0)); }
    if (nb && !pl.fast_lz) launch_lz_tiles_parse(g, tg, f.cfg, r.ws_set[set], tokens, tmeta, sb, e);
    const uint64_t seg_here = (ends && last_batch) ? r.seg_end : ~0ull;
    {
        StageTimer t(e, sb, ZGPU_STAGE_PARSE);
        launch_cont_tokens(g, tg, tokens, tmeta, e->ct_st, e->ct_tokoff, t0 == 0 ? f.d_carry_in : e->ct_carry, e->ct_T, e->ct_blk, seg_here, f.mode == ZGPU_CONT_FINISH && seg_here != ~0ull, seg_here != ~0ull ? r.sp : ~0ull, r.nblk_cap, f.cfg.slow != 0, sb);
    }
    {
        StageTimer t(e, sb, ZGPU_STAGE_HUFFMAN);
        launch_huffman_cont(g, e->ct_T, r.nblk_cap, e->ct_blk, e->ct_st, e->ct_slots, sb, f.cfg.strategy == kFixed);
    }
    {
        StageTimer t(e, sb, ZGPU_STAGE_STITCH);
        launch_cont_stitch(e->ct_blk, e->ct_st, e->ct_pos, e->ct_slots, kSlotStride, f.d_buf, f.cs->abs0, f.d_out, f.out_cap & ~3ull, r.nblk_cap, e->ct_T, e->ct_carry, seg_here, sb);
    }
    if (pl.pipe) ZGPU_HIP_CHECK(hipEventRecord(e->ct_ev_b[set], sb));
    const hipError_t he = hipGetLastError();
    if (he != hipSuccess) return zgpu::fail_hip(e, he, "kernel launch", __FILE__, __LINE__);
    return ZGPU_OK;
}

// The state after the feed: where the stream stands now (cs), levels 1-3 the history's bits for the next feed, the result.  k_next: where the tile behind
// the last one would be entered
static int cont_state_after(zgpu_engine *e, const ContFeed &f, const ContPlan &pl, const ContState &hs, uint16_t k_next, uint32_t adler, uint32_t crc)
{
    zgpu_cont_state *const cs = f.cs;
    const hipStream_t st = f.st;
    const uint64_t ntiles = pl.ntiles, w0 = pl.w0;
    if (ntiles) {
        const uint64_t wb_last = w0 + (ntiles - 1) * kTileStride, lim = pl.end - wb_last, h1_last = lim < kTileH1 ? lim : kTileH1;
        cs->entry = cs->abs0 + wb_last + h1_last + k_next;
    }
    if (pl.fast_lz && ntiles) { // the history's bits for the next feed: the 32512 positions (or all there are) in front of where the parse stands
        const uint64_t wb_last = w0 + (ntiles - 1) * kTileStride, e_buf = cs->entry - cs->abs0, nw0 = e_buf > kTileStride && e_buf - kTileStride > w0 ? e_buf - kTileStride : w0;
        const uint32_t x0 = (uint32_t)(nw0 - wb_last), count = (uint32_t)(e_buf - nw0);
        launch_fast_hist(e->cf_prev2, e->cf_prev, x0, count, e->cf_hist, st);
        ZGPU_HIP_CHECK(hipMemcpyAsync(f.h_hist, e->cf_hist, (size_t)kInsWords * 4, hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    }
    if (f.mode != ZGPU_CONT_MORE) cs->entry = cs->abs0 + f.buf_bytes;
    cs->block_start = hs.block_start; cs->carry_ntok = hs.carry_n; cs->data_type = hs.data_type; cs->first_block = hs.first_block; cs->last_eob = hs.last_eob;
    uint64_t out_bytes;
    if (f.mode == ZGPU_CONT_FINISH) { out_bytes = (hs.out_bits + 7) >> 3; cs->bit_count = 0; cs->bit_value = 0; } // bi_windup
    else {
        out_bytes = hs.out_bits >> 3; cs->bit_count = (uint32_t)(hs.out_bits & 7); cs->bit_value = 0;
        if (cs->bit_count) {
            uint8_t last = 0;
            ZGPU_HIP_CHECK(hipMemcpyAsync(&last, f.d_out + out_bytes, 1, hipMemcpyDeviceToHost, st));
            ZGPU_HIP_CHECK(hipStreamSynchronize(st));
            cs->bit_value = last & ((1u << cs->bit_count) - 1u);
        }
    }
    zgpu_deflate_result *const res = f.res;
    res->out_bytes = out_bytes; res->nchunks = ntiles; res->adler32 = adler; res->crc32 = crc; res->data_type = hs.data_type; res->ntokens = hs.ntokens;
    return ZGPU_OK;
}

static int deflate_cont(zgpu_engine *e, const ContFeed &f)
{
    const LevelCfg &cfg = f.cfg;
    zgpu_cont_state *const cs = f.cs;
    zgpu_deflate_result *const res = f.res;
    const hipStream_t st = f.st;
    // check and plan
    if (cont_fast_lz(cfg) && (!lz_fastwin_serves(cfg) || cfg.strategy == kRle || !f.h_hist))
        return fail(e, ZGPU_STREAM_ERROR, "continuous stream at levels 1..3: the levels' own parameters, not Z_RLE");
    if (cs->entry < cs->abs0 || cs->entry > cs->abs0 + f.buf_bytes || cs->carry_ntok >= kBlockTokens || cs->bit_count > 7) return fail(e, ZGPU_STREAM_ERROR, "continuous stream: state out of range");
    if ((reinterpret_cast<uintptr_t>(f.d_out) & 3) != 0) return fail(e, ZGPU_STREAM_ERROR, "continuous stream: the output must be 4-byte aligned");
    const ContKnobs kn = read_cont_knobs();
    const bool ends = f.mode != ZGPU_CONT_MORE;
    const ContPlan pl = plan_cont(cfg, cs->entry, cs->abs0, f.buf_bytes, f.mode, plan_engine(e, &cfg), kn);
    const uint64_t ntiles = pl.ntiles;
    if (!ends && ntiles == 0) { res->out_bytes = 0; res->nchunks = 0; res->ntokens = 0; res->adler32 = 1; res->crc32 = 0; res->data_type = cs->data_type; if (f.check_from < f.buf_bytes) return fail(e, ZGPU_STREAM_ERROR, "continuous stream: a feed that parses nothing brings no bytes"); return ZGPU_OK; }
    const uint32_t batch = pl.batch;
    // reserve the workspaces
    int rc = reserve_cont(e, pl, kn);
    if (rc) return rc;
    // the state the kernels start from
    if (pl.fast_lz) ZGPU_HIP_CHECK(hipMemcpyAsync(e->cf_prev, f.h_hist, (size_t)kInsWords * 4, hipMemcpyHostToDevice, st)); // (pageable: the copy has read it when the call returns)
    ContRun r{f, pl, kn, {}, {}, {nullptr, nullptr}, ~0ull, ~0ull, 0, nullptr};
    r.seg_end = ends ? cs->abs0 + f.buf_bytes : ~0ull; r.sp = ends ? cont_special_pos(r.seg_end) : ~0ull;
    uint32_t nexcl_dev = 0;
    if (f.nexcl && !pl.fast_lz && (rc = upload_excl(e, f, &nexcl_dev))) return rc; // (levels 1-3 know which positions are in the chains bit by bit: hist bits)
    ContState hs{};
    hs.out_bits = f.prefix_bits; hs.block_start = cs->block_start; hs.carry_n = cs->carry_ntok; hs.data_type = cs->data_type; hs.last_eob = cs->last_eob;
    hs.first_block = cs->first_block; hs.e_next = cs->entry;
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->ct_st, &hs, sizeof hs, hipMemcpyHostToDevice, st));
    { const uint16_t z = 0; ZGPU_HIP_CHECK(hipMemcpyAsync(e->ct_entry, &z, 2, hipMemcpyHostToDevice, st)); }
    const bool check_sort = !e->exact_sort;
    const size_t ws_half = (lz_sorted_workspace_bytes(batch) + 255) & ~(size_t)255;
    r.ws_set[0] = e->par_ws; r.ws_set[1] = e->par_ws + (pl.pipe ? ws_half : 0);
    if (check_sort) { ZGPU_HIP_CHECK(hipMemsetAsync(lz_sorted_fault_word(r.ws_set[0]), 0, 4, st)); if (pl.pipe) ZGPU_HIP_CHECK(hipMemsetAsync(lz_sorted_fault_word(r.ws_set[1]), 0, 4, st)); }
    ChunkGeom &g = r.g;
    g.in = f.d_buf; g.in_bytes = f.buf_bytes; g.chunk_size = kChunkMax; g.final_chunk = ~0ull; g.block_tokens = kBlockTokens; g.slot_stride = kSlotStride;
    g.tile_w0 = pl.w0; g.tile_stride = kTileStride; g.excl = nexcl_dev ? e->ct_excl : nullptr; g.nexcl = nexcl_dev;
    TileGeom &tg = r.tg;
    tg.abs0 = cs->abs0; tg.e0 = pl.e0; tg.end = pl.end; tg.nil_pos = (r.sp != ~0ull && r.sp >= cs->abs0 && r.sp < r.seg_end) ? r.sp - cs->abs0 : ~0ull; tg.abs0_nil = 1;
    tg.exits = e->ct_exits; tg.entry = e->ct_entry;
    // blocks the per-batch buffers have room for (the three grow together, ensure_cont_ws; the smallest counts should a growth ever have failed half way)
    r.nblk_cap = (uint32_t)std::min({e->ct_blk.cap, e->ct_pos.cap - 1, e->ct_slots.cap / kSlotStride});
    const hipStream_t sb = r.sb = pl.pipe ? e->ct_stream : st;
    if (pl.pipe) { ZGPU_HIP_CHECK(hipEventRecord(e->ct_ev_a[0], st)); ZGPU_HIP_CHECK(hipStreamWaitEvent(sb, e->ct_ev_a[0], 0)); } // (the second stream starts behind what the caller has queued: the input, the state)
    // the batches
    uint64_t kbatch = 0;
    for (uint64_t t0 = 0; t0 == 0 || t0 < ntiles; t0 += batch, kbatch++) { // (a feed without tiles still closes the block that is filling)
        if ((rc = cont_batch(e, r, t0, kbatch))) return rc;
        if (ntiles == 0) break;
    }
    if (pl.pipe) { ZGPU_HIP_CHECK(hipEventRecord(e->ct_ev_b[0], sb)); ZGPU_HIP_CHECK(hipStreamWaitEvent(st, e->ct_ev_b[0], 0)); } // everything the second stream has made lies in front of what follows
    // checksums of the bytes this feed brought
    uint32_t adler = 1, crc = 0;
    if (f.check_from < f.buf_bytes) {
        StageTimer t(e, st, ZGPU_STAGE_STITCH);
        if ((rc = checksum_pass(e, f.d_buf + f.check_from, f.buf_bytes - f.check_from, f.want_crc ? 3u : 1u, 65536, e->ct_ckmeta, st, &adler, &crc))) return rc;
    }
    // read back
    uint16_t k_next = 0;
    uint32_t sort_fault = 0, sort_fault2 = 0;
    ZGPU_HIP_CHECK(hipMemcpyAsync(&hs, e->ct_st, sizeof hs, hipMemcpyDeviceToHost, st));
    if (ntiles) ZGPU_HIP_CHECK(hipMemcpyAsync(&k_next, e->ct_entry + ntiles, 2, hipMemcpyDeviceToHost, st));
    if (check_sort) ZGPU_HIP_CHECK(hipMemcpyAsync(&sort_fault, lz_sorted_fault_word(r.ws_set[0]), 4, hipMemcpyDeviceToHost, st));
    if (check_sort && pl.pipe) ZGPU_HIP_CHECK(hipMemcpyAsync(&sort_fault2, lz_sorted_fault_word(r.ws_set[1]), 4, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    collect_spans(e);
    if (sort_fault | sort_fault2) { e->exact_sort = 1; return deflate_cont(e, f); } // (nothing of cs or of the incoming carry has been touched yet)
    if (hs.overflow) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    e->last_tok_match = -1;
    if (cfg.slow && f.mode == ZGPU_CONT_FLUSH && hs.total != 0 && hs.total <= e->ct_T.cap) { // what deflate_slow leaves in prev_length: 0 behind a match (deflate.c:1630-1636)
        uint32_t t = 0;
        ZGPU_HIP_CHECK(hipMemcpyAsync(&t, e->ct_T + (hs.total - 1), 4, hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        e->last_tok_match = (t >> 8) != 0;
    }
    return cont_state_after(e, f, pl, hs, k_next, adler, crc);
}

// ZGPU_F_CONTINUOUS: the whole input as ONE stream, in one feed that finishes it
int deflate_cont_oneshot(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const zgpu_deflate_params *p, uint8_t *d_out, uint64_t out_cap, zgpu_deflate_result *res, hipStream_t st)
{
    if (!e || !p || !res || (!d_in && in_bytes) || !d_out) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    if (p->level < 1 || p->level > 9 || p->strategy < 0 || p->strategy > (int)kFixed) return fail(e, ZGPU_STREAM_ERROR, "level 1..9, strategy 0..4");
    if (p->prime || (p->flags & (ZGPU_F_POS0 | ZGPU_F_POS0_ALL)) || !(p->flags & ZGPU_F_FINAL) || e->geo_w != 15 || e->geo_m != 8) return fail(e, ZGPU_STREAM_ERROR, "continuous stream: FINAL, no prime, the default geometry");
    if (p->flags & ZGPU_F_BGZF_WRAP) return fail(e, ZGPU_STREAM_ERROR, "BGZF blocks: segment calls only");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const bool wrap = p->flags & ZGPU_F_ZLIB_WRAP, gz = p->flags & ZGPU_F_GZIP_WRAP;
    if (wrap && gz) return fail(e, ZGPU_STREAM_ERROR, "one wrapper at a time");
    const uint32_t head_bytes = wrap ? 2 : gz ? 10 : 0, tail_bytes = wrap ? 4 : gz ? 8 : 0;
    if (out_cap < head_bytes + tail_bytes + 8) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    const FrameHead fh = frame_head(p->level, p->strategy, wrap, gz);
    uint8_t hdr[12] = {0};
    memcpy(hdr, fh.b, fh.n);
    ZGPU_HIP_CHECK(hipMemcpyAsync(d_out, hdr, (head_bytes + 4) & ~3u, hipMemcpyHostToDevice, st)); // (zero-filled to a whole word: the first block's bits are ORed in behind the header)
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    zgpu_cont_state cs{}; cs.data_type = 2; cs.first_block = 1; cs.last_eob = 8;
    ContFeed f{}; f.d_buf = d_in; f.buf_bytes = in_bytes; f.check_from = 0; f.mode = ZGPU_CONT_FINISH; f.d_out = d_out; f.out_cap = out_cap - tail_bytes; f.prefix_bits = 8ull * head_bytes;
    f.want_crc = gz || (p->flags & ZGPU_F_CRC32);
    std::vector<uint32_t> hist(kInsWords + 8, 0u); // (a fresh stream: nothing is in the chains)
    f.h_hist = hist.data();
    int rc = ensure_cont_ws(e, 1, 1);
    if (rc) return rc;
    f.cfg = level_cfg_for(e, p->level, p->strategy); f.cs = &cs; f.d_carry_in = e->ct_carry_in; f.res = res; f.st = st;
    rc = deflate_cont(e, f);
    if (rc) return rc;
    if ((wrap || gz) && (rc = write_trailer(e, gz, res->adler32, res->crc32, in_bytes, d_out, &res->out_bytes, st))) return rc;
    if (!f.want_crc) res->crc32 = 0;
    return ZGPU_OK;
}

} // namespace zgpu

using namespace zgpu;

extern "C" {
#pragma GCC visibility push(default)

int zgpu_deflate_cont_set_stale(zgpu_engine *e, int prev0, int byte_before)
{
    if (!e) return ZGPU_STREAM_ERROR;
    e->fast_prev0 = prev0 != 0; e->before_buf = (byte_before >= 0 && byte_before <= 255) ? byte_before : -1;
    return ZGPU_OK;
}
int zgpu_deflate_cont_last_match(zgpu_engine *e) { return e ? e->last_tok_match : -1; }

uint64_t zgpu_deflate_cont_bound(uint64_t in_bytes)
{
    // deflateBound's own arithmetic for a stream whose blocks may not be stored (deflate.c:513-515) plus a word per block boundary and the framing:
    // what a feed of in_bytes can write
    return in_bytes + ((in_bytes + 7) >> 3) + ((in_bytes + 63) >> 6) + 5 * (in_bytes / 16383 + 2) + 64;
}

int zgpu_deflate_cont_host(zgpu_engine *e, const void *hist, uint64_t hist_bytes, const void *in, uint64_t in_bytes, uint64_t check_from, const zgpu_deflate_params *p, int mode,
                           zgpu_cont_state *cs, uint32_t *carry_tok, uint32_t *hist_bits, const uint64_t *excl, uint32_t nexcl, void *out, uint64_t out_cap, zgpu_deflate_result *res)
{
    if (!e || !p || !res || !cs || !carry_tok || (!hist && hist_bytes) || (!in && in_bytes) || !out) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    const uint64_t buf_bytes = hist_bytes + in_bytes;
    if (p->level < 1 || p->level > 9 || p->strategy < 0 || p->strategy > (int)kFixed || mode < ZGPU_CONT_MORE || mode > ZGPU_CONT_FINISH) return fail(e, ZGPU_STREAM_ERROR, "level 1..9, strategy 0..4, a ZGPU_CONT_* mode");
    if (e->geo_w != 15 || e->geo_m != 8) return fail(e, ZGPU_STREAM_ERROR, "continuous stream: the default geometry");
    if (p->flags & ZGPU_F_BGZF_WRAP) return fail(e, ZGPU_STREAM_ERROR, "BGZF blocks: segment calls only");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const uint64_t bound = zgpu_deflate_cont_bound(buf_bytes) + kContCarry * 4;
    int rc = ensure_stage(e, buf_bytes, bound);
    if (rc) return rc;
    if ((rc = ensure_cont_ws(e, 1, 1))) return rc;
    ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
    if (hist_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, hist, hist_bytes, hipMemcpyHostToDevice, e->stream));
    if (in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in + hist_bytes, in, in_bytes, hipMemcpyHostToDevice, e->stream));
    if (cs->carry_ntok) ZGPU_HIP_CHECK(hipMemcpyAsync(e->ct_carry_in, carry_tok, (size_t)cs->carry_ntok * 4, hipMemcpyHostToDevice, e->stream));
    const uint32_t first_word = cs->bit_value & ((1u << cs->bit_count) - 1u);
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_out, &first_word, 4, hipMemcpyHostToDevice, e->stream));
    ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
    ContFeed f{}; f.d_buf = e->stage_in; f.buf_bytes = buf_bytes; f.check_from = check_from; f.mode = mode; f.h_excl = excl; f.nexcl = nexcl;
    f.d_out = e->stage_out; f.out_cap = bound; f.prefix_bits = cs->bit_count; f.want_crc = (p->flags & ZGPU_F_CRC32) != 0; f.h_hist = hist_bits;
    f.cfg = level_cfg_for(e, p->level, p->strategy); f.cs = cs; f.d_carry_in = e->ct_carry_in; f.res = res; f.st = e->stream;
    rc = deflate_cont(e, f);
    if (rc) return rc;
    if (res->out_bytes > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    if (res->out_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost, e->stream));
    if (cs->carry_ntok) ZGPU_HIP_CHECK(hipMemcpyAsync(carry_tok, e->ct_carry, (size_t)cs->carry_ntok * 4, hipMemcpyDeviceToHost, e->stream));
    ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
    if (!f.want_crc) res->crc32 = 0;
    return ZGPU_OK;
}

#pragma GCC visibility pop
} // extern "C"
