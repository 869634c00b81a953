// zgpu_deflate.hip -- host side of the chunk and segment compressor: deflate_device (a call's plan is zgpu_deflate_plan.h's, this file reserves the
// workspaces and queues the batches), its C entry points in include/zamd_gpu.h, the output bounds, geometry and tuning, and BGZF encode, which is a
// segments call.  No kernel lives here.
#include "zgpu_engine.h"
#include "zgpu_deflate_plan.h"
#include <cstdlib>
#include <atomic>
#include <thread>

namespace zgpu {

int ensure_deflate_ws(zgpu_engine *e, uint32_t batch, bool serial, uint64_t nchunks_total, bool geo)
{
    int rc;
    bool grew;
    if (geo) { // wider slots (blocks that may not be stored grow), head[] of up to 65536 entries, a flag word array per chunk
        if ((rc = e->geo_slots.reserve(e, (size_t)batch * kGeoSlotStride))) return rc;
        if ((rc = e->geo_tables.reserve(e, (size_t)batch * kGeoTableEntries, &grew))) return rc;
        if (grew) {
            ZGPU_HIP_CHECK(hipMemsetAsync(e->geo_tables, 0, e->geo_tables.cap * sizeof(uint4), e->stream));
            ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
        }
        if ((rc = e->geo_nostore.reserve(e, (size_t)batch * kGeoNostoreWords))) return rc;
    }
    if ((rc = e->tokens.reserve(e, (size_t)batch * kChunkMax))) return rc;
    if ((rc = e->meta.reserve(e, (size_t)batch))) return rc;
    if ((rc = e->slots.reserve(e, (size_t)batch * kSlotStride))) return rc;
    if (serial && !geo) {
        if ((rc = e->tables.reserve(e, (size_t)batch * kSerialTableEntries, &grew))) return rc;
        if (grew) {
            ZGPU_HIP_CHECK(hipMemsetAsync(e->tables, 0, e->tables.cap * sizeof(uint4), e->stream));
            ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
        }
    }
    if (!serial && batch > e->par_cap) {
        const size_t wa = lz_parallel_workspace_bytes(batch), wb = lz_sorted_workspace_bytes(batch);
        e->par_cap = 0;
        if ((rc = e->par_ws.reserve(e, wa > wb ? wa : wb))) return rc;
        e->par_cap = batch;
    }
    return e->offsets.reserve(e, (size_t)nchunks_total + 1);
}

static void zlib_header(int level, int strategy, uint8_t hdr[2]) // qcsrc/deflate.c:625-641
{
    unsigned h = (8u + (7u << 4)) << 8, lf = (strategy >= 2 || level < 2) ? 0 : level < 6 ? 1 : level == 6 ? 2 : 3;
    h |= lf << 6; h += 31 - h % 31;
    hdr[0] = (uint8_t)(h >> 8); hdr[1] = (uint8_t)h;
}

// what a stream that is not part of a wrapped segment call starts with: the zlib header, or the gzip header deflate() writes when no gz_header
// was set (qcsrc/deflate.c:578-596); OS_CODE 3 as the reference builds here
FrameHead frame_head(int level, int strategy, bool wrap, bool gz, bool bgzf)
{
    FrameHead fh{};
    if (bgzf) { // what bgzip writes: FEXTRA, no MTIME, XFL 0, OS 255, the one subfield 'B' 'C' of two bytes -- BSIZE, filled in per block by frame_kernel
        const uint8_t hdr[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, 0, 0};
        for (int i = 0; i < 18; i++) fh.b[i] = hdr[i];
        fh.n = 18; fh.gzip = 1; fh.bgzf = 1;
        return fh;
    }
    if (wrap) { zlib_header(level, strategy, fh.b); fh.n = 2; }
    if (gz) {
        const uint8_t hdr[10] = {31, 139, 8, 0, 0, 0, 0, 0, (uint8_t)(level == 9 ? 2 : (strategy >= 2 || level < 2) ? 4 : 0), 3};
        for (int i = 0; i < 10; i++) fh.b[i] = hdr[i];
        fh.n = 10; fh.gzip = 1;
    }
    return fh;
}

// ... and ends with, behind d_out[*out_total]: zlib's Adler-32, big-endian; gzip's CRC-32 and the input length mod 2^32, both little-endian (qcsrc/deflate.c:833-843)
int write_trailer(zgpu_engine *e, bool gz, uint32_t adler, uint32_t crc, uint64_t in_bytes, uint8_t *d_out, uint64_t *out_total, hipStream_t st)
{
    const uint32_t isz = (uint32_t)in_bytes, n = gz ? 8 : 4;
    const uint8_t zl[4] = {(uint8_t)(adler >> 24), (uint8_t)(adler >> 16), (uint8_t)(adler >> 8), (uint8_t)adler};
    const uint8_t gt[8] = {(uint8_t)crc, (uint8_t)(crc >> 8), (uint8_t)(crc >> 16), (uint8_t)(crc >> 24), (uint8_t)isz, (uint8_t)(isz >> 8), (uint8_t)(isz >> 16), (uint8_t)(isz >> 24)};
    ZGPU_HIP_CHECK(hipMemcpyAsync(d_out + *out_total, gz ? gt : zl, n, hipMemcpyHostToDevice, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    *out_total += n;
    return ZGPU_OK;
}

LevelCfg level_cfg_for(const zgpu_engine *e, int level, int strategy) { return level_cfg_tuned(level, strategy, e->tuned != 0, e->tune); }

// What the plans ask of the engine and of the device (whose memory is asked: the engine's device is the current one).  cfg: the parameters the call
// will run with, nullptr where it names no level
PlanEngine plan_engine(const zgpu_engine *e, const LevelCfg *cfg)
{
    PlanEngine pe;
    pe.geo_w = e->geo_w; pe.geo_m = e->geo_m;
    pe.tuned = e->tuned != 0;
    for (int i = 0; i < 4; i++) pe.tune[i] = e->tune[i];
    pe.exact_sort = e->exact_sort != 0;
    pe.lz_parallel = lz_parallel_available();
    pe.fastwin_serves = cfg && lz_fastwin_serves(*cfg);
    pe.sorted_ws_chunk = lz_sorted_workspace_bytes(1);
    pe.batch_cap = e->batch_cap(); pe.par_cap = e->par_cap; pe.ct_tiles = e->ct_tiles();
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) pe.free_bytes = free_b;
    return pe;
}

static DeflateKnobs read_deflate_knobs()
{
    DeflateKnobs kn;
    static int auto_env = -1; // (read once a process)
    if (auto_env < 0) { const char *v = getenv("ZGPU_LZ_DEFAULT"); auto_env = v ? atoi(v) : 0; }
    kn.lz_default = auto_env;
    const char *ho = getenv("ZGPU_HAND_ON");
    kn.hand_on = ho ? ho[0] : 0;
    kn.batch_chunks = env_u32("ZGPU_BATCH_CHUNKS", 0); kn.host_batch = env_u32("ZGPU_HOST_BATCH", 0); kn.first_batch = env_u32("ZGPU_FIRST_BATCH", 0);
    return kn;
}

// One call of deflate_device: the input d_in[0, in_bytes) in chunks of p->chunk_size, or in the segments of d_seg, to d_out[0, out_cap)
struct DeflateCall {
    const uint8_t *d_in; uint64_t in_bytes;
    const uint64_t *d_seg; uint64_t nseg; // d_seg (or nullptr): device table of nseg + 1 offsets; then every segment is one chunk and chunk_size is ignored
    const zgpu_deflate_params *p;
    uint8_t *d_out; uint64_t out_cap;
    zgpu_deflate_result *res;
    hipStream_t st;
    uint64_t *d_chunk_offsets = nullptr; // receives nchunks + 1 offsets into d_out
    uint32_t skip0 = 0;                  // a preset dictionary: the one chunk starts with this many bytes of window
    // h_src (uniform chunking only): the input still lies in host memory; every batch's bytes are copied to d_in on the engine's copy stream right
    // before the batch's kernels are queued, so the copy of batch k+1 runs under the kernels of batch k.
    const uint8_t *h_src = nullptr;
    // h_dst: what the batches so far have produced goes to the caller's buffer (h_cap bytes) while the next ones are compressed; *h_copied: how much went
    uint8_t *h_dst = nullptr; uint64_t h_cap = 0; uint64_t *h_copied = nullptr;
    bool seg_checked = false;            // BGZF: the segment table is known to hold no segment over 65280 bytes
    zgpu_deflate_item *d_items = nullptr; // segment calls: a record per segment
};

// The thread that copies finished batches home.  Copies to pageable memory hold the calling thread, so they are a second thread's: it waits for
// batch k's event, reads the stream length behind it (pinned) and copies the new bytes on a stream of its own.  The checks of deflate_device
// return from the middle of its loop: the destructor tells the thread to give up, so that it never outlives the call.
class BatchHomer {
    static constexpr size_t kGiveUp = (size_t)-1;
    zgpu_engine *e = nullptr; const uint8_t *d_out = nullptr; uint8_t *h_dst = nullptr; uint64_t h_cap = 0;
    std::thread homer;
    std::atomic<size_t> issued{0};
    std::atomic<int> homer_rc{0};
    uint64_t homed = 0;
    void run(size_t nbatches)
    {
        if (hipSetDevice(e->device) != hipSuccess) { homer_rc = 1; return; }
        for (size_t k = 0; k < nbatches; k++) {
            while (issued.load(std::memory_order_acquire) <= k) std::this_thread::yield();
            if (issued.load() == kGiveUp) return; // the call gave up
            if (hipEventSynchronize(e->done_ev[k]) != hipSuccess) { homer_rc = 1; return; }
            uint64_t upto = e->pin_tot[k];
            if (upto > h_cap) upto = h_cap;
            if (upto > homed) {
                if (hipMemcpyAsync(h_dst + homed, d_out + homed, upto - homed, hipMemcpyDeviceToHost, e->d2h_stream) != hipSuccess ||
                    hipStreamSynchronize(e->d2h_stream) != hipSuccess) { homer_rc = 1; return; }
                homed = upto;
            }
        }
    }
    void join(bool give_up) { if (homer.joinable()) { if (give_up) issued.store(kGiveUp); homer.join(); } }
public:
    static constexpr size_t kMaxBatches = 4096; // (the pinned totals)
    ~BatchHomer() { join(true); }
    bool on() const { return e != nullptr; }
    int start(zgpu_engine *e_, const DeflateCall &c, size_t nbatches)
    {
        e = e_; d_out = c.d_out; h_dst = c.h_dst; h_cap = c.h_cap;
        if (!e->pin_tot) ZGPU_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&e->pin_tot), kMaxBatches * sizeof(uint64_t), hipHostMallocDefault));
        if (!e->d2h_stream) ZGPU_HIP_CHECK(hipStreamCreateWithFlags(&e->d2h_stream, hipStreamNonBlocking));
        while (e->done_ev.size() < nbatches) { hipEvent_t ev; ZGPU_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); e->done_ev.push_back(ev); }
        homer = std::thread([this, nbatches]() { run(nbatches); });
        return ZGPU_OK;
    }
    int queued(size_t k, hipStream_t st) // batch k's kernels are queued on st: the stream's length behind them (RunState::out_total) comes to pin_tot[k]
    {
        hipError_t he = hipMemcpyAsync(&e->pin_tot[k], e->run, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipEventRecord(e->done_ev[k], st);
        if (he != hipSuccess) return fail_hip(e, he, "batch hand-over", __FILE__, __LINE__);
        issued.store(k + 1, std::memory_order_release);
        return ZGPU_OK;
    }
    int finish(uint64_t *h_copied) // every batch is queued: waits until the last one is home
    {
        join(false);
        if (homer_rc.load()) return fail(e, ZGPU_ERRNO, "copy of finished batches to the host failed");
        if (h_copied) *h_copied = homed;
        return ZGPU_OK;
    }
};

// BSIZE has 16 bits: no segment of a BGZF call may be longer than what always fits (the table is the caller's, in device memory)
static int check_bgzf_segments(zgpu_engine *e, const DeflateCall &c)
{
    uint32_t over = 0;
    uint32_t *flag = &static_cast<RunState *>(e->run)->pad;
    ZGPU_HIP_CHECK(hipMemsetAsync(flag, 0, 4, c.st));
    launch_seg_limit(c.d_seg, c.nseg, c.in_bytes, kBgzfBlockMax, flag, c.st);
    ZGPU_HIP_CHECK(hipMemcpyAsync(&over, flag, 4, hipMemcpyDeviceToHost, c.st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(c.st));
    if (over) return fail(e, ZGPU_STREAM_ERROR, "BGZF blocks: a segment is longer than 65280 bytes (or the table leaves the input)");
    return ZGPU_OK;
}

// the workspaces of a planned call; *hand_piece: chunks of one launch of the wave-per-chunk kernel over the chunks handed on
static int reserve_deflate(zgpu_engine *e, const DeflatePlan &pl, uint32_t *hand_piece)
{
    int rc = ensure_deflate_ws(e, pl.batch, pl.serial, pl.nchunks, pl.geo);
    if (rc) return rc;
    *hand_piece = pl.hand_piece;
    if (pl.hand_on) {
        if ((rc = ensure_deflate_ws(e, pl.hand_piece, false, pl.nchunks))) return rc;
        if (e->par_cap > pl.hand_piece) *hand_piece = e->par_cap < pl.batch ? e->par_cap : pl.batch; // (an earlier call has left more)
        if ((rc = e->hand_list.reserve(e, (size_t)pl.batch + 1))) return rc;
    }
    return ZGPU_OK;
}

static ChunkGeom chunk_geom(const zgpu_engine *e, const DeflateCall &c, const DeflatePlan &pl)
{
    const zgpu_deflate_params *p = c.p;
    ChunkGeom g{};
    g.in = c.d_in; g.in_bytes = c.in_bytes; g.seg_off = c.d_seg; g.chunk_size = pl.chunk_size;
    g.final_chunk = (!c.d_seg && (p->flags & ZGPU_F_FINAL)) ? pl.nchunks - 1 : ~0ull;
    g.all_final = (c.d_seg && (p->flags & ZGPU_F_FINAL)) ? 1u : 0u;
    g.pos0_mode = (p->flags & ZGPU_F_POS0_ALL) ? 2u : (p->flags & ZGPU_F_POS0) ? 1u : 0u;
    g.skip0 = c.skip0;
    g.block_tokens = pl.block_tokens;
    g.slot_stride = pl.geo ? kGeoSlotStride : kSlotStride;
    g.nostore_bits = pl.geo ? e->geo_nostore : nullptr;
    g.prime = (p->prime >> 16) ? ((p->prime & 0xffff0000u) | (p->prime & ((1u << (p->prime >> 16)) - 1u))) : 0u;
    return g;
}

// this batch's input: host -> device on the copy stream, the kernels behind it on st wait for it
static int copy_batch_in(zgpu_engine *e, const DeflateCall &c, const BatchSteps &s, uint32_t chunk_size)
{
    const uint64_t c1 = s.c0 + s.nb();
    const uint64_t lo = s.c0 * chunk_size, hi = c1 * (uint64_t)chunk_size < c.in_bytes ? c1 * (uint64_t)chunk_size : c.in_bytes;
    const hipEvent_t ev = engine_copy_event(e, s.k); // (nullptr where none could be made: recording it fails)
    ZGPU_HIP_CHECK(hipMemcpyAsync(const_cast<uint8_t *>(c.d_in) + lo, c.h_src + lo, hi - lo, hipMemcpyHostToDevice, e->copy_stream));
    ZGPU_HIP_CHECK(hipEventRecord(ev, e->copy_stream));
    ZGPU_HIP_CHECK(hipStreamWaitEvent(c.st, ev, 0));
    return ZGPU_OK;
}

// the tokens of one batch; *adler_done: the implementation has computed the chunks' Adler-32 on the way (the sort of the default path)
static int lz_batch(zgpu_engine *e, const ChunkGeom &g, const DeflatePlan &pl, uint32_t hand_piece, hipStream_t st, bool *adler_done)
{
    *adler_done = false;
    if (!pl.serial) {
        if (pl.impl == ZGPU_LZ_PARALLEL) launch_lz_parallel(g, pl.cfg, e->par_ws, e->tokens, e->meta, st, e);
        else *adler_done = launch_lz_sorted(g, pl.cfg, e->par_ws, e->tokens, e->meta, st, e, e->exact_sort, pl.impl);
        return ZGPU_OK;
    }
    StageTimer t(e, st, ZGPU_STAGE_LZ_SERIAL);
    // (a tag that these tables have not seen: 0 is what fresh tables hold; should the counter ever wrap, they are zeroed again)
    if (++e->serial_tag == 0) {
        if (e->tables) ZGPU_HIP_CHECK(hipMemsetAsync(e->tables, 0, e->tables.cap * sizeof(uint4), st));
        if (e->geo_tables) ZGPU_HIP_CHECK(hipMemsetAsync(e->geo_tables, 0, e->geo_tables.cap * sizeof(uint4), st));
        e->serial_tag = 1;
    }
    if (pl.geo) launch_lz_serial(g, pl.cfg, e->geo_tables, e->tokens, e->meta, st, e->geo_nostore, false, e->serial_tag);
    else launch_lz_serial(g, pl.cfg, e->tables, e->tokens, e->meta, st, nullptr, pl.hand_on, e->serial_tag);
    if (pl.hand_on) { // the chunks the loop gave up, as a list, through the wave-per-chunk kernel (their number decides the launch: one word comes home)
        launch_collect_handed_on(e->meta, g.nchunks, e->hand_list + 1, e->hand_list, st);
        uint32_t handed = 0;
        ZGPU_HIP_CHECK(hipMemcpyAsync(&handed, e->hand_list, 4, hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        for (uint32_t at = 0; at < handed; at += hand_piece) {
            ChunkGeom gl = g; gl.nchunks = handed - at < hand_piece ? handed - at : hand_piece; gl.chunk_map = e->hand_list + 1 + at;
            launch_lz_sorted(gl, pl.cfg, e->par_ws, e->tokens, e->meta, st, e, e->exact_sort, ZGPU_LZ_FASTWIN);
        }
        e->handed_on += handed;
    }
    return ZGPU_OK;
}

// the blocks of one batch from its tokens, the chunks' checksums, and the blocks' bits to where they belong in the output (body_cap bytes of it are the body's)
static void blocks_batch(zgpu_engine *e, const DeflateCall &c, const DeflatePlan &pl, const ChunkGeom &g, const FrameHead &fh, uint64_t body_cap, bool adler_done)
{
    const hipStream_t st = c.st;
    uint8_t *const slots = pl.geo ? e->geo_slots : e->slots;
    {
        StageTimer t(e, st, ZGPU_STAGE_HUFFMAN);
        launch_huffman(g, e->tokens, e->meta, slots, st, pl.cfg.strategy == kFixed);
    }
    StageTimer t(e, st, ZGPU_STAGE_STITCH);
    if (!adler_done) launch_adler(g, e->meta, st);
    if (pl.with_crc) launch_crc(g, e->meta, st);
    if (pl.seg_wrap) launch_frame(slots, e->meta, e->offsets, c.d_seg, g.chunk0, g.nchunks, c.d_out, body_cap, g.slot_stride, e->run, pl.with_crc, fh, st);
    else {
        launch_scan(e->meta, g.nchunks, g.chunk0, e->offsets, e->run, body_cap, st, pl.with_crc);
        launch_stitch(slots, e->meta, e->offsets, g.chunk0, g.nchunks, c.d_out, body_cap, g.slot_stride, st);
    }
    if (c.d_items) launch_seg_items(e->meta, e->offsets, c.d_seg, g.chunk0, g.nchunks, pl.with_crc, c.d_items, st); // (segment calls only: d_seg is there)
}

static int deflate_device(zgpu_engine *e, const DeflateCall &c)
{
    if (!e) return ZGPU_STREAM_ERROR;
    const zgpu_deflate_params *const p = c.p;
    const hipStream_t st = c.st;
    // check and plan
    PlanCall pc;
    pc.args = p && c.res && (c.d_in || !c.in_bytes) && c.d_out;
    if (p) { pc.level = p->level; pc.strategy = p->strategy; pc.lz_impl = p->lz_impl; pc.chunk_size = p->chunk_size; pc.flags = p->flags; pc.prime = p->prime; }
    pc.in_bytes = c.in_bytes; pc.seg = c.d_seg != nullptr; pc.nseg = c.nseg; pc.skip0 = c.skip0; pc.host_in = c.h_src != nullptr;
    PlanEngine pe; pe.geo_w = e->geo_w; pe.geo_m = e->geo_m;
    DeflatePlan pl = plan_deflate_args(pc, pe);
    if (pl.rc) return fail(e, pl.rc, pl.msg);
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    int rc;
    if ((p->flags & ZGPU_F_BGZF_WRAP) && c.nseg && !c.seg_checked && (rc = check_bgzf_segments(e, c))) return rc;
    const LevelCfg lc = level_cfg_for(e, p->level, p->strategy);
    pl = plan_deflate(pc, plan_engine(e, &lc), read_deflate_knobs());
    if (pl.rc) return fail(e, pl.rc, pl.msg);
    // reserve the workspaces
    uint32_t hand_piece = 0;
    if ((rc = reserve_deflate(e, pl, &hand_piece))) return rc;
    // the run's state, the header
    const FrameHead fh = frame_head(p->level, p->strategy, pl.wrap, pl.gz, pl.bgzf);
    ChunkGeom g = chunk_geom(e, c, pl);
    const uint64_t body_cap = pl.tail_bytes ? (c.out_cap >= pl.head_bytes + pl.tail_bytes ? c.out_cap - pl.tail_bytes : 0) : c.out_cap;
    RunState rs{}; rs.out_total = pl.head_bytes; rs.adler_a = 1; rs.adler_b = 0; rs.data_type = 2;
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->run, &rs, sizeof rs, hipMemcpyHostToDevice, st));
    uint32_t sort_fault = 0;
    if (pl.check_sort) ZGPU_HIP_CHECK(hipMemsetAsync(lz_sorted_fault_word(e->par_ws), 0, 4, st));
    if (!pl.seg_wrap && pl.head_bytes && c.out_cap >= pl.head_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(c.d_out, fh.b, pl.head_bytes, hipMemcpyHostToDevice, st));
    // the batches: copy in, LZ77, blocks and stitch, hand home
    const size_t nbatches = plan_nbatches(pl);
    BatchHomer home;
    if (c.h_dst && c.h_src && nbatches > 1 && nbatches <= BatchHomer::kMaxBatches && (rc = home.start(e, c, nbatches))) return rc;
    for (BatchSteps s(pl); s.more(); s.next()) {
        g.chunk0 = s.c0; g.nchunks = s.nb();
        if (c.h_src && c.in_bytes && (rc = copy_batch_in(e, c, s, pl.chunk_size))) return rc;
        bool adler_done;
        if ((rc = lz_batch(e, g, pl, hand_piece, st, &adler_done))) return rc;
        blocks_batch(e, c, pl, g, fh, body_cap, adler_done);
        if (home.on() && (rc = home.queued(s.k, st))) return rc;
        const hipError_t he = hipGetLastError();
        if (he != hipSuccess) return zgpu::fail_hip(e, he, "kernel launch", __FILE__, __LINE__);
    }
    if (home.on() && (rc = home.finish(c.h_copied))) return rc;
    // read back
    ZGPU_HIP_CHECK(hipMemcpyAsync(&rs, e->run, sizeof rs, hipMemcpyDeviceToHost, st));
    if (pl.check_sort) ZGPU_HIP_CHECK(hipMemcpyAsync(&sort_fault, lz_sorted_fault_word(e->par_ws), 4, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    collect_spans(e);
    if (sort_fault) { // the LDS did not serve an atomic's lanes in lane order: redo the call with the sort that does not rely on it
        e->exact_sort = 1;
        return deflate_device(e, c);
    }
    // the trailer, the result
    if (rs.overflow || (pl.tail_bytes && c.out_cap < rs.out_total + pl.tail_bytes)) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    const uint32_t adler = rs.adler_a | (rs.adler_b << 16);
    if ((pl.wrap || pl.gz) && !pl.seg_wrap && (rc = write_trailer(e, pl.gz, adler, rs.crc, c.in_bytes, c.d_out, &rs.out_total, st))) return rc;
    if (c.d_chunk_offsets) {
        ZGPU_HIP_CHECK(hipMemcpyAsync(c.d_chunk_offsets, e->offsets, (pl.nchunks + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    }
    zgpu_deflate_result *const res = c.res;
    res->out_bytes = rs.out_total; res->nchunks = pl.nchunks; res->adler32 = adler; res->data_type = rs.data_type; res->ntokens = rs.ntokens;
    res->crc32 = pl.with_crc ? rs.crc : 0;
    return ZGPU_OK;
}

} // namespace zgpu

using namespace zgpu;

extern "C" {
#pragma GCC visibility push(default)

uint64_t zgpu_deflate_bound(uint64_t in_bytes, uint32_t chunk_size)
{
    if (chunk_size == 0 || chunk_size > kChunkMax) chunk_size = kChunkMax;
    uint64_t nchunks = in_bytes ? (in_bytes + chunk_size - 1) / chunk_size : 1;
    return in_bytes + nchunks * 40 + 16; // <= 6 block headers of 5 bytes + 5-byte marker per chunk, + zlib framing
}

// The same for a stream made with deflateInit2(windowBits, memLevel): blocks of as few as 127 tokens (a header each), and blocks that may not be
// stored because their start has left a small window (deflateBound's arithmetic, deflate.c:513-515, covers those).
uint64_t zgpu_deflate_bound_geometry(uint64_t in_bytes, uint32_t chunk_size, int window_bits, int mem_level)
{
    if (window_bits == 15 && mem_level == 8) return zgpu_deflate_bound(in_bytes, chunk_size);
    if (chunk_size == 0 || chunk_size > kChunkMax) chunk_size = kChunkMax;
    if (mem_level < 1 || mem_level > 9) mem_level = 1;
    const uint64_t nchunks = in_bytes ? (in_bytes + chunk_size - 1) / chunk_size : 1, blocks = chunk_size / ((1u << (mem_level + 6)) - 1u) + 2;
    return in_bytes + ((in_bytes + 7) >> 3) + ((in_bytes + 63) >> 6) + nchunks * (5 * blocks + 64) + 16;
}

int zgpu_deflate_set_geometry(zgpu_engine *e, int window_bits, int mem_level)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (window_bits < 9 || window_bits > 15 || mem_level < 1 || mem_level > 9) return fail(e, ZGPU_STREAM_ERROR, "windowBits 9..15, memLevel 1..9");
    e->geo_w = window_bits; e->geo_m = mem_level;
    return ZGPU_OK;
}

int zgpu_deflate_set_tuning(zgpu_engine *e, int on, uint32_t good_length, uint32_t max_lazy, uint32_t nice_length, uint32_t max_chain)
{
    if (!e) return ZGPU_STREAM_ERROR;
    e->tuned = on != 0; e->tune[0] = good_length; e->tune[1] = max_lazy; e->tune[2] = nice_length; e->tune[3] = max_chain;
    return ZGPU_OK;
}

int zgpu_deflate_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const zgpu_deflate_params *p, void *d_out, uint64_t out_cap,
                        uint64_t *d_chunk_offsets, zgpu_deflate_result *res, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    if (p && (p->flags & ZGPU_F_CONTINUOUS)) return deflate_cont_oneshot(e, static_cast<const uint8_t *>(d_in), in_bytes, p, static_cast<uint8_t *>(d_out), out_cap, res, st);
    DeflateCall c{};
    c.d_in = static_cast<const uint8_t *>(d_in); c.in_bytes = in_bytes; c.p = p; c.d_out = static_cast<uint8_t *>(d_out); c.out_cap = out_cap; c.res = res; c.st = st;
    c.d_chunk_offsets = d_chunk_offsets;
    return deflate_device(e, c);
}

int zgpu_deflate_dict_chunk_host(zgpu_engine *e, const void *window, uint32_t window_bytes, uint32_t dict_bytes, const zgpu_deflate_params *p,
                                 void *out, uint64_t out_cap, zgpu_deflate_result *res)
{
    if (!e || !p || !res || !window || !out) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const uint64_t bound = zgpu_deflate_bound_geometry(window_bytes, kChunkMax, e ? e->geo_w : 15, e ? e->geo_m : 8);
    int rc = ensure_stage(e, window_bytes, bound);
    if (rc) return rc;
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, window, window_bytes, hipMemcpyHostToDevice, e->stream));
    zgpu_deflate_params q = *p;
    q.chunk_size = kChunkMax;
    DeflateCall c{};
    c.d_in = e->stage_in; c.in_bytes = window_bytes; c.p = &q; c.d_out = e->stage_out; c.out_cap = bound; c.res = res; c.st = e->stream;
    c.skip0 = dict_bytes;
    rc = deflate_device(e, c);
    if (rc) return rc;
    if (res->out_bytes > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    ZGPU_HIP_CHECK(hipMemcpyAsync(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost, e->stream));
    ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
    return ZGPU_OK;
}

int zgpu_deflate_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const zgpu_deflate_params *p, void *out, uint64_t out_cap,
                      uint64_t *chunk_offsets, zgpu_deflate_result *res)
{
    if (!e || !p || !res || (!in && in_bytes) || !out) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    if (p->flags & ZGPU_F_CONTINUOUS) { // one continuous stream: staged whole, compressed in one feed
        const uint64_t cb = zgpu_deflate_cont_bound(in_bytes) + 32;
        int rc2 = ensure_stage(e, in_bytes, cb);
        if (rc2) return rc2;
        ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
        if (in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, in, in_bytes, hipMemcpyHostToDevice, e->stream));
        rc2 = deflate_cont_oneshot(e, e->stage_in, in_bytes, p, e->stage_out, cb, res, e->stream);
        if (rc2) return rc2;
        if (res->out_bytes > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
        ZGPU_HIP_CHECK(hipMemcpyAsync(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost, e->stream));
        ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
        return ZGPU_OK;
    }
    const uint32_t chunk_size = p->chunk_size ? p->chunk_size : kChunkMax;
    const uint64_t bound = zgpu_deflate_bound_geometry(in_bytes, chunk_size, e ? e->geo_w : 15, e ? e->geo_m : 8);
    int rc = ensure_stage(e, in_bytes, bound);
    if (rc) return rc;
    // (the copy stream must not run ahead of the previous call's kernels, which may still read the staging buffer: it starts behind them)
    ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
    const bool overlap = in_bytes > (uint64_t)8192 * chunk_size; // (more than one batch: otherwise there is nothing to overlap the copy with)
    if (!overlap && in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, in, in_bytes, hipMemcpyHostToDevice, e->stream));
    uint64_t homed = 0; // bytes of the stream that went to `out` while later batches were compressed
    DeflateCall c{};
    c.d_in = e->stage_in; c.in_bytes = in_bytes; c.p = p; c.d_out = e->stage_out; c.out_cap = bound; c.res = res; c.st = e->stream;
    if (overlap) { c.h_src = static_cast<const uint8_t *>(in); c.h_dst = static_cast<uint8_t *>(out); }
    c.h_cap = out_cap; c.h_copied = &homed;
    rc = deflate_device(e, c);
    if (rc) return rc;
    if (res->out_bytes > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    if (res->out_bytes > homed) ZGPU_HIP_CHECK(hipMemcpyAsync(static_cast<uint8_t *>(out) + homed, e->stage_out + homed, res->out_bytes - homed, hipMemcpyDeviceToHost, e->stream));
    if (chunk_offsets) ZGPU_HIP_CHECK(hipMemcpyAsync(chunk_offsets, e->offsets, (res->nchunks + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
    return ZGPU_OK;
}

uint64_t zgpu_deflate_segments_bound(uint64_t nseg, uint64_t in_bytes, uint32_t flags)
{
    // raw: what zgpu_deflate_segments_host stages for the default geometry; a wrapper adds its header and trailer to every segment
    return in_bytes + nseg * (40 + (uint64_t)((flags & ZGPU_F_BGZF_WRAP) ? 26 : (flags & ZGPU_F_GZIP_WRAP) ? 18 : (flags & ZGPU_F_ZLIB_WRAP) ? 6 : 0)) + 16;
}

int zgpu_deflate_segments_items_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_seg_offsets, uint64_t nseg,
                                       const zgpu_deflate_params *p, void *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                                       zgpu_deflate_result *res, zgpu_deflate_item *d_items, void *hip_stream)
{
    if (!e || !d_seg_offsets) return ZGPU_STREAM_ERROR;
    DeflateCall c{};
    c.d_in = static_cast<const uint8_t *>(d_in); c.in_bytes = in_bytes; c.d_seg = d_seg_offsets; c.nseg = nseg; c.p = p;
    c.d_out = static_cast<uint8_t *>(d_out); c.out_cap = out_cap; c.res = res; c.st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    c.d_chunk_offsets = d_out_offsets; c.d_items = d_items;
    return deflate_device(e, c);
}

int zgpu_deflate_segments_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_seg_offsets, uint64_t nseg,
                                 const zgpu_deflate_params *p, void *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                                 zgpu_deflate_result *res, void *hip_stream)
{
    return zgpu_deflate_segments_items_device(e, d_in, in_bytes, d_seg_offsets, nseg, p, d_out, out_cap, d_out_offsets, res, nullptr, hip_stream);
}

int zgpu_deflate_segments_items_host(zgpu_engine *e, const void *in, const uint64_t *seg_offsets, uint64_t nseg, const zgpu_deflate_params *p,
                                     void *out, uint64_t out_cap, uint64_t *out_offsets, zgpu_deflate_result *res, zgpu_deflate_item *items)
{
    if (!e || !p || !res || !in || !out || !seg_offsets || nseg == 0) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const uint64_t in_bytes = seg_offsets[nseg];
    for (uint64_t k = 0; k < nseg; k++)
        if (seg_offsets[k + 1] < seg_offsets[k] || seg_offsets[k + 1] - seg_offsets[k] > kChunkMax) return fail(e, ZGPU_STREAM_ERROR, "segment longer than 65536 bytes");
    // (every segment may be a chunk of its own: with a non-default geometry each gets the allowance of a full chunk)
    const uint64_t bound = (e->geo_w != 15 || e->geo_m != 8) ? in_bytes + zgpu_deflate_bound_geometry(nseg * (uint64_t)kChunkMax, kChunkMax, e->geo_w, e->geo_m) - nseg * (uint64_t)kChunkMax + ((nseg * (uint64_t)kChunkMax) >> 3)
                                                             : in_bytes + nseg * 40 + 16;
    const uint64_t framed = bound + nseg * (uint64_t)((p->flags & ZGPU_F_BGZF_WRAP) ? 26 : (p->flags & ZGPU_F_GZIP_WRAP) ? 18 : (p->flags & ZGPU_F_ZLIB_WRAP) ? 6 : 0);
    const uint64_t tab_off = (in_bytes + 63) & ~63ull; // segment table staged behind the data, the records (when asked for) behind the table
    const uint64_t items_off = (tab_off + (nseg + 1) * sizeof(uint64_t) + 63) & ~63ull;
    int rc = ensure_stage(e, items_off + (items ? nseg * sizeof(zgpu_deflate_item) : 0) + 64, framed);
    if (rc) return rc;
    if (in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, in, in_bytes, hipMemcpyHostToDevice, e->stream));
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in + tab_off, seg_offsets, (nseg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
    zgpu_deflate_item *d_items = items ? reinterpret_cast<zgpu_deflate_item *>(e->stage_in + items_off) : nullptr;
    DeflateCall c{};
    c.d_in = e->stage_in; c.in_bytes = in_bytes; c.d_seg = reinterpret_cast<const uint64_t *>(e->stage_in + tab_off); c.nseg = nseg; c.p = p;
    c.d_out = e->stage_out; c.out_cap = framed; c.res = res; c.st = e->stream;
    c.d_items = d_items;
    rc = deflate_device(e, c);
    if (rc) return rc;
    if (res->out_bytes > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    ZGPU_HIP_CHECK(hipMemcpyAsync(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost, e->stream));
    if (out_offsets) ZGPU_HIP_CHECK(hipMemcpyAsync(out_offsets, e->offsets, (nseg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    if (items) ZGPU_HIP_CHECK(hipMemcpyAsync(items, d_items, nseg * sizeof(zgpu_deflate_item), hipMemcpyDeviceToHost, e->stream));
    ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
    return ZGPU_OK;
}

int zgpu_deflate_segments_host(zgpu_engine *e, const void *in, const uint64_t *seg_offsets, uint64_t nseg, const zgpu_deflate_params *p,
                               void *out, uint64_t out_cap, uint64_t *out_offsets, zgpu_deflate_result *res)
{
    return zgpu_deflate_segments_items_host(e, in, seg_offsets, nseg, p, out, out_cap, out_offsets, res, nullptr);
}

// ---- BGZF encode: the segments path over a table cut on the device, and the end block behind it ----
static const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

uint64_t zgpu_bgzf_bound(uint64_t in_bytes, uint32_t block_size)
{
    if (block_size == 0 || block_size > kBgzfBlockMax) block_size = kBgzfBlockMax;
    const uint64_t nblocks = (in_bytes + block_size - 1) / block_size;
    return zgpu_deflate_segments_bound(nblocks, in_bytes, ZGPU_F_FINAL | ZGPU_F_BGZF_WRAP) + sizeof kBgzfEof;
}

// One BGZF encode: in_bytes of d_in at level / strategy in blocks of block_size, to d_out[0, out_cap)
struct BgzfCall {
    const uint8_t *d_in; uint64_t in_bytes; int level, strategy; uint32_t block_size;
    uint64_t *d_seg;         // room for nblocks + 1 offsets (device)
    uint8_t *d_out; uint64_t out_cap;
    uint64_t *d_out_offsets; // optional, nblocks + 2
};
static int bgzf_deflate(zgpu_engine *e, const BgzfCall &b, zgpu_deflate_result *res, hipStream_t st)
{
    const uint64_t nblocks = (b.in_bytes + b.block_size - 1) / b.block_size;
    zgpu_deflate_result r{};
    r.adler32 = 1; r.data_type = 2;
    if (nblocks) {
        zgpu_deflate_params p{};
        p.level = b.level; p.strategy = b.strategy; p.flags = ZGPU_F_FINAL | ZGPU_F_BGZF_WRAP; p.lz_impl = ZGPU_LZ_AUTO;
        launch_bgzf_cut(b.in_bytes, b.block_size, nblocks, b.d_seg, st);
        DeflateCall c{};
        c.d_in = b.d_in; c.in_bytes = b.in_bytes; c.d_seg = b.d_seg; c.nseg = nblocks; c.p = &p; c.d_out = b.d_out; c.out_cap = b.out_cap; c.res = &r; c.st = st;
        c.d_chunk_offsets = b.d_out_offsets;
        c.seg_checked = true; // (a table cut here needs no length check)
        const int rc = deflate_device(e, c);
        if (rc) return rc;
    }
    if (b.out_cap < r.out_bytes + sizeof kBgzfEof) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    const uint64_t marks[2] = {r.out_bytes, r.out_bytes + sizeof kBgzfEof};
    ZGPU_HIP_CHECK(hipMemcpyAsync(b.d_out + r.out_bytes, kBgzfEof, sizeof kBgzfEof, hipMemcpyHostToDevice, st));
    if (b.d_out_offsets) ZGPU_HIP_CHECK(hipMemcpyAsync(b.d_out_offsets + nblocks, marks, sizeof marks, hipMemcpyHostToDevice, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    r.out_bytes += sizeof kBgzfEof; r.nchunks = nblocks;
    *res = r;
    return ZGPU_OK;
}

static int bgzf_deflate_args(zgpu_engine *e, const void *in, uint64_t in_bytes, int *level, int strategy, uint32_t *block_size, const void *out, const zgpu_deflate_result *res)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!res || !out || (!in && in_bytes)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    if (*level == -1) *level = 6;
    if (*level < 1 || *level > 9) return fail(e, ZGPU_STREAM_ERROR, "BGZF encode: level must be 1..9 (or -1 for 6)");
    if (strategy < 0 || strategy > (int)kFixed) return fail(e, ZGPU_STREAM_ERROR, "strategy must be 0..4");
    if (*block_size == 0) *block_size = kBgzfBlockMax;
    if (*block_size > kBgzfBlockMax) return fail(e, ZGPU_STREAM_ERROR, "BGZF encode: block_size is at most 65280");
    return ZGPU_OK;
}

int zgpu_bgzf_deflate_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, int level, int strategy, uint32_t block_size, void *d_out, uint64_t out_cap,
                             uint64_t *d_out_offsets, zgpu_deflate_result *res, void *hip_stream)
{
    int rc = bgzf_deflate_args(e, d_in, in_bytes, &level, strategy, &block_size, d_out, res);
    if (rc) return rc;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    const uint64_t nblocks = (in_bytes + block_size - 1) / block_size;
    if ((rc = e->inf_offs.reserve(e, nblocks + 1))) return rc; // (the segment table: scratch no deflate call uses)
    const BgzfCall b{static_cast<const uint8_t *>(d_in), in_bytes, level, strategy, block_size, e->inf_offs, static_cast<uint8_t *>(d_out), out_cap, d_out_offsets};
    return bgzf_deflate(e, b, res, st);
}

int zgpu_bgzf_deflate_host(zgpu_engine *e, const void *in, uint64_t in_bytes, int level, int strategy, uint32_t block_size, void *out, uint64_t out_cap,
                           uint64_t *out_offsets, zgpu_deflate_result *res)
{
    int rc = bgzf_deflate_args(e, in, in_bytes, &level, strategy, &block_size, out, res);
    if (rc) return rc;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const uint64_t nblocks = (in_bytes + block_size - 1) / block_size, bound = zgpu_bgzf_bound(in_bytes, block_size);
    // staged behind the data: the segment table (nblocks + 1) and the blocks' offsets (nblocks + 2)
    const uint64_t tab_off = (in_bytes + 63) & ~63ull, ooff_off = tab_off + (((nblocks + 1) * sizeof(uint64_t) + 63) & ~63ull);
    if ((rc = ensure_stage(e, ooff_off + (nblocks + 2) * sizeof(uint64_t), bound))) return rc;
    hipStream_t st = e->stream;
    if (in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, in, in_bytes, hipMemcpyHostToDevice, st));
    uint64_t *d_ooff = reinterpret_cast<uint64_t *>(e->stage_in + ooff_off);
    const BgzfCall b{e->stage_in, in_bytes, level, strategy, block_size, reinterpret_cast<uint64_t *>(e->stage_in + tab_off), e->stage_out, bound, d_ooff};
    rc = bgzf_deflate(e, b, res, st);
    if (rc) return rc;
    if (res->out_bytes > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    ZGPU_HIP_CHECK(hipMemcpyAsync(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost, st));
    if (out_offsets) ZGPU_HIP_CHECK(hipMemcpyAsync(out_offsets, d_ooff, (nblocks + 2) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    return ZGPU_OK;
}

#pragma GCC visibility pop
} // extern "C"
