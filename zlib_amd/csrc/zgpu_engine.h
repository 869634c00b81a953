// zgpu_engine.h -- internal (not installed): what the translation units of the engine share on the HOST side.  The engine struct and its owned
// device buffers, and one prototype for every function that is defined in one .hip file and called from another.  Every file that defines one of
// them includes this header too, so a signature that drifts is a compile error.  Default arguments live here only.
#pragma once
#include "zgpu_common.h"
#include "../../include/zamd_gpu.h"
#include <vector>

namespace zgpu {

int fail_hip(zgpu_engine *e, hipError_t err, const char *what, const char *file, int line); // sets the engine's error text; ZGPU_MEM_ERROR for hipErrorOutOfMemory, else ZGPU_ERRNO
int fail(zgpu_engine *e, int code, const char *msg);                                       // sets the engine's error text, returns code

// A device buffer the engine owns: typed, grow-only, freed with the engine.  Growth frees first and then allocates exactly the requested count --
// no doubling, no copy of the old contents; the slack some callers want is in what they ask for.  Reads as the pointer it holds.
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0; // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
    // n <= cap: nothing.  A failed allocation leaves the buffer empty (cap 0) and is reported through fail_hip (e == nullptr: the code only, no error
    // text -- for a caller that can do without the buffer).  *grew: the buffer is a new one
    int reserve(zgpu_engine *e, size_t n, bool *grew = nullptr)
    {
        if (grew) *grew = false;
        if (n <= cap) return ZGPU_OK;
        release();
        const hipError_t err = hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(T));
        if (err != hipSuccess) { p = nullptr; return fail_hip(e, err, "hipMalloc of an engine buffer", __FILE__, __LINE__); }
        cap = n;
        if (grew) *grew = true;
        return ZGPU_OK;
    }
};

// Offsets of the pieces of one allocation, in the order they are asked for: every piece rounded up to 256 bytes; `off` is the size so far
struct Carve {
    size_t off = 0;
    size_t operator()(size_t bytes) { const size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return at; }
};

} // namespace zgpu

namespace zgpu { struct StreamsRoundPart; struct StreamsRound; } // zgpu_deflate_streams_plan.h
struct StageSpan { int stage; hipEvent_t a, b; };

struct zgpu_engine {
    template <typename T> using DevBuf = zgpu::DevBuf<T>;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr; // H2D of the *_host entry points: the next batch's input moves while this batch's kernels run
    std::vector<hipEvent_t> copy_ev;
    hipStream_t d2h_stream = nullptr;  // D2H of zgpu_deflate_host: finished batches' bytes go home while later batches are compressed (a second host thread)
    std::vector<hipEvent_t> done_ev;
    uint64_t *pin_tot = nullptr;       // pinned: out_total behind every batch
    char err[512] = {0};
    // deflate workspace: tokens, meta and slots are one group, sized for batch_cap() chunks
    DevBuf<uint32_t> tokens;
    DevBuf<zgpu::ChunkMeta> meta;
    DevBuf<uint8_t> slots;
    uint32_t batch_cap() const { return (uint32_t)meta.cap; }
    DevBuf<uint4> tables;        // serial LZ only: zeroed when allocated, after that `serial_tag` tells one launch's buckets from another's (SerialLzT::insert)
    uint32_t serial_tag = 0;
    DevBuf<uint8_t> par_ws;      // parallel LZ only (bytes): the larger of the two implementations' workspaces for par_cap chunks
    uint32_t par_cap = 0;
    int tuned = 0; uint32_t tune[4] = {0, 0, 0, 0}; // zgpu_deflate_set_tuning: good, lazy, nice, chain instead of the level's
    int fast_prev0 = 0, before_buf = -1;            // zgpu_deflate_cont_set_stale: deflate_fast feeds search with prev_length 0; the byte in front of the feed's buffer (-1: none)
    int last_tok_match = -1;                        // zgpu_deflate_cont_last_match: the last deflate_slow feed that ended a segment ended on a match (1), a literal (0), made no token (-1)
    uint64_t handed_on = 0; // (diagnostic: chunks handed on since the engine was made)
    DevBuf<uint32_t> hand_list; // chunks the lane-per-chunk loop handed on: [0] their number, [1..] their indices in the batch
    int geo_w = 15, geo_m = 8;   // zgpu_deflate_set_geometry: deflateInit2's windowBits and memLevel
    DevBuf<uint8_t> geo_slots; DevBuf<uint4> geo_tables; DevBuf<uint32_t> geo_nostore; // the workspace of a non-default geometry (one group)
    int exact_sort = 0;          // sticky: the fast sort's self-check failed once on this engine (zgpu_lz_sort.hip, pass V)
    DevBuf<uint64_t> offsets;    // nchunks+1 segment offsets of the current call
    DevBuf<zgpu::RunState> run;  // one
    // staging for the *_host entry points (bytes)
    DevBuf<uint8_t> stage_in, stage_out;
    // inflate scratch (status and slots: bytes)
    DevBuf<uint8_t> inf_status;
    DevBuf<zgpu::ChunkMeta> inf_meta;
    DevBuf<uint64_t> inf_offs;
    DevBuf<uint8_t> inf_slots;
    DevBuf<uint8_t> inf_dict; uint32_t inf_dict_len = 0; // preset dictionary of the next inflate calls (zgpu_inflate_set_dictionary)
    uint32_t inf_checks = 3;                             // checks of the decoded bytes (zgpu_inflate_set_checks)
    // continuous stream (deflate_cont): per batch of tiles (one group, for ct_tiles() tiles) / per feed (ct_entry)
    DevBuf<uint16_t> ct_exits, ct_entry, ct_comp, ct_gentry;
    DevBuf<uint32_t> ct_tokoff, ct_T, ct_carry, ct_carry_in;
    DevBuf<zgpu::ContBlk> ct_blk; DevBuf<uint64_t> ct_pos; DevBuf<uint8_t> ct_slots; DevBuf<zgpu::ContState> ct_st;
    uint32_t ct_tiles() const { return ct_tokoff.cap ? (uint32_t)(ct_tokoff.cap - 1) : 0; } // (ct_tokoff: a word per tile and one more)
    DevBuf<zgpu::ChunkMeta> ct_ckmeta;
    DevBuf<uint64_t> ct_excl;
    // many streams in one call (zgpu_deflate_streams.hip): per call -- the tiles' rows and entries, a state and the checksums per item, the totals, the
    // plan (the parts of every batch back to back, a record per batch, the tiles in front of every item); per batch of tiles -- the token offsets (a
    // word per tile and one more per stream), whose every block slot is; the host entry's tables, rooms' records and packed streams
    DevBuf<zgpu::TileRow> ds_rows; DevBuf<uint16_t> ds_entry; DevBuf<zgpu::ContState> ds_st; DevBuf<zgpu_check_item> ds_check; DevBuf<unsigned long long> ds_totals;
    DevBuf<uint32_t> ds_tokoff, ds_blk_item; DevBuf<zgpu::StreamsRoundPart> ds_parts; DevBuf<zgpu::StreamsRound> ds_rounds; DevBuf<uint64_t> ds_tile0;
    DevBuf<uint64_t> ds_in_off, ds_oo, ds_po; DevBuf<zgpu_deflate_batch_item> ds_items; DevBuf<uint8_t> ds_packed;
    // ... levels 1-3: the rounds of fastwin_tile_kernel (the per-batch ones are one group)
    DevBuf<uint16_t> cf_exit_a, cf_exit_b; DevBuf<uint32_t> cf_ins0, cf_ins1, cf_prev, cf_prev2, cf_hist, cf_count;
    DevBuf<uint8_t> cf_cur, cf_act_a, cf_act_b, cf_changed, cf_kept; DevBuf<uint32_t> cf_list_a, cf_list_b, cf_used; DevBuf<uint16_t> cf_entry_used;
    DevBuf<uint32_t> cf_dbg, cf_dstat; // (ZGPU_FAST_TRACE; cf_dstat ZGPU_FAST_STATS as well)
    hipStream_t ct_stream = nullptr; hipEvent_t ct_ev_a[2] = {nullptr, nullptr}, ct_ev_b[2] = {nullptr, nullptr}; // levels 4-9: a batch's blocks are made on a second stream under the next batch's walkers
    uint64_t cf_rounds = 0, cf_tile_parses = 0; // (diagnostic: rounds and tile parses since the engine was made)
    uint64_t cf_stat[6] = {};                   // (ZGPU_FAST_STATS: FastTiles::stat summed over the rounds since the engine was made)
    // BGZF block finder (zgpu_bgzf.hip): per 4096 positions (bz_cnt, bz_base), per candidate (the others), one result record
    DevBuf<uint32_t> bz_cnt, bz_isize, bz_jump_a, bz_jump_b, bz_reach, bz_res;
    DevBuf<uint64_t> bz_base, bz_pos, bz_next, bz_in_off, bz_out_off;
    DevBuf<zgpu_inflate_item> bz_items;
    // multi-member gzip (zgpu_gzip.hip): the finder's bz_* buffers serve it too; per candidate the input end, the ISIZE guess, the trial layout
    // (one more), where the member ends; the candidates' records of the first decode (bz_items holds the members')
    DevBuf<uint64_t> gz_in_end, gz_trial, gz_next; DevBuf<uint32_t> gz_guess;
    DevBuf<zgpu_inflate_item> gz_items;
    // packed batch decode (zgpu_inflate_batch_packed_*): where every item's range ends, the decoder's records until they are merged with the sizing pass's
    DevBuf<uint64_t> pk_hi; DevBuf<zgpu_inflate_item> pk_items;
    // batch checksums (zgpu_checksum.hip): pieces in front of every item (n + 1), the bad-table flag, three words per piece (a, b, crc)
    DevBuf<uint64_t> ck_piece0; DevBuf<uint32_t> ck_flag, ck_part;
    // profiling
    bool prof = false;
    double ms[ZGPU_STAGE_COUNT] = {0};
    uint64_t launches[ZGPU_STAGE_COUNT] = {0};
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<StageSpan> spans;

    zgpu_engine() = default;
    zgpu_engine(const zgpu_engine &) = delete;
    zgpu_engine &operator=(const zgpu_engine &) = delete;
    ~zgpu_engine(); // waits for the main stream, destroys events and streams; the buffers free themselves
};

namespace zgpu {

// ---- zgpu_engine.hip ----
void collect_spans(zgpu_engine *e);
int ensure_stage(zgpu_engine *e, uint64_t in_bytes, uint64_t out_bytes);
hipEvent_t engine_copy_event(zgpu_engine *e, size_t i);
// stage timing of the other files' launches with the engine's event pool
void prof_span_begin(zgpu_engine *e, hipStream_t st, hipEvent_t *a);
void prof_span_end(zgpu_engine *e, hipStream_t st, int stage, hipEvent_t a);
struct StageTimer { // a stage's launches in one scope
    zgpu_engine *e; hipStream_t st; int stage; hipEvent_t a{};
    StageTimer(zgpu_engine *e_, hipStream_t st_, int stage_) : e(e_), st(st_), stage(stage_) { prof_span_begin(e, st, &a); }
    ~StageTimer() { prof_span_end(e, st, stage, a); }
};
uint32_t env_u32(const char *name, uint32_t dflt); // an environment knob: its value when it is a number above 0, else dflt
// Adler-32 (mask bit 0) and CRC-32 (bit 1) of d_bytes[0, nbytes) from 64 KiB pieces, at most batch_cap of them a launch, their records in `meta`
int checksum_pass(zgpu_engine *e, const uint8_t *d_bytes, uint64_t nbytes, uint32_t mask, uint32_t batch_cap, DevBuf<ChunkMeta> &meta, hipStream_t st, uint32_t *adler, uint32_t *crc);

// ---- zgpu_deflate.hip ----
// the chunked compressor's workspace for `batch` chunks a launch (serial: the lane-per-chunk loop's tables, else the sorted buckets; geo: a non-default
// geometry's wider group) and the offsets of a call of nchunks_total chunks; the tiles of the continuous stream and the checksum entry points use it too
int ensure_deflate_ws(zgpu_engine *e, uint32_t batch, bool serial, uint64_t nchunks_total, bool geo = false);
LevelCfg level_cfg_for(const zgpu_engine *e, int level, int strategy); // the level's parameters, or zgpu_deflate_set_tuning's
FrameHead frame_head(int level, int strategy, bool wrap, bool gz, bool bgzf = false);
int write_trailer(zgpu_engine *e, bool gz, uint32_t adler, uint32_t crc, uint64_t in_bytes, uint8_t *d_out, uint64_t *out_total, hipStream_t st);
struct PlanEngine; // zgpu_deflate_plan.h
PlanEngine plan_engine(const zgpu_engine *e, const LevelCfg *cfg);

// ---- zgpu_deflate_streams.hip ----
const char *streams_refuse(const zgpu_engine *e, const zgpu_deflate_params *p); // why the batch compress of many streams does not serve these parameters, nullptr: it does
void streams_list_geom(const uint8_t *d_in, uint64_t in_bytes, uint16_t *exits, uint16_t *entry, ChunkGeom *g, TileGeom *tg); // a list of tiles that comes row by row: what both batch calls give the LZ stage

// ---- zgpu_deflate_cont.hip ----
int deflate_cont_oneshot(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const zgpu_deflate_params *p, uint8_t *d_out, uint64_t out_cap, zgpu_deflate_result *res, hipStream_t st);

// ---- zgpu_lz_serial.hip ----
void launch_lz_serial(const ChunkGeom &g, LevelCfg cfg, uint4 *tables, uint32_t *tokens, ChunkMeta *meta, hipStream_t st, uint32_t *nostore_bits, bool hand_on, uint32_t tag);

// ---- zgpu_huffman.hip ----
void launch_huffman(const ChunkGeom &g, const uint32_t *tokens, ChunkMeta *meta, uint8_t *slots, hipStream_t st, bool fixed_trees);
void launch_huffman_cont(const ChunkGeom &g, const uint32_t *compact_tokens, uint32_t nblk, ContBlk *blk, ContState *cst, uint8_t *slots, hipStream_t st, bool fixed_trees);
void launch_huffman_streams(const ChunkGeom &g, const uint32_t *batch_tokens, uint32_t nslots, ContBlk *blk, ContState *states, const uint32_t *blk_item, uint8_t *slots, hipStream_t st,
                            bool fixed_trees);

// ---- zgpu_stitch.hip ----
void launch_collect_handed_on(const ChunkMeta *meta, uint32_t n, uint32_t *list, uint32_t *count, hipStream_t st);
void launch_adler(const ChunkGeom &g, ChunkMeta *meta, hipStream_t st);
void launch_crc(const ChunkGeom &g, ChunkMeta *meta, hipStream_t st);
void launch_scan(const ChunkMeta *meta, uint32_t nchunks, uint64_t chunk0, uint64_t *offsets, void *run, uint64_t out_cap, hipStream_t st, bool with_crc = false);
void launch_frame(const uint8_t *slots, const ChunkMeta *meta, uint64_t *offsets, const uint64_t *seg_off, uint64_t chunk0, uint32_t nchunks, uint8_t *out,
                  uint64_t out_cap, uint32_t slot_stride, void *run, bool with_crc, const FrameHead &h, hipStream_t st);
void launch_stitch(const uint8_t *slots, const ChunkMeta *meta, const uint64_t *offsets, uint64_t chunk0, uint32_t nchunks, uint8_t *out,
                   uint64_t out_cap, uint32_t slot_stride, hipStream_t st);
void launch_bgzf_cut(uint64_t in_bytes, uint32_t block_size, uint64_t nseg, uint64_t *seg_off, hipStream_t st); // seg_off[k] = min(k * block_size, in_bytes), k = 0..nseg
void launch_seg_limit(const uint64_t *seg_off, uint64_t nseg, uint64_t in_bytes, uint32_t limit, uint32_t *flag, hipStream_t st); // flag[0] |= 1: a segment over `limit` bytes
// records of the batch's segments behind its scan: where each stream lies in the output (offsets) and what ChunkMeta knows of its input
void launch_seg_items(const ChunkMeta *meta, const uint64_t *offsets, const uint64_t *seg_off, uint64_t chunk0, uint32_t nchunks, bool with_crc, zgpu_deflate_item *items, hipStream_t st);
void launch_corpus(uint32_t kind, uint64_t seed, uint64_t first_chunk, uint64_t nchunks, uint8_t *out, hipStream_t st);
void launch_batch_finish(const BatchItemState *items, uint64_t n, const ChunkMeta *meta, const uint8_t *in, uint32_t do_adler, uint32_t do_crc,
                         zgpu_inflate_item *out_items, unsigned long long *nfailed, hipStream_t st);

// ---- zgpu_lz_parallel.hip ----
bool lz_parallel_available();
size_t lz_parallel_workspace_bytes(uint32_t batch_chunks);
void launch_lz_parallel(const ChunkGeom &g, LevelCfg cfg, void *workspace, uint32_t *tokens, ChunkMeta *meta, hipStream_t st, zgpu_engine *prof);
void launch_parse(const ChunkGeom &g, LevelCfg cfg, const uint2 *recs, uint32_t *tokens, ChunkMeta *meta, hipStream_t st);

// ---- zgpu_lz_parse.hip ----
void launch_parse2(const ChunkGeom &g, LevelCfg cfg, const uint2 *recs, uint32_t *tokens, ChunkMeta *meta, hipStream_t st);
void launch_parse_tile(const ChunkGeom &g, LevelCfg cfg, const uint32_t *gm, const uint32_t *gs, uint32_t *tokens, ChunkMeta *meta, const TileGeom &tg, hipStream_t st);

// ---- zgpu_lz_sorted.hip ----
size_t lz_sorted_workspace_bytes(uint32_t batch_chunks);
uint32_t *lz_sorted_fault_word(void *workspace);
bool launch_lz_sorted(const ChunkGeom &g, LevelCfg cfg, void *workspace, uint32_t *tokens, ChunkMeta *meta, hipStream_t st, zgpu_engine *prof, int exact_sort,
                      int impl); // impl: ZGPU_LZ_SORTED, _WALK, _FAST or _FASTWIN
// continuous stream
void launch_lz_tiles(const ChunkGeom &g, const TileGeom &tg, LevelCfg cfg, void *workspace, ChunkMeta *meta, uint16_t *comp, uint16_t *gentry, hipStream_t st, zgpu_engine *prof,
                     int exact_sort);
void launch_lz_tiles_parse(const ChunkGeom &g, const TileGeom &tg, LevelCfg cfg, void *workspace, uint32_t *tokens, ChunkMeta *meta, hipStream_t st, zgpu_engine *prof);
void launch_sort_tiles(const ChunkGeom &g, void *workspace, ChunkMeta *meta, hipStream_t st, zgpu_engine *prof, int exact_sort, const uint16_t **S_out, const uint32_t **ir_out);

// ---- zgpu_lz_fastwin.hip ----
bool lz_fastwin_serves(const LevelCfg &cfg);
void launch_lz_fastwin(const ChunkGeom &g, LevelCfg cfg, const uint16_t *S, const uint32_t *ir, uint32_t *tokens, ChunkMeta *meta, hipStream_t st);
void launch_lz_fastwin_tiles(const ChunkGeom &g, const TileGeom &tg, const FastTiles &ft, LevelCfg cfg, const uint16_t *S, const uint32_t *ir, uint32_t *tokens, ChunkMeta *meta, uint32_t ngrid,
                             hipStream_t st);
void launch_fast_init(uint8_t *cur, uint8_t *active, uint16_t *exit_cur, uint32_t n, hipStream_t st);
void launch_fast_flip_list(uint8_t *cur, uint16_t *exit_cur, const uint16_t *exit_new, const uint32_t *list, uint32_t n, hipStream_t st);
void launch_fast_flip(uint8_t *cur, const uint8_t *active, uint8_t *active_next, const uint8_t *changed, uint16_t *exit_cur, const uint16_t *exit_new, uint32_t n, uint32_t round,
                      uint32_t *count, uint32_t *list, const uint8_t *kept, hipStream_t st);
void launch_fast_finish(const uint8_t *cur, const uint16_t *exit_cur, const uint32_t *ins0, const uint32_t *ins1, uint32_t n, uint16_t *entry_after, uint32_t *prev_ins, uint32_t *prev_prev_ins,
                        const uint32_t *low, hipStream_t st);
void launch_fast_hist(const uint32_t *before, const uint32_t *last, uint32_t x0, uint32_t count, uint32_t *out, hipStream_t st);

// ---- zgpu_cont.hip ----
uint32_t chain_groups(uint32_t ntiles);
uint64_t cont_special_pos(uint64_t n);
void launch_chain(const uint16_t *exits, uint32_t ntiles, uint16_t *comp, uint16_t *gentry, uint16_t *entry, hipStream_t st);
void launch_cont_tokens(const ChunkGeom &g, const TileGeom &tg, const uint32_t *tokens, const ChunkMeta *tmeta, ContState *st, uint32_t *tokoff, const uint32_t *carry, uint32_t *T,
                        ContBlk *blk, uint64_t seg_end, bool final_block, uint64_t sp, uint32_t nblk_cap, bool slow, hipStream_t s);
void launch_cont_stitch(const ContBlk *blk, ContState *st, uint64_t *pos, const uint8_t *slots, uint32_t slot_stride, const uint8_t *in, uint64_t abs0, uint8_t *out, uint64_t out_cap,
                        uint32_t nblk_cap, const uint32_t *T, uint32_t *carry, uint64_t seg_end, hipStream_t s);

// the batched block layer: one round (batch of tiles) of a batch call over many streams, everything in device memory
struct ContBatch {
    const StreamsRoundPart *parts; const StreamsRound *round; // the round's parts and their number (streams_round_plan on the host, senq_round_kernel on the device)
    const uint64_t *in_off, *oo, *tile0; uint64_t t0;          // the caller's tables, the tiles in front of every item, the round's first tile in the list
    const uint8_t *in; uint8_t *out; uint32_t flags, slow, nslots_max;
    ContState *st; const uint16_t *entry;                      // per item; per tile of the list
    const uint32_t *tokens; const ChunkMeta *tmeta;            // per tile of the round
    uint32_t *tokoff, *carry, *T; ContBlk *blk; uint64_t *pos; const uint8_t *slots; uint32_t *blk_item;
};
void launch_cont_batch_tokens(const ContBatch &q, uint32_t nparts_max, uint32_t ntiles_max, hipStream_t s); // (the launches' extents: the round's numbers, or bounds of them)
void launch_cont_batch_stitch(const ContBatch &q, uint32_t nparts_max, hipStream_t s);

// ---- zgpu_streams.hip ----
// state: nullptr, or the stream-ordered call's table check (state[k] != 0 marks an item it has failed); totals: cleared by the head launch unless nullptr
void launch_streams_head(const uint64_t *in_off, const uint64_t *oo, const uint32_t *state, uint64_t n, const FrameHead &fh, uint32_t flags, ContState *st, uint8_t *out, uint16_t *entry0,
                         unsigned long long *totals, hipStream_t s);
void launch_streams_entry(const TileRow *rows, uint32_t ntiles, uint16_t *entry, hipStream_t s);
void launch_streams_finish(const uint64_t *in_off, const uint64_t *oo, const uint32_t *state, uint64_t n, const FrameHead &fh, uint32_t flags, const ContState *st,
                           const zgpu_check_item *chk, bool want_crc, uint8_t *out, zgpu_deflate_batch_item *items, unsigned long long *totals, hipStream_t s);
void launch_streams_pack(const uint8_t *rooms, const uint64_t *oo, const uint64_t *po, uint64_t n, uint64_t total, uint8_t *packed, hipStream_t s);

// ---- zgpu_streams_batch.hip: the stream-ordered call's plan, made on the device ----
void launch_senq_clear(unsigned long long *cnt, uint32_t *fault, zgpu_deflate_batch_summary *summary, hipStream_t s);
void launch_senq_scan(const uint64_t *in_off, const uint64_t *oo, uint64_t n, uint64_t in_bytes, uint64_t out_cap, uint32_t *state, uint64_t *tile0, uint64_t *piece0,
                      unsigned long long *cnt, hipStream_t s);
void launch_senq_rows(const uint64_t *in_off, const uint64_t *tile0, uint64_t n, uint64_t nrows, TileRow *rows, hipStream_t s);
// a round's parts and their number; the exit rows and records of its padding rows (rows, exits, meta: the round's)
void launch_senq_round(const uint64_t *tile0, uint64_t n, uint64_t t0, uint32_t batch, const TileRow *rows, StreamsRoundPart *parts, StreamsRound *round, uint16_t *exits, ChunkMeta *meta,
                       hipStream_t s);
void launch_senq_layout(const uint64_t *in_off, uint64_t n, uint64_t in_bytes, uint32_t flags, uint64_t *oo, hipStream_t s);
void launch_senq_summary(const uint32_t *fault, uint64_t n, const unsigned long long *cnt, zgpu_deflate_batch_item *items, zgpu_deflate_batch_summary *summary, hipStream_t s);

// ---- zgpu_inflate.hip ----
// One launch of the decoder, inflate_kernel_t: segments [chunk0, chunk0 + nchunks) of `offsets`, one workgroup each, records to status[0, nchunks).  The
// defaults are those of a stream that stands alone (batch items, the sizing pass, the pieces of a foreign stream)
struct InfLaunch {
    const uint8_t *in; uint64_t in_bytes; const uint64_t *offsets; uint64_t chunk0; uint32_t nchunks;
    uint8_t *out; uint64_t out_cap; InfStatus *status;
    uint64_t last_chunk = ~0ull; uint32_t chunk_size = kWholeStream; ChunkMeta *meta = nullptr;
    const uint8_t *dict = nullptr; uint32_t dict_len = 0; uint32_t stream_mode = 1;
    uint32_t checks = 0; // kInfBatchFold only: the checks to fold (bit 0 Adler-32, bit 1 CRC-32)
};
// kInfPieces: always the 32 KiB ring of 16-bit symbols; kInfSizes: no ring at all; kInfVerify: the 32 KiB ring and no destination -- `out` is not
// used, `out_cap` carries the checks to compute (bit 0 Adler-32, bit 1 CRC-32) and `meta` takes one record per item: out_bytes, adler_a, adler_b, crc;
// kInfBatchFold: kInfBatch that also folds what it stores (ring_kb counts, as for kInfBatch) -- `out` and `out_cap` are the destination's, `checks`
// says what to fold, `meta` takes one record per item as for kInfVerify; kInfPieceSizes: kInfPieces' rows (sp.rows) counted as kInfSizes counts, one wave per
// slot and no ring -- `out` and the page pool are not used, sp.ends and sp.need take one record per slot; kInfPieces with sp.mid == nullptr: no pages, the
// tails and the end records alone; kInfPieceVerify: kInfPieces' rows read as kInfPieces reads them and written as kInfVerify writes -- the byte ring
// preloaded from sp.windows, reach from sp.ostart, `out_cap` the checks to compute, one PieceCheck per slot to sp.checks, `out` and `meta` not used
enum InfKind { kInfChunks, kInfBatch, kInfSizes, kInfPieces, kInfVerify, kInfBatchFold, kInfPieceSizes, kInfPieceVerify };
constexpr int kInfNoRing = 0; // ring_kb of a kInfSizes, kInfPieces, kInfPieceSizes, kInfPieceVerify or kInfVerify launch: the kind fixes the ring, the launcher does not look at the value
int inflate_ring_kb(); // ZGPU_INF_RING_KB, read at EVERY call (the tests run the same streams through all three): 8, 16, anything else 32; not set: the build's default
void launch_inflate_decode(InfKind kind, int ring_kb, const InfLaunch &a, const SpecArgs &sp, hipStream_t st);
int output_checksums(zgpu_engine *e, const uint8_t *d_out, uint64_t nbytes, uint64_t out_cap, zgpu_inflate_result *res, hipStream_t st);
int inflate_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_offsets, uint64_t nchunks, uint32_t chunk_size, uint8_t *d_out, uint64_t out_cap,
                zgpu_inflate_result *res, hipStream_t st, uint32_t stream_mode = 0, const uint64_t *h_offsets = nullptr, bool open_end = false, uint8_t *h_dst = nullptr, uint64_t h_cap = 0);

// ---- zgpu_inflate_stream.hip: the kernels of a stream decoded in pieces, over the pieces of many streams ----
void launch_spec_find_table(const uint8_t *d_in, uint64_t in_bytes, const PieceTarget *table, uint32_t ntargets, uint64_t *found, hipStream_t st);
void launch_spec_resolve_items(const SpecArgs &sp, uint32_t nslots, uint32_t nitems, const uint2 *ranges, const uint8_t *entry, uint8_t *windows, const uint64_t *out_start,
                               PieceItem *items, uint8_t *d_out, hipStream_t st);
void launch_spec_windows_items(uint16_t *tails, uint32_t nslots, uint32_t nitems, const uint2 *ranges, const uint8_t *entry, uint8_t *windows, hipStream_t st); // the windows of the same, nothing resolved

// ---- zgpu_inflate_batch_pieces.hip: the long items of a blocking batch decode, in pieces ----
struct BatchPiecesKnobs { uint64_t min_bytes, round_bytes; };
BatchPiecesKnobs batch_pieces_knobs(); // ZGPU_BATCH_PIECES_MIN_BYTES, ZGPU_BATCH_PIECES_ROUND_BYTES, read at EVERY call (the tests switch them within one process)
uint64_t batch_pieces_count(int which); // 0: items decoded in pieces, 1: long items that fell back to the one-workgroup decoder
size_t batch_pieces_scratch_bytes(uint64_t max_long); // the room the piece path wants at `scr` (256-byte aligned) for a call with room for max_long long items
PieceItem *batch_pieces_items(uint8_t *scr);           // ... and where the list the header kernel fills (PiecesList::items) lies in it
// d_hdr: the call's eight counters (PiecesList::hdr) and hdr what the caller read of them behind the header kernel (hdr[kHdrLong]: the number of long
// items, not 0).  Round by round find, select, decode, chain, windows and resolve over the pieces of all long items, the records of the clean ones to
// status[k], the others through one more kInfBatch launch; states[k].code of every long item is put back to the header's ZGPU_OK (the caller's first
// merge has put the empty segment's verdict there), so that the caller's second merge takes the record.  Ends with a read-back of the counters
int batch_pieces_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, uint8_t *d_out, uint64_t out_cap, uint64_t max_long, uint8_t *scr, unsigned long long *d_hdr,
                     const unsigned long long *hdr, BatchItemState *states, InfStatus *status, uint64_t round_bytes, int ring_kb, hipStream_t st);
// The sizing form (the sizing pass of zgpu_inflate_batch_sizes_* / _packed_*): the same list, finders and selection; the pieces are COUNTED (kInfPieceSizes),
// pieces_sizes_chain (zgpu_inflate_pieces_plan.h) is the verdict, a clean item's record is the one kInfSizes writes for it and every other item goes
// through one kInfSizes launch.  No destination, no pages, no windows, no resolve pass.
struct BatchPiecesSizesKnobs { uint64_t min_bytes, round_slots; }; // round_slots 0: no cap
BatchPiecesSizesKnobs batch_pieces_sizes_knobs(); // ZGPU_BATCH_PIECES_SIZES_MIN_BYTES (not set: ZGPU_BATCH_PIECES_MIN_BYTES), ZGPU_BATCH_PIECES_SIZES_ROUND_SLOTS, read at EVERY call
uint64_t batch_pieces_sizes_count(int which); // 0: long items sized in pieces, 1: long items of a sizing pass that fell back to the one-wave sizing kernel
int batch_pieces_sizes_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, uint64_t max_long, uint8_t *scr, unsigned long long *d_hdr, const unsigned long long *hdr,
                           BatchItemState *states, InfStatus *status, uint64_t round_slots, hipStream_t st);
// The verify form (the blocking integrity test, inflate_batch_verify_run): the same list, finders and selection; the pieces are decoded twice inside LDS --
// the tails pass (kInfPieces without pages), pieces_verify_chain, the window kernels, the check pass (kInfPieceVerify) -- and pieces_verify_confirm
// (zgpu_common.h) joins a clean item's check values into meta[k], its record into status[k] as kInfVerify writes them; every other item goes through one
// kInfVerify launch.  No destination, no pages, no resolve pass: a round's scratch is pieces_verify_round_plan's, bounded by the slot cap.
struct BatchPiecesVerifyKnobs { uint64_t min_bytes, round_slots; }; // round_slots: pieces_verify_slot_cap of the knob
BatchPiecesVerifyKnobs batch_pieces_verify_knobs(); // ZGPU_BATCH_PIECES_VERIFY_MIN_BYTES (not set: ZGPU_BATCH_PIECES_MIN_BYTES where set, else kPiecesVerifyMinBytesDefault), ZGPU_BATCH_PIECES_VERIFY_ROUND_SLOTS, read at EVERY call
uint64_t batch_pieces_verify_count(int which); // 0: long items verified in pieces, 1: long items of an integrity test that fell back to the one-workgroup verifier
size_t batch_pieces_verify_scratch_bytes(uint64_t max_long); // batch_pieces_scratch_bytes and the fallback's compact check records (the list lies where batch_pieces_items says)
int batch_pieces_verify_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, uint32_t checks, uint64_t max_long, uint8_t *scr, unsigned long long *d_hdr,
                            const unsigned long long *hdr, BatchItemState *states, InfStatus *status, ChunkMeta *meta, uint64_t round_slots, hipStream_t st);

// ---- zgpu_inflate_batch.hip ----
int inflate_batch_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, uint32_t checks, uint8_t *d_out, uint64_t out_cap,
                      const uint64_t *d_out_off, zgpu_inflate_item *d_items, uint64_t *nfailed, hipStream_t st);
int inflate_batch_run_ranges(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_lo, const uint64_t *d_in_hi, uint64_t n, int wrap, uint32_t checks,
                             uint8_t *d_out, uint64_t out_cap, const uint64_t *d_out_lo, const uint64_t *d_out_hi, zgpu_inflate_item *d_items, uint64_t *nfailed,
                             const BatchItemState **states, hipStream_t st, bool no_pieces = false);
int inflate_batch_sizes_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, zgpu_inflate_item *d_items, uint64_t *nfailed,
                            hipStream_t st);
int inflate_batch_verify_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, uint32_t checks, zgpu_inflate_item *d_items,
                             uint64_t *nfailed, const BatchItemState **states, hipStream_t st);
int inflate_batch_packed_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_in_off, uint64_t n, int wrap, uint32_t checks, uint32_t align,
                             uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, zgpu_inflate_item *d_items, uint64_t *total, uint64_t *nfailed, hipStream_t st,
                             bool stage_out = false);

// ---- zgpu_checksum.hip ----
int checksum_batch_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t n, uint32_t checks, zgpu_check_item *d_items, hipStream_t st);
void checksum_batch_enqueue(const uint8_t *d_in, const uint64_t *d_off, const uint32_t *state, const uint64_t *piece0, uint64_t n, uint64_t npieces_max, uint32_t checks, void *part,
                            zgpu_check_item *d_items, hipStream_t st);

} // namespace zgpu
