// zgpu_deflate_plan.h -- internal (not installed): what a compress call DECIDES before it touches the device, as functions of plain values -- which
// LZ77 implementation serves it, how many chunks or tiles go into one batch, in what steps the batches grow, in how many phases round 0 of the
// levels 1-3 tiles runs.  No HIP call, no getenv: the callers (zgpu_deflate.hip, zgpu_deflate_cont.hip) read the environment into the knob structs and the
// device into PlanEngine, and tests/tools/deflate_plan_model.cpp prints the same plans on a machine without a GPU.  Besides zgpu_common.h only the
// public header is included, for the names of the flags, implementations and codes.
#pragma once
#include "zgpu_common.h"
#include "../../include/zamd_gpu.h"

namespace zgpu {

// What the engine is set to and what it holds when the call arrives
struct PlanEngine {
    int geo_w = 15, geo_m = 8;                       // zgpu_deflate_set_geometry
    bool tuned = false; uint32_t tune[4] = {0, 0, 0, 0}; // zgpu_deflate_set_tuning: good, lazy, nice, chain
    bool exact_sort = false;                         // the fast sort's self-check failed once on this engine
    bool lz_parallel = true;                         // lz_parallel_available()
    bool fastwin_serves = false;                     // lz_fastwin_serves() of the level's (or deflateTune's) parameters; false where there is no such level
    uint64_t sorted_ws_chunk = 0;                    // lz_sorted_workspace_bytes(1)
    uint32_t batch_cap = 0, par_cap = 0, ct_tiles = 0; // chunks / chunks of buckets / tiles the workspaces have room for
    uint64_t free_bytes = 0;                         // free device memory; 0: not known, no memory cap
};

// The caller's parameters of a chunk or segment call
struct PlanCall {
    bool args = false;       // none of the pointers the call needs is null
    int level = 0, strategy = 0, lz_impl = ZGPU_LZ_AUTO;
    uint32_t chunk_size = 0, flags = 0, prime = 0;
    uint64_t in_bytes = 0;
    bool seg = false; uint64_t nseg = 0; // a segment table, its segments
    uint32_t skip0 = 0;      // dictionary bytes in front of the one chunk
    bool host_in = false;    // the input still lies in host memory and comes batch by batch
};

// Environment knobs of the chunk path; 0 / not set: the default, which the plan knows
struct DeflateKnobs {
    int lz_default = 0;       // ZGPU_LZ_DEFAULT (read once a process)
    char hand_on = 0;         // ZGPU_HAND_ON: the value's first character
    uint32_t batch_chunks = 0, host_batch = 0, first_batch = 0; // ZGPU_BATCH_CHUNKS, ZGPU_HOST_BATCH, ZGPU_FIRST_BATCH
};

struct DeflatePlan {
    int rc = ZGPU_OK; const char *msg = nullptr; // a refusal: nothing else is filled in
    LevelCfg cfg{};          // the level's or deflateTune's parameters, the strategy's chain budget and the geometry applied
    int impl = 0;            // ZGPU_LZ_*, never AUTO
    bool serial = false, hand_on = false, geo = false, check_sort = false, with_crc = false;
    bool wrap = false, gz = false, bgzf = false, seg_wrap = false;
    uint32_t chunk_size = 0, block_tokens = 0, head_bytes = 0, tail_bytes = 0;
    uint64_t nchunks = 0;
    uint32_t batch = 0;      // chunks of a full batch
    uint32_t hand_piece = 0; // hand_on: chunks of one launch of the wave-per-chunk kernel, before what an earlier call has left (par_cap) is looked at
    uint32_t first = 0;      // chunks of the first batch
};

inline DeflatePlan plan_refused(const char *msg) { DeflatePlan pl; pl.rc = ZGPU_STREAM_ERROR; pl.msg = msg; return pl; }

// the level's parameters, or deflateTune's (deflate.c:453-470): the level keeps its function, the four parameters are the caller's
inline LevelCfg level_cfg_tuned(int level, int strategy, bool tuned, const uint32_t tune[4])
{
    LevelCfg cfg = level_cfg(level);
    cfg.strategy = (uint32_t)strategy;
    if (tuned) {
        // (a budget of 0 never runs out in the reference: its loop counts down past zero, deflate.c:1163 -- here the largest budget there is, whose quarter no
        //  chain of a chunk, 65535 candidates at the most, reaches either.  Any other max_chain is kept as it is: the quarter of 70000 is 17500.)
        cfg.good = tune[0]; cfg.lazy = tune[1]; cfg.nice = tune[2]; cfg.chain = tune[3] ? tune[3] : 0xffffffffu;
        if (cfg.nice > kMaxMatch) cfg.nice = kMaxMatch; // (no match is longer: the same searches)
    }
    return cfg;
}

// The implementations that search every position ONCE, with nothing in hand, and leave two records per position -- the full budget's and the quarter's --
// for the parse to pick from (ZGPU_LZ_SORTED, ZGPU_LZ_PARALLEL; ParseCtx::take) rest on relations that hold in every level's row and that deflateTune
// can break.  nullptr: the row is served; else why not.  (cfg: the strategy's chain budget applied.)
inline const char *records_refuse(const LevelCfg &cfg, int impl)
{
    const bool searches = cfg.strategy != kHuffmanOnly && cfg.strategy != kRle; // (Z_RLE: the nearest candidate only, no quarter; ParseCtx::take)
    // a quarter budget of 0 never runs out (deflate.c:1163): with good_length bytes in hand the search goes through the whole chain, not max_chain candidates
    if (searches && cfg.chain < 4) return "ZGPU_LZ_SORTED / ZGPU_LZ_PARALLEL do not serve a max_chain below 4 (deflateTune): its quarter budget never runs out";
    // with nice_length bytes or more in hand a candidate of nice_length bytes is passed over and the walk goes on; the record's walk ended there
    if (searches && cfg.lazy > cfg.nice && cfg.nice < kMaxMatch) return "ZGPU_LZ_SORTED / ZGPU_LZ_PARALLEL do not serve max_lazy > nice_length (deflateTune)";
    // match3_kernel counts a walk's candidates in 12 bits of a key (level 9's 4096 fill them)
    if (searches && impl == ZGPU_LZ_SORTED && cfg.chain > 4096) return "ZGPU_LZ_SORTED does not serve a max_chain above 4096 (deflateTune)";
    return nullptr;
}

// The wave-per-chunk kernels of levels 1-3 (ZGPU_LZ_FASTWIN, zgpu_lz_fastwin.hip; lz_fastwin_serves) are instantiated for the levels' three pairs of max_chain and
// nice_length and start every search with the full budget (prev_length = 2 < good_length = 4).  max_insert_length (cfg.lazy) is a run-time value, but it must stay
// below nice_length: the token walk decides whether a match's strings go into the chains from the length the lanes have COMPARED, which for a match of
// nice_length bytes or more is not its length yet ("longm", in both kernels) -- right only while every such match is longer than max_insert_length.
// Anything else -- a deflateTune row -- goes to the lane-per-chunk loop; the same predicate guards the continuous stream and the hand-on.
inline bool fastwin_row_serves(const LevelCfg &cfg)
{
    if (cfg.slow || cfg.good != 4 || cfg.lazy >= cfg.nice) return false;
    return (cfg.chain == 4 && cfg.nice == 8) || (cfg.chain == 8 && cfg.nice == 16) || (cfg.chain == 32 && cfg.nice == 32);
}

// deflate_fast on the sorted buckets (ZGPU_LZ_FAST, fast_kernel) holds the index of the seven positions behind a token's start, which is all a level's
// max_insert_length (4, 5, 6) asks for, and starts every search with the full budget, as prev_length = 2 < good_length = 4 has it.
inline const char *fast_refuse(const LevelCfg &cfg)
{
    if (cfg.lazy > 7) return "ZGPU_LZ_FAST does not serve a max_insert_length above 7 (deflateTune)";
    if (cfg.good <= 2) return "ZGPU_LZ_FAST does not serve a good_length below 3 (deflateTune): every search of deflate_fast is quartered";
    return nullptr;
}

// What is refused before anything is asked of the device (a BGZF call's segment table is measured there, behind these)
inline DeflatePlan plan_deflate_args(const PlanCall &c, const PlanEngine &eng)
{
    constexpr uint32_t kWrappers = ZGPU_F_ZLIB_WRAP | ZGPU_F_GZIP_WRAP;
    if (!c.args) return plan_refused("null argument");
    if (c.level < 1 || c.level > 9) return plan_refused("level must be 1..9");
    if (c.chunk_size > kChunkMax) return plan_refused("chunk_size must be 1..65536");
    if ((c.flags & kWrappers) && !(c.flags & ZGPU_F_FINAL)) return plan_refused("a wrapper needs FINAL");
    if ((c.flags & ZGPU_F_ZLIB_WRAP) && (c.flags & ZGPU_F_GZIP_WRAP)) return plan_refused("one wrapper at a time");
    if (c.prime && ((c.prime >> 16) > 16 || (c.flags & kWrappers))) return plan_refused("prime: at most 16 bits, no wrapper");
    const bool bgzf = c.flags & ZGPU_F_BGZF_WRAP;
    if (bgzf && (!c.seg || !(c.flags & ZGPU_F_FINAL) || (c.flags & (kWrappers | ZGPU_F_CONTINUOUS)) || c.prime || c.skip0))
        return plan_refused("BGZF blocks: segment calls only, with FINAL and no other wrapper");
    if (bgzf && (eng.geo_w != 15 || eng.geo_m != 8)) return plan_refused("BGZF blocks need the default geometry (windowBits 15, memLevel 8)");
    return DeflatePlan{};
}

// ZGPU_LZ_AUTO: the implementation of the call, and whether the lane-per-chunk loop hands the chunks that do not compress on to the wave-per-chunk kernel
inline int plan_auto_impl(const PlanCall &c, const PlanEngine &eng, const DeflateKnobs &kn, const LevelCfg &cfg, bool walk_ok, bool *hand_on)
{
    const int auto_env = kn.lz_default; // ZGPU_LZ_DEFAULT=3: A/B runs of the all-position search
    int impl = (cfg.slow && eng.lz_parallel) ? ((walk_ok && auto_env != ZGPU_LZ_SORTED) ? ZGPU_LZ_WALK : ZGPU_LZ_SORTED) : ZGPU_LZ_SERIAL;
    // levels 1-3: the head[]/prev[] loop.  deflate_fast on the sorted buckets (ZGPU_LZ_FAST, fast_kernel in zgpu_lz_fast.hip) is a second
    // implementation for the parity tests and for ZGPU_LZ_DEFAULT=5: it asks memory four times less often and is no faster
    if (!cfg.slow && eng.lz_parallel && walk_ok && !c.skip0 && auto_env == ZGPU_LZ_FAST) impl = ZGPU_LZ_FAST;
    // levels 1-3: a wave per chunk, window and chain bits in LDS (zgpu_lz_fastwin.hip) -- 5 ms a chunk whatever the size of the call, three chunks per
    // CU; the lane-per-chunk loop takes 28 ms a chunk and needs tens of thousands of them in flight.  Measured crossovers against the loop with its
    // hand-on (chunks per launch, 4 GiB = 65536; profiles/r03_crossover_levels_1_3.txt): levels 1 and 2 about 16000 -- a host batch --, level 3 (32
    // candidates a lane) about 3000.  ZGPU_LZ_DEFAULT=1 keeps the loop, =6 the waves.
    if (!cfg.slow && eng.lz_parallel && walk_ok && !c.skip0 && eng.fastwin_serves && auto_env != ZGPU_LZ_FAST && auto_env != ZGPU_LZ_SERIAL) {
        const uint64_t cs0 = c.chunk_size ? c.chunk_size : kChunkMax;
        uint64_t nch0 = c.seg ? c.nseg : (c.in_bytes + cs0 - 1) / cs0;
        { // what counts is the chunks of ONE launch: host input goes batch by batch (see plan_deflate), and every batch of the loop would pay its latency again
            const uint64_t per_launch = c.host_in ? (kn.host_batch ? kn.host_batch : 65536) : (kn.batch_chunks ? kn.batch_chunks : 65536); // (levels 1-3: see host_batch in plan_deflate)
            if (nch0 > per_launch) nch0 = per_launch;
        }
        // (round 4: without the ring in LDS eleven chunks share a CU and the waves' form scales with the launch -- level 1: 1 GiB 58.6 ms against the loop's 150.9, 3 GiB 164 against 225,
        // 4 GiB 217.6 against 213 with the hand-on; level 2: 2 GiB 160 against 208, 3 GiB 237 against 240; level 3: 256 MiB 110 against 149, 1 GiB 328 against 299)
        const uint64_t upto = cfg.chain == 4 ? 61440 : cfg.chain == 8 ? 45056 : 10240;
        // ZGPU_HAND_ON=0: the loop keeps every chunk (A/B runs); 2: the loop + hand-on whatever the size of the call (tests)
        if (kn.hand_on == '2' && auto_env == 0) *hand_on = true;
        else if (nch0 <= upto || auto_env == ZGPU_LZ_FASTWIN) impl = ZGPU_LZ_FASTWIN;
        else *hand_on = kn.hand_on != '0';
    }
    return impl;
}

// Chunks of a full batch.  One batch = one launch of every stage.  The lane-per-chunk stages (serial LZ77, parse) need tens of thousands of
// chunks in flight to fill 256 CUs, so batches are as large as device memory allows (~1 MiB of workspace per chunk).
inline uint32_t plan_batch(const PlanCall &c, const PlanEngine &eng, const DeflateKnobs &kn, const DeflatePlan &pl)
{
    uint32_t batch_max = kn.batch_chunks ? kn.batch_chunks : 65536; // (small values are for tests: several launches per call)
    // host input: the copy of batch k+1 runs under the kernels of batch k.  Batches must stay large: the block-construction and sort kernels are
    // latency-bound and need every workgroup slot of the chip filled several times over (2048 chunks per launch: 2.2x the time per byte of
    // 65536, rocprofv3 timeline of scripts/host_trace.py); the copy moves 57 GB/s and is over long before the kernels are
    // (levels 1-3: both of their kernels want the launch as large as it gets -- the loop's time hardly grows with the chunks, 170 ms for 32768 and 245 for
    // 65536 at level 1 -- and take far longer than the copy they would hide, so host input is not cut up there)
    const uint32_t host_batch = kn.host_batch ? kn.host_batch : (pl.cfg.slow ? 16384 : 65536); // (A/B runs; measured at 4 GiB, level 6: 8192 184.8 ms, 16384 176.3, 32768 178.5)
    if (c.host_in && batch_max > host_batch) batch_max = host_batch;
    if (eng.free_bytes) {
        const uint64_t per_chunk = (uint64_t)kChunkMax * 4 + kSlotStride +
                                   (pl.geo ? (uint64_t)kGeoSlotStride + (uint64_t)kGeoTableEntries * sizeof(uint4)
                                           : pl.serial ? (uint64_t)kSerialTableEntries * sizeof(uint4) + (pl.hand_on ? eng.sorted_ws_chunk / 4 : 0) : eng.sorted_ws_chunk);
        const uint64_t held = (uint64_t)eng.batch_cap * per_chunk; // what this engine already owns can be reused
        const uint64_t budget = (eng.free_bytes + held) / 10 * 6;
        uint64_t fit = budget / per_chunk; // chunks that fit; never below 256, whatever the device reports
        if (fit < 256) fit = 256;
        if (fit < batch_max) batch_max = (uint32_t)fit;
    }
    return (uint32_t)(pl.nchunks < batch_max ? pl.nchunks : batch_max);
}

// The plan of a chunk or segment call (deflate_device), or its refusal
inline DeflatePlan plan_deflate(const PlanCall &c, const PlanEngine &eng, const DeflateKnobs &kn)
{
    constexpr uint32_t kWrappers = ZGPU_F_ZLIB_WRAP | ZGPU_F_GZIP_WRAP;
    DeflatePlan pl = plan_deflate_args(c, eng);
    if (pl.rc) return pl;
    pl.chunk_size = c.chunk_size ? c.chunk_size : kChunkMax;
    pl.bgzf = c.flags & ZGPU_F_BGZF_WRAP;
    if (c.strategy < 0 || c.strategy > (int)kFixed) return plan_refused("strategy must be 0..4");
    LevelCfg &cfg = pl.cfg;
    cfg = level_cfg_tuned(c.level, c.strategy, eng.tuned, eng.tune);
    // the chain budget of the all-position search says it all for two strategies (deflate.c:1594-1599): no candidate at all,
    // or the nearest one only (and then only at distance 1, see match3_kernel)
    if (cfg.slow && cfg.strategy == kHuffmanOnly) cfg.chain = 0;
    if (cfg.slow && cfg.strategy == kRle) cfg.chain = 1;
    // deflateInit2's geometry (zgpu_deflate_set_geometry): anything but windowBits 15 / memLevel 8 goes to the lane-per-chunk loop, the one
    // implementation whose window size, hash width and block length are run-time values
    pl.geo = eng.geo_w != 15 || eng.geo_m != 8;
    if (pl.geo) { cfg.w_bits = (uint32_t)eng.geo_w; cfg.hash_bits = (uint32_t)eng.geo_m + 7; }
    const uint32_t max_dist = (pl.geo ? 1u << eng.geo_w : kWSize) - kMinLookahead;
    int impl = c.lz_impl;
    if (pl.geo && impl != ZGPU_LZ_AUTO && impl != ZGPU_LZ_SERIAL) return plan_refused("a non-default windowBits / memLevel is served by ZGPU_LZ_SERIAL only");
    // the parse-driven search plays deflate_slow's own game; the two strategies that are chain budgets of the all-position search
    // (Z_HUFFMAN_ONLY, Z_RLE) stay with that search
    const bool walk_ok = cfg.strategy != kHuffmanOnly && cfg.strategy != kRle;
    // levels 1-3 above the crossover: the lane-per-chunk loop hands the chunks that do not compress on to the wave-per-chunk kernel (lz_serial_chunk)
    bool hand_on = false;
    if (impl == ZGPU_LZ_AUTO) {
        impl = plan_auto_impl(c, eng, kn, cfg, walk_ok, &hand_on);
        // (ZGPU_LZ_DEFAULT=3 / =5 on a row that implementation does not serve: the default path refuses nothing)
        if (impl == ZGPU_LZ_SORTED && walk_ok && records_refuse(cfg, impl)) impl = ZGPU_LZ_WALK;
        if (impl == ZGPU_LZ_FAST && fast_refuse(cfg)) impl = ZGPU_LZ_SERIAL;
    }
    if ((impl == ZGPU_LZ_PARALLEL || impl == ZGPU_LZ_SORTED || impl == ZGPU_LZ_WALK) && (!cfg.slow || !eng.lz_parallel)) return plan_refused("parallel LZ77 serves levels 4..9 only");
    if (impl == ZGPU_LZ_FAST && (cfg.slow || !walk_ok || c.skip0 || !eng.lz_parallel)) return plan_refused("ZGPU_LZ_FAST serves levels 1..3, not Z_HUFFMAN_ONLY / Z_RLE, no dictionary chunk");
    if (impl == ZGPU_LZ_FASTWIN && (cfg.slow || !walk_ok || c.skip0 || !eng.lz_parallel || !eng.fastwin_serves))
        return plan_refused("ZGPU_LZ_FASTWIN serves levels 1..3 with their own parameters, not Z_HUFFMAN_ONLY / Z_RLE, no dictionary chunk");
    if ((impl == ZGPU_LZ_PARALLEL || impl == ZGPU_LZ_SORTED) && records_refuse(cfg, impl)) return plan_refused(records_refuse(cfg, impl));
    if (impl == ZGPU_LZ_FAST && fast_refuse(cfg)) return plan_refused(fast_refuse(cfg));
    if (impl < ZGPU_LZ_SERIAL || impl > ZGPU_LZ_FASTWIN) return plan_refused("unknown lz_impl");
    if (impl == ZGPU_LZ_PARALLEL && c.strategy != 0) return plan_refused("ZGPU_LZ_PARALLEL serves the default strategy only");
    if (impl == ZGPU_LZ_WALK && !walk_ok) return plan_refused("ZGPU_LZ_WALK does not serve Z_HUFFMAN_ONLY / Z_RLE");
    if (c.skip0) { // a preset dictionary in front of the one chunk: the lane-per-chunk loop is the implementation that starts mid-window
        if (c.seg || c.in_bytes > kChunkMax || c.skip0 < kMinMatch || c.skip0 > max_dist || c.skip0 > c.in_bytes || (c.flags & (kWrappers | ZGPU_F_POS0 | ZGPU_F_POS0_ALL)))
            return plan_refused("dictionary chunk: 3..32506 dictionary bytes + data <= 65536, no wrapper");
        impl = ZGPU_LZ_SERIAL;
    }
    if (pl.geo) impl = ZGPU_LZ_SERIAL;
    pl.impl = impl;
    pl.serial = impl == ZGPU_LZ_SERIAL;
    pl.hand_on = hand_on && pl.serial && !pl.geo && c.lz_impl == ZGPU_LZ_AUTO;
    if (c.seg && (c.nseg == 0 || ((c.flags & kWrappers) && (!(c.flags & ZGPU_F_FINAL) || ((c.flags & ZGPU_F_ZLIB_WRAP) && (c.flags & ZGPU_F_GZIP_WRAP))))))
        return plan_refused("segment mode: nseg >= 1, a wrapper needs FINAL (one of zlib / gzip)");
    pl.nchunks = c.seg ? c.nseg : (c.in_bytes ? (c.in_bytes + pl.chunk_size - 1) / pl.chunk_size : 1);
    pl.batch = plan_batch(c, eng, kn, pl);
    if (pl.hand_on) pl.hand_piece = pl.batch / 4 < 4096 ? (pl.batch < 4096 ? pl.batch : 4096) : pl.batch / 4; // the sorted buckets' workspace: for a quarter of the batch at a time
    pl.wrap = c.flags & ZGPU_F_ZLIB_WRAP; pl.gz = (c.flags & ZGPU_F_GZIP_WRAP) || pl.bgzf; // (a BGZF block is a gzip member)
    pl.with_crc = pl.gz || (c.flags & ZGPU_F_CRC32);
    // segments with a wrapper: every segment is a stream of its own, framed by launch_frame; the call itself has no header or trailer
    pl.seg_wrap = c.seg && (pl.wrap || pl.gz);
    pl.head_bytes = pl.seg_wrap ? 0 : pl.wrap ? 2 : pl.gz ? 10 : 0; pl.tail_bytes = pl.seg_wrap ? 0 : pl.wrap ? 4 : pl.gz ? 8 : 0;
    pl.block_tokens = pl.geo ? (1u << (eng.geo_m + 6)) - 1u : kBlockTokens;
    pl.check_sort = (impl == ZGPU_LZ_SORTED || impl == ZGPU_LZ_WALK || impl == ZGPU_LZ_FAST || impl == ZGPU_LZ_FASTWIN || pl.hand_on) && !eng.exact_sort;
    // host input, several batches: nothing runs under the first one's copy, so it is short (2048 chunks) and the next ones double up to the full
    // batch -- a copy moves a chunk 2.3 times as fast as the kernels compress one, so each batch's copy still ends under the kernels of the batch
    // before it -- and what the short launches cost the latency-bound kernels (see plan_batch) is less than what the shorter wait saves
    // (1 GiB: 58.3 -> 55.5 ms; profiles/r02_host_batches_ab.txt)
    const uint32_t first_env = kn.first_batch ? kn.first_batch : 2048; // (chunks; A/B runs)
    pl.first = (c.host_in && cfg.slow && pl.batch >= 2 * first_env && pl.nchunks > first_env) ? first_env : pl.batch; // (levels 1-3: no ramp either)
    return pl;
}

// The batches of a planned call, one after the other: the first is pl.first chunks, each next one twice the one before until the full batch is reached
struct BatchSteps {
    uint64_t nchunks, c0 = 0; // c0: the batch's first chunk
    uint32_t batch, step;
    size_t k = 0;             // the batch's number
    explicit BatchSteps(const DeflatePlan &pl) : nchunks(pl.nchunks), batch(pl.batch), step(pl.first) {}
    bool more() const { return c0 < nchunks; }
    uint32_t nb() const { return (uint32_t)(nchunks - c0 < step ? nchunks - c0 : step); } // chunks of this batch
    void next() { c0 += step; step = step >= batch / 2 ? batch : step * 2; k++; }
};
inline size_t plan_nbatches(const DeflatePlan &pl)
{
    BatchSteps s(pl);
    while (s.more()) s.next();
    return s.k;
}

// ---- the continuous stream (deflate_cont) ----
struct ContKnobs {
    uint32_t batch_tiles = 0; bool batch_tiles_set = false; // ZGPU_CONT_BATCH_TILES: its value; it is set at all
    int pipe = 0;            // ZGPU_CONT_PIPE
    uint32_t fast_run = 0;   // ZGPU_FAST_RUN
    bool trace = false;      // ZGPU_FAST_TRACE
    bool stats = false;      // ZGPU_FAST_STATS
};

struct ContPlan {
    bool fast_lz = false;    // levels 1-3: the rounds of fastwin_tile_kernel
    uint64_t e0 = 0, w0 = 0, end = 0; // buffer offsets: where the parse stands, where the first tile's 64 KiB start, up to where the feed is parsed
    uint64_t ntiles = 0;
    bool pipe = false;       // two sets of per-batch buffers, the blocks on a second stream
    uint32_t batch = 0;      // tiles of a full batch (at least 1)
    uint32_t batch_fit = ~0u; // what the device's memory admits
};

// The special position of a segment that ends at stream position n: the position 32768 k + 65274 in [n - 261, n], ~0 if there is none.  Less than
// MIN_LOOKAHEAD is left there, so the reference slides its window one loop top early (zgpu_cont.hip, cont_slides) and the position's first candidate,
// exactly MAX_DIST back, is NIL.  Every user of the position calls this one function
__host__ __device__ inline uint64_t cont_special(uint64_t n)
{
    if (n < 65274u) return ~0ull;
    const uint64_t sp = (n - 65274u) / 32768u * 32768u + 65274u;
    return sp + 261u >= n ? sp : ~0ull;
}

// levels 1-3 with Z_HUFFMAN_ONLY: no match is ever looked for, no chain ever asked: the walkers' path (every byte a literal) serves it
inline bool cont_fast_lz(const LevelCfg &cfg) { return !cfg.slow && cfg.strategy != kHuffmanOnly; }

// One feed: cs->entry, cs->abs0 and the feed's buffer length and mode (the state has been checked: abs0 <= entry <= abs0 + buf_bytes)
inline ContPlan plan_cont(const LevelCfg &cfg, uint64_t entry, uint64_t abs0, uint64_t buf_bytes, int mode, const PlanEngine &eng, const ContKnobs &kn)
{
    ContPlan pl;
    pl.fast_lz = cont_fast_lz(cfg);
    pl.e0 = entry - abs0; pl.w0 = pl.e0 > kTileStride ? pl.e0 - kTileStride : 0;
    const uint64_t e0 = pl.e0, w0 = pl.w0;
    pl.end = mode != ZGPU_CONT_MORE ? buf_bytes : (buf_bytes > kTileSlack ? buf_bytes - kTileSlack : 0);
    const uint64_t end = pl.end;
    pl.ntiles = end > e0 ? (end <= w0 + kTileH1 ? 1 : (end - w0 - kTileH1 + kTileStride - 1) / kTileStride + 1) : 0;
    const uint64_t ntiles = pl.ntiles;
    uint32_t batch_max = kn.batch_tiles ? kn.batch_tiles : (pl.fast_lz ? 65536 : 32768); // (levels 1-3: every batch ends with a tail of rounds that are one tile's latency each, 4 GiB 1395 -> 1149 ms with twice the batch)
    if (eng.free_bytes) {
        const uint64_t per_tile = eng.sorted_ws_chunk + (uint64_t)kChunkMax * 4 + (uint64_t)(kTileStride + kTileSlack) * 4 + 3 * (uint64_t)kSlotStride + kSlotStride;
        // what this engine holds already and would use again, piece by piece (the chunked path's buffers serve the tiles too): counted as free, or the batch would
        // grow from call to call as more of the same memory is held -- and a later call of a series would stop to allocate (seen in bench.py: 44 035, 64 837, 66 052 tiles)
        const uint64_t held = (uint64_t)eng.batch_cap * ((uint64_t)kChunkMax * 4 + kSlotStride) + (uint64_t)eng.par_cap * eng.sorted_ws_chunk + (uint64_t)eng.ct_tiles * ((uint64_t)(kTileStride + kTileSlack) * 4 + 3 * (uint64_t)kSlotStride);
        uint64_t fit = (eng.free_bytes + held) / 10 * 6 / per_tile;
        if (fit < 64) fit = 64;
        if (fit < batch_max) batch_max = (uint32_t)fit;
        pl.batch_fit = fit < 0xffffffffull ? (uint32_t)fit : ~0u;
    }
    // levels 1-3: no short batch at the end -- its tail of rounds is as long as a full batch's (2 GiB are 66 052 tiles: one batch, not 65 536 + 516; 4 GiB two of 66 052, not
    // two and 1 032 tiles that take 70 ms).  A remainder below an eighth of a batch is spread over the others if memory admits it, and the batches are of one size.
    if (pl.fast_lz && ntiles > batch_max && !kn.batch_tiles_set) {
        uint64_t nbat = (ntiles + batch_max - 1) / batch_max;
        const uint64_t rem = ntiles % batch_max;
        if (rem && rem < batch_max / 8) nbat--;
        const uint64_t even = (ntiles + nbat - 1) / nbat;
        if (even <= pl.batch_fit) batch_max = (uint32_t)even;
    }
    // levels 4-9, more than one batch: two sets of per-batch buffers, half a batch each -- batch k's tokens, blocks and bits are made on a second stream
    // while batch k + 1 is sorted and walked on the first (ZGPU_CONT_PIPE=0: one after the other, for A/B runs)
    // ZGPU_CONT_PIPE: 1: feeds of 2048 tiles and more, 2: whatever the size of the feed (tests).  Off by default: measured at 4 GiB, level 6, 242 ms against 238 --
    // two walker workgroups fill a CU's LDS, so the other stream's kernels run beside the sort only, and both are bound by the same memory system
    pl.pipe = !pl.fast_lz && (kn.pipe == 2 ? ntiles >= 2 : kn.pipe == 1 && ntiles >= 2048);
    if (pl.pipe) { // at least four batches, so that all but the first one's walkers and the last one's blocks have something running beside them
        const uint64_t want = (ntiles + 3) / 4;
        if (batch_max >= 2048) batch_max /= 2;
        if (want >= 1024 && want < batch_max) batch_max = (uint32_t)want;
    }
    pl.batch = (uint32_t)(ntiles < batch_max ? (ntiles ? ntiles : 1) : batch_max);
    return pl;
}

// levels 1-3 (lz_tiles_fast): round 0 of a batch of nb tiles in K phases (fast_run: ZGPU_FAST_RUN=K; 1: all tiles at once, as until round 4).  A tile that starts from nothing
// (a warm-up over its history) knows little about which of the positions in front of it are in the chains, and most tiles were parsed again four or five times before their
// neighbours' guesses had settled.  So only every K-th tile guesses; the K - 1 behind it are parsed one phase after the other, each from where the tile in front ended and
// with that tile's bits -- by the third or fourth of a run those are the stream's.  (1 + 1 / K) parses per tile instead of 2, and the rounds that follow start from a far
// better state; the price is K launches with 1 / K of the tiles each, so K grows with the batch.
inline uint32_t plan_fast_phases(uint32_t nb, uint32_t fast_run)
{
    uint32_t K = fast_run;
    if (K == 0) {
        K = nb / 256; if (K < 1) K = 1; if (K > 16) K = 16; // (measured: 64 MiB 146 -> 108 ms with 8, 256 MiB 309 -> 170 with 16, 1 GiB 2029 -> 427; no gain below 16 MiB, where every launch is one tile's latency)
        // ... and no phase larger than the chip holds at once: eleven one-wave workgroups of 13.3 KiB LDS a CU are 2 816 tiles, a phase of 4 128 (a batch of 66 052 in 16) runs as two
        // waves of workgroups, the second a third full -- 4 GiB at level 1: 16 phases 672 ms, 22 (3 003 tiles each) 673, 24 (2 752) 577, 32 654, 44 711
        // (the bound is the 2 816 the chip holds, so that a batch of 66 052 runs in the 24 phases measured best: 2 752 a phase made it 25, four tiles over 24 * 2 752)
        const uint32_t kw = (nb + 2815) / 2816;
        if (kw > K) K = kw;
    }
    if (K > 64) K = 64;
    return K;
}

} // namespace zgpu
