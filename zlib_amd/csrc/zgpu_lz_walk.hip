// zgpu_lz_walk.hip -- K2w walk_kernel, the parse-driven search of the sorted-bucket LZ77 stage: the default at levels 4-9, for chunks (with the rest
// of the parse behind it) and for the tiles of a continuous stream (zgpu_lz_sorted.hip has the map).
#include "zgpu_lz_sorted.h"
#define ZGPU_PARSE_HEADER_ONLY
#include "zgpu_lz_parse.h"
#include <cstdlib>

namespace zgpu {

// ------------------------------------------------------------------------------------------------- K2w
// Parse-driven search (levels 4-9; replaces match3_kernel + the game stage of parse2_kernel).  match3 searches every
// position with the full chain budget because the parse that decides which searches matter runs after it; deflate_slow
// itself (deflate.c:1554-1674) calls longest_match at a quarter of the positions, often with a quarter of the budget, and
// walks a sixth of the candidates (tests/tools/walk_model.c).  Here the parse drives the search:
//
//   * The chunk is cut into blocks of 64 positions; a WALKER (one lane) takes a block and runs the reference's loop from the
//     block's first position in the neutral state (nothing in hand, prev_length = MIN_MATCH-1), calling for searches as the
//     loop does: at a neutral position with the full budget, at the position behind a match shorter than max_lazy with the
//     match as the seed (and a quarter of the budget from good_match on).
//   * Whatever happens from a neutral position depends on that position alone, so a walker that arrives, neutral, at a
//     position another walker has been at in the same state stops there (one bit per position in LDS, claimed with an atomic
//     OR): every neutral position is worked on once, and parses started 64 positions apart fall into step after a match or
//     two (0.8 neutral positions on average, tests/tools/walk_model.c).  The walkers' paths form a forest in which the path
//     from position 0 -- the reference's parse -- is complete.  A walker whose path has merged takes the next block.
//   * A lane searches like a lane of match3 (same step: two-byte quick check at the best length, candidates that pass are
//     parked on the wave's stack, 64 parked candidates are compared at full occupancy and folded into their owners' keys),
//     but the lanes of a wave are at different points of different searches.  They advance in bodies of four candidates; a
//     lane whose search is over waits until the wave's next PASS (when 16 lanes wait, or none is searching), which plays
//     the parse for all of them, claims positions, hands out blocks and starts the next searches.  Everything a start needs
//     from memory (index and rank of the position: one dword of `ir`) is fetched at least one pass ahead, for the position
//     behind the current one and for the position behind the match in hand.
//   * Output: for every neutral position r that a game started from, gm[r] = (m - r) << 24 | len << 15 | dist of the match the
//     game ends with, and bit r of the chunk's bitmap gs: what parse2_kernel's stage A1 derives from match3's records,
//     restricted to the positions some walker stood on (which include the whole path).  The lite form of the parse (zgpu_lz_parse_body.inc)
//     does the rest: behind the walkers in the same workgroup (chunks), or as parse2_kernel<true, true> once the tiles' entries are known.
//     A chunk's walkers (MODE 1) do not write gm / gs: a finished game is appended to the log of its window of kP2Win positions (lrec, lpos; slots
//     from a counter in LDS), which is what the fused parse reads -- dense, and only the games (zgpu_lz_parse.h, LOG).  A store into gm dirtied
//     a partial line somewhere in 256 KiB, and the parse read all of gm back, a window at a time, to throw three words in four away.
#ifndef ZGPU_WTRIG
#define ZGPU_WTRIG 48 // lanes waiting for a pass that make the wave run one
#endif
#ifndef ZGPU_WBLK
#define ZGPU_WBLK 64 // positions per block
#endif
// The end of a chunk (MODE 1): blocks go out in position order, so when the counter runs out every walker is somewhere inside one of the last blocks
// and the lanes fall idle one by one for up to a block's time.  The last ZGPU_WTAPER32 positions of a chunk are therefore handed out in blocks of 32
// and the last ZGPU_WTAPER16 in blocks of 16: what is in flight at the end is short, and a lane that finishes late finds a short block to take.
// (Set both to 0 for uniform blocks.  A chunk with no more blocks than walkers keeps uniform blocks: there is nothing to balance.)
#ifndef ZGPU_WTAPER32
#define ZGPU_WTAPER32 16384
#endif
#ifndef ZGPU_WTAPER16
#define ZGPU_WTAPER16 4096
#endif
#ifndef ZGPU_WNEU_SHIFT
#define ZGPU_WNEU_SHIFT 0 // walkers meet at positions that are multiples of 1 << this (fewer bits in LDS, a little more duplicate work)
#endif
#ifndef ZGPU_WFOLD_AT
#define ZGPU_WFOLD_AT 64 // parked candidates that make a wave compare them (at most 64 more arrive with one step: the stack holds 128)
#endif
constexpr uint32_t kWFoldAt = ZGPU_WFOLD_AT;
constexpr uint32_t kWThreads = 512, kWWaves = kWThreads / 64, kWBlk = ZGPU_WBLK, kWTrig = ZGPU_WTRIG, kWNeuShift = ZGPU_WNEU_SHIFT;
constexpr uint32_t kWNeuBytes = (kChunkMax >> kWNeuShift) / 8;
constexpr uint32_t kWTaper32 = ZGPU_WTAPER32, kWTaper16 = ZGPU_WTAPER16, kWTaperMin = kWThreads * kWBlk; // (chunks of at most kWTaperMin positions: uniform blocks)
static_assert(kWTaper16 <= kWTaper32 && kWTaper32 <= kWTaperMin && kWTaper32 % 64 == 0 && kWTaper16 % 64 == 0, "the tapered end lies inside a chunk that has one");
static_assert((kWTaper32 == 0 && kWTaper16 == 0) || kWBlk == 64, "blocks of 32 and 16 follow blocks of 64");
static_assert(kWTaper32 == 0 || kWNeuShift <= (kWTaper16 ? 4 : 5), "a short block's start must be a meeting position of its own, or the walker in front passes through it and the block is never taken");
// the block map of a chunk of n positions: blocks of kWBlk below b32, of 32 in [b32, b16), of 16 from b16 on (b32 a multiple of 64, b16 of 32)
struct WalkTaper {
    uint32_t b32, b16, n64, n32, nblk;
    // (forced inline: taken in late, the object stayed on the stack -- 32 bytes of scratch that nothing reads -- once the kernel had grown by the whole-chunk tail)
    __host__ __device__ __forceinline__ explicit WalkTaper(uint32_t n)
    {
        const bool on = n > kWTaperMin && kWTaper32 != 0;
        b32 = on ? (n - kWTaper32) & ~63u : n;
        b16 = on ? (n - kWTaper16) & ~31u : n;
        n64 = on ? b32 / 64 : (n + kWBlk - 1) / kWBlk; n32 = (b16 - b32) / 32;
        nblk = n64 + n32 + (n - b16 + 15) / 16;
    }
    __host__ __device__ __forceinline__ uint32_t start(uint32_t b) const { return b < n64 ? b * kWBlk : b < n64 + n32 ? b32 + (b - n64) * 32 : b16 + (b - n64 - n32) * 16; }
};
extern "C" __attribute__((visibility("default"))) void zgpu_walk_block_map(uint32_t n, uint32_t *out) // (tests: where a chunk's walkers start) b32, b16, blocks
{
    const WalkTaper t(n);
    out[0] = t.b32; out[1] = t.b16; out[2] = t.nblk;
}
constexpr uint32_t kWOffLcnt = kM3DataLds + 16 + kWNeuBytes + kWWaves * kM3WaveLds; // entries in each window's log (a chunk's walkers; they outlive them)
constexpr uint32_t kWLds = kWOffLcnt + kP2Wins * 4;
static_assert(2 * kWLds <= 160 * 1024, "two walker workgroups per CU");
enum : uint32_t { W_NEED = 0, W_LIMBO = 1, W_READY = 2, W_SEARCH = 3, W_DONE = 4 };
#ifdef ZGPU_WALK_STATS // debug build only: 0 bodies, 1 active lane-steps, 2 passes, 3 lanes served by passes, 4 searches, 5 folds, 6 parked, 7 limbo starts;
                       // the end of a chunk (scripts/walk_stats.py): 8 / 9 live lanes (not W_DONE) summed over the passes before / after the wave has seen the
                       // block counter run out, 10 / 11 the passes in each
__device__ unsigned long long walk_stats[12];
extern "C" __attribute__((visibility("default"))) void zgpu_debug_walk_stats(unsigned long long *out, int reset)
{
    unsigned long long z[12] = {};
    hipMemcpyFromSymbol(out, HIP_SYMBOL(walk_stats), sizeof z);
    if (reset) hipMemcpyToSymbol(HIP_SYMBOL(walk_stats), z, sizeof z);
}
#define W_STAT(i, v) do { const unsigned long long v_ = (unsigned long long)(v); if (lane == 0) atomicAdd(&walk_stats[i], v_); } while (0)
#define W_SOUT0() bool ws_out = false
#define W_SLIVE() do { W_STAT(ws_out ? 9 : 8, __popcll(__builtin_amdgcn_ballot_w64(st != W_DONE))); W_STAT(ws_out ? 11 : 10, 1); } while (0)
#define W_SOUT() do { ws_out = ws_out || __builtin_amdgcn_ballot_w64(st == W_DONE) != 0; } while (0) // (W_DONE comes from an empty counter alone)
__device__ unsigned long long walk_log_stats[6]; // walk_kernel<1> (scripts/walk_log_stats.py): 0 games logged, 1 the fullest log of a window; chunks by the tail they
                                                 // took: 2 the whole-chunk form, 3 the windowed one for their games (more than the capacity), 4 the windowed one behind
                                                 // a whole-chunk threading that did not hold; 5 chunks of the whole-chunk form whose game starts were fewer
                                                 // than their log entries (two games logged at one position: must stay 0, zgpu_lz_tail.h stage 2)
extern "C" __attribute__((visibility("default"))) void zgpu_debug_walk_log_stats(unsigned long long *out, int reset)
{
    unsigned long long z[6] = {};
    hipMemcpyFromSymbol(out, HIP_SYMBOL(walk_log_stats), sizeof z);
    if (reset) hipMemcpyToSymbol(HIP_SYMBOL(walk_log_stats), z, sizeof z);
}
#else
#define W_STAT(i, v) do { } while (0)
#define W_SOUT0() do { } while (0)
#define W_SLIVE() do { } while (0)
#define W_SOUT() do { } while (0)
#endif
#ifdef ZGPU_WALK_TIME // debug build only (scripts/walk_time.py): clock cycles of a wave in 0 passes (rest), 1 bodies (without 2), 2 folds inside bodies, 3 setup, 4 drain folds, 5 parse + claims, 6 blocks
                      // and, over those (by when, not by what): 8 from the first pass that finds the block counter run out to the wave's exit from the
                      // walker loop (the ramp-down), 9 from that exit to the release of the barrier in front of the tail
__device__ unsigned long long walk_time[10];
extern "C" __attribute__((visibility("default"))) void zgpu_debug_walk_time(unsigned long long *out, int reset)
{
    unsigned long long z[10] = {};
    hipMemcpyFromSymbol(out, HIP_SYMBOL(walk_time), sizeof z);
    if (reset) hipMemcpyToSymbol(HIP_SYMBOL(walk_time), z, sizeof z);
}
// (summed in registers, written once when the wave is done: an atomic per section would sit in the wave's memory counter and be waited for
// by the next section that needs a load)
#define W_T0() unsigned long long wt_prev = __builtin_readcyclecounter(), wt_fold = 0, wt_lds = 0, wt_take = 0, wt_out = 0, wt_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define W_T(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); wt_acc[i] += t_ - wt_prev - ((i) == 1 ? wt_fold + wt_lds + wt_take : 0); \
                    if ((i) == 1) { wt_acc[2] += wt_fold; wt_acc[3] += wt_lds; wt_acc[7] += wt_take; } wt_fold = wt_lds = wt_take = 0; wt_prev = t_; } while (0)
#define W_TF(stmt) do { const unsigned long long f0_ = __builtin_readcyclecounter(); stmt; wt_fold += __builtin_readcyclecounter() - f0_; } while (0)
#define W_TL(stmt) do { const unsigned long long f0_ = __builtin_readcyclecounter(); stmt; wt_lds += __builtin_readcyclecounter() - f0_; } while (0)   // the body's batch of byte reads (candidates' and scan string's)
#define W_TK(stmt) do { const unsigned long long f0_ = __builtin_readcyclecounter(); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stmt; wt_take += __builtin_readcyclecounter() - f0_; } while (0) // waiting for the groups a pass asked for
#define W_TOUT() do { if (!wt_out && __builtin_amdgcn_ballot_w64(st == W_DONE)) wt_out = wt_prev; } while (0) // (behind W_T(6): the hand-out that came back empty)
#define W_TEXIT() do { wt_acc[8] = wt_prev - wt_out; } while (0)                                                // (behind W_T(0); a wave leaves through an empty hand-out)
#define W_TEND() do { wt_acc[9] = __builtin_readcyclecounter() - wt_prev; if (lane == 0) for (int i_ = 0; i_ < 10; i_++) atomicAdd(&walk_time[i_], wt_acc[i_]); } while (0)
#else
#define W_T0() do { } while (0)
#define W_T(i) do { } while (0)
#define W_TF(stmt) stmt
#define W_TL(stmt) stmt
#define W_TK(stmt) stmt
#define W_TOUT() do { } while (0)
#define W_TEXIT() do { } while (0)
#define W_TEND() do { } while (0)
#endif
#ifdef ZGPU_P2_TIME // debug build only (scripts/p2_time.py fused): the clock of the parse (zgpu_lz_parse.h) for the tail behind a chunk's walkers -- 0 .. 6 its stages,
                    // 7 the workgroup's time in front of it (staging, walkers, barrier), all lane 0's 100 MHz wall clock
__device__ unsigned long long p2_fused_time[8];
extern "C" __attribute__((visibility("default"))) void zgpu_debug_p2_fused_time(unsigned long long *out, int reset)
{
    unsigned long long z[8] = {};
    hipMemcpyFromSymbol(out, HIP_SYMBOL(p2_fused_time), sizeof z);
    if (reset) hipMemcpyToSymbol(HIP_SYMBOL(p2_fused_time), z, sizeof z);
}
#define P2_TIME_ARR p2_fused_time
#endif
// b + the high / low half of w, b | the high half of w: one instruction each (SDWA picks the half), b | (w & m)
__device__ inline uint32_t add_w1(uint32_t b, uint32_t w) { uint32_t r; asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "v"(b), "v"(w)); return r; }
__device__ inline uint32_t add_w0(uint32_t b, uint32_t w) { uint32_t r; asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "v"(b), "v"(w)); return r; }
__device__ inline uint32_t or_w1(uint32_t b, uint32_t w) { uint32_t r; asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "v"(b), "v"(w)); return r; }
__device__ inline uint32_t and_or(uint32_t w, uint32_t m, uint32_t b) { uint32_t r; asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(w), "s"(m), "v"(b)); return r; }
__device__ inline uint32_t sel_mask(unsigned long long m, uint32_t if_set, uint32_t if_clear) { uint32_t r; asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if_clear), "v"(if_set), "s"(m)); return r; }

// TILE (continuous stream): where the parse leaves the tile as a function of where it enters it.  The games the walkers have played (gm, one bit per game
// start in gs) are a forest over the positions [h0, h1): a game started at r ends in the neutral position q = m + len, literals follow up to the next game
// start.  Every possible entry h0 + k is the start of a walker, so the path from it lies in the forest.  Game starts are numbered (prefix counts of gs), the
// successor of each is looked up, and pointer jumping (N[i] = N[N[i]], in place) takes every start to the exit of its path in log2(depth) rounds: no serial
// walk through the tile.  exits[k] = (neutral position the parse entered at h0 + k ends in) - h1, 0 .. 512.  T lanes, LDS from `pl` (the chunk bytes are dead).
template <uint32_t T>
__device__ __forceinline__ void tile_exits(uint8_t *pl, const uint32_t *gm, const uint32_t *gs, uint32_t h0, uint32_t h1, uint32_t nent, uint16_t *exits, uint32_t tid)
{
    constexpr uint32_t kWords = kChunkMax / 32;
    static_assert(kWords % T == 0 && T % 64 == 0 && T <= 1024, "workgroup size");
    uint32_t *HAS = reinterpret_cast<uint32_t *>(pl);
    uint16_t *wcnt = reinterpret_cast<uint16_t *>(pl + kWords * 4);
    uint32_t *wtot = reinterpret_cast<uint32_t *>(pl + kWords * 6);
    uint16_t *N = reinterpret_cast<uint16_t *>(pl + kWords * 6 + 64);
    constexpr uint32_t kCapNodes = (kM3DataLds - (kWords * 6 + 64)) / 2; // game starts the table has room for
    static_assert(kCapNodes < 0x8000u && kCapNodes > kTileH1 / 3, "a path's game starts are three positions apart at least; different paths' need not be");
    const uint32_t lane = tid & 63, wave = tid >> 6;
    constexpr uint32_t per = kWords / T;
    uint32_t sum = 0, cnt[per];
#pragma unroll
    for (uint32_t i = 0; i < per; i++) {
        const uint32_t w = tid * per + i, v = __hip_atomic_load(gs + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        HAS[w] = v; cnt[i] = (uint32_t)__builtin_popcount(v); sum += cnt[i];
    }
    uint32_t x = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if ((int)lane >= d) x += y; }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    uint32_t b = x - sum;
    for (uint32_t w = 0; w < wave; w++) b += wtot[w];
#pragma unroll
    for (uint32_t i = 0; i < per; i++) { wcnt[tid * per + i] = (uint16_t)b; b += cnt[i]; }
    __syncthreads();
    uint32_t nn = 0;
    for (uint32_t w = 0; w < T / 64; w++) nn += wtot[w]; // game starts of the tile
    auto rank_of = [&](uint32_t p) { return (uint32_t)wcnt[p >> 5] + (uint32_t)__builtin_popcount(HAS[p >> 5] & ~(~0u << (p & 31u))); };
    if (nn > kCapNodes) { // (uniform) walkers that never met -- long runs, short periods: every entry's path is walked by a lane of its own, a global load per game
        for (uint32_t k = tid; k < kTileExitStride; k += T) {
            uint32_t v = 0;
            if (k < nent) {
                const uint32_t e = h0 + k;
                uint32_t p = e < h1 ? next_bit(HAS, e, kWords) : kNone, x = e > h1 ? e : h1;
                while (p != kNone && p < h1) {
                    const uint32_t gv = __hip_atomic_load(gm + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), q = p + (gv >> 24) + ((gv >> 15) & 511u);
                    x = q > h1 ? q : h1;
                    p = q < h1 ? next_bit(HAS, q, kWords) : kNone;
                }
                v = x - h1;
            }
            exits[k] = (uint16_t)v;
        }
        return;
    }
    constexpr uint32_t kExit = 0x8000u; // N[i] = kExit | (exit - h1), or the number of the next game start on the path
    for (uint32_t p0 = h0 & ~31u; p0 < h1; p0 += T * 8) {
        uint32_t gv[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) { const uint32_t p = p0 + u * T + tid; gv[u] = p < h1 ? __hip_atomic_load(gm + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u; } // (all of them: loads under a per-lane condition are waited for one by one)
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) {
            const uint32_t p = p0 + u * T + tid;
            if (p < h1 && ((HAS[p >> 5] >> (p & 31u)) & 1u)) {
                const uint32_t q = p + (gv[u] >> 24) + ((gv[u] >> 15) & 511u);
                uint32_t v = kExit | (q > h1 ? q - h1 : 0u);
                if (q < h1) { const uint32_t t = next_bit(HAS, q, kWords); if (t != kNone && t < h1) v = rank_of(t); }
                N[rank_of(p)] = (uint16_t)v;
            }
        }
    }
    __syncthreads();
    for (;;) {
        bool more = false;
        for (uint32_t i = tid; i < nn; i += T) {
            const uint32_t v = N[i];
            if (!(v & kExit)) { const uint32_t w = N[v]; N[i] = (uint16_t)w; more = more || !(w & kExit); } // (another lane may move N[v] on meanwhile: old or new, both lie further down i's path)
        }
        if (!__syncthreads_or(more)) break;
    }
    for (uint32_t k = tid; k < kTileExitStride; k += T) {
        uint32_t v = 0;
        if (k < nent) {
            const uint32_t e = h0 + k, t = e < h1 ? next_bit(HAS, e, kWords) : kNone;
            v = (t == kNone || t >= h1) ? (e > h1 ? e - h1 : 0u) : ((uint32_t)N[rank_of(t)] & 0x7fffu);
        }
        exits[k] = (uint16_t)v;
    }
}

// FUSE: when its walkers are done the workgroup goes on with the rest of the parse itself (parse_chunk, zgpu_lz_parse.h, in the LDS the
// chunk bytes lived in).  That part is all latency -- a window at a time, one wave threading the path -- and leaves the CU's vector
// units to the other workgroup's walkers, which are bound by exactly those; as a kernel of its own it cost as much as a third of the walk.
// Once the walkers are done the neutral bitmap and the waves' rings and slots are dead as well: the parse's arrays lie over all of the workgroup's LDS
// but the logs' counts -- J .. sh_entry in the first kP2LdsBytes, END behind them.
static_assert(kP2LogLdsBytes <= kWOffLcnt, "the parse works in the memory of the chunk bytes, the neutral bitmap and the rings");
} // namespace zgpu
#include "zgpu_lz_tail.h"
namespace zgpu {
// The tail has two forms.  A chunk whose logs hold at most tail_cap games (a kernel argument, kWTailCap at the most: the room of the table of successors
// by game, zgpu_lz_tail.h) takes the whole-chunk form; a chunk with more -- zeros, short periods, de Bruijn input: 13 to 31 thousand -- takes the windowed
// one, and so does a chunk whose whole-chunk threading did not hold.  The choice is the workgroup's (the counts are in LDS), made before either form has
// written anything; both lie over the same LDS and read the same logs.
constexpr uint32_t kWTailCap = TailLds<kWThreads>::kCap;
static_assert(TailLds<kWThreads>::kBytes <= kWOffLcnt && kWTailCap >= 12288, "the whole-chunk tail works in the same memory; every chunk of the bench corpora at levels 4-9 fits it (profiles/r07_walk_log_summary.txt)");
// MODE 3: MODE 2 with the launch's tiles given row by row (TileRow), each tile a tile of its own stream.
// MODE 1: a chunk, the rest of the parse behind its walkers (FUSE); 2: a TILE of a continuous stream (zgpu_cont.hip) -- walkers start at every possible
// entry of the tile and at every 64th position of its range [h0, h1), stop at h1, and the workgroup ends with the tile's exit as a function of its entry.
template <int MODE>
__global__ void __launch_bounds__(kWThreads, kWThreads / 128) walk_kernel(ChunkGeom g, LevelCfg cfg, const uint16_t *__restrict__ S_all, const uint32_t *__restrict__ ir_all,
                                                            uint32_t *__restrict__ gm_all, uint32_t *__restrict__ gs_all, uint32_t *__restrict__ tokens, ChunkMeta *meta, TileGeom tg, uint32_t tail_cap)
{
    // (gm_all, gs_all: MODE 2 -- the games by position and their bitmaps; MODE 1 -- the logs' records, lrec, and positions, lpos)
    static_assert(MODE == 1 || MODE == 2 || MODE == 3, "a chunk, a tile, a tile of a launch over many streams");
    constexpr bool FUSE = MODE == 1, TILE = MODE >= 2, ROWS = MODE == 3;
    static_assert(!FUSE || kWNeuShift == 0, "a log holds kP2Win games: a position must start one game at most, so every neutral position is claimed");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    if constexpr (ROWS) { if (g.rows[blockIdx.x].n == 0) return; } // a padding row (zgpu_deflate_streams_plan.h, streams_pad_row): a tile that parses nothing
    uint32_t *d32 = lds;
    uint32_t *ctrl = lds + kM3DataLds / 4; // [0]: next block to hand out
    uint32_t *NEU = ctrl + 4;              // bit p: some walker stands, or stood, at p with nothing in hand
    uint32_t *lcnt = lds + kWOffLcnt / 4;  // FUSE: games in the log of each window of kP2Win positions
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t ring = (uint32_t)__builtin_amdgcn_readfirstlane(lds_off(lds) + kM3DataLds + 16 + kWNeuBytes + wave * kM3WaveLds), slot = ring + kRing * 4;
    uint64_t lo; uint32_t n;
    chunk_span<ROWS>(g, c, lo, n);
    const uint8_t *src = g.in + lo;
    const uint16_t *S = S_all + (size_t)c * kSStride + kSPad;
    const uint32_t *ir = ir_all + (size_t)c * kChunkMax;
    uint32_t *gm = gm_all + (size_t)c * kChunkMax, *gs = gs_all + (size_t)c * (kChunkMax / 32);
    uint32_t *lrec = gm; uint16_t *lpos = reinterpret_cast<uint16_t *>(gs_all) + (size_t)c * kChunkMax; // (FUSE)
    uint32_t th0 = 0, th1 = n, tnent = 0, tnent_all = 0, nil_local = ~0u; // TILE: the range the tile parses, its entries, the position whose first candidate at MAX_DIST is NIL
    uint32_t base = chunk_base(g, c);
    if (TILE) {
        uint64_t wb; uint32_t nl;
        tile_span<ROWS>(g, tg, c, wb, nl, th0, th1, tnent);
        tnent_all = tnent;
        if (tnent > th1 - th0) tnent = th1 - th0; // (walkers start inside the range only; an entry at or behind h1 passes the tile by)
        if constexpr (ROWS) { base = g.rows[c].base; nil_local = g.rows[c].nil_local; } // (the tile's own stream's, zgpu_deflate_streams_plan.h)
        else {
        base = (tg.abs0_nil && tg.abs0 + wb == 0) ? 0u : 1u; // only the stream's own position 0 is NIL; a tile's local 0 is out of every parsed position's reach
        if (tg.nil_pos >= wb && tg.nil_pos - wb < kChunkMax) nil_local = (uint32_t)(tg.nil_pos - wb);
        }
    }
    const uint32_t npos = n >= 3 ? n - 2 : 0;
#ifdef ZGPU_P2_TIME
    const unsigned long long p2_t_in = wall_clock64();
#endif
    stage_chunk<kWThreads>(src, n, d32, tid);
    for (uint32_t i = tid; i < kChunkMax / 32; i += kWThreads) { if (i < kWNeuBytes / 4) NEU[i] = 0; if (!FUSE) gs[i] = 0; }
    if (tid < 8) d32[(kChunkMax + 64) / 4 + tid] = 0xffffffffu; // the word the quick check reads where a zero word would look like a hit
    if (tid == 0) ctrl[0] = 0;
    if (FUSE && tid < kP2Wins) lcnt[tid] = 0;
    __syncthreads();
    int slide_at; // visited positions >= slide_at see the slid window (ParseCtx::slide_at, zgpu_lz_parse.hip)
    {
        const int room = (int)(2 * kWSize - base), b0 = (int)n < room ? (int)n : room;
        const int a = b0 - (int)kMinLookahead + 1, b = (int)(kWSize + kMaxDist) - (int)base;
        slide_at = a > b ? a : b;
    }
    // blocks: TILE -- one per entry, then one per 64 positions of the rest of the range; a chunk -- WalkTaper
    const WalkTaper taper(n);
    const uint32_t chainF = cfg.chain, chainQ = cfg.chain >> 2, dbase = lds_off(d32), nblk = TILE ? tnent + (th1 - th0 - tnent + kWBlk - 1) / kWBlk : taper.nblk;
    const uint32_t wlim = TILE ? th1 : n; // a walker that arrives here, neutral, is done with the chunk / the tile
    const bool vexact = (chainF & 7u) != 0 || (chainQ & 7u) != 0 || cfg.strategy == kRle; // a chain may end inside a group of eight with entries of its own bucket behind it (see the bodies)
    // what a parked candidate carries besides its position: the owner's lane (bits 16-21), "first of its chain" (bit 22) and, from bit 23, the length of
    // the match the search started with in hand (at most 258) -- set when a search starts
    uint32_t lanebits = lane << 16;
    const uint32_t dummy = ring + (kRing - 1) * 4;
    // walker
    uint32_t st = W_NEED, x = 0, handL = kMinMatch - 1, handM = 0, handD = 0, gstart = 0;
    uint32_t irx = 0, irn = 0, irE = 0, irl = 0; // idx | rank << 16 of: x, x + 1, the position behind the match in hand, a position asked for in the last pass
    bool haveE = false;
    // search (as in match3_kernel); keys: len >= nice: 1<<31 | q<<9 | len, else len<<16 | q -- nearest candidate first = largest q
    uint32_t rem = 0, best = kMinMatch - 1, key_seen = 0, sentinel = 0, boff = dbase + 1;
    uint32_t sw0 = 0, sw1 = 0; // the eight bytes at x, from the start of a search on (fold)
    // candidates arrive in groups of eight (16 bytes of S).  A lane's loads are scattered over S: nothing is shared between lanes and
    // every group comes from L2 or beyond, a latency of several bodies; streaming the groups one body ahead (as match3 does with
    // its coalesced loads) left every body waiting for memory.  So a pass fetches the first 32 candidates of the searches it
    // starts at once (F0..F3; most chains are no longer), the lanes take them over one body later (G0..G3, consumed by rotation),
    // and a chain that goes on after 32 candidates is refilled by the next pass.
    int gi = -(int)kSPad; // gi: S index of the next group to fetch
    uint32_t firstb = 0; // 1 << 22 while the lane's search has not examined its first candidate (the one the reference allows at MAX_DIST exactly)
    uint4 G0 = make_uint4(0, 0, 0, 0), G1 = G0, G2 = G0, G3 = G0, F0 = G0, F1 = G0, F2 = G0, F3 = G0;
    uint32_t left = 0;  // groups in G0..G3
    bool cont = false;  // out of candidates in registers, chain not finished
    unsigned long long amask = 0, jmask = 0; // lanes walking a chain; lanes that join them when their first group has arrived
    uint32_t tail = 0;

    auto fold = [&]() {
        const uint32_t cnt = tail < 64 ? tail : 64;
        W_STAT(5, 1); W_STAT(6, cnt);
        tail = (uint32_t)__builtin_amdgcn_readfirstlane(tail - cnt);
        // The owner's position and the first eight bytes of its scan string come out of the owner's registers (x, sw0, sw1), by ds_bpermute, in one
        // flight with the candidate's first eight bytes, whose address needs the entry alone: one wait where the owner's position, read back from LDS,
        // and then the two strings took one each.  ds_bpermute returns nothing from a lane that is switched off, and the owners of a fold's entries
        // are any lanes of the wave: so all 64 lanes read an entry (the lanes at and above cnt a stale one of the ring -- some lane, some position of
        // the chunk) and permute, and only the compare and the ds_max stand under lane < cnt.  x, sw0 and sw1 are those of the search the parked
        // candidate belongs to because a pass folds the stack empty before it moves any x.
        const uint32_t e = lds_ld32(ring + ((tail + lane) << 2)); // (tail + lane <= 126: inside the ring)
        const uint32_t q = e & 0xffffu, o = (e >> 16) & 63u, qa = dbase + q;
        uint32_t po, xa, xb;
        {
            uint64_t va; uint32_t va2, ow0, ow1;
            asm volatile("ds_bpermute_b32 %0, %5, %6\n\tds_bpermute_b32 %1, %5, %7\n\tds_bpermute_b32 %2, %5, %8\n\t"
                         "ds_read2_b32 %3, %9 offset1:1\n\tds_read_b32 %4, %9 offset:8\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(po), "=&v"(ow0), "=&v"(ow1), "=&v"(va), "=&v"(va2) : "v"(o << 2), "v"(x), "v"(sw0), "v"(sw1), "v"(qa & ~3u) : "memory");
            xa = __builtin_amdgcn_alignbyte((uint32_t)(va >> 32), (uint32_t)va, qa & 3) ^ ow0;
            xb = __builtin_amdgcn_alignbyte(va2, (uint32_t)(va >> 32), qa & 3) ^ ow1;
        }
        if (lane < cnt) {
            const uint32_t look = n - po, cap = look < kMaxMatch ? look : kMaxMatch, nice = cfg.nice < look ? cfg.nice : look;
            // the candidate must be in reach: the first one of a chain at most MAX_DIST back (deflate.c:1588), the others strictly less
            // (deflate.c:1163), none at the NIL position.  Positions descend along a chain, so refusing them here one by one is the
            // reference's "the chain ends at the first candidate out of reach".
            const bool reach = po - q <= kMaxDist - ((e >> 22) & 1u ? 0u : 1u) && q + base >= 1u;
            uint32_t l = 0;
            while ((xa | xb) == 0 && l + 8 < cap) { // eight more bytes of both strings per round trip
                l += 8;
                lds_cmp8(qa + l, dbase + po + l, xa, xb);
            }
            uint32_t len = xa ? l + ((uint32_t)__builtin_ctz(xa) >> 3) : xb ? l + 4 + ((uint32_t)__builtin_ctz(xb) >> 3) : l + 8;
            len = len < cap ? len : cap;
            // a candidate ends the walk when it is nice AND longer than the match in hand (deflate.c:1126-1160: best_len starts at prev_length, and only a
            // candidate that improves on it is looked at for nice_match).  With max_lazy > nice_length -- deflateTune; no level's row -- a search starts with
            // nice_length bytes or more in hand: a candidate of nice..seed bytes is passed over like any other that does not improve (its plain key stays
            // below the sentinel), and the walk goes on
            if (len >= kMinMatch && reach) lds_max32(slot + o * 4, (len >= nice && len > (e >> 23)) ? (0x80000000u | (q << 9) | len) : ((len << 16) | q));
        }
        const uint32_t key = lds_ld32(slot + lane * 4);
        if (key != key_seen) {
            key_seen = key;
            best = (key >> 31) ? key & 0x1ffu : key >> 16;
            boff = dbase + best - 1; // (the scan string's bytes at the new best length are read by the next body, with its candidates')
        }
        amask &= ~mask_lt_i32((int)key, 0); // nice_match: that walk is over (deflate.c:1224)
    };
    auto gload = [&](int gi) -> uint4 { gi = gi < -(int)kSPad ? -(int)kSPad : gi; return reinterpret_cast<const U128u *>(S + gi)->v; };

    W_T0();
    W_SOUT0();
    W_T(3);
    for (;;) {
        // ================================================= pass: the parse for every lane whose search is over =================================================
        while (tail) fold();
        W_T(4);
        if (cont && (key_seen >> 31)) cont = false; // (the drain found a nice_match: no refill)
        const bool fin = st == W_SEARCH && !(((amask | jmask) >> lane) & 1ull) && !cont;
        W_STAT(2, 1); W_STAT(3, __popcll(__builtin_amdgcn_ballot_w64(fin || st == W_LIMBO || st == W_NEED)));
        W_SLIVE();
        if (st == W_LIMBO) { irx = irl; st = W_READY; } // what the last pass asked for has arrived
        uint32_t y = 0, irY = 0, rec = 0;
        bool toN = false, haveIr = false, emit = false;
        if (fin) {
            uint32_t len = kMinMatch - 1, dist = 0;
            if (key_seen != sentinel) {
                const bool nz = key_seen >> 31;
                len = nz ? key_seen & 0x1ffu : key_seen >> 16;
                dist = x - (nz ? (key_seen >> 9) & 0xffffu : key_seen & 0xffffu);
            }
            if (len <= 5 && (cfg.strategy == kFiltered || (len == kMinMatch && dist > kTooFar))) len = kMinMatch - 1; // deflate.c:1601-1611
            if (len > handL) { // a (longer) match at x: the byte before it, if a match was in hand, becomes a literal (deflate.c:1642-1651)
                if (handL < kMinMatch) gstart = x;
                handL = len; handD = dist; handM = x;
                if (len < cfg.lazy && x + 1 < npos) { x = x + 1; irx = irn; st = W_READY; } // look one position further (deflate.c:1588)
                else emit = true;
                haveE = false; // (the position behind the match in hand has moved)
            } else if (handL >= kMinMatch) emit = true;            // the match in hand stands (deflate.c:1611-1634)
            else { y = x + 1; irY = irn; toN = haveIr = true; }    // a literal
            if (emit) {
                rec = ((handM - gstart) << 24) | (handL << 15) | handD;
                if (!FUSE) {
                    gm[gstart] = rec;
                    atomicOr(&gs[gstart >> 5], 1u << (gstart & 31u));
                }
                y = handM + handL; irY = irE; haveIr = haveE; toN = true;
                handL = kMinMatch - 1;
            }
        }
        // The pass's two LDS atomics -- the slot in the log of the game's window (FUSE) and the meeting bit at y -- depend on registers alone: both are
        // issued from straight-line code by every lane and waited for once.  A lane that has no game to log, or no position to claim, adds 0 to (ORs 0
        // into) its own word of the wave's ring, which the drain has left empty: harmless.  The eight bytes a search that starts in this pass keeps of
        // its scan string (sw0, sw1) ride along: wherever the lane starts one, it is at y if the lane turns neutral here and at x otherwise (a block handed
        // out below is not searched before the next pass).
        const uint32_t yc = y >> kWNeuShift, ybit = 1u << (yc & 31u);
        const bool meet = (y & ((1u << kWNeuShift) - 1u)) == 0; // (elsewhere walkers pass each other unseen: the same work twice, the same result)
        const bool claim = toN && y < wlim && meet;
        const uint32_t own = ring + lane * 4, lw = gstart / kP2Win;
        const uint32_t xs = dbase + (toN ? y : x); // (y <= n: inside the chunk or its zero pad)
        uint32_t lslot = 0, yold, tw2; uint64_t tw;
        if (FUSE) {
            asm volatile("ds_add_rtn_u32 %0, %4, %5\n\tds_or_rtn_b32 %1, %6, %7\n\tds_read2_b32 %2, %8 offset1:1\n\tds_read_b32 %3, %8 offset:8\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(lslot), "=&v"(yold), "=&v"(tw), "=&v"(tw2)
                         : "v"(emit ? lds_off(lcnt) + lw * 4 : own), "v"(emit ? 1u : 0u), "v"(claim ? lds_off(NEU) + (yc >> 5) * 4 : own), "v"(claim ? ybit : 0u), "v"(xs & ~3u) : "memory");
        } else {
            asm volatile("ds_or_rtn_b32 %0, %3, %4\n\tds_read2_b32 %1, %5 offset1:1\n\tds_read_b32 %2, %5 offset:8\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(yold), "=&v"(tw), "=&v"(tw2) : "v"(claim ? lds_off(NEU) + (yc >> 5) * 4 : own), "v"(claim ? ybit : 0u), "v"(xs & ~3u) : "memory");
        }
        const uint32_t tw0 = __builtin_amdgcn_alignbyte((uint32_t)(tw >> 32), (uint32_t)tw, xs & 3), tw1 = __builtin_amdgcn_alignbyte(tw2, (uint32_t)(tw >> 32), xs & 3);
        if (FUSE && emit) { // appended to the log of the game's window: slots go out in time order, so the stores in flight fill a few lines side by side
            const uint32_t at = lw * kP2Win + lslot; // (at most one game per position: the slot is below kP2Win)
            lrec[at] = rec; lpos[at] = (uint16_t)gstart;
        }
        if (toN) { // neutral at y
            st = W_NEED;
            if (y < wlim && (!meet || !(yold & ybit))) { // nobody has been here: go on
                x = y;
                if (haveIr) { irx = irY; st = W_READY; }
                else { irl = y < npos ? ir[y] : 0; st = W_LIMBO; W_STAT(7, 1); }
            }
        }
        W_T(5);
        {   // blocks for the walkers that have none
            const unsigned long long nm = __builtin_amdgcn_ballot_w64(st == W_NEED);
            if (nm) {
                const int first = __builtin_ctzll(nm);
                uint32_t b0 = 0;
                if ((int)lane == first) b0 = atomicAdd(&ctrl[0], (uint32_t)__popcll(nm));
                b0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, first);
                if (st == W_NEED) {
                    const uint32_t b = b0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(nm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nm, 0));
                    if (b >= nblk) st = W_DONE;
                    else {
                        const uint32_t y2 = TILE ? (b < tnent ? th0 + b : th0 + tnent + (b - tnent) * kWBlk) : taper.start(b), bit = 1u << ((y2 >> kWNeuShift) & 31u);
                        if (!(atomicOr(&NEU[(y2 >> kWNeuShift) >> 5], bit) & bit)) { x = y2; handL = kMinMatch - 1; irl = y2 < npos ? ir[y2] : 0; st = W_LIMBO; }
                        // (else: a walker from further down passed through here; the next pass asks for another block)
                    }
                }
            }
        }
        W_T(6);
        W_TOUT(); W_SOUT();
        bool fresh = false;
        if (st == W_READY) { // start the search at x with the match in hand (length handL, 2: none) as the seed
            const uint32_t seed = handL, idx = irx & 0xffffu, rank = irx >> 16, budget = seed >= cfg.good ? (chainQ ? chainQ : 0xffffu) : chainF; // (a quarter of fewer than 4 never runs out, deflate.c:1163)
            uint32_t avail = (x < npos && seed < cfg.lazy) ? (rank < budget ? rank : budget) : 0; // (deflate.c:1588: no search once the match in hand reaches max_lazy)
            irn = x + 1 < npos ? ir[x + 1] : 0;
            if (seed >= kMinMatch) { const uint32_t E = handM + handL; irE = E < npos ? ir[E] : 0; haveE = true; }
            // the one position whose first candidate can sit at window index 32768: NIL after the slide (deflate.c:1309-1312)
            if (TILE) {
                if (x == nil_local && avail != 0 && x - (uint32_t)S[idx - 1] == kMaxDist) avail = 0;
                if (cfg.strategy == kHuffmanOnly) avail = 0;                                                            // deflate.c:1594: no search at all
                if (cfg.strategy == kRle && avail != 0) avail = x - (uint32_t)S[idx - 1] == 1 ? 1u : 0u;                // deflate.c:1596-1599: the nearest candidate, at distance 1 only
            }
            else if (x + base == kWSize + kMaxDist && avail != 0 && (int)x >= slide_at && (uint32_t)S[idx - 1] + base == kWSize) avail = 0;
            best = seed; sentinel = (seed << 16) | 0xffffu; key_seen = sentinel; boff = dbase + best - 1;
            lds_st32(slot + lane * 4, sentinel);
            sw0 = tw0; sw1 = tw1; // the eight bytes at x (read with the pass's atomics)
            lanebits = (lane << 16) | (seed << 23);
            rem = avail; firstb = 1u << 22;
            gi = (int)idx - 8;
            st = W_SEARCH;
            fresh = avail != 0;
            W_STAT(4, 1);
        }
        if (cont) { cont = false; fresh = true; } // refill
        jmask = __builtin_amdgcn_ballot_w64(fresh);
        if (fresh) { // only the lanes that start or refill load, and only the groups the chain has (a scattered 16-byte load is 64 requests to the
                     // address unit whatever the lanes ask for; F0..F3 are read back by these lanes alone)
            F0 = gload(gi);
            if (rem > 8) F1 = gload(gi - 8);
            if (rem > 16) F2 = gload(gi - 16);
            if (rem > 24) F3 = gload(gi - 24);
            gi -= 32;
        }
        W_T(0);
        if (__builtin_amdgcn_ballot_w64(st != W_DONE) == 0) { W_TEXIT(); break; }
        const unsigned long long smask = __builtin_amdgcn_ballot_w64(st == W_SEARCH);
        const uint32_t idle = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(st == W_LIMBO || st == W_NEED));

        // ================================================= bodies of eight candidates until enough lanes wait =================================================
        for (bool first = true;; first = false) {
            const unsigned long long amask0 = amask; // the lanes that examine a group in this body
            if (amask) {
                W_STAT(0, 1);
                // the quick-check bytes of all eight candidates in one round trip, read at the best length the body starts with: a fold
                // inside the body moves best/boff for the next body, the rest of this one goes on with what it read (walking with a
                // stale best length is exact, see match3_kernel).  The scan string's own two bytes at that length (scan0) ride in the same
                // batch, from boff + x: they and the candidates' are read at one best length by construction, and neither a fold nor the
                // start of a search has to fetch them and wait.  A lane that examines nothing reads the zero pad for its candidates and the
                // 0xFF words behind it for its scan bytes, so that a hit is a hit of a real candidate and no step needs the walking mask
                // (whether a candidate is in reach is checked when it is compared in full, fold()).
                // Addresses straight from the halves of G0 (SDWA: no extraction).  Which of the eight are candidates at all is NOT checked here:
                // a lane that examines nothing compares two fixed words that differ; a lane whose chain ends inside the group reads on into
                // the entries below its bucket, whose hashes -- so their first three bytes -- differ from the scan string's: the full comparison
                // (fold) finds fewer than MIN_MATCH bytes and drops them.  Only a chain cut short by the BUDGET goes on into entries of its own
                // bucket that must not be looked at: budgets are multiples of eight (whole groups) except at level 4, in tuned configurations and
                // for Z_RLE -- `vexact`: there a lane examines nv = min(rem, 8) candidates, the hits of the entries past them are masked out, and
                // a lane that examines nothing compares with a value no two bytes can make (ONE uniform branch behind the compares: a branch per
                // candidate, though never taken at levels 5-9, made their bodies a fifth longer: profiles/walk_fold_summary.txt).
                uint32_t bb[8], a[8], boff_e, as;
                boff_e = boff; as = boff + x;
                if (!vexact) { // the lanes that examine nothing read ONE common word (a broadcast): with whatever their registers held they were a third of the kernel's bank conflicts
                    const uint32_t boff_i = dbase + kChunkMax + 8u;
                    G0.x = sel_mask(amask0, G0.x, 0u); G0.y = sel_mask(amask0, G0.y, 0u); G0.z = sel_mask(amask0, G0.z, 0u); G0.w = sel_mask(amask0, G0.w, 0u);
                    boff_e = sel_mask(amask0, boff, boff_i); as = sel_mask(amask0, as, boff_i + 64u);
                }
                a[0] = add_w1(boff_e, G0.w); a[1] = add_w0(boff_e, G0.w); a[2] = add_w1(boff_e, G0.z); a[3] = add_w0(boff_e, G0.z); // nearest candidate = highest address
                a[4] = add_w1(boff_e, G0.y); a[5] = add_w0(boff_e, G0.y); a[6] = add_w1(boff_e, G0.x); a[7] = add_w0(boff_e, G0.x);
                uint32_t hi[8], s0, s1; // (d16 loads would fill both halves of one register, but with SRAM ECC on they clear the other half)
                W_TL(
                    asm volatile("ds_read_u8 %0, %18\n\tds_read_u8 %8, %18 offset:1\n\tds_read_u8 %1, %19\n\tds_read_u8 %9, %19 offset:1\n\t"
                                 "ds_read_u8 %2, %20\n\tds_read_u8 %10, %20 offset:1\n\tds_read_u8 %3, %21\n\tds_read_u8 %11, %21 offset:1\n\t"
                                 "ds_read_u8 %4, %22\n\tds_read_u8 %12, %22 offset:1\n\tds_read_u8 %5, %23\n\tds_read_u8 %13, %23 offset:1\n\t"
                                 "ds_read_u8 %6, %24\n\tds_read_u8 %14, %24 offset:1\n\tds_read_u8 %7, %25\n\tds_read_u8 %15, %25 offset:1\n\t"
                                 "ds_read_u8 %16, %26\n\tds_read_u8 %17, %26 offset:1\n\t"
                                 "s_waitcnt lgkmcnt(0)"
                                 : "=&v"(bb[0]), "=&v"(bb[1]), "=&v"(bb[2]), "=&v"(bb[3]), "=&v"(bb[4]), "=&v"(bb[5]), "=&v"(bb[6]), "=&v"(bb[7]),
                                   "=&v"(hi[0]), "=&v"(hi[1]), "=&v"(hi[2]), "=&v"(hi[3]), "=&v"(hi[4]), "=&v"(hi[5]), "=&v"(hi[6]), "=&v"(hi[7]), "=&v"(s0), "=&v"(s1)
                                 : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(as) : "memory"));
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) bb[j] |= hi[j] << 16;
                const uint32_t scan0 = s0 | (s1 << 16);
                W_STAT(1, __popcll(amask0) * 8);
                // The hits of all eight comparisons are counted first (scalar), then parked in one straight run: no branch and no fold between
                // two candidates -- a wave's critical path through a body is what bounds the kernel, not the number of its instructions.  The stack
                // holds 127 entries: when these do not fit on top of what is parked it is folded empty first, and the (rare: runs, zeros) body with
                // more hits than the stack holds takes the candidates one by one as before.
                const uint32_t lf = lanebits | firstb;
                unsigned long long mm[8];
                uint32_t total = 0;
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) mm[j] = mask_eq_u32(bb[j], scan0);
                if (vexact) { // (uniform)
#pragma unroll
                    for (uint32_t j = 0; j < 8; j++) mm[j] &= amask0 & mask_gt_u32(rem, j);
                }
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) total += (uint32_t)__popcll(mm[j]);
                auto entry_of = [&](uint32_t j) -> uint32_t {
                    const uint32_t wd = j < 2 ? G0.w : j < 4 ? G0.z : j < 6 ? G0.y : G0.x, lb = j == 0 ? lf : lanebits;
                    return (j & 1) ? and_or(wd, 0xffffu, lb) : or_w1(lb, wd);
                };
                if (total) {
                    if (tail + total > kRing - 1) { while (tail) W_TF(fold()); }
                    if (total <= kRing - 1) {
                        // (only the lanes with a hit store: the others' stores to a common dummy word were the kernel's largest source of bank conflicts)
                        uint32_t ta[8], te[8];
#pragma unroll
                        for (uint32_t j = 0; j < 8; j++) {
                            ta[j] = stack_slot(mm[j], ring + (tail << 2)); te[j] = entry_of(j);
                            tail += (uint32_t)__popcll(mm[j]);
                        }
                        tail = (uint32_t)__builtin_amdgcn_readfirstlane(tail);
                        unsigned long long sv;
                        asm volatile("s_mov_b64 %0, exec\n\t"
                                     "s_mov_b64 exec, %17\n\tds_write_b32 %1, %9\n\ts_mov_b64 exec, %18\n\tds_write_b32 %2, %10\n\t"
                                     "s_mov_b64 exec, %19\n\tds_write_b32 %3, %11\n\ts_mov_b64 exec, %20\n\tds_write_b32 %4, %12\n\t"
                                     "s_mov_b64 exec, %21\n\tds_write_b32 %5, %13\n\ts_mov_b64 exec, %22\n\tds_write_b32 %6, %14\n\t"
                                     "s_mov_b64 exec, %23\n\tds_write_b32 %7, %15\n\ts_mov_b64 exec, %24\n\tds_write_b32 %8, %16\n\t"
                                     "s_mov_b64 exec, %0"
                                     : "=&s"(sv)
                                     : "v"(ta[0]), "v"(ta[1]), "v"(ta[2]), "v"(ta[3]), "v"(ta[4]), "v"(ta[5]), "v"(ta[6]), "v"(ta[7]),
                                       "v"(te[0]), "v"(te[1]), "v"(te[2]), "v"(te[3]), "v"(te[4]), "v"(te[5]), "v"(te[6]), "v"(te[7]),
                                       "s"(mm[0]), "s"(mm[1]), "s"(mm[2]), "s"(mm[3]), "s"(mm[4]), "s"(mm[5]), "s"(mm[6]), "s"(mm[7]) : "memory");
                    } else {
#pragma unroll
                        for (uint32_t j = 0; j < 8; j++) {
                            if (mm[j]) {
                                stack_push(mm[j], (uint32_t)__builtin_amdgcn_readfirstlane(ring + (tail << 2)), dummy, entry_of(j));
                                tail = (uint32_t)__builtin_amdgcn_readfirstlane(tail + (uint32_t)__popcll(mm[j]));
                                if (tail >= kWFoldAt) W_TF(fold());
                            }
                        }
                    }
                    while (tail >= kWFoldAt) W_TF(fold());
                }
                amask &= mask_gt_u32(rem, 8u); // lanes whose chain goes on (a fold may have ended others: nice_match)
                firstb = sel_mask(amask0, 0u, firstb);
            }
            G0 = G1; G1 = G2; G2 = G3;
            left = left ? left - 1 : 0;
            if (first && jmask) { // the searches the pass started or refilled: their 32 candidates have had a body's time to arrive
                W_TK(if ((jmask >> lane) & 1ull) { G0 = F0; G1 = F1; G2 = F2; G3 = F3; left = 4; });
            }
            rem = sel_mask(amask0, rem > 8 ? rem - 8 : 0, rem);
            {   // lanes that walk on but have nothing left in registers wait for the next pass
                const unsigned long long cm = amask & mask_eq_u32(left, 0u);
                cont = cont || ((cm >> lane) & 1ull);
                amask &= ~cm;
            }
            amask |= jmask; jmask = 0;
            if (amask == 0 || (uint32_t)__popcll(smask & ~amask) + idle >= kWTrig) break;
        }
        W_T(1);
    }
    if (TILE) {
        __syncthreads(); // every walker of the tile is done: gm / gs are complete
        W_TEND();
        tile_exits<kWThreads>(reinterpret_cast<uint8_t *>(lds), gm, gs, th0, th1, tnent_all, tg.exits + (size_t)c * kTileExitStride, tid);
        if (ROWS && tnent_all == 1) { // a stream's first tile is entered at 0 whatever the tile in front of it in the launch did: its exit is a constant, and the chain over the launch's tiles (zgpu_cont.hip) restarts here
            __syncthreads();
            uint16_t *ex = tg.exits + (size_t)c * kTileExitStride;
            const uint16_t v = __hip_atomic_load(ex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (uint32_t k = 1 + tid; k < kTileEntries; k += kWThreads) ex[k] = v;
        }
    }
    if (FUSE) {
        __syncthreads(); // every walker of the chunk is done: the logs and their counts are complete (and written: the barrier waits for the stores)
        W_TEND();
#ifdef ZGPU_P2_TIME
        if (tid == 0) atomicAdd(&p2_fused_time[7], wall_clock64() - p2_t_in);
#endif
#ifdef ZGPU_WALK_STATS
        if (tid < kP2Wins) { atomicAdd(&walk_log_stats[0], (unsigned long long)lcnt[tid]); atomicMax(&walk_log_stats[1], (unsigned long long)lcnt[tid]); }
#endif
        uint32_t nlog = 0; // (uniform) games in the chunk's logs
#pragma unroll
        for (uint32_t a = 0; a < kP2Wins; a++) nlog += (uint32_t)__builtin_amdgcn_readfirstlane((int)lcnt[a]);
        const bool whole = tail_cap != 0 && nlog <= tail_cap; // (tail_cap 0: every chunk through the windowed tail)
        bool done = false;
        if (whole) done = tail_chunk<kWThreads>(reinterpret_cast<uint8_t *>(lds), lcnt, lpos, lrec, src, n, base, slide_at, tokens + (size_t)c * kChunkMax, meta[c], tid);
#ifdef ZGPU_WALK_STATS
        if (tid == 0) atomicAdd(&walk_log_stats[done ? 2 : whole ? 4 : 3], 1ull);
#endif
        if (!done) { // the windowed tail (zgpu_lz_parse_body.inc with LOG), from its start
            constexpr uint32_t kP2Threads = kWThreads;
            constexpr bool LITE = true, FUSED = true, TILE = false, ROWS = false, LOG = true;
            const uint2 *recs = nullptr;
            const uint32_t *gmv_all = nullptr, *gsv_all = nullptr; // (the position-indexed form: tiles only)
            uint8_t *pl = reinterpret_cast<uint8_t *>(lds);
            uint16_t *const J = reinterpret_cast<uint16_t *>(pl + kP2OffJ);
            uint32_t *const HAS = reinterpret_cast<uint32_t *>(pl + kP2OffHAS), *const MARK = reinterpret_cast<uint32_t *>(pl + kP2OffMARK), *const COV = reinterpret_cast<uint32_t *>(pl + kP2OffCOV),
                     *const MAT = reinterpret_cast<uint32_t *>(pl + kP2OffMAT), *const wbase = reinterpret_cast<uint32_t *>(pl + kP2OffWbase), *const VIS = reinterpret_cast<uint32_t *>(pl + kP2OffVIS),
                     *const EXITS = reinterpret_cast<uint32_t *>(pl + kP2OffEXITS), *const wave_tot = reinterpret_cast<uint32_t *>(pl + kP2OffWtot);
            uint32_t &sh_entry = *reinterpret_cast<uint32_t *>(pl + kP2OffEntry), &sh_exit = *reinterpret_cast<uint32_t *>(pl + kP2OffEntry + 4);
            uint16_t *const END = reinterpret_cast<uint16_t *>(pl + kP2OffEND);
#include "zgpu_lz_parse_body.inc"
        }
    }
}

template <int MODE> static void launch_walk(const ChunkGeom &g, LevelCfg cfg, const SortedWs &ws, uint32_t *tokens, ChunkMeta *meta, const TileGeom &tg, hipStream_t st)
{
    static bool opt_in = false; // (one per MODE)
    if (!opt_in) { hipFuncSetAttribute(reinterpret_cast<const void *>(walk_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWLds); opt_in = true; }
    uint32_t *games = MODE == 1 ? ws.lrec() : ws.gm(), *starts = MODE == 1 ? reinterpret_cast<uint32_t *>(ws.lpos()) : ws.gs();
    uint32_t tail_cap = kWTailCap; // ZGPU_WALK_TAIL_CAP (tests; read per launch): the games a chunk may have to take the whole-chunk tail, 0: none does
    if (MODE == 1) { const char *v = getenv("ZGPU_WALK_TAIL_CAP"); char *end = nullptr; const unsigned long x = v ? strtoul(v, &end, 10) : 0; if (v && end != v) tail_cap = x < kWTailCap ? (uint32_t)x : kWTailCap; } // (a value without digits is ignored)
    hipLaunchKernelGGL(walk_kernel<MODE>, dim3(g.nchunks), dim3(kWThreads), kWLds, st, g, cfg, ws.S, ws.ir, games, starts, tokens, meta, tg, tail_cap);
}
void launch_walk_chunks(const ChunkGeom &g, LevelCfg cfg, const SortedWs &ws, uint32_t *tokens, ChunkMeta *meta, hipStream_t st) { launch_walk<1>(g, cfg, ws, tokens, meta, TileGeom{}, st); }
void launch_walk_tiles(const ChunkGeom &g, const TileGeom &tg, LevelCfg cfg, const SortedWs &ws, ChunkMeta *meta, hipStream_t st)
{
    if (geom_rows(g)) launch_walk<3>(g, cfg, ws, nullptr, meta, tg, st); // (many streams' tiles)
    else launch_walk<2>(g, cfg, ws, nullptr, meta, tg, st); // (a tile's walkers write games and exits, no tokens)
}

} // namespace zgpu
