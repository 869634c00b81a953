// zgpu_lz_tail.h -- the whole-chunk form of the parse behind a chunk's walkers (walk_kernel<1>, zgpu_lz_walk.hip): what zgpu_lz_parse_body.inc does
// with LOG, without its loop over windows of kP2Win positions.  (Device code; the includer has included zgpu_lz_parse.h.)
//
// The windowed tail threads the path eight times, a window at a time, because J -- the successor of every POSITION -- is 16 bits a position and a window
// of them is what LDS has room for.  With the logs the tail needs the successors of GAMES only, and a chunk has far fewer games than positions
// (profiles/r07_walk_log_summary.txt: 7 800 on a Silesia-mix chunk at level 6).  So the games are numbered in position order (their RANK: a prefix count
// over the bitmap HAS), N[rank] is the rank of the game the parse plays next, and everything from there to the match bits works on ranks:
//   1  has(p)      a bit per game start; the chunk's log entries -- all windows' logs, taken as one list -- are shared out, entry f to lane f % T, and STAY
//                  in the lane's registers (position and record, kWtRounds of each) until the last token is stored: the logs are read once
//   2  numbers     prefix counts of HAS per word (RC): rank_of(p)
//   3  successors  N[rank_of(p)] = rank of the first game start at or behind the game's end, kWtNone where the path leaves the chunk
//   4  blocks      the ranks in blocks of kWtBlk = 64: a lane walks its block from the block's first game through N (visited ranks: a 64-bit mask) and
//                  records where the walk leaves the block
//   5  thread      the true path through the blocks' exits, optimistic form (see A2 of the windowed tail): wave 0 walks the exits out of its registers,
//                  a wave-uniform step a block, and notes where the path enters each block it visits
//   6  meet        every visited block walks the path from its entry to where it meets the block's own walk, on its own lane; MARK: a bit per rank;
//                  a block the path runs through without meeting must leave it where the block's walk does -- if one does not, the assumption has
//                  failed and the caller runs the windowed tail from its start (nothing it reads has been touched: the logs, their counts)
//   B  matches     MAT / COV of the games whose rank is marked (the `onp` idiom of the windowed stage B)
//   C  indices     one prefix scan over the chunk's 2048 token words
//   D  tokens      match tokens by game; literals by position, four in a row a lane, a run's bytes asked for in front of the stores of the run before
//   3  cuts        parse_block_cuts, as the windowed tail
// Successors point forward (a game ends behind its start), so ranks along a walk rise strictly: every loop below ends after at most as many steps as
// there are ranks in its range, whatever the logs hold, and nothing waits for another workgroup.
#pragma once

namespace zgpu {

constexpr uint32_t kWtRounds = 24, kWtBlk = 64, kWtNone = 0xffffu;
template <uint32_t T> struct TailLds { // offsets in bytes; T lanes
    static constexpr uint32_t kCap = kWtRounds * T;            // games N has room for
    static constexpr uint32_t kBlocks = kCap / kWtBlk;         // blocks of ranks at the most
    static constexpr uint32_t kHAS = 0, kCOV = kHAS + kP2Words * 4, kMAT = kCOV + kP2Words * 4, kWbase = kMAT + kP2Words * 4, kRC = kWbase + (kP2Words + 4) * 4,
                              kN = kRC + kP2Words * 2, kMARK = kN + kCap * 2, kEX = kMARK + kCap / 8, kENT = kEX + kBlocks * 2, kWtot = kENT + kBlocks * 2,
                              kFlag = kWtot + 64, kBytes = kFlag + 16;
    static_assert(kCap < kWtNone && kCap % kWtBlk == 0 && kBlocks % 64 == 0 && kBlocks <= T && kP2Words % T == 0 && T % 64 == 0 && T / 64 <= 16, "workgroup size");
};

#ifdef ZGPU_P2_TIME // debug build only (scripts/p2_time.py fused): the whole-chunk tail's stages 0 .. 9 in the order of the list above (lane 0's 100 MHz wall
                    // clock, summed over the chunks), 10 the chunks that went through it, 11 those of them whose threading check failed
__device__ unsigned long long p2_tail_time[12];
extern "C" __attribute__((visibility("default"))) void zgpu_debug_p2_tail_time(unsigned long long *out, int reset)
{
    unsigned long long z[12] = {};
    hipMemcpyFromSymbol(out, HIP_SYMBOL(p2_tail_time), sizeof z);
    if (reset) hipMemcpyToSymbol(HIP_SYMBOL(p2_tail_time), z, sizeof z);
}
#define WT_T0() unsigned long long wt_prev_ = wall_clock64(), wt_acc_[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define WT_T(i) do { if (tid == 0) { const unsigned long long t_ = wall_clock64(); wt_acc_[i] += t_ - wt_prev_; wt_prev_ = t_; } } while (0)
#define WT_TEND(failed) do { if (tid == 0) { for (int i_ = 0; i_ < 10; i_++) atomicAdd(&p2_tail_time[i_], wt_acc_[i_]); atomicAdd(&p2_tail_time[10], 1ull); \
                                              if (failed) atomicAdd(&p2_tail_time[11], 1ull); } } while (0)
#else
#define WT_T0() do { } while (0)
#define WT_T(i) do { } while (0)
#define WT_TEND(failed) do { } while (0)
#endif

// scan of v over the workgroup's lanes in lane order: returns the exclusive prefix of this lane, total = the sum (wtot: T / 64 words of LDS; one barrier)
template <uint32_t T> __device__ __forceinline__ uint32_t tail_scan(uint32_t v, uint32_t *wtot, uint32_t tid, uint32_t &total)
{
    const uint32_t lane = tid & 63, wave = tid >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if ((int)lane >= d) x += y; }
    if (lane == 63) wtot[wave] = x; // (the readers of the scan before are past a barrier of the caller's)
    __syncthreads();
    uint32_t b = x - v, tot = 0;
    for (uint32_t w = 0; w < T / 64; w++) { const uint32_t t = wtot[w]; tot += t; if (w < wave) b += t; }
    total = tot;
    return b;
}

// The tail of chunk `n` bytes at src.  pl: the workgroup's LDS from its start (TailLds<T>::kBytes of it); lcnt: the windows' log counts (LDS, outside
// pl's range), whose sum the caller has found to be at most TailLds<T>::kCap; lpos / lrec: the chunk's logs; base, slide_at: as the parse's ParseCtx.
// Returns false -- with nothing written to tok or out -- when the optimistic threading did not hold (uniform).
template <uint32_t T>
__device__ __forceinline__ bool tail_chunk(uint8_t *pl, const uint32_t *lcnt, const uint16_t *lpos, const uint32_t *lrec, const uint8_t *src, uint32_t n, uint32_t base,
                                           int slide_at, uint32_t *tok, ChunkMeta &out, uint32_t tid_all)
{
    using L = TailLds<T>;
    constexpr uint32_t kOwn = kP2Batch, kRun = 4 * kOwn * T; // stage D's literals go out in runs of kRun positions, kOwn dwords a lane
    static_assert(kWtRounds % kP2Batch == 0 && kP2Wins == 8, "whole batches");
    uint32_t *const HAS = reinterpret_cast<uint32_t *>(pl + L::kHAS), *const COV = reinterpret_cast<uint32_t *>(pl + L::kCOV), *const MAT = reinterpret_cast<uint32_t *>(pl + L::kMAT),
             *const wbase = reinterpret_cast<uint32_t *>(pl + L::kWbase), *const MARK = reinterpret_cast<uint32_t *>(pl + L::kMARK), *const wtot = reinterpret_cast<uint32_t *>(pl + L::kWtot),
             *const flag = reinterpret_cast<uint32_t *>(pl + L::kFlag);
    uint16_t *const RC = reinterpret_cast<uint16_t *>(pl + L::kRC), *const N = reinterpret_cast<uint16_t *>(pl + L::kN), *const EX = reinterpret_cast<uint16_t *>(pl + L::kEX),
             *const ENT = reinterpret_cast<uint16_t *>(pl + L::kENT);
    // The lane's number is opaque, and made so anew in front of every stage (WT_TID), as inside a window of the windowed tail: everything a stage derives
    // from it alone -- the numbers of a lane's twenty-four list entries, the offsets of its bytes -- the compiler otherwise computes once and keeps in
    // registers to the end, beside the games that have to stay there (it spilled instead).
    uint32_t tid = tid_all;
#define WT_TID() do { tid = tid_all; asm volatile("" : "+v"(tid)); } while (0)
    WT_TID();
    const uint32_t lane = tid_all & 63, wave = tid_all >> 6;
    const uint32_t nwords = (n + 31) >> 5;
    const uint32_t *lpos2 = reinterpret_cast<const uint32_t *>(lpos);
    WT_T0();

    // ---- 1. has(p): the log entries, all in flight before the first wait ----
    uint32_t cum[kP2Wins + 1]; // (uniform) entries in front of each window's log in the list of all of them
    cum[0] = 0;
#pragma unroll
    for (uint32_t a = 0; a < kP2Wins; a++) cum[a + 1] = cum[a] + (uint32_t)__builtin_amdgcn_readfirstlane((int)lcnt[a]);
    const uint32_t nlog = cum[kP2Wins];
    for (uint32_t i = tid; i < kP2Words; i += T) { HAS[i] = 0; COV[i] = 0; MAT[i] = 0; }
    if (tid < L::kBlocks) ENT[tid] = (uint16_t)kWtNone;
    if (tid == 0) *flag = 0;
    auto slot_of = [&](uint32_t i) { // where entry i * T + tid of the list lies in the logs: entry f - cum[a] of window a's (entry 0 of the first where the lane has none)
        const uint32_t f = i * T + tid;
        uint32_t at = f;
#pragma unroll
        for (uint32_t a = 1; a < kP2Wins; a++) at = f >= cum[a] ? a * kP2Win + (f - cum[a]) : at;
        return f < nlog ? at : 0u;
    };
    uint32_t gq[kWtRounds], gm[kWtRounds]; // the lane's games: the dword its position lies in (positions are read two to a dword and taken out below: nothing
                                           // is done to a loaded value before every load is out), the record
#pragma unroll
    for (uint32_t i = 0; i < kWtRounds; i++) {
        gq[i] = 0; gm[i] = 0;
        if (i * T < nlog) { // (uniform: the rounds are cut off by scalar branches; inside a round every lane loads)
            const uint32_t at = slot_of(i);
            gq[i] = p2_ld<true>(lpos2 + (at >> 1));
            gm[i] = p2_ld<true>(lrec + at);
        }
    }
    __syncthreads();
    WT_TID();
    uint32_t gp[kWtRounds / 2]; // the games' starts, two to a register; a round's entry is a game when i * T + tid < nlog
    auto is_game = [&](uint32_t i) { return i * T + tid < nlog; };
    auto pos_of = [&](uint32_t i) { return (gp[i >> 1] >> ((i & 1u) << 4)) & 0xffffu; };
#pragma unroll
    for (uint32_t i = 0; i < kWtRounds; i += 2)
        gp[i >> 1] = ((gq[i] >> ((slot_of(i) & 1u) << 4)) & 0xffffu) | ((gq[i + 1] >> ((slot_of(i + 1) & 1u) << 4)) << 16);
#pragma unroll
    for (uint32_t i = 0; i < kWtRounds; i++) {
        if (!is_game(i)) gm[i] = 0;
        if (is_game(i)) { const uint32_t p = pos_of(i); atomicOr(&HAS[p >> 5], 1u << (p & 31u)); }
    }
    WT_T(0);

    // ---- 2. the games' numbers ----
    WT_TID();
    constexpr uint32_t kPer = kP2Words / T;
    uint32_t nn;
    {
        uint32_t cnt[kPer], sum = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kPer; i++) { cnt[i] = (uint32_t)__builtin_popcount(HAS[tid * kPer + i]); sum += cnt[i]; }
        uint32_t b = tail_scan<T>(sum, wtot, tid, nn);
#pragma unroll
        for (uint32_t i = 0; i < kPer; i++) { RC[tid * kPer + i] = (uint16_t)b; b += cnt[i]; }
        __syncthreads();
    }
    // (nn <= nlog <= kCap: a position starts one game at most -- a neutral position is claimed by one walker -- so nn == nlog; whatever the logs hold, a rank is
    // below nn and inside N.  Two log entries at one position would share a rank and write N[rank] twice: the ZGPU_WALK_STATS build counts the chunks where
    // nn != nlog, see walk_log_stats in zgpu_lz_walk.hip)
#ifdef ZGPU_WALK_STATS
    if (tid == 0 && nn != nlog) atomicAdd(&walk_log_stats[5], 1ull);
#endif
    auto rank_of = [&](uint32_t p) { return (uint32_t)RC[p >> 5] + (uint32_t)__builtin_popcount(HAS[p >> 5] & ~(~0u << (p & 31u))); };
    WT_T(1);

    // ---- 3. successors by rank ----
    WT_TID();
#pragma unroll
    for (uint32_t i = 0; i < kWtRounds; i++) {
        if (is_game(i)) {
            const uint32_t p = pos_of(i), x = p + (gm[i] >> 24) + ((gm[i] >> 15) & 511u);
            uint32_t w = x >> 5, s = kWtNone;
            if (w < nwords) {
                uint32_t hv = HAS[w], v = hv & (~0u << (x & 31u));
                while (v == 0 && ++w < nwords) { hv = HAS[w]; v = hv; }
                if (v) s = (uint32_t)RC[w] + (uint32_t)__builtin_popcount(hv & ~(~0u << (uint32_t)__builtin_ctz(v)));
            }
            N[rank_of(p)] = (uint16_t)s;
        }
    }
    __syncthreads();
    WT_T(2);

    // ---- 4. every block's own walk ----
    WT_TID();
    const uint32_t nblk = (nn + kWtBlk - 1) / kWtBlk, r0 = tid * kWtBlk, r1 = r0 + kWtBlk < nn ? r0 + kWtBlk : nn; // (this lane's block: ranks [r0, r1), tid < nblk)
    uint64_t vis = 0;
    uint32_t myexit = kWtNone;
    if (tid < nblk) {
        uint32_t x = r0;
        while (x < r1) { vis |= 1ull << (x - r0); const uint32_t s = N[x]; x = s > x ? s : x + 1; } // (N[x] > x: the guard holds the bound whatever N holds)
        myexit = x;
        EX[tid] = (uint16_t)x;
    }
    __syncthreads();
    WT_T(3);

    // ---- 5. the path through the exits ----
    WT_TID();
    if (wave == 0 && nn != 0) {
        uint32_t ex[L::kBlocks / 64];
#pragma unroll
        for (uint32_t j = 0; j < L::kBlocks / 64; j++) ex[j] = EX[j * 64 + lane]; // (blocks at and above nblk: never asked for)
        uint32_t cb = 0, ce = 0; // (uniform) the path enters block cb at rank ce
        // (the one serial stretch of the tail: a few dozen instructions a block on one wave, which shares its SIMD with three waves of the other workgroup's
        // walkers at the same priority)
        for (uint32_t step = 0; step < L::kBlocks; step++) { // (cb rises with every step)
            if (lane == 0) ENT[cb] = (uint16_t)ce;
            uint32_t e = 0;
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(cb >> 6));
#pragma unroll
            for (uint32_t j = 0; j < L::kBlocks / 64; j++) if (hi == j) e = (uint32_t)__builtin_amdgcn_readlane((int)ex[j], (int)(cb & 63u));
            if (e == kWtNone) break;
            ce = e; cb = e / kWtBlk; // (e: a rank at or behind the end of block cb)
            if (cb >= L::kBlocks) break; // (cannot happen: ranks are below kCap)
        }
    }
    __syncthreads();
    WT_T(4);

    // ---- 6. from the entry to the meeting point, block by block ----
    WT_TID();
    if (tid < nblk) {
        uint32_t x = ENT[tid];
        uint64_t m = 0;
        bool met = false;
        const bool on = x != kWtNone;
        while (x < r1) { // (kWtNone: at or above any r1)
            const uint64_t below = ~0ull << (x - r0);
            if ((vis >> (x - r0)) & 1ull) { m |= vis & below; met = true; break; } // met: the rest of the block's walk is the path
            m |= below & ~(below << 1);
            const uint32_t s = N[x];
            x = s > x ? s : x + 1;
        }
        MARK[2 * tid] = (uint32_t)m; MARK[2 * tid + 1] = (uint32_t)(m >> 32);
        if (on && !met && x != myexit) *flag = 1;
    }
    __syncthreads();
    const bool ok = *flag == 0;
    WT_T(5);
    if (!ok) { WT_TEND(1); __syncthreads(); return false; } // (the flag has been read by everyone before the windowed tail writes over it)

    // ---- B. matches of the path ----
    WT_TID();
    uint32_t onp = 0; // bit i: the game of round i is on the path (the games themselves are not touched: zgpu_lz_parse_body.inc, stage B)
#pragma unroll
    for (uint32_t i = 0; i < kWtRounds; i++) {
        bool on_path = false;
        if (is_game(i)) { const uint32_t r = rank_of(pos_of(i)); on_path = (MARK[r >> 5] >> (r & 31u)) & 1u; }
        onp |= on_path ? 1u << i : 0u;
        if (on_path) {
            const uint32_t m = pos_of(i) + (gm[i] >> 24), Lm = (gm[i] >> 15) & 511u;
            atomicOr(&MAT[m >> 5], 1u << (m & 31u));
            const uint32_t a = m + 1, z = m + Lm; // [a, z)
            for (uint32_t wd = a >> 5; wd <= (z - 1) >> 5; wd++) {
                const uint32_t lo_b = wd == (a >> 5) ? (a & 31u) : 0u, hi_b = wd == ((z - 1) >> 5) ? ((z - 1) & 31u) : 31u;
                atomicOr(&COV[wd], (~0u << lo_b) & (~0u >> (31u - hi_b)));
            }
        }
    }
    __syncthreads();
    WT_T(6);

    // ---- C. token positions = positions not inside a match; exclusive prefix counts per word ----
    WT_TID();
    uint32_t ntok;
    {
        uint32_t tw[kPer], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < kPer; i++) {
            const uint32_t wd = tid * kPer + i;
            tw[i] = wd < nwords ? ~COV[wd] : 0u;
            if (wd == nwords - 1 && (n & 31u)) tw[i] &= ~0u >> (32u - (n & 31u));
            sum += (uint32_t)__builtin_popcount(tw[i]);
        }
        uint32_t b = tail_scan<T>(sum, wtot, tid, ntok);
#pragma unroll
        for (uint32_t i = 0; i < kPer; i++) { const uint32_t wd = tid * kPer + i; wbase[wd] = b; COV[wd] = tw[i]; b += (uint32_t)__builtin_popcount(tw[i]); }
        __syncthreads();
    }
    const uint32_t *TOK = COV;
    auto index_of = [&](uint32_t p) { return wbase[p >> 5] + (uint32_t)__builtin_popcount(TOK[p >> 5] & ~(~0u << (p & 31u))); };
    WT_T(7);

    // ---- D. tokens ----
    // (indices first, then the stores in one run, each a 32-bit offset from `tok`, bytes and indices pinned in front of the run: zgpu_lz_parse_body.inc, stage D)
    auto tok_put = [&](uint32_t idx, uint32_t v) { *reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(tok) + (idx << 2)) = v; }; // (idx < kChunkMax)
    WT_TID();
#pragma unroll
    for (uint32_t ib = 0; ib < kWtRounds; ib += kP2Batch) { // the match tokens, by game -- first: the games leave the registers in front of the literals' bytes
        if (ib * T < nlog) {
            uint32_t mx[kP2Batch], mt[kP2Batch];
#pragma unroll
            for (uint32_t u = 0; u < kP2Batch; u++) {
                const uint32_t gv = ((onp >> (ib + u)) & 1u) ? gm[ib + u] : 0u, m = pos_of(ib + u) + (gv >> 24);
                mt[u] = gv ? tok_match(gv & 32767u, ((gv >> 15) & 511u) - kMinMatch) : 0u;
                mx[u] = gv ? index_of(m) : kNone; // (m < n: the match lies inside the chunk)
            }
#pragma unroll
            for (uint32_t u = 0; u < kP2Batch; u++) asm volatile("" : "+v"(mx[u]), "+v"(mt[u]));
#pragma unroll
            for (uint32_t u = 0; u < kP2Batch; u++) if (mx[u] != kNone) tok_put(mx[u], mt[u]);
        }
    }
    // Literals: a lane takes four positions in a row, p = 4 (k T + tid) .. p + 3, and ONE word of each of TOK, MAT and wbase, which the four share.  Their
    // bytes come as the two aligned dwords they lie in (an aligned dword does not cross a page: the bytes in front of the chunk's first and behind its last
    // are there to be read), asked for whether or not the positions are tokens and clamped to the chunk's last dword, so that no load stands under a
    // lane's condition: such a load is waited for where it stands.  kOwn positions-of-four a lane make a run of kRun positions, and a run's bytes are
    // asked for in front of the stores of the run before.
    const uint32_t sa = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u), dlast = (sa + n - 1) >> 2; // (uniform) src's offset in its dword; the chunk's last dword
    const uint32_t *src4 = reinterpret_cast<const uint32_t *>(src - sa);
    auto run_fetch = [&](uint32_t w0, uint32_t (&lit)[kOwn]) {
        WT_TID();
#pragma unroll
        for (uint32_t i = 0; i < kOwn; i++) {
            const uint32_t d = w0 / 4 + i * T + tid; // position p = 4 d: bytes sa .. sa + 3 of the dwords d, d + 1
            uint32_t v = 0;
            if (w0 < n) v = __builtin_amdgcn_alignbyte(src4[d + 1 < dlast ? d + 1 : dlast], src4[d < dlast ? d : dlast], sa); // (uniform branch)
            lit[i] = v;
        }
    };
    auto run_store = [&](uint32_t w0, uint32_t (&lit)[kOwn]) {
        WT_TID();
#pragma unroll
        for (uint32_t i = 0; i < kOwn; i++) {
            const uint32_t p = w0 + 4 * (i * T + tid), sh = p & 31u; // (p < kChunkMax: a word of the arrays, tokens or not)
            const uint32_t tw = TOK[p >> 5], lw = ((tw & ~MAT[p >> 5]) >> sh) & 15u; // the four positions that are literals (TOK is empty from n on)
            uint32_t ix = wbase[p >> 5] + (uint32_t)__builtin_popcount(tw & ~(~0u << sh));
            asm volatile("" : "+v"(lit[i]), "+v"(ix));
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                if ((lw >> j) & 1u) tok_put(ix, tok_lit((lit[i] >> (8 * j)) & 255u));
                ix += (tw >> (sh + j)) & 1u;
            }
        }
    };
    {
        uint32_t la[kOwn], lb[kOwn];
        run_fetch(0, la);
        for (uint32_t w0 = 0; w0 < n; w0 += 2 * kRun) {
            run_fetch(w0 + kRun, lb);     // (past n: nothing is loaded)
            run_store(w0, la);
            run_fetch(w0 + 2 * kRun, la);
            if (w0 + kRun < n) run_store(w0 + kRun, lb);
        }
    }
    WT_T(8);

    // ---- 3. block cuts and the stored-block veto ----
    WT_TID();
    if (tid == 0) parse_block_cuts(slide_at, base, TOK, MAT, wbase, n, nwords, kP2Words, ntok, out);
    WT_T(9);
    WT_TEND(0);
#undef WT_TID
    return true;
}

} // namespace zgpu
