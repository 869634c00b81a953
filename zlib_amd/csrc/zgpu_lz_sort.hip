// zgpu_lz_sort.hip -- the sorts of the sorted-bucket LZ77 stage (zgpu_lz_sorted.hip has the map): K1c sort4_kernel, K1' sort_kernel + heads_below_kernel.
#include "zgpu_lz_sorted.h"
#include <cstdlib>

#include <atomic>
static std::atomic<int> g_inject_sort_fault{0};
extern "C" __attribute__((visibility("default"))) void zgpu_debug_inject_sort_fault(void) { g_inject_sort_fault.store(1); }

namespace zgpu {

constexpr uint32_t kSuperS = 1024;   // positions per superblock of the sort passes

// For block w of 64 S indices (1024 lanes, lane w holds the 64 head bits of its block): the distance from index 64*w down
// to the last bucket head below the block, 65535 if there is none (w == 0) or it is farther.  The rank of an S entry in
// its bucket is its distance from the last head at or below it, and this is the part of it that lies outside its own block.
__device__ inline uint32_t heads_below(unsigned long long x, uint32_t tid, uint32_t *wave_scratch)
{
    const uint32_t lane = tid & 63, wave = tid >> 6;
    const uint32_t v = x ? 64u * tid + 64u - (uint32_t)__builtin_clzll(x) : 0; // 1 + index of the highest head of the block, 0: none
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(inc, d); if ((int)lane >= d && y > inc) inc = y; }
    if (lane == 63) wave_scratch[wave] = inc;
    __syncthreads();
    uint32_t ex = __shfl_up(inc, 1);
    if (lane == 0) ex = 0;
    for (uint32_t w = 0; w < wave; w++) { const uint32_t y = wave_scratch[w]; if (y > ex) ex = y; }
    const uint32_t dist = 64u * tid - (ex - 1);
    return ex && dist < 65535u ? dist : 65535u;
}

__global__ void __launch_bounds__(1024) heads_below_kernel(uint32_t *__restrict__ heads_all) // after sort_kernel (the fallback path)
{
    __shared__ uint32_t scratch[16];
    uint32_t *hd = heads_all + (size_t)blockIdx.x * kHeadStride;
    const uint32_t b = heads_below(reinterpret_cast<const unsigned long long *>(hd)[threadIdx.x], threadIdx.x, scratch);
    reinterpret_cast<uint16_t *>(hd + kHeadWords)[threadIdx.x] = (uint16_t)b;
}

// ------------------------------------------------------------------------------------------------- K1'
// One 256-lane workgroup (4 waves) per chunk.  Pass A is sequential in position order only among positions that share a
// hash, so the hash space is split four ways: every wave sweeps all positions but counts only the hashes with
// (h & 3) == its wave number -- four sequential sweeps run side by side on the four SIMDs with a quarter of the
// duplicate-resolution work each.  Passes B and C are plainly parallel over the 256 lanes.
#ifndef ZGPU_SORT_WAVES
#define ZGPU_SORT_WAVES 8
#endif
constexpr uint32_t kSortWaves = ZGPU_SORT_WAVES, kSortThreads = 64 * kSortWaves; // waves per chunk: 4 or 8 (or 16)

template <bool ROWS>
__global__ void __launch_bounds__(kSortThreads) sort_kernel(ChunkGeom g, uint16_t *__restrict__ S_all, uint16_t *__restrict__ rank_all, uint32_t *__restrict__ heads_all,
                                                            uint32_t *__restrict__ ir_all)
{
    __shared__ uint16_t cnt[kHashSize];                                         // counts, then bucket starts
    __shared__ __attribute__((aligned(16))) uint32_t in_stage[kSuperS / 4 + 4]; // 1 KiB of input + 8 bytes of the next
    __shared__ __attribute__((aligned(16))) uint16_t out_stage[kSuperS];
    __shared__ uint8_t tag[4096];
    __shared__ uint32_t wave_tot[kSortWaves];
    if constexpr (ROWS) { if (g.rows[blockIdx.x].n == 0) return; } // a padding row (zgpu_deflate_streams_plan.h, streams_pad_row): a tile that parses nothing
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t lo; uint32_t n;
    chunk_span<ROWS>(g, c, lo, n);
    const uint8_t *src = g.in + lo;
    uint16_t *S = S_all + (size_t)c * kSStride + kSPad, *rk = rank_all + (size_t)c * kChunkMax;
    uint32_t *hd = heads_all + (size_t)c * kHeadStride, *ir = ir_all + (size_t)c * kChunkMax;
    if (tid < kSPad) S[-(int)kSPad + (int)tid] = 0;
    for (uint32_t i = tid; i < kChunkMax / 32; i += kSortThreads) hd[i] = 0; // (pass C sets bits; the barriers of pass A lie in between)
    for (uint32_t i = tid; i < kHashSize / 2; i += kSortThreads) reinterpret_cast<uint32_t *>(cnt)[i] = 0;
    const uint32_t npos = n >= 3 ? n - 2 : 0;
    volatile uint16_t *vcnt = cnt;
    volatile uint8_t *vtag = tag;
    const unsigned long long lt_mask = (1ull << lane) - 1;
    const bool aligned = (reinterpret_cast<uintptr_t>(src) & 3) == 0;
    auto fetch = [&](uint32_t sb) -> uint32_t { // dword `tid` of superblock sb (threads 0..255), zero padded past n
        if (tid >= kSuperS / 4) return 0;
        const uint32_t a = sb * kSuperS + tid * 4;
        if (a + 4 <= n && aligned) return *reinterpret_cast<const uint32_t *>(src + a);
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; k++) if (a + k < n) v |= (uint32_t)src[a + k] << (8 * k);
        return v;
    };
    auto flush = [&](uint16_t *dst_base, uint32_t sb) { // out_stage -> global, 8 bytes per lane (threads 0..255)
        if (tid >= kSuperS / 4) return;
        const uint32_t p0 = sb * kSuperS + tid * 4;
        if (p0 + 4 <= n) *reinterpret_cast<uint2 *>(dst_base + p0) = reinterpret_cast<const uint2 *>(out_stage)[tid];
        else for (uint32_t k = 0; k < 4; k++) if (p0 + k < n) dst_base[p0 + k] = out_stage[tid * 4 + k];
    };
    const uint32_t nsuper = (n + kSuperS - 1) / kSuperS;
    const uint8_t *s8 = reinterpret_cast<const uint8_t *>(in_stage);

    // ---- pass A: rank(p) = number of earlier positions with the same hash ----
    uint32_t cur = fetch(0), nxt = fetch(1);
    __syncthreads();
    for (uint32_t sb = 0; sb < nsuper; sb++) {
        if (tid < kSuperS / 4) in_stage[tid] = cur;
        if (tid < 2) in_stage[kSuperS / 4 + tid] = __shfl(nxt, tid);
        if (sb > 0) flush(rk, sb - 1);
        cur = nxt; nxt = fetch(sb + 2);
        __syncthreads();
        const uint32_t base_p = sb * kSuperS;
#pragma unroll 1
        for (uint32_t st = 0; st < kSuperS / 64; st++) {
            const uint32_t o = st * 64 + lane, p = base_p + o;
            const uint32_t h = hash3(s8[o], s8[o + 1], s8[o + 2]);
            const bool out = g.nexcl != 0 && p < npos && excl_has(g, lo + p); // (continuous stream: a position in front of an earlier flush point is in no chain)
            const bool live = p < npos && !out && (h & (kSortWaves - 1)) == wave; // this wave owns its share of the hash space
            uint32_t old = 0;
            if (live) old = vcnt[h];
            // lanes of this step that share a hash: detected through a small tag table (a false alarm is harmless; the
            // index keeps the two ownership bits, so waves never touch each other's tags)
            if (live) vtag[h & 4095] = (uint8_t)lane;
            const uint32_t seen = live ? (uint32_t)vtag[h & 4095] : lane;
            unsigned long long clash = __ballot(live && seen != lane);
            uint32_t rank = old, group = 1;
            bool last = live;
            while (clash) {
                const int f = __ffsll((long long)clash) - 1;
                const uint32_t h0 = __builtin_amdgcn_readlane(h, f);
                const unsigned long long grp = __ballot(live && h == h0);
                if (live && h == h0) {
                    rank = old + (uint32_t)__popcll(grp & lt_mask);
                    group = (uint32_t)__popcll(grp);
                    last = (grp >> lane) == 1ull;
                }
                clash &= ~grp;
            }
            if (live && last) vcnt[h] = (uint16_t)(old + group);
            if (live) out_stage[o] = (uint16_t)rank;
            else if ((p >= npos || out) && wave == 0) out_stage[o] = out ? 0xffffu : 0;
        }
        __syncthreads();
    }
    if (nsuper && tid < kSuperS / 4) { const uint32_t p0 = (nsuper - 1) * kSuperS + tid * 4; for (uint32_t k = 0; k < 4; k++) if (p0 + k < n) rk[p0 + k] = out_stage[tid * 4 + k]; }
    __syncthreads();

    // ---- pass B: exclusive scan of the 32768 counts -> bucket starts (in place), 128 consecutive counts per lane ----
    {
        const uint32_t per = kHashSize / kSortThreads;
        uint32_t sum = 0;
        for (uint32_t i = 0; i < per; i++) sum += cnt[tid * per + i];
        uint32_t x = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if ((int)lane >= d) x += y; }
        if (lane == 63) wave_tot[wave] = x;
        __syncthreads();
        uint32_t basev = x - sum;
        for (uint32_t w = 0; w < wave; w++) basev += wave_tot[w];
        for (uint32_t i = 0; i < per; i++) { const uint32_t v = cnt[tid * per + i]; cnt[tid * per + i] = (uint16_t)basev; basev += v; }
    }
    __syncthreads();

    // ---- pass C: idx(p) = start(hash) + rank(p);  S[idx] = p ----
    cur = fetch(0); nxt = fetch(1);
    for (uint32_t sb = 0; sb < nsuper; sb++) {
        if (tid < kSuperS / 4) in_stage[tid] = cur;
        if (tid < 2) in_stage[kSuperS / 4 + tid] = __shfl(nxt, tid);
        cur = nxt; nxt = fetch(sb + 2);
        __syncthreads();
        const uint32_t base_p = sb * kSuperS;
#pragma unroll
        for (uint32_t st = 0; st < kSuperS / kSortThreads; st++) {
            const uint32_t o = st * kSortThreads + tid, p = base_p + o;
            if (p < npos) {
                const uint32_t h = hash3(s8[o], s8[o + 1], s8[o + 2]), r = rk[p], id = (uint32_t)cnt[h] + r;
                if (r == 0xffffu) continue; // not in the chains
                S[id] = (uint16_t)p;
                ir[p] = id | (r << 16);
                if (r == 0) atomicOr(&hd[id >> 5], 1u << (id & 31u)); // bucket head
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------- K1c
// The default sort.  What makes a counting sort that keeps equal keys in position order sequential is the ranking,
// rank(p) = count[h(p)]++ taken in position order.  On this hardware one LDS atomic instruction serves the lanes that
// hit the same address in ascending lane order (scripts/micro/lds_atomic_order.hip: no exception in 5e10 lane-operations),
// and the LDS serves the instructions of a CU in arrival order.  So 64 positions are ranked by ONE ds_add_rtn_u32 (two
// 16-bit counts per word; the add is 1 or 1<<16), and all that has to be sequenced is the order in which the 16 waves of
// the workgroup issue their instructions: a token in LDS walks round the waves, a turn is 8 instructions (512 positions)
// followed by the token store -- same wave, same queue, so the next holder's atomics arrive behind them.  Hashes are
// computed, and ranks taken over, outside the turn.
// The lane order inside an atomic is an observed property, not an architected one: pass V checks the result (a bucket
// must ascend), and a violation makes the engine redo the call with sort_kernel above, which relies on ballots only.
// Output: S (positions, u16), ir (idx | rank << 16 by position) and one bit per S index that marks the first entry of a
// bucket -- the rank of an entry in its bucket, which bounds its chain, is its distance from the last marked index.
//
// A lane keeps ITS positions through all passes -- the 64 of pass A's turns (turn T = wave + 16 j, step u: position
// 512 T + 64 u + lane) -- one register each: the hash, then hash | rank << 16, then the position's `ir` word, from which pass
// C1 scatters.  The input is read once, and what goes to HBM is S, ir and the head bits.  (The kernel's first form kept the
// ranks in a scratch array by position, because a lane's passes worked on different positions: 43 GB of the sort's 77 GB per
// 4 GiB went there and back.  DESIGN.md, K1'' and K1''', has the history.)
//   pass A   rank(p): the token round.  The chunk's Adler-32 rides along: the pass has every byte of the chunk in a register once,
//            for a few instructions a position -- a kernel of its own re-read the input for 0.7 ms per 4 GiB.
//   pass B   exclusive scan of the 32768 counts -> bucket starts, in place (the count of hash h is half (h & 1) of word h >> 1);
//            32 consecutive counts, four 16-byte vectors, per lane.
//   pass C0  idx(p) = start(hash) + rank: the position's ir word, written and kept; a bit per bucket head.
//   pass C1  the scatter itself, through LDS (a scattered 2-byte store to HBM costs a whole partial line): the half of S with
//            idx >> 15 == half is assembled in the memory of the dead count table and written out in order, 16 bytes per lane and step.
//   pass V   the self-check, on those 16 bytes as they go out: inside a bucket the positions must ascend.
// Continuous stream: positions in front of earlier flush points have three bytes but are in no chain -- no rank, no place in S
// (kNone32 in the lane's register, as for the positions the chunk does not have).
// Passes A and C0 have two forms of a turn: the general one, which asks of every position whether the chunk has it, whether four bytes can be
// loaded at it and whether it is in the chains, and a straight one without lane masks for a turn of which all that is known beforehand
// (whole_turn below: all but the last turn of a full chunk).  The kernel is bound by the instructions it issues, not by the token round
// (-DZGPU_SORT_TIME, scripts/sort_time.py: the poll loop is 6 % of a wave's time), and keeps one workgroup per CU: a form with 16 bits of state
// per position and two 512-lane workgroups per CU was measured and was slower (DESIGN.md section 4, K1'''').
constexpr uint32_t kS4Threads = 1024, kS4Waves = kS4Threads / 64, kS4TurnSteps = 8, kS4TurnPos = 64 * kS4TurnSteps;
struct __attribute__((packed, aligned(1))) U32u { uint32_t v; };
__device__ inline uint32_t lds_add_rtn32_nowait(uint32_t a, uint32_t v) { uint32_t o; asm volatile("ds_add_rtn_u32 %0, %1, %2" : "=v"(o) : "v"(a), "v"(v) : "memory"); return o; }

#ifdef ZGPU_SORT_TIME // debug build only (scripts/sort_time.py): clock cycles of a wave in 0 setup, 1 pass A (without 2), 2 waiting for the token, 3 pass B, 4 pass C0,
                      // 5 head bits out + heads_below, 6 pass C1 + V, 7 a turn's atomics from issue to result (taken out of 1); a section ends behind its barrier, so it holds
                      // the wait for the slowest wave.  sort_time[8]: the most workgroups seen on one CU at a time.
__device__ unsigned long long sort_time[9];
__device__ unsigned int sort_on_cu[16 * 256];
extern "C" __attribute__((visibility("default"))) void zgpu_debug_sort_time(unsigned long long *out, int reset)
{
    unsigned long long z[9] = {};
    hipMemcpyFromSymbol(out, HIP_SYMBOL(sort_time), sizeof z);
    if (reset) hipMemcpyToSymbol(HIP_SYMBOL(sort_time), z, sizeof z);
}
// (summed in registers, written once when the wave is done, as walk_kernel's clock, zgpu_lz_walk.hip)
#define S_T0() unsigned long long st_prev = __builtin_readcyclecounter(), st_tok = 0, st_atm = 0, st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; \
    const uint32_t st_cu = ((__builtin_amdgcn_s_getreg((31 << 11) | 20) & 15u) << 8) | ((__builtin_amdgcn_s_getreg((31 << 11) | 4) >> 8) & 255u); /* XCC_ID, HW_ID: cu, sh, se */ \
    if (threadIdx.x == 0) atomicMax(&sort_time[8], (unsigned long long)atomicAdd(&sort_on_cu[st_cu], 1u) + 1)
#define S_T(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); st_acc[i] += t_ - st_prev - ((i) == 1 ? st_tok + st_atm : 0); if ((i) == 1) { st_acc[2] += st_tok; st_acc[7] += st_atm; } st_tok = st_atm = 0; st_prev = t_; } while (0)
#define S_TOK(stmt) do { const unsigned long long f0_ = __builtin_readcyclecounter(); stmt; st_tok += __builtin_readcyclecounter() - f0_; } while (0)
#define S_A0() const unsigned long long a0_ = __builtin_readcyclecounter()
#define S_A1() st_atm += __builtin_readcyclecounter() - a0_
#define S_TEND() do { if (lane == 0) for (int i_ = 0; i_ < 8; i_++) atomicAdd(&sort_time[i_], st_acc[i_]); if (threadIdx.x == 0) atomicSub(&sort_on_cu[st_cu], 1u); } while (0)
#else
#define S_A0() do { } while (0)
#define S_A1() do { } while (0)
#define S_T0() do { } while (0)
#define S_T(i) do { } while (0)
#define S_TOK(stmt) stmt
#define S_TEND() do { } while (0)
#endif

template <bool ROWS> // (ROWS: the tiles of many streams, row by row -- TileRow)
__global__ void __launch_bounds__(kS4Threads) sort4_kernel(ChunkGeom g, uint16_t *__restrict__ S_all, uint32_t *__restrict__ heads_all, uint32_t *__restrict__ fault,
                                                           uint32_t *__restrict__ ir_all, ChunkMeta *__restrict__ meta)
{
    __shared__ uint32_t ad1[kS4Waves];
    __shared__ uint64_t ad2[kS4Waves];
    __shared__ __attribute__((aligned(16))) uint32_t cnt[kHashSize / 2]; // count of hash h in half (h & 1) of word h >> 1; later the bucket starts
    __shared__ uint32_t wave_tot[kS4Waves];
    __shared__ uint32_t token;
    __shared__ __attribute__((aligned(8))) uint32_t heads[kChunkMax / 32]; // bit i: S[i] is the first entry of its bucket
    if constexpr (ROWS) { if (g.rows[blockIdx.x].n == 0) return; } // a padding row (zgpu_deflate_streams_plan.h, streams_pad_row): a tile that parses nothing
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    S_T0();
    uint64_t lo; uint32_t n;
    chunk_span<ROWS>(g, c, lo, n);
    const uint8_t *src = g.in + lo;
    uint16_t *S = S_all + (size_t)c * kSStride + kSPad;
    uint32_t *hd = heads_all + (size_t)c * kHeadStride, *ir = ir_all + (size_t)c * kChunkMax;
    if (threadIdx.x < kSPad) S[-(int)kSPad + (int)threadIdx.x] = 0; // the pad reads as "position 0" (match3's finished lanes)
    uint32_t last_of_half0 = 0;
    const uint32_t npos = n >= 3 ? n - 2 : 0, nturns = (npos + kS4TurnPos - 1) / kS4TurnPos;
    // (continuous stream: the positions of the chunk that are in no chain, and those that are)
    const uint32_t nout = g.nexcl ? excl_lower(g, lo + npos) - excl_lower(g, lo) : 0u, nin = npos - nout;
    const uint32_t cnt_a = lds_off(cnt), tok_a = lds_off(&token);
    {
        uint4 *z = reinterpret_cast<uint4 *>(cnt);
        for (uint32_t i = tid; i < kHashSize * 2 / 16; i += kS4Threads) z[i] = make_uint4(0, 0, 0, 0);
        if (tid == 0) token = 0;
        for (uint32_t i = tid; i < kChunkMax / 32; i += kS4Threads) heads[i] = 0;
    }
    __syncthreads();
    S_T(0);
    auto bytes3 = [&](uint32_t p) -> uint32_t { // b0 | b1<<8 | b2<<16 of position p < npos
        if (p + 4 <= n) return reinterpret_cast<const U32u *>(src + p)->v & 0xffffffu;
        return (uint32_t)src[p] | ((uint32_t)src[p + 1] << 8) | ((uint32_t)src[p + 2] << 16);
    };
    auto hash_of = [](uint32_t v) { return hash3(v & 255u, (v >> 8) & 255u, v >> 16); };
    constexpr uint32_t kTurnsPerWave = kChunkMax / kS4TurnPos / kS4Waves; // 8
    constexpr uint32_t kNone32 = 0xffffffffu;
    uint32_t pk[kTurnsPerWave][kS4TurnSteps]; // this lane's 64 positions: hash -> hash | rank << 16 -> index | rank << 16; kNone32: no position, or not in the chains

    // A turn in the middle of the chunk -- all but the last of a full one: every position exists, has four bytes to load and is in the chains.
    // The sort is bound by the instructions it issues (DESIGN.md 4, K1'''), and the general form of passes A and C0 spends more of them on the
    // conditions of a position, lane masks and branches, than on its hash: such a turn takes a straight path in both.  (T: a scalar.)
    auto whole_turn = [&](uint32_t T) { return nout == 0 && T * kS4TurnPos + kS4TurnPos + 3 <= n; };

    // ---- pass A: rank(p) ----
    {
        uint32_t s1 = 0, s2 = 0; // Adler: sum of this lane's bytes, and of (n - p) * byte (64 positions a lane: below 2^32)
        auto preload = [&](uint32_t Tv, uint32_t (&h)[kS4TurnSteps]) {
            const uint32_t T = __builtin_amdgcn_readfirstlane(Tv); // (the wave's number: the same in all lanes, and now the compiler knows)
            if (whole_turn(T)) { // (scalar)
                const uint8_t *q = src + T * kS4TurnPos + lane;
#pragma unroll
                for (uint32_t u = 0; u < kS4TurnSteps; u++) {
                    const uint32_t v = reinterpret_cast<const U32u *>(q + 64 * u)->v & 0xffffffu, b0 = v & 255u;
                    h[u] = hash_of(v);
                    s1 += b0; s2 += (n - (T * kS4TurnPos + 64 * u + lane)) * b0;
                }
                return;
            }
#pragma unroll
            for (uint32_t u = 0; u < kS4TurnSteps; u++) {
                const uint32_t p = T * kS4TurnPos + 64 * u + lane, v = p < npos ? bytes3(p) : 0u;
                h[u] = p < npos ? hash_of(v) : kNone32;
                if (nout && p < npos && excl_has(g, lo + p)) h[u] = kNone32;
                s1 += v & 255u; s2 += (n - p) * (v & 255u);
            }
        };
#pragma unroll
        for (uint32_t j = 0; j < kTurnsPerWave; j++)
#pragma unroll
            for (uint32_t u = 0; u < kS4TurnSteps; u++) pk[j][u] = kNone32;
        if (wave < nturns) preload(wave, pk[0]);
#pragma unroll
        for (uint32_t j = 0; j < kTurnsPerWave; j++) {
            const uint32_t T = wave + j * kS4Waves;
            __builtin_amdgcn_sched_barrier(0);
            if (T < nturns) { // (uniform)
                uint32_t aa[kS4TurnSteps], vv[kS4TurnSteps], old[kS4TurnSteps]; // nothing but the atomics happens while the token is held
#pragma unroll
                for (uint32_t u = 0; u < kS4TurnSteps; u++) {
                    const bool ok = pk[j][u] != kNone32;
                    aa[u] = cnt_a + (ok ? (pk[j][u] >> 1) << 2 : 0);
                    vv[u] = ok ? 1u << ((pk[j][u] & 1u) << 4) : 0; // adding 0 is harmless
                }
                S_TOK(while (lds_ld32(tok_a) != T) __builtin_amdgcn_s_sleep(1));
                S_A0();
#pragma unroll
                for (uint32_t u = 0; u < kS4TurnSteps; u++) old[u] = lds_add_rtn32_nowait(aa[u], vv[u]);
                lds_st32(tok_a, T + 1);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(old[0]), "+v"(old[1]), "+v"(old[2]), "+v"(old[3]), "+v"(old[4]), "+v"(old[5]), "+v"(old[6]), "+v"(old[7])::"memory");
                S_A1();
                static_assert(kS4TurnSteps == 8, "the wait names eight results");
#pragma unroll
                for (uint32_t u = 0; u < kS4TurnSteps; u++)
                    if (pk[j][u] != kNone32) pk[j][u] |= ((old[u] >> ((pk[j][u] & 1u) << 4)) & 0xffffu) << 16;
                if (j + 1 < kTurnsPerWave && T + kS4Waves < nturns) preload(T + kS4Waves, pk[j + 1 < kTurnsPerWave ? j + 1 : j]);
            }
        }
        uint64_t t2 = s2;
        for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o); t2 += __shfl_down(t2, o); }
        if (lane == 0) { ad1[wave] = s1; ad2[wave] = t2; }
    }
    __syncthreads();
    S_T(1);
    if (tid == 0) { // A = 1 + sum b_i, B = n + sum (n - i) b_i (mod 65521); the last two bytes start no three-byte string and are added here
        uint64_t a = 1, b = n;
        for (uint32_t w = 0; w < kS4Waves; w++) { a += ad1[w]; b += ad2[w] % 65521u; }
        for (uint32_t p = npos; p < n; p++) { a += src[p]; b += (uint64_t)(n - p) * src[p]; }
        ChunkMeta &mc = meta[chunk_of(g, c)];
        mc.adler_a = (uint32_t)(a % 65521u); mc.adler_b = (uint32_t)(b % 65521u); mc.in_bytes = n;
    }

    // ---- pass B: exclusive scan of the 32768 counts -> bucket starts (in place) ----
    {
        constexpr uint32_t per = kHashSize / kS4Threads, nv = per * 2 / 16; // counts and 16-byte vectors per lane
        static_assert(per % 8 == 0, "a lane scans whole 16-byte vectors");
        uint4 *c4 = reinterpret_cast<uint4 *>(cnt) + tid * nv;
        uint32_t v[nv * 4], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < nv; i++) { const uint4 q = c4[i]; v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w; }
#pragma unroll
        for (uint32_t i = 0; i < nv * 4; i++) sum += (v[i] & 0xffffu) + (v[i] >> 16);
        uint32_t x = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if ((int)lane >= d) x += y; }
        if (lane == 63) wave_tot[wave] = x;
        __syncthreads();
        uint32_t basev = x - sum;
        for (uint32_t w = 0; w < wave; w++) basev += wave_tot[w];
#pragma unroll
        for (uint32_t i = 0; i < nv * 4; i++) {
            const uint32_t c0 = v[i] & 0xffffu, c1 = v[i] >> 16;
            v[i] = (basev & 0xffffu) | ((basev + c0) << 16);
            basev += c0 + c1;
        }
#pragma unroll
        for (uint32_t i = 0; i < nv; i++) c4[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    }
    __syncthreads();
    S_T(3);

    // ---- pass C0: idx(p) = start(hash) + rank: the position's ir word, written and kept; a bit per bucket head ----
    const uint16_t *start = reinterpret_cast<const uint16_t *>(cnt);
#pragma unroll
    for (uint32_t j = 0; j < kTurnsPerWave; j++) {
        const uint32_t T = __builtin_amdgcn_readfirstlane(wave + j * kS4Waves);
        __builtin_amdgcn_sched_barrier(0); // one turn's eight at a time: all 64 in flight do not fit the registers
        if (T < nturns && whole_turn(T)) { // (scalar) every position has a rank: no lane masks
            uint32_t *irp = ir + T * kS4TurnPos + lane;
#pragma unroll
            for (uint32_t u = 0; u < kS4TurnSteps; u++) {
                const uint32_t r = pk[j][u] >> 16, id = (uint32_t)start[pk[j][u] & 0x7fffu] + r;
                pk[j][u] = id | (r << 16);
                irp[64 * u] = pk[j][u];
                if (r == 0) atomicOr(&heads[id >> 5], 1u << (id & 31u));
            }
        } else if (T < nturns) {
#pragma unroll
            for (uint32_t u = 0; u < kS4TurnSteps; u++) {
                const uint32_t p = T * kS4TurnPos + 64 * u + lane;
                if (pk[j][u] != kNone32) {
                    const uint32_t r = pk[j][u] >> 16, id = (uint32_t)start[pk[j][u] & 0x7fffu] + r;
                    pk[j][u] = id | (r << 16);
                    ir[p] = pk[j][u];
                    if (r == 0) atomicOr(&heads[id >> 5], 1u << (id & 31u));
                }
            }
        }
    }
    __syncthreads();
    S_T(4);
    for (uint32_t i = tid; i < kChunkMax / 32; i += kS4Threads) hd[i] = heads[i];
    reinterpret_cast<uint16_t *>(hd + kHeadWords)[tid] = (uint16_t)heads_below(reinterpret_cast<const unsigned long long *>(heads)[tid], tid, wave_tot);
    S_T(5);

    // ---- pass C1: the scatter through LDS, half of S at a time, and pass V, the self-check ----
    uint16_t *stage = reinterpret_cast<uint16_t *>(cnt);
    bool bad = false;
    for (uint32_t half = 0; half < 2 && half * 32768u < nin; half++) {
        __syncthreads(); // the table (pass C0), or the previous half's write-out, is done with this memory
#pragma unroll
        for (uint32_t j = 0; j < kTurnsPerWave; j++) {
            const uint32_t T = wave + j * kS4Waves;
            __builtin_amdgcn_sched_barrier(0);
            if (T < nturns) {
#pragma unroll
                for (uint32_t u = 0; u < kS4TurnSteps; u++) {
                    asm volatile("" : "+v"(pk[j][u])); // (nothing derived from it is kept across the two halves: there are no registers for that)
                    if (pk[j][u] != kNone32 && ((pk[j][u] >> 15) & 1u) == half) stage[pk[j][u] & 32767u] = (uint16_t)(T * kS4TurnPos + 64 * u + lane);
                }
            }
        }
        __syncthreads();
        const uint32_t cntH = nin - half * 32768u < 32768u ? nin - half * 32768u : 32768u; // entries of this half
        for (uint32_t v = tid; v * 8 < cntH; v += kS4Threads) { // 8 entries = 16 bytes per lane and step
            const uint4 q = reinterpret_cast<const uint4 *>(stage)[v];
            *reinterpret_cast<uint4 *>(S + half * 32768u + v * 8) = q; // S is 16-byte aligned (kSPad); the tail past nin is don't-care
            // pass V: inside a bucket the positions must ascend (the lane order of the LDS atomic, see above)
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            const uint32_t hb = (heads[(half * 32768u + v * 8) >> 5] >> ((v * 8) & 31u)) & 0xffu;
            uint32_t prev = v ? stage[v * 8 - 1] : (half ? last_of_half0 : 0);
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                const uint32_t cur = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
                if (v * 8 + k < cntH && !((hb >> k) & 1u) && prev >= cur) bad = true;
                prev = cur;
            }
        }
        if (half == 0 && nin > 32768u) { __syncthreads(); last_of_half0 = stage[32767]; } // (uniform branch)
    }
    if (bad) atomicOr(fault, 1u);
    S_T(6);
    S_TEND();
}

// The sort of a batch of chunks or tiles: sort4_kernel, or -- `exact_sort` (the engine sets it after pass V has reported a fault) or ZGPU_SORT=1 --
// the ballot-only sort_kernel + heads_below_kernel.  Returns true when the sort has left the chunks' Adler-32 in meta[] (sort4_kernel does; the
// ballot-only sort does not).
bool launch_sort(const ChunkGeom &g, const SortedWs &ws, ChunkMeta *meta, hipStream_t st, zgpu_engine *prof, int exact_sort)
{
    static int sort_env = -1;
    if (sort_env < 0) { const char *e = getenv("ZGPU_SORT"); sort_env = e ? atoi(e) : 4; } // 4: sort4_kernel, 1: the ballot-ranked sort
    const bool exact = exact_sort || sort_env == 1;
    hipEvent_t ev{};
    prof_span_begin(prof, st, &ev);
    if (exact) {
        if (geom_rows(g)) hipLaunchKernelGGL(sort_kernel<true>, dim3(g.nchunks), dim3(kSortThreads), 0, st, g, ws.S, ws.rk, ws.heads, ws.ir);
        else hipLaunchKernelGGL(sort_kernel<false>, dim3(g.nchunks), dim3(kSortThreads), 0, st, g, ws.S, ws.rk, ws.heads, ws.ir);
        hipLaunchKernelGGL(heads_below_kernel, dim3(g.nchunks), dim3(1024), 0, st, ws.heads);
    } else {
        if (geom_rows(g)) hipLaunchKernelGGL(sort4_kernel<true>, dim3(g.nchunks), dim3(kS4Threads), 0, st, g, ws.S, ws.heads, ws.fault, ws.ir, meta);
        else hipLaunchKernelGGL(sort4_kernel<false>, dim3(g.nchunks), dim3(kS4Threads), 0, st, g, ws.S, ws.heads, ws.fault, ws.ir, meta);
        if (g_inject_sort_fault.exchange(0)) hipMemsetAsync(ws.fault, 1, 4, st); // zgpu_debug_inject_sort_fault(): exercise the engine's fallback without a real fault
    }
    prof_span_end(prof, st, ZGPU_STAGE_CHAIN, ev);
    return !exact;
}

} // namespace zgpu
