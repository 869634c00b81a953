// zgpu_lz_match3.hip -- K2'' match3_kernel, the all-position search of the sorted-bucket LZ77 stage (ZGPU_LZ_SORTED; zgpu_lz_sorted.hip has the map).
#include "zgpu_lz_sorted.h"

namespace zgpu {

// ------------------------------------------------------------------------------------------------- K2''
// Lockstep form of the same search.  A wave takes 64 CONSECUTIVE entries of S (one work item = one block of 64 S
// indices); lane L searches position S[wi], wi = 64*blk + L, and all lanes examine their k-th candidate S[wi-1-k] in the
// same step.  Neighbouring entries of S belong to the same hash bucket, so their chains have (almost) the same length and
// the candidate loads of a step are one contiguous, coalesced run of S.
//
// The full string comparison is taken out of the walk altogether.  longest_match's result has an order-free statement:
// with len(k) = common prefix of the scan string and candidate k (capped by the lookahead), the walk ends at the FIRST k
// with len(k) >= nice_match (deflate.c:1224) and returns that candidate; otherwise it returns the largest len(k), the
// earliest k among equals (deflate.c:1198, strict >).  Both are the maximum of one integer key per candidate:
//       len >= nice :  1<<31 | (4095-k)<<16 | len            len < nice :  len<<16 | (4095-k)
// So a candidate that passes the two-byte quick check (deflate.c:1187-1190) is merely appended to a per-wave ring in LDS,
// and whenever 64 of them have gathered, the 64 lanes compute 64 prefix lengths at full occupancy -- any lane serves any
// owner -- and fold the keys into the owner's slot with an LDS atomic max.  The owners then read their slot back and walk
// on with the new best length.  Walking with a stale (shorter) best length is exact: the quick check against it rejects
// only candidates that match at most that many bytes, which can be neither an improvement nor a nice_match stop; and
// whatever was appended after the stopping candidate loses against its key.  The quarter-budget result (deflate.c:1146)
// is the slot as it stands once every candidate k < chain/4 has been folded.
#ifndef ZGPU_M3_PERIOD
#define ZGPU_M3_PERIOD 128 // steps between forced folds (keeps the walkers' best length fresh); a power of two <= 256
#endif
#ifdef ZGPU_M3_STATS // debug build only (scripts/m3_stats.py): 0 wave-steps, 1 active lane-steps, 2 ring entries, 3 folds, 4 fold iterations, 5 positions
__device__ unsigned long long m3_stats[8];
extern "C" __attribute__((visibility("default"))) void zgpu_debug_m3_stats(unsigned long long *out, int reset)
{
    unsigned long long z[8] = {};
    hipMemcpyFromSymbol(out, HIP_SYMBOL(m3_stats), sizeof z);
    if (reset) hipMemcpyToSymbol(HIP_SYMBOL(m3_stats), z, sizeof z);
}
#define M3_STAT(i, v) do { const unsigned long long v_ = (unsigned long long)(v); if (lane == 0) atomicAdd(&m3_stats[i], v_); } while (0)
#else
#define M3_STAT(i, v) do { } while (0)
#endif
constexpr uint32_t kM2Threads = 1024;
constexpr uint32_t kM3Lds = kM3DataLds + 16 + (kM2Threads / 64) * kM3WaveLds; // (kRing, kM3WaveLds, kM3DataLds: zgpu_lz_sorted.h -- walk_kernel's LDS begins the same way)

__global__ void __launch_bounds__(kM2Threads, 8) match3_kernel(ChunkGeom g, LevelCfg cfg, const uint16_t *__restrict__ S_all, const uint32_t *__restrict__ heads_all,
                                                               uint2 *__restrict__ recs)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *d32 = lds;
    uint32_t *work_next = lds + kM3DataLds / 4; // next unassigned block of S
    const uint8_t *d8 = reinterpret_cast<const uint8_t *>(d32);
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t ring = (uint32_t)__builtin_amdgcn_readfirstlane(lds_off(lds) + kM3DataLds + 16 + wave * kM3WaveLds), slot = ring + kRing * 4, pw = slot + 64 * 4; // LDS byte offsets
    uint64_t lo; uint32_t n;
    chunk_span(g, c, lo, n);
    const uint8_t *src = g.in + lo;
    const uint16_t *S = S_all + (size_t)c * kSStride + kSPad;
    const unsigned long long *hd = reinterpret_cast<const unsigned long long *>(heads_all + (size_t)c * kHeadStride); // bit i: S[i] starts a bucket
    uint2 *rec = recs + (size_t)c * kChunkMax;
    const uint32_t npos = n >= 3 ? n - 2 : 0;
    const uint32_t base = chunk_base(g, c);
    stage_chunk<kM2Threads>(src, n, d32, tid);
    if (tid == 0) *work_next = 0;
    for (uint32_t q2 = npos + tid; q2 < n; q2 += kM2Threads) rec[q2] = make_uint2((uint32_t)src[q2] << 24, 0); // the last two positions carry no hash
    __syncthreads();

    const uint32_t chainF = cfg.chain, chainQ = cfg.chain >> 2, dbase = lds_off(d32), nblk = (npos + 63) >> 6;
    const uint16_t *hb = reinterpret_cast<const uint16_t *>(heads_all + (size_t)c * kHeadStride + kHeadWords); // heads_below per block
    auto grab = [&]() { uint32_t b = 0; if (lane == 0) b = atomicAdd(work_next, 1u); return (uint32_t)__builtin_amdgcn_readfirstlane(b); };
    // the next block's entry, head bits and heads_below are fetched while the current block is searched
    uint32_t blk = grab(), p_nx = 0, below_nx = 0;
    unsigned long long m_nx = 0;
    if (blk < nblk) { const uint32_t wi = (blk << 6) + lane; p_nx = wi < npos ? S[wi] : 0; m_nx = hd[blk]; below_nx = hb[blk]; }
    while (blk < nblk) {
        const uint32_t wi = (blk << 6) + lane;
        const bool valid = wi < npos;
        const uint32_t p = p_nx, below = below_nx;
        const unsigned long long m = m_nx;
        const uint32_t blk_nx = grab();
        if (blk_nx < nblk) { const uint32_t wn = (blk_nx << 6) + lane; p_nx = wn < npos ? S[wn] : 0; m_nx = hd[blk_nx]; below_nx = hb[blk_nx]; }
        uint32_t avail = 0;
        {   // rank of an entry in its bucket = distance from the last bucket head at or below it; only min(rank, chain) matters
            const unsigned long long mine = m & ((2ull << lane) - 1);
            const uint32_t rank = mine ? (uint32_t)__builtin_clzll(mine) - (63 - lane) : lane + below;
            if (valid) avail = rank < chainF ? rank : chainF;
        }
        const int w = (int)(p + base);
        int thr = (w - (int)kMaxDist > 1 ? w - (int)kMaxDist : 1) - (int)base;                 // first candidate: dist <= MAX_DIST, not NIL
        const int thr_next = (w - (int)kMaxDist + 1 > 1 ? w - (int)kMaxDist + 1 : 1) - (int)base; // later ones: strictly inside
        if (cfg.strategy == kRle && thr < (int)p - 1) thr = (int)p - 1; // Z_RLE: the head of the chain counts only at distance 1 (deflate.c:1596)
        uint32_t best = kMinMatch - 1, key_seen = 0, snapkey = 0;
        uint32_t scan2 = (uint32_t)d8[p + 1] | ((uint32_t)d8[p + 2] << 8);
        uint32_t boff = dbase + best - 1;
        unsigned long long amask = mask_gt_u32(avail, 0u); // lanes still walking (wave-uniform)
        bool snap_taken = false;
        const uint16_t *sp = S + wi; // candidate k is sp[-1-k]
        lds_st32(slot + lane * 4, 0);
        lds_st16(pw + lane * 2, p);
        uint32_t tail = 0; // entries on the ring (wave-uniform)
        const uint32_t lanebits = lane << 16, dummy = ring + (kRing - 1) * 4; // (the stack never holds more than 127 entries: its last word is free)
        M3_STAT(5, __popcll(__builtin_amdgcn_ballot_w64(valid)));

        // fold up to 64 ring entries into their owners' slots, then let every owner pick up its new best length
        auto fold = [&](uint32_t kcur) {
            const uint32_t cnt = tail < 64 ? tail : 64;
            M3_STAT(3, 1);
            tail = (uint32_t)__builtin_amdgcn_readfirstlane(tail - cnt); // the ring is a stack: any order of folding gives the same maxima
            if (lane < cnt) {
                const uint32_t e = lds_ld32(ring + ((tail + lane) << 2));
                const uint32_t q = e & 0xffffu, o = (e >> 16) & 63u;
                const uint32_t k = kcur - ((kcur - (e >> 22)) & 1023u);
                const uint32_t po = lds_ld16(pw + o * 2), look = n - po, cap = look < kMaxMatch ? look : kMaxMatch, nice = cfg.nice < look ? cfg.nice : look;
                uint32_t l = 0, x;
                for (;;) {
                    x = lds_ld32u(dbase + q + l) ^ lds_ld32u(dbase + po + l);
                    M3_STAT(4, 1); // (counts only the iterations lane 0 takes part in)
                    if (x != 0 || l + 4 >= cap) break;
                    l += 4;
                }
                uint32_t len = x ? l + ((uint32_t)__builtin_ctz(x) >> 3) : l + 4;
                len = len < cap ? len : cap;
                if (len >= kMinMatch) {
                    const uint32_t key = len >= nice ? (0x80000000u | ((4095u - k) << 16) | len) : ((len << 16) | (4095u - k));
                    lds_max32(slot + o * 4, key);
                }
            }
            const uint32_t key = lds_ld32(slot + lane * 4);
            if (key != key_seen) {
                key_seen = key;
                best = (key >> 31) ? key & 0x1ffu : key >> 16;
                boff = dbase + best - 1;
                scan2 = (uint32_t)d8[p + best - 1] | ((uint32_t)d8[p + best] << 8);
            }
            amask &= ~mask_lt_i32((int)key, 0); // a nice_match key: the walk of that lane is over (deflate.c:1224)
        };

        // four candidates per load, the nearest in the top 16 bits; the index is clamped so that lanes whose walk is over load
        // something harmless instead of being masked off
        // ... and lanes whose walk is over read the zeroed pad in front of S: candidate "position 0" for all of them, so their
        // (unused) quick-check reads fall on a handful of LDS words instead of 64 random ones (the LDS pipe is 80 % busy)
        auto group = [&](uint32_t k0) -> uint64_t {
            int gi = (int)wi - 4 - (int)k0, gsel;
            gi = gi < -(int)kSPad ? -(int)kSPad : gi;
            asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(gsel) : "v"(-(int)kSPad), "v"(gi), "s"(amask));
            return reinterpret_cast<const U64u *>(S + gsel)->v;
        };
        uint64_t cq = group(0);
        uint32_t k = 0;
        // the quarter budget need not be a multiple of the four candidates of a step (deflateTune: max_chain 13 or 100 give 3 and 25): the snapshot is
        // taken in front of candidate chainQ, at the top of step snapK or, for snapJ != 0, between two candidates of it.
        // A quarter of 0 (max_chain 1..3) never comes here: the reference's count-down passes zero there and the search with a good match in hand is
        // unbounded (walk_kernel: budget 0xffff), which a record of at most chainF candidates cannot hold -- plan_deflate (records_refuse) refuses the row,
        // as it does max_lazy > nice_length (the record is made with nothing in hand) and, for this kernel, a max_chain above 4096 (12 bits of a key count the candidates)
        const uint32_t snapK = chainQ & ~3u, snapJ = chainQ & 3u;
        for (;; k += 4) {
            if (amask == 0) break;
            if (k == chainQ) {
                while (tail) fold(k);
                snapkey = key_seen; snap_taken = true;
            } else if ((k & (ZGPU_M3_PERIOD - 1)) == 0) { while (tail) fold(k); }
            const uint64_t cqn = group(k + 4);
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                // no divergent control flow in the step: every lane reads (idle ones a harmless in-range address), masks decide
                const uint32_t q = (uint32_t)(cq >> (48 - 16 * j)) & 0xffffu;
                if (j != 0 && j == snapJ && k == snapK) { // (wave-uniform; entries on the ring are candidates below k + j)
                    while (tail) fold(k + j);
                    snapkey = key_seen; snap_taken = true;
                }
                uint32_t b0, b1;
                lds_ld2bytes(boff + q, b0, b1);
                amask &= mask_le_i32(thr, (int)q); // beyond MAX_DIST (or the NIL position): the chain ends here (deflate.c:1163)
                if (k == 0 && j == 0) thr = thr_next;
                const unsigned long long m = amask & mask_eq_u32(b0 | (b1 << 8), scan2);
                M3_STAT(0, 1); M3_STAT(1, __popcll(amask)); M3_STAT(2, __popcll(m));
                if (m) {
                    stack_push(m, (uint32_t)__builtin_amdgcn_readfirstlane(ring + (tail << 2)), dummy, q | lanebits | ((k + j) << 22));
                    tail = (uint32_t)__builtin_amdgcn_readfirstlane(tail + (uint32_t)__popcll(m));
                    if (tail >= 64) fold(k + j);
                }
                amask &= mask_gt_u32(avail, k + j + 1);
            }
            cq = cqn;
        }
        while (tail) fold(k);
        if (!snap_taken) snapkey = key_seen;
        if (valid) {
            uint32_t full = 0, snap = 0, flags = 0;
            if (key_seen) {
                const uint32_t kb = 4095u - ((key_seen >> 31) ? (key_seen >> 16) & 0xfffu : key_seen & 0xfffu);
                full = best | ((p - (uint32_t)sp[-1 - (int)kb]) << 9);
            }
            if (snapkey) {
                const uint32_t ks = 4095u - ((snapkey >> 31) ? (snapkey >> 16) & 0xfffu : snapkey & 0xfffu);
                const uint32_t sl = (snapkey >> 31) ? snapkey & 0x1ffu : snapkey >> 16;
                snap = sl | ((p - (uint32_t)sp[-1 - (int)ks]) << 9);
            }
            // the one position whose first candidate can sit at window index 32768 (NIL after the slide, deflate.c:1309-1312)
            if (p + base == kWSize + kMaxDist && avail != 0 && (uint32_t)sp[-1] + base == kWSize) flags = 1;
            rec[p] = make_uint2(full | ((uint32_t)d8[p] << 24), snap | (flags << 24));
        }
        blk = blk_nx;
    }
}

void launch_match3(const ChunkGeom &g, LevelCfg cfg, const SortedWs &ws, hipStream_t st)
{
    static bool opt_in3 = false;
    if (!opt_in3) { hipFuncSetAttribute(reinterpret_cast<const void *>(match3_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kM3Lds); opt_in3 = true; }
    hipLaunchKernelGGL(match3_kernel, dim3(g.nchunks), dim3(kM2Threads), kM3Lds, st, g, cfg, ws.S, ws.heads, ws.recs);
}

} // namespace zgpu
