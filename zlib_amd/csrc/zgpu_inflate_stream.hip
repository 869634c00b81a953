// zgpu_inflate_stream.hip -- streams that carry no side table: split at their flush markers, or (a stream that was not produced in chunks) decoded in
// pieces from block starts a finder believes in; the one-workgroup decoder (inflate_run, zgpu_inflate.hip) is the fallback whose verdicts stand.
#include "zgpu_common.h"
#include "zgpu_engine.h"
#include "zgpu_inflate_dev.h"
#include "../../include/zamd_gpu.h"
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <vector>

static std::atomic<uint64_t> g_spec_done{0}, g_whole_done{0};
namespace zgpu {
// ---- chunk boundaries of a stream that carries no side table: every full-flush marker 00 00 FF FF ends a segment ----
__global__ void __launch_bounds__(256) marker_scan_kernel(const uint8_t *__restrict__ in, uint64_t n, uint64_t *cand, uint32_t cap, uint32_t *count)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 4 <= n; i += stride) {
        if (in[i] == 0 && in[i + 1] == 0 && in[i + 2] == 0xFF && in[i + 3] == 0xFF) {
            const uint32_t k = atomicAdd(count, 1u);
            if (k < cap) cand[k] = i + 4;
        }
    }
}

// ======================================================================================================================================
// A stream that was not produced in chunks (any other zlib's output), decoded in pieces all the same.
//   1. spec_find_kernel: behind every `spacing` bytes of the input, the first bit offset that reads as the header of a dynamic block the
//      decoder would accept (type bits, counts in range, a complete code-length code -- checked by every lane for its own offset --, then
//      the code lengths and the two codes through the decoder's own dynamic_header()).  Such a header at a wrong offset is possible
//      but rare; step 3 finds out.
//   2. inflate_kernel_t<true>: one workgroup per piece, from its start to the first block boundary at or behind the next piece's start,
//      into 16-bit symbols: a byte, or a marker for "byte j of the 32 KiB in front of this piece".
//   3. the host checks the chain: every piece must have ended exactly where the next one started, the last with the final block.  Anything
//      else (a false start, damaged data, input that stops early) and the stream goes to the one-workgroup decoder, whose verdicts stand.
//   4. spec_window_kernel: piece by piece, the last 32 KiB of output with the markers replaced (the only serial step: 32 K look-ups each);
//      spec_resolve_kernel: every page of symbols to its place in the output, markers looked up in the window of the piece in front.
// ======================================================================================================================================
// The block finder's third sieve, one candidate per lane: do the code lengths behind the header at bit `cb` (its three type bits included) describe
// a literal/length and a distance code inflate_table would accept (inftrees.c:106-138), with a code for the end of the block?  Everything a lane
// needs is its own: the bits come from global memory, the code-length code is decoded canonically (counts per length, symbols in
// (length, symbol) order in 19 bytes of LDS), the lengths are summed as they are read.  A yes is confirmed by the decoder's own parse.
__device__ inline bool lane_header_ok(const uint32_t *__restrict__ g32, uint64_t gdwords, uint64_t cb, uint64_t total_bits, uint8_t *sorted)
{
    auto bits33 = [&](uint64_t p) -> uint64_t { // the 33 bits (at least) at absolute bit p
        const uint64_t wi = p >> 5;
        const uint32_t w0 = wi < gdwords ? g32[wi] : 0u, w1 = wi + 1 < gdwords ? g32[wi + 1] : 0u;
        return ((((uint64_t)w1) << 32) | w0) >> (p & 31u);
    };
    uint64_t p = cb + 3;
    if (p + 14 + 57 > total_bits) return false;
    const uint32_t hdr = (uint32_t)bits33(p) & 0x3fffu; p += 14;
    const uint32_t nlen = (hdr & 31u) + 257, ndist = ((hdr >> 5) & 31u) + 1, ncode = (hdr >> 10) + 4;
    if (nlen > 286 || ndist > 30) return false;
    const uint64_t y = (bits33(p) & 0x3fffffffull) | ((bits33(p + 30) & 0x7ffffffull) << 30);
    p += 3 * ncode;
    // lengths by symbol (three bits each), counts by length (a byte each)
    constexpr uint32_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint64_t bysym = 0, counts = 0;
#pragma unroll
    for (uint32_t i = 0; i < 19; i++) {
        const uint32_t l = i < ncode ? (uint32_t)(y >> (3 * i)) & 7u : 0u;
        bysym |= (uint64_t)l << (3 * order[i]);
        counts += l ? 1ull << (8 * l) : 0ull;
    }
    uint32_t k = 0;
    for (uint32_t l = 1; l <= 7; l++)
        for (uint32_t sy = 0; sy < 19; sy++) if (((uint32_t)(bysym >> (3 * sy)) & 7u) == l) sorted[k++] = (uint8_t)sy;
    const uint32_t all = nlen + ndist;
    uint32_t have = 0, prev = 0, kl = 0, kd = 0, eob = 0, big = 0; // big: bit 0 a literal/length code longer than one bit, bit 1 a distance code
    while (have < all) {
        if (p + 14 > total_bits) return false;
        uint32_t w = (uint32_t)bits33(p);
        uint32_t code = 0, first = 0, index = 0, sym = 0xffu, len = 1;
        for (; len <= 7; len++) {
            code |= w & 1u; w >>= 1;
            const uint32_t cnt = (uint32_t)(counts >> (8 * len)) & 255u;
            if (code < first + cnt) { sym = sorted[index + code - first]; break; }
            index += cnt; first = (first + cnt) << 1; code <<= 1;
        }
        if (sym == 0xffu) return false;
        p += len;
        uint32_t rep = 1, val = sym;
        if (sym >= 16) {
            if (sym == 16) { if (have == 0) return false; val = prev; rep = 3 + (w & 3u); p += 2; }
            else if (sym == 17) { val = 0; rep = 3 + (w & 7u); p += 3; }
            else { val = 0; rep = 11 + (w & 127u); p += 7; }
            if (have + rep > all) return false;
        }
        if (val) {
            const uint32_t inl = have >= nlen ? 0u : (have + rep <= nlen ? rep : nlen - have), unit = 32768u >> val;
            kl += inl * unit; kd += (rep - inl) * unit;
            if (kl > 32768u || kd > 32768u) return false;
            if (val > 1) big |= (inl ? 1u : 0u) | (rep > inl ? 2u : 0u);
            if (have <= 256 && have + rep > 256) eob = val;
        }
        prev = val; have += rep;
    }
    const bool lit_ok = kl == 32768u || (kl == 16384u && !(big & 1u));
    const bool dist_ok = kd == 32768u || kd == 0u || (kd == 16384u && !(big & 2u));
    return eob != 0 && lit_ok && dist_ok;
}
#ifdef ZGPU_FIND_TIME // debug build only: clock per phase of the block finder, summed over the finders
__device__ unsigned long long find_time[8];
extern "C" __attribute__((visibility("default"))) void zgpu_debug_find_time(unsigned long long *out, int reset)
{
    unsigned long long z[8] = {};
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(find_time), sizeof z);
    if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(find_time), z, sizeof z);
}
#define FT(i) do { const unsigned long long t_ = wall_clock64(); ft[i] += t_ - ftp; ftp = t_; } while (0)
#else
#define FT(i) do { } while (0)
#endif
// table (the finders of MANY streams, zgpu_inflate_batch_pieces.hip): finder blockIdx.x scans bits [lo_bit, hi_bit) of the buffer, lo_bit a multiple of 128,
// and its stream ends at byte `limit`, which stands in for in_bytes in every bound below: a finder never looks past the item it belongs to.
__global__ void __launch_bounds__(64) spec_find_kernel(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t spacing, uint32_t ntargets, uint64_t *found,
                                                       const PieceTarget *__restrict__ table = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    InflateLdsFind &L = *reinterpret_cast<InflateLdsFind *>(lds_raw);
    const uint32_t t = blockIdx.x + 1, lane = threadIdx.x;
    if (t > ntargets) return;
    const uint64_t buf_bytes = in_bytes;
    if (table) { const uint64_t lim = table[t - 1].limit; in_bytes = lim < in_bytes ? lim : in_bytes; }
    const uint64_t total_bits = in_bytes * 8, lo_bit = table ? table[t - 1].lo_bit : (uint64_t)t * spacing * 8;
    const uint64_t hi_raw = table ? table[t - 1].hi_bit : (uint64_t)(t + 1) * spacing * 8;
    const uint64_t hi_bit = hi_raw < total_bits ? hi_raw : total_bits;
    const uint32_t *g32 = reinterpret_cast<const uint32_t *>(in); // (the input buffer is a device allocation: aligned)
    const uint64_t gdwords = (in_bytes + 3) >> 2;
    uint64_t result = ~0ull;
#ifdef ZGPU_FIND_TIME
    unsigned long long ft[8] = {}, ftp = wall_clock64(), nval = 0;
#endif
    // does a dynamic block the decoder would accept start at bit `cand` (its three type bits are not looked at)?
    auto dynamic_at = [&](uint64_t cand) -> bool {
        BitSrc b;
        b.g32 = g32; b.gdwords = gdwords; b.d0 = cand >> 5; b.filled = 0; b.rd = 0; b.hold = 0; b.bits = 0;
        const uint64_t left = total_bits - (cand & ~31ull);
        b.seg_bits = left > 0xFFFF0000ull ? 0xFFFF0000u : (uint32_t)left;
        wave_sync();
        stage_fill(b, L.stage, lane);
        wave_sync();
        prime(b, L.stage);
        refill(b, L.stage); refill(b, L.stage);
        drop(b, (uint32_t)cand & 31u);
        drop(b, 3);
        CodeRows lr{}, dr{};
        const uint32_t err = dynamic_header<true>(L, b, lane, lr, dr);
        wave_sync();
        // (a block needs its end-of-block code; inflate_table does not ask for it, a block start worth trusting does)
        return !err && uni(L.lens[256]) != 0 && consumed_bits(b) <= b.seg_bits;
    };
    // Stored blocks: data that does not compress (an archive of compressed files) arrives in them, full of block headers that are none of this
    // stream's.  The first byte offset B of the region that reads as LEN, ~LEN behind three zero header bits and zero padding, and whose block is
    // followed by a header that holds as well (stored: LEN, ~LEN again; dynamic: as above) is reported too: the host starts a piece AT its LEN and
    // strikes the dynamic "starts" found inside the block's bytes.
    // the candidates that passed the second sieve wait here (a handful per block) until a lane each can read their code lengths
    uint64_t *wait = reinterpret_cast<uint64_t *>(L.tok); // 64 entries
    uint32_t nwait = 0;
    auto settle = [&]() { // third sieve for up to 64 waiting candidates at once, then the decoder's parse for what is left, in order
        const uint64_t cb = lane < nwait ? wait[lane] : 0ull;
        const bool yes = lane < nwait && lane_header_ok(g32, gdwords, cb, total_bits, reinterpret_cast<uint8_t *>(L.ltab) + lane * 20);
        uint64_t mm = __ballot(yes);
        nwait = 0;
        wave_sync();
        while (mm && result == ~0ull) {
            const uint32_t l = (uint32_t)__builtin_ctzll(mm); mm &= mm - 1;
            const uint64_t cand = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(cb >> 32), (int)l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cb, (int)l);
#ifdef ZGPU_FIND_TIME
            nval++;
#endif
            if (dynamic_at(cand)) result = cand;
        }
    };
    uint64_t stored = ~0ull;
    {
        const uint64_t lo_byte = lo_bit >> 3, hi_byte = hi_bit >> 3;
        for (uint64_t o0 = lo_byte; o0 < hi_byte && stored == ~0ull; o0 += 256) {
            const uint64_t o = o0 + lane * 4, wi = o >> 2; // (lo_byte is a multiple of 4096 -- table: of 16, behind its item's first byte --, t >= 1: wi >= 1)
            const uint32_t dp = wi - 1 < gdwords ? g32[wi - 1] : 0u, d0 = wi < gdwords ? g32[wi] : 0u, d1 = wi + 1 < gdwords ? g32[wi + 1] : 0u;
            uint32_t hit = 0, wsel = 0;
#pragma unroll
            for (int k = 3; k >= 0; k--) {
                const uint32_t w = k == 0 ? d0 : __builtin_amdgcn_alignbyte(d1, d0, k), pb = k == 0 ? dp >> 24 : (d0 >> (8 * (k - 1))) & 255u;
                if (((w ^ (w >> 16)) & 0xFFFFu) == 0xFFFFu && (pb >> 5) == 0 && o + k + 4 <= in_bytes && o + k < hi_byte) { hit |= 1u << k; }
            }
            uint64_t m = __ballot(hit != 0);
            while (m && stored == ~0ull) {
                const uint32_t l = (uint32_t)__builtin_ctzll(m); m &= m - 1;
                uint32_t hk = (uint32_t)__builtin_amdgcn_readlane((int)hit, (int)l);
                const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)d0, (int)l), e1 = (uint32_t)__builtin_amdgcn_readlane((int)d1, (int)l);
                while (hk && stored == ~0ull) {
                    const uint32_t k = (uint32_t)__builtin_ctz(hk); hk &= hk - 1;
                    const uint64_t B = o0 + l * 4 + k;
                    const uint32_t len = (uint32_t)((((uint64_t)e1 << 32) | e0) >> (8 * k)) & 0xFFFFu;
                    const uint64_t N = B + 4 + len; // the header behind the block: it begins a byte
                    if (N + 5 > in_bytes) continue;
                    const uint32_t hb = in[N], type = (hb >> 1) & 3u;
                    bool good = false;
                    if (type == 0) good = ((((uint32_t)in[N + 1] | ((uint32_t)in[N + 2] << 8)) ^ ((uint32_t)in[N + 3] | ((uint32_t)in[N + 4] << 8))) & 0xFFFFu) == 0xFFFFu && (hb >> 3) == 0;
                    else if (type == 2) good = dynamic_at(N * 8);
                    if (good) stored = B;
                }
            }
        }
    }
    FT(0); // the stored sieve
    // the bytes to scan come through LDS, kScanBytes at a time
    uint32_t *scan = reinterpret_cast<uint32_t *>(L.out);
    const uint4 *g128 = reinterpret_cast<const uint4 *>(in);
    const uint64_t gvecs = table ? buf_bytes >> 4 : (in_bytes + 15) >> 4; // (the allocation behind `in` is padded: ensure_stage; table: the caller's buffer, whole vectors of it only)
    for (uint64_t blk = lo_bit; blk < hi_bit && result == ~0ull; blk += kScanBytes * 8) {
        wave_sync();
#pragma unroll
        for (uint32_t k = 0; k < kScanBytes / 16 / 64 + 1; k++) {
            const uint32_t v = k * 64 + lane;
            const uint64_t gv = (blk >> 7) + v;
            uint4 q = make_uint4(0, 0, 0, 0);
            if (v <= kScanBytes / 16 && gv < gvecs) q = g128[gv];
            if (v <= kScanBytes / 16) reinterpret_cast<uint4 *>(scan)[v] = q;
        }
        wave_sync();
        const uint64_t blk_hi = blk + kScanBytes * 8 < hi_bit ? blk + kScanBytes * 8 : hi_bit;
        FT(1); // staging
        // Three sieves.  (1) BFINAL 0, BTYPE 2, HLIT <= 29, HDIST <= 29 -- one offset in nine passes -- for 32 offsets per lane at a time, on the 64 bits
        // that start at the lane's first offset: the type bits are ~x & ~(x >> 1) & (x >> 2), a count of 30 or 31 has its upper four bits set; the
        // survivors are listed in LDS in offset order.  (2) whenever 64 are listed (and at the end of the block), one per lane: the code-length
        // code must be complete (inftrees.c:106-138: sum of 2^-len == 1).  (3) what is left, in order, through the decoder's own header parse.
        uint32_t listed = 0;
        uint16_t *list = reinterpret_cast<uint16_t *>(L.out + kScanBytes + 64);
        for (uint64_t base = blk; base < blk_hi + 2048 && result == ~0ull; base += 2048) {
            if (base < blk_hi) {
                const uint32_t rel0 = (uint32_t)(base - blk) + lane * 32, wi = rel0 >> 5;
                const uint64_t x = ((uint64_t)scan[wi + 1] << 32) | scan[wi];
                uint64_t cm = ~x & ~(x >> 1) & (x >> 2) & ~((x >> 4) & (x >> 5) & (x >> 6) & (x >> 7)) & ~((x >> 9) & (x >> 10) & (x >> 11) & (x >> 12)) & 0xFFFFFFFFull;
                const uint64_t left = base + lane * 32 < blk_hi ? blk_hi - (base + lane * 32) : 0; // offsets of this lane inside the block
                if (left < 32) cm &= (1ull << left) - 1;
                const uint32_t cnt = (uint32_t)__builtin_popcountll(cm), incl = wave_prefix_sum(cnt);
                uint32_t at = listed + incl - cnt;
                while (cm) { list[at++] = (uint16_t)(rel0 + (uint32_t)__builtin_ctzll(cm)); cm &= cm - 1; }
                listed += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                if (listed < 64 && base + 2048 < blk_hi) continue;
            }
            FT(2); // sieve 1
            wave_sync();
            uint32_t lhead = 0; // the list is taken from the front, 64 at a time; what is left (fewer than 64) moves down behind the loop
            while (listed && result == ~0ull && (listed >= 64 || base + 2048 >= blk_hi)) {
                const uint32_t take = listed < 64 ? listed : 64;
                const uint32_t rel = lane < take ? list[lhead + lane] : 0u, wi = rel >> 5, sh = rel & 31u;
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; k++) w[k] = scan[wi + k];
                const uint32_t b0 = __builtin_amdgcn_alignbit(w[1], w[0], sh), b1 = __builtin_amdgcn_alignbit(w[2], w[1], sh), b2 = __builtin_amdgcn_alignbit(w[3], w[2], sh);
                const uint32_t ncode = ((b0 >> 13) & 15u) + 4;
                uint64_t y = ((((uint64_t)b1 << 32) | b0) >> 17) | ((uint64_t)b2 << 47);
                y &= (1ull << (3 * ncode)) - 1; // lengths that are not sent are 0
                const uint32_t ylo = (uint32_t)y, ymid = (uint32_t)(y >> 30);
                uint32_t kraft = 0;
#pragma unroll
                for (uint32_t i = 0; i < 10; i++) kraft += (128u >> ((ylo >> (3 * i)) & 7u)) & 127u; // a length of 0 counts nothing
#pragma unroll
                for (uint32_t i = 0; i < 9; i++) kraft += (128u >> ((ymid >> (3 * i)) & 7u)) & 127u;
                const bool ok = lane < take && blk + rel + 17 + 3 * ncode < hi_bit && kraft == 128;
                uint64_t m = __ballot(ok);
                lhead += take; listed -= take;
                FT(3); // sieve 2
                if (m) {
                    const uint32_t add = (uint32_t)__builtin_popcountll(m);
                    if (nwait + add > 64) { settle(); FT(4); }
                    if (ok) wait[nwait + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = blk + rel;
                    nwait += add;
                    wave_sync();
                }
            }
            if (nwait >= 32 || (nwait && base + 2048 >= blk_hi && blk + kScanBytes * 8 >= hi_bit)) { settle(); FT(4); } // (half a wave of them, or the region's last)
            if (lhead) { // fewer than 64 are left: to the front
                const uint32_t moved = lane < listed ? list[lhead + lane] : 0u;
                wave_sync();
                if (lane < listed) list[lane] = (uint16_t)moved;
                wave_sync();
            }
        }
    }
    if (lane == 0) { found[t - 1] = result; found[ntargets + t - 1] = stored; }
#ifdef ZGPU_FIND_TIME
    if (lane == 0) { ft[5] = nval; ft[6] = 1; for (int i = 0; i < 8; i++) if (ft[i]) atomicAdd(&find_time[i], ft[i]); }
#endif
}

// The windows: window[i] = the last 32 KiB of the output up to the end of piece i = piece i's tail with its markers looked up in window[i - 1] -- a
// chain as long as the stream has pieces.  Looking up is associative, so the chain is cut into groups:
//   spec_window_rel_kernel  one workgroup per group: piece by piece, the tail with its markers looked up in the previous RELATIVE window, whose own
//                           markers name bytes of the window in front of the group (kept in place of the tail);
//   spec_window_grp_kernel  one workgroup: group by group, the window behind the group's last piece as bytes (the only chain over the whole stream);
//   spec_window_abs_kernel  one workgroup per piece: its relative window with the markers looked up in the window in front of its group.
// A marker that names a byte in front of the stream's first is found out by spec_resolve_kernel (every produced byte passes there).
__device__ inline void window_barrier() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } // (loads of the next tail stay in flight)
__device__ inline uint4 lookup8(uint4 q, const uint16_t *prev) // eight symbols; markers replaced by prev[index] (a symbol again)
{
    uint32_t ws[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t lo = ws[k] & 0xFFFFu, hi = ws[k] >> 16;
        if (lo & 0x8000u) lo = prev[lo & 0x7FFFu];
        if (hi & 0x8000u) hi = prev[hi & 0x7FFFu];
        ws[k] = lo | (hi << 16);
    }
    return make_uint4(ws[0], ws[1], ws[2], ws[3]);
}
// ranges (the pieces of MANY streams, zgpu_inflate_batch_pieces.hip): workgroup g composes pieces [ranges[g].x, ranges[g].y), the chained pieces of one item --
// the composition restarts at every item's first piece, in front of which nothing lies, so an item's relative windows are its windows already and
// spec_window_abs_kernel, given one entry of zeros for all (group = 0), only turns them into bytes.  spec_window_grp_kernel has nothing to do there.
// Termination: one step per piece of the range, which the chain kernel bounds by the item's slots.
__global__ void __launch_bounds__(1024) spec_window_rel_kernel(uint16_t *tails, uint32_t nseg, uint32_t group, const uint2 *__restrict__ ranges = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    uint16_t *win = reinterpret_cast<uint16_t *>(lds_raw); // two windows of kOutRing symbols
    const uint32_t tid = threadIdx.x, first = ranges ? ranges[blockIdx.x].x : blockIdx.x * group;
    const uint32_t last_raw = ranges ? ranges[blockIdx.x].y : first + group, last = last_raw < nseg ? last_raw : nseg;
    if (first >= last) return;
    constexpr uint32_t kPer = kOutRing / 8 / 1024;
    uint4 nxt[kPer];
#pragma unroll
    for (uint32_t r = 0; r < kPer; r++) nxt[r] = reinterpret_cast<const uint4 *>(tails + (uint64_t)first * kOutRing)[r * 1024 + tid];
    for (uint32_t i = first; i < last; i++) {
        const uint16_t *prev = win + ((i + 1) & 1) * kOutRing;
        uint16_t *cur = win + (i & 1) * kOutRing;
        uint4 q4[kPer];
#pragma unroll
        for (uint32_t r = 0; r < kPer; r++) q4[r] = nxt[r];
        if (i + 1 < last) {
#pragma unroll
            for (uint32_t r = 0; r < kPer; r++) nxt[r] = reinterpret_cast<const uint4 *>(tails + (uint64_t)(i + 1) * kOutRing)[r * 1024 + tid];
        }
#pragma unroll
        for (uint32_t r = 0; r < kPer; r++) {
            const uint4 o = i == first ? q4[r] : lookup8(q4[r], prev); // (the group's first piece is relative to the window in front of the group as it is)
            reinterpret_cast<uint4 *>(cur)[r * 1024 + tid] = o;
            if (i != first) reinterpret_cast<uint4 *>(tails + (uint64_t)i * kOutRing)[r * 1024 + tid] = o;
        }
        window_barrier();
    }
}
__global__ void __launch_bounds__(1024) spec_window_grp_kernel(const uint16_t *__restrict__ tails, uint32_t nseg, uint32_t group, uint8_t *__restrict__ entry)
{
    // entry[g] = the window in front of group g, as bytes (group 0: nothing is known, and nothing valid refers to it)
    __shared__ uint16_t win[2][kOutRing]; // bytes, kept as symbols so that lookup8 serves
    const uint32_t tid = threadIdx.x, ngroups = (nseg + group - 1) / group;
    constexpr uint32_t kPer = kOutRing / 8 / 1024;
    for (uint32_t r = 0; r < kPer; r++) reinterpret_cast<uint4 *>(win[1])[r * 1024 + tid] = make_uint4(0, 0, 0, 0);
    for (uint32_t r = tid; r < kOutRing / 16; r += 1024) reinterpret_cast<uint4 *>(entry)[r] = make_uint4(0, 0, 0, 0);
    window_barrier();
    uint4 nxt[kPer];
    auto last_of = [&](uint32_t g) { return (g + 1) * group < nseg ? (g + 1) * group - 1 : nseg - 1; };
#pragma unroll
    for (uint32_t r = 0; r < kPer; r++) nxt[r] = reinterpret_cast<const uint4 *>(tails + (uint64_t)last_of(0) * kOutRing)[r * 1024 + tid];
    for (uint32_t g = 0; g + 1 < ngroups; g++) {
        const uint16_t *prev = win[(g + 1) & 1];
        uint16_t *cur = win[g & 1];
        uint4 q4[kPer];
#pragma unroll
        for (uint32_t r = 0; r < kPer; r++) q4[r] = nxt[r];
        if (g + 2 < ngroups) {
#pragma unroll
            for (uint32_t r = 0; r < kPer; r++) nxt[r] = reinterpret_cast<const uint4 *>(tails + (uint64_t)last_of(g + 1) * kOutRing)[r * 1024 + tid];
        }
#pragma unroll
        for (uint32_t r = 0; r < kPer; r++) {
            uint4 o = lookup8(q4[r], prev);
            o.x &= 0x00FF00FFu; o.y &= 0x00FF00FFu; o.z &= 0x00FF00FFu; o.w &= 0x00FF00FFu; // (what was a marker in group 0's entry is a byte nobody may use)
            reinterpret_cast<uint4 *>(cur)[r * 1024 + tid] = o;
            const uint32_t b0 = (o.x & 255u) | ((o.x >> 8) & 0xFF00u) | ((o.y & 255u) << 16) | ((o.y >> 16) << 24);
            const uint32_t b1 = (o.z & 255u) | ((o.z >> 8) & 0xFF00u) | ((o.w & 255u) << 16) | ((o.w >> 16) << 24);
            reinterpret_cast<uint2 *>(entry + (uint64_t)(g + 1) * kOutRing)[r * 1024 + tid] = make_uint2(b0, b1);
        }
        window_barrier();
    }
}
__global__ void __launch_bounds__(256) spec_window_abs_kernel(const uint16_t *__restrict__ tails, uint32_t nseg, uint32_t group, const uint8_t *__restrict__ entry,
                                                              uint8_t *__restrict__ windows)
{
    const uint32_t i = blockIdx.x;
    if (i >= nseg) return;
    const uint8_t *e = entry + (uint64_t)(group ? i / group : 0u) * kOutRing; // (group 0: one entry for every piece)
    const uint4 *t4 = reinterpret_cast<const uint4 *>(tails + (uint64_t)i * kOutRing);
    for (uint32_t v = threadIdx.x; v < kOutRing / 8; v += 256) {
        const uint4 q = t4[v];
        const uint32_t ws[4] = {q.x, q.y, q.z, q.w};
        uint32_t o8[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t sym = (ws[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
            const uint32_t byte = (sym & 0x8000u) ? e[sym & 0x7FFFu] : (sym & 255u);
            o8[k >> 2] |= byte << ((k & 3) * 8);
        }
        reinterpret_cast<uint2 *>(windows + (uint64_t)i * kOutRing)[v] = make_uint2(o8[0], o8[1]);
    }
}

// One workgroup per page of symbols: to its place in the output, markers through the window of the piece in front.
__global__ void __launch_bounds__(256) spec_resolve_kernel(const uint16_t *__restrict__ mid, const uint64_t *__restrict__ page_owner, uint32_t npages, const SpecEnd *__restrict__ ends,
                                                           uint32_t nseg, const uint8_t *__restrict__ windows, const uint64_t *__restrict__ out_start, uint32_t dict_len,
                                                           uint8_t *__restrict__ out, uint64_t out_cap, uint32_t *flag, const PieceRow *__restrict__ rows = nullptr,
                                                           PieceItem *items = nullptr, const uint32_t *npages_dev = nullptr)
{
    // rows, items (the pieces of MANY streams, zgpu_inflate_batch_pieces.hip): out_start[seg] counts from the first byte of the piece's item, "not the first
    // segment" is "not a first piece", the output ends where the item's range ends, and a marker that reaches in front of the item's first byte sets the
    // item's flag.  Pieces of an item whose chain did not hold, or behind its final block, are left out.  npages_dev: the pages taken, read here.
    const uint32_t pg = blockIdx.x;
    if (npages_dev) npages = npages_dev[0] < npages ? npages_dev[0] : npages;
    if (pg >= npages) return;
    const uint64_t ow = page_owner[pg];
    const uint32_t seg = (uint32_t)(ow >> 32), k = (uint32_t)ow;
    if (seg >= nseg) return; // a piece behind the end of the stream
    bool head = seg == 0;
    uint64_t base = 0;
    if (rows) {
        const uint32_t it = rows[seg].item;
        if (it == kPieceNoItem || !items[it].clean || seg - items[it].slot0 >= items[it].npieces) return;
        head = rows[seg].first != 0; base = items[it].out_lo; out_cap = items[it].out_hi; flag = &items[it].bad;
    }
    const uint32_t len = ends[seg].out_bytes, from = k * kOutHalf;
    if (from >= len) return;
    const uint32_t n = len - from < kOutHalf ? len - from : kOutHalf;
    const uint64_t at = base + out_start[seg] + from;
    const uint64_t have_prev = head ? 0 : out_start[seg] + dict_len;
    const uint32_t vf_prev = have_prev >= kOutRing ? 0u : kOutRing - (uint32_t)have_prev;
    const uint8_t *win = !head ? windows + (uint64_t)(seg - 1) * kOutRing : windows;
    const uint16_t *src = mid + (uint64_t)pg * kOutHalf;
    uint32_t bad = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const uint32_t sym = src[i];
        uint32_t byte = sym & 255u;
        if (sym & 0x8000u) {
            const uint32_t idx = sym & 0x7FFFu;
            if (!head && idx >= vf_prev) byte = win[idx]; else { byte = 0; bad = 1; }
        }
        if (at + i < out_cap) out[at + i] = (uint8_t)byte;
    }
    if (bad) atomicOr(flag, 1u);
}

static void spec_opt_in()
{
    static bool opt_in = false;
    if (opt_in) return;
    hipFuncSetAttribute(reinterpret_cast<const void *>(spec_find_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InflateLdsFind));
    hipFuncSetAttribute(reinterpret_cast<const void *>(spec_window_rel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * kOutRing));
    opt_in = true;
}

// The same kernels over the pieces of many streams (zgpu_inflate_batch_pieces.hip): the finders of a table; the windows of every item's chained pieces and
// every page to its place inside its item's range.  `entry`: kOutRing zeros.
void launch_spec_find_table(const uint8_t *d_in, uint64_t in_bytes, const PieceTarget *table, uint32_t ntargets, uint64_t *found, hipStream_t st)
{
    spec_opt_in();
    if (ntargets) hipLaunchKernelGGL(spec_find_kernel, dim3(ntargets), dim3(64), sizeof(InflateLdsFind), st, d_in, in_bytes, (uint64_t)0, ntargets, found, table);
}
void launch_spec_resolve_items(const SpecArgs &sp, uint32_t nslots, uint32_t nitems, const uint2 *ranges, const uint8_t *entry, uint8_t *windows, const uint64_t *out_start,
                               PieceItem *items, uint8_t *d_out, hipStream_t st)
{
    spec_opt_in();
    if (!nslots || !nitems) return;
    hipLaunchKernelGGL(spec_window_rel_kernel, dim3(nitems), dim3(1024), 4 * kOutRing, st, sp.tails, nslots, 0u, ranges);
    hipLaunchKernelGGL(spec_window_abs_kernel, dim3(nslots), dim3(256), 0, st, sp.tails, nslots, 0u, entry, windows);
    hipLaunchKernelGGL(spec_resolve_kernel, dim3(sp.page_cap), dim3(256), 0, st, sp.mid, sp.page_owner, sp.page_cap, sp.ends, nslots, windows, out_start, 0u, d_out, (uint64_t)0,
                       static_cast<uint32_t *>(nullptr), sp.rows, items, sp.page_count);
}
// the windows alone (the verify form of the piece path: there is nothing to resolve into)
void launch_spec_windows_items(uint16_t *tails, uint32_t nslots, uint32_t nitems, const uint2 *ranges, const uint8_t *entry, uint8_t *windows, hipStream_t st)
{
    spec_opt_in();
    if (!nslots || !nitems) return;
    hipLaunchKernelGGL(spec_window_rel_kernel, dim3(nitems), dim3(1024), 4 * kOutRing, st, tails, nslots, 0u, ranges);
    hipLaunchKernelGGL(spec_window_abs_kernel, dim3(nslots), dim3(256), 0, st, tails, nslots, 0u, entry, windows);
}

// 0: decoded (res complete); 1: not this way (the caller uses the one-workgroup decoder); anything else: an error of the engine
// start_bit (0..7): the deflate data begins at that bit of the first byte (a stream taken up again where an earlier call's last whole piece ended)
static int inflate_spec_run(zgpu_engine *e, const uint8_t *d_in, const uint8_t *h_in, uint64_t in_bytes, uint8_t *d_out, uint64_t out_cap, zgpu_inflate_result *res,
                            hipStream_t st, uint32_t stream_mode, uint32_t start_bit = 0, bool force = false)
{
    // force: whatever the size (a stream that goes on at a bit offset has no other decoder: one piece is one workgroup)
    static long min_bytes = -1;
    if (min_bytes < 0) { const char *v = getenv("ZGPU_SPEC_MIN_BYTES"); min_bytes = v ? atol(v) : 128 * 1024; }
    if ((!force && (long)in_bytes < min_bytes) || in_bytes >= (1ull << 40) || (reinterpret_cast<uintptr_t>(d_in) & 15)) return 1;
    res->adler32 = 1; res->crc32 = 0; res->in_used = in_bytes; res->in_used_bits = 0; res->stream_end = 0; res->incomplete = 0;
    uint64_t spacing = (in_bytes / 4096 + 4095) & ~4095ull;
    if (spacing < 32768) spacing = 32768;
    // the finders stand four times as close as the pieces will be (each scans to the next finder at most; of what they find the host keeps starts
    // at least three quarters of `spacing` apart)
    const uint64_t fspacing = spacing / 4 < 16384 ? 16384 : (spacing / 4 + 4095) & ~4095ull;
    const uint32_t ntargets = (uint32_t)((in_bytes - 1) / fspacing);
    if (ntargets < 3 && !force) return 1;
    if (e->inf_status.reserve(e, (size_t)ntargets * 16 + 64)) return ZGPU_MEM_ERROR;
    uint64_t *d_found = reinterpret_cast<uint64_t *>(e->inf_status.p);
    spec_opt_in();
    hipEvent_t ev{};
    prof_span_begin(e, st, &ev);
    if (ntargets) hipLaunchKernelGGL(spec_find_kernel, dim3(ntargets), dim3(64), sizeof(InflateLdsFind), st, d_in, in_bytes, fspacing, ntargets, d_found);
    std::vector<uint64_t> found(2 * (size_t)ntargets);
    if (ntargets) ZGPU_HIP_CHECK(hipMemcpyAsync(found.data(), d_found, found.size() * 8, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    // starts: bit positions; kind 1 = the LEN of a stored block (a byte position; the block's header bits lie up to 10 bits in front)
    const uint64_t kStoredFlag = 1ull << 62;
    std::vector<uint64_t> starts;
    std::vector<uint8_t> kind;
    {
        // what lies inside a stored block the finders vouch for is data, whatever it looks like
        std::vector<std::pair<uint64_t, uint64_t>> raw; // [first bit, behind the last bit) of stored data
        for (uint32_t i = 0; i < ntargets; i++) {
            const uint64_t B = found[ntargets + i];
            if (B != ~0ull && B + 4 <= in_bytes) raw.emplace_back(B * 8, (B + 4 + ((uint64_t)h_in[B] | ((uint64_t)h_in[B + 1] << 8))) * 8);
        }
        std::vector<std::pair<uint64_t, uint8_t>> all;
        for (uint32_t i = 0; i < ntargets; i++) {
            const uint64_t d = found[i], B = found[ntargets + i];
            if (B != ~0ull) all.emplace_back(B * 8, (uint8_t)1);
            if (d == ~0ull) continue;
            // (raw ascends with the finders; a stored block is at most 64 KiB and the finders stand 16 KiB apart or more: a few entries can reach d)
            size_t q = (size_t)(std::upper_bound(raw.begin(), raw.end(), std::pair<uint64_t, uint64_t>(d, ~(uint64_t)0)) - raw.begin());
            bool inside = false;
            for (int back = 0; back < 8 && q > 0; back++) { q--; inside = inside || (raw[q].first <= d && d < raw[q].second); }
            if (!inside) all.emplace_back(d, (uint8_t)0);
        }
        std::sort(all.begin(), all.end());
        starts.push_back(start_bit); kind.push_back(0);
        for (const auto &c : all)
            if (c.first >= starts.back() + spacing * 6 && c.first + spacing * 2 < in_bytes * 8) { starts.push_back(c.first); kind.push_back(c.second); }
        starts.push_back(in_bytes * 8); kind.push_back(0);
    }
    uint32_t nseg = (uint32_t)starts.size() - 1;
    // does the piece that ended at bit `eb` hand over to start j?
    auto links = [&](uint64_t eb, size_t j) -> bool {
        if (!kind[j]) return eb == starts[j];
        if (eb + 3 > starts[j] || eb + 10 < starts[j]) return false;
        for (uint64_t q = eb; q < starts[j]; q++) if ((h_in[q >> 3] >> (q & 7)) & 1u) return false; // BFINAL 0, stored, padding of zeros
        return true;
    };
    static const bool dbg = getenv("ZGPU_SPEC_DEBUG") != nullptr;
    if (dbg) {
        fprintf(stderr, "[spec] %llu bytes, spacing %llu, %u targets, %u pieces; first starts:", (unsigned long long)in_bytes, (unsigned long long)spacing, ntargets, nseg);
        for (uint32_t i = 0; i < nseg && i < 6; i++) fprintf(stderr, " %llu", (unsigned long long)starts[i]);
        fprintf(stderr, "\n");
    }
    if (nseg < 3 && !force) { prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev); return 1; }
    // pages: what the output can hold, or -- when the caller's buffer is far larger than this stream can fill -- eight times the input first
    uint64_t guess = in_bytes * 8 + (16u << 20);
    int repairs = 0;
    for (int attempt = 0;;) {
        const uint64_t room = out_cap < guess ? out_cap : guess;
        const uint64_t pages64 = room / kOutHalf + nseg + 2;
        if (pages64 >= 0xFFFFFFFFull) { prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev); return 1; }
        const uint32_t page_cap = (uint32_t)pages64;
        // one allocation: starts | ends | out_start | status | counters | page owners | windows | tails | pages
        Carve carve;
        const size_t o_starts = carve((size_t)(nseg + 1) * 8), o_ends = carve((size_t)nseg * sizeof(SpecEnd)), o_ostart = carve((size_t)(nseg + 1) * 8),
                     o_status = carve((size_t)nseg * sizeof(InfStatus)), o_cnt = carve(64), o_owner = carve((size_t)page_cap * 8),
                     o_win = carve((size_t)nseg * kOutRing), o_entry = carve((size_t)(nseg / 8 + 2) * kOutRing), o_tails = carve((size_t)nseg * kOutRing * 2), o_mid = carve((size_t)page_cap * kOutHalf * 2);
        uint8_t *base = e->inf_slots.reserve(nullptr, carve.off) ? nullptr : e->inf_slots.p; // (declining is no error: no error text)
        if (!base) { prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev); return 1; } // (no room for the symbols: the slow way needs none)
        uint64_t *d_starts = reinterpret_cast<uint64_t *>(base + o_starts), *d_ostart = reinterpret_cast<uint64_t *>(base + o_ostart);
        SpecEnd *d_ends = reinterpret_cast<SpecEnd *>(base + o_ends);
        uint32_t *d_cnt = reinterpret_cast<uint32_t *>(base + o_cnt);
        SpecArgs sp{};
        sp.mid = reinterpret_cast<uint16_t *>(base + o_mid); sp.page_owner = reinterpret_cast<uint64_t *>(base + o_owner); sp.page_count = d_cnt; sp.page_cap = page_cap;
        sp.tails = reinterpret_cast<uint16_t *>(base + o_tails); sp.ends = d_ends;
        std::vector<uint64_t> up(starts);
        for (size_t i = 0; i < up.size(); i++) if (kind[i]) up[i] |= kStoredFlag;
        ZGPU_HIP_CHECK(hipMemcpy(d_starts, up.data(), (size_t)(nseg + 1) * 8, hipMemcpyHostToDevice));
        ZGPU_HIP_CHECK(hipMemsetAsync(d_cnt, 0, 64, st));
        ZGPU_HIP_CHECK(hipMemsetAsync(d_ends, 0xFF, (size_t)nseg * sizeof(SpecEnd), st));
        InfLaunch a{d_in, in_bytes, d_starts, 0, nseg, d_out, out_cap, reinterpret_cast<InfStatus *>(base + o_status)};
        a.dict = e->inf_dict.p; a.dict_len = e->inf_dict_len;
        launch_inflate_decode(kInfPieces, kInfNoRing, a, sp, st);
        ZGPU_HIP_CHECK(hipGetLastError());
        std::vector<SpecEnd> ends(nseg);
        uint32_t cnt[2] = {0, 0};
        ZGPU_HIP_CHECK(hipMemcpyAsync(ends.data(), d_ends, (size_t)nseg * sizeof(SpecEnd), hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipMemcpyAsync(cnt, d_cnt, 8, hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        // the chain
        uint32_t used_seg = 0; uint64_t total = 0; bool ended = false, dry = false;
        for (uint32_t i = 0; i < nseg; i++) {
            if (ends[i].flags >> 8) break;               // an error (or never written)
            total += ends[i].out_bytes; used_seg = i + 1; dry = dry || (ends[i].flags & 2u);
            if (ends[i].flags & 1u) { ended = true; break; }
            if (i + 1 == nseg || !links(ends[i].end_bit, i + 1)) break;
        }
        // A piece that ran past the next start (or several): those were no block starts -- a deflate stream inside a stored block looks like one, and so
        // does one pattern in 10^9 or so.  Every piece on the chain so far began at a real boundary, so where the last one ended is one too: the false starts go,
        // that boundary becomes a start unless it is one, and the pieces are decoded again (three times at most; then the one-workgroup decoder).
        if (!ended && used_seg >= 1 && used_seg < nseg && !(ends[used_seg - 1].flags >> 8) && !links(ends[used_seg - 1].end_bit, used_seg) && repairs < 3) {
            std::vector<uint64_t> fixed(starts.begin(), starts.begin() + used_seg);
            std::vector<uint8_t> fkind(kind.begin(), kind.begin() + used_seg);
            uint32_t i = used_seg - 1;
            for (;;) { // follow the chain as far as it goes over the starts that are real
                const uint64_t eb = ends[i].end_bit;
                if (eb >= in_bytes * 8) break;
                const uint32_t j = (uint32_t)(std::lower_bound(starts.begin() + i + 1, starts.begin() + nseg, eb) - starts.begin());
                if (j < nseg && links(eb, j) && !(ends[j].flags >> 8) && !(ends[j].flags & 1u)) { fixed.push_back(starts[j]); fkind.push_back(kind[j]); i = j; continue; }
                fixed.push_back(eb); fkind.push_back(0);
                for (uint32_t k = j; k < nseg; k++) if (starts[k] > eb + 10) { fixed.push_back(starts[k]); fkind.push_back(kind[k]); } // (unchecked from here on)
                break;
            }
            if (dbg) fprintf(stderr, "[spec] chain broke behind piece %u (end %llu, next start %llu): %u pieces -> %zu, decoding again\n", used_seg - 1,
                             (unsigned long long)ends[used_seg - 1].end_bit, (unsigned long long)starts[used_seg], nseg, fixed.size());
            fixed.push_back(in_bytes * 8); fkind.push_back(0);
            starts.swap(fixed); kind.swap(fkind);
            nseg = (uint32_t)starts.size() - 1;
            repairs++;
            if (nseg < 2 && !force) { prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev); return 1; }
            continue;
        }
        // stream mode, every piece chained and the last one ran out of input inside a block: the stream is not all there yet, and the pieces in front
        // of the last one are delivered -- they end at a block boundary (a bit position), where the next call takes the stream up again with their last
        // 32 KiB as its window (inflate.c:323-371 updatewindow)
        const bool partial = !ended && stream_mode && used_seg >= 1 && used_seg + 1 == nseg && (ends[nseg - 1].flags >> 8) == kMsgTruncated && links(ends[used_seg - 1].end_bit, used_seg);
        const uint64_t end_bit = used_seg ? ends[used_seg - 1].end_bit : 0;
        const uint64_t end_byte = ended ? (end_bit + 7) >> 3 : partial ? end_bit >> 3 : 0;
        if (dbg) {
            fprintf(stderr, "[spec] chain: %u of %u pieces, ended %d, total %llu, pages %u of %u, dry %d\n", used_seg, nseg, (int)ended, (unsigned long long)total, cnt[0], page_cap, (int)dry);
            for (uint32_t i = used_seg ? used_seg - 1 : 0; i < nseg && i < used_seg + 2; i++)
                fprintf(stderr, "[spec]   piece %u: start %llu end %llu next %llu out %u flags %#x\n", i, (unsigned long long)starts[i], (unsigned long long)ends[i].end_bit,
                        (unsigned long long)starts[i + 1], ends[i].out_bytes, ends[i].flags);
        }
        if (!(ended || partial) || (!stream_mode && end_byte != in_bytes)) { prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev); return 1; }
        if (total > out_cap) {
            prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev);
            res->out_bytes = total; res->first_bad_chunk = -1; res->error_code = ZGPU_BUF_ERROR; res->error_msg = 0;
            collect_spans(e);
            return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
        }
        if (dry) { // the pool was sized from the guess: now the size is known
            if (attempt) { prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev); return 1; }
            guess = total + kOutHalf;
            attempt++;
            continue;
        }
        const uint32_t npages = cnt[0] < page_cap ? cnt[0] : page_cap;
        {
            std::vector<uint64_t> ostart(used_seg + 1);
            uint64_t pos = 0;
            for (uint32_t i = 0; i < used_seg; i++) { ostart[i] = pos; pos += ends[i].out_bytes; }
            ostart[used_seg] = pos;
            ZGPU_HIP_CHECK(hipMemcpyAsync(d_ostart, ostart.data(), (size_t)(used_seg + 1) * 8, hipMemcpyHostToDevice, st));
            ZGPU_HIP_CHECK(hipStreamSynchronize(st)); // (ostart is a local)
            uint32_t group = 8;
            while (group * group < used_seg) group++;
            const uint32_t ngroups = (used_seg + group - 1) / group;
            hipLaunchKernelGGL(spec_window_rel_kernel, dim3(ngroups), dim3(1024), 4 * kOutRing, st, sp.tails, used_seg, group);
            hipLaunchKernelGGL(spec_window_grp_kernel, dim3(1), dim3(1024), 0, st, sp.tails, used_seg, group, base + o_entry);
            hipLaunchKernelGGL(spec_window_abs_kernel, dim3(used_seg), dim3(256), 0, st, sp.tails, used_seg, group, base + o_entry, base + o_win);
        }
        if (npages) hipLaunchKernelGGL(spec_resolve_kernel, dim3(npages), dim3(256), 0, st, sp.mid, sp.page_owner, npages, d_ends, used_seg, base + o_win, d_ostart,
                                       e->inf_dict_len, d_out, out_cap, d_cnt + 4);
        ZGPU_HIP_CHECK(hipGetLastError());
        uint32_t flag = 0;
        ZGPU_HIP_CHECK(hipMemcpyAsync(&flag, d_cnt + 4, 4, hipMemcpyDeviceToHost, st));
        prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev);
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        if (dbg) fprintf(stderr, "[spec] resolved %u pages, flag %u\n", npages, flag);
        if (flag) return 1;
        res->out_bytes = total; res->first_bad_chunk = -1; res->error_code = 0; res->error_msg = 0;
        res->in_used = end_byte; res->in_used_bits = partial ? (uint32_t)(end_bit & 7u) : 0u; res->stream_end = (stream_mode && ended) ? 1 : 0; res->incomplete = partial ? 1 : 0;
        g_spec_done++;
        return output_checksums(e, d_out, total, out_cap, res, st);
    }
}
} // namespace zgpu

using namespace zgpu;

// Decode a raw deflate body made of full-flush-separated segments without a side table.  Candidate boundaries are the
// marker positions; a candidate that is not a real boundary (the pattern can occur inside stored or coded data) makes its
// segment fail to decode and is merged away.  On success *offsets_out (optional) receives the validated boundaries.
// flags & ZGPU_INF_STREAM: `in` is the rest of a stream, not a delimited body: it ends where its final block ends (res->in_used,
// res->stream_end) whatever follows, and input that stops inside a block yields the segments before it (res->incomplete).
static int inflate_stream_host(zgpu_engine *e, const void *in, uint64_t in_bytes, uint32_t flags, void *out, uint64_t out_cap, zgpu_inflate_result *res,
                               std::vector<uint64_t> *offsets_out, uint32_t start_bit = 0)
{
    if (!e || !in || !res || in_bytes == 0 || start_bit > 7) return fail(e, ZGPU_STREAM_ERROR, "bad inflate arguments");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const uint32_t stream_mode = (flags & ZGPU_INF_STREAM) ? 1u : 0u;
    if (start_bit) { // the stream goes on inside its first byte (behind the last whole piece of an earlier call): the pieces are the decoder that starts at a bit
        int rc0 = ensure_stage(e, in_bytes + 256, out_cap ? out_cap : 1); // (the input, then the offsets of the fallback below)
        if (rc0) return rc0;
        uint8_t *d_in0 = e->stage_in;
        ZGPU_HIP_CHECK(hipMemcpyAsync(d_in0, in, in_bytes, hipMemcpyHostToDevice, st));
        // (ZGPU_SPEC_DECLINE_AT_BIT=1, tests: the pieces say "not this way" although the stream is whole)
        const int src = getenv("ZGPU_SPEC_DECLINE_AT_BIT") ? 1 : inflate_spec_run(e, d_in0, static_cast<const uint8_t *>(in), in_bytes, e->stage_out, out_cap, res, st, stream_mode, start_bit, true);
        if (src == ZGPU_OK) { if (out && res->out_bytes) ZGPU_HIP_CHECK(hipMemcpy(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost)); return ZGPU_OK; }
        if (src != 1) return src;
        // The pieces do not chain: damage, most likely, or a harmless reason (no scratch room, too many repairs of the chain -- stored blocks full of
        // what reads as headers --, a flag of the resolve pass).  The verdict is the one-workgroup decoder's, started at the same bit of the same bytes.
        // (Not on a copy shifted to bit 0: a stored block aligns to the bytes of the stream, and in the shifted copy it read its LEN from the wrong bits.)
        if (in_bytes >= (1ull << 29)) return fail(e, ZGPU_DATA_ERROR, "stream too long for the one-workgroup decoder");
        const uint64_t h_offs[2] = {0, in_bytes};
        uint64_t *d_offs0 = reinterpret_cast<uint64_t *>(d_in0 + ((in_bytes + 127) & ~63ull));
        ZGPU_HIP_CHECK(hipMemcpyAsync(d_offs0, h_offs, sizeof h_offs, hipMemcpyHostToDevice, st));
        g_whole_done++;
        const int rc2 = inflate_run(e, d_in0, in_bytes, d_offs0, 1, kWholeStream, e->stage_out, out_cap, res, st, stream_mode | (start_bit << 8), h_offs);
        // stream mode: input that stops inside a block is not an error, nothing of it is taken (the stream still goes on at start_bit)
        if (stream_mode && ((rc2 == ZGPU_DATA_ERROR && res->error_msg == kMsgTruncated) || (rc2 == ZGPU_OK && res->incomplete))) {
            res->incomplete = 1; res->in_used = 0; res->in_used_bits = start_bit; res->out_bytes = 0; res->stream_end = 0; return ZGPU_OK;
        }
        if (rc2 != ZGPU_OK) return rc2;
        if (out && res->out_bytes) ZGPU_HIP_CHECK(hipMemcpy(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost));
        return ZGPU_OK;
    }
    const uint64_t max_cand = in_bytes / 5 + 2;
    int rc = ensure_stage(e, in_bytes + 64 + (max_cand + 2) * 2 * sizeof(uint64_t) + 64, out_cap ? out_cap : 1);
    if (rc) return rc;
    uint8_t *d_in = e->stage_in;
    const uint64_t tab_off = (in_bytes + 127) & ~63ull;
    uint64_t *d_cand = reinterpret_cast<uint64_t *>(d_in + tab_off);          // candidates, later the offsets table
    uint64_t *d_offs = d_cand + max_cand + 2;
    if (e->inf_status.reserve(e, 64 * 1024)) return ZGPU_MEM_ERROR;
    uint32_t *d_count = reinterpret_cast<uint32_t *>(e->inf_status.p);
    ZGPU_HIP_CHECK(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, st));
    ZGPU_HIP_CHECK(hipMemsetAsync(d_count, 0, 4, st));
    hipLaunchKernelGGL(marker_scan_kernel, dim3(2048), dim3(256), 0, st, d_in, in_bytes, d_cand, (uint32_t)max_cand, d_count);
    uint32_t ncand = 0;
    ZGPU_HIP_CHECK(hipMemcpyAsync(&ncand, d_count, 4, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    std::vector<uint64_t> b(ncand + 2);
    if (ncand) ZGPU_HIP_CHECK(hipMemcpy(b.data() + 1, d_cand, (size_t)ncand * sizeof(uint64_t), hipMemcpyDeviceToHost));
    b[0] = 0;
    std::sort(b.begin() + 1, b.begin() + 1 + ncand);
    b[ncand + 1] = in_bytes;
    b.erase(std::unique(b.begin(), b.end()), b.end()); // a marker can end exactly at the end of the body
    // A candidate that is not a boundary costs one more pass over the input; streams of other producers (sync-flushed protocols put a
    // marker behind every message and keep the window across it) can hold thousands that are none.  So: a few passes that merge the
    // failing segment into its successor, then -- and at once when a segment fails in the way a kept window looks (a distance that
    // reaches back before the segment, more than 64 KiB of output) -- the stream is decoded from end to end by one workgroup.
    bool whole = false;
    // not one marker in a long body: no chunked stream of this library looks like that -- the pieces are tried at once (the pass below would decode 64 KiB
    // of it, find that the one segment goes on, and come to the same place)
    bool tried_pieces = false;
    if (ncand == 0 && in_bytes >= (1u << 20)) {
        tried_pieces = true;
        const int src = inflate_spec_run(e, d_in, static_cast<const uint8_t *>(in), in_bytes, e->stage_out, out_cap, res, st, stream_mode);
        if (src != 1) {
            if (src != ZGPU_OK) return src;
            if (out && res->out_bytes) ZGPU_HIP_CHECK(hipMemcpy(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost));
            if (offsets_out) *offsets_out = b;
            return ZGPU_OK;
        }
    }
    // stream mode: input that ends with a flush marker may simply be all there is so far -- then the last segment is a segment like the
    // others and none of them has to hold the final block
    const uint8_t *hin = static_cast<const uint8_t *>(in);
    bool open_end = stream_mode && in_bytes >= 4 && hin[in_bytes - 4] == 0 && hin[in_bytes - 3] == 0 && hin[in_bytes - 2] == 0xFF && hin[in_bytes - 1] == 0xFF;
    for (int pass = 0;; pass++) {
        const uint64_t nseg = b.size() - 1;
        ZGPU_HIP_CHECK(hipMemcpyAsync(d_offs, b.data(), b.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        rc = inflate_run(e, d_in, in_bytes, d_offs, nseg, 0, e->stage_out, out_cap, res, st, stream_mode, b.data(), open_end);
        if (rc == ZGPU_OK) break;
        if (rc != ZGPU_DATA_ERROR) return rc;
        const bool last_bad = res->first_bad_chunk >= 0 && (uint64_t)res->first_bad_chunk + 1 == nseg;
        if (open_end && last_bad && res->error_msg == kMsgTruncated) { open_end = false; pass--; continue; } // (the marker was data: an incomplete tail after all)
        if (last_bad && res->error_msg == kMsgTruncated) return rc; // the body stops early (strict mode; stream mode reports it as incomplete)
        const bool window_kept = res->error_msg == kMsgTooFar || res->error_msg == kMsgOutput;
        if (!last_bad && !window_kept && pass < 4) { b.erase(b.begin() + res->first_bad_chunk + 1); continue; } // not a boundary after all
        whole = true;
        break;
    }
    if (whole && !tried_pieces) {
        const int src = inflate_spec_run(e, d_in, hin, in_bytes, e->stage_out, out_cap, res, st, stream_mode);
        if (src != 1 && src != ZGPU_OK) return src;
        whole = src == 1;
        if (!whole) b.assign({0, in_bytes});
    }
    if (whole) {
        if (in_bytes >= (1ull << 29)) return fail(e, ZGPU_DATA_ERROR, "stream too long for the one-workgroup decoder");
        b.assign({0, in_bytes});
        g_whole_done++;
        ZGPU_HIP_CHECK(hipMemcpyAsync(d_offs, b.data(), b.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        rc = inflate_run(e, d_in, in_bytes, d_offs, 1, kWholeStream, e->stage_out, out_cap, res, st, stream_mode, b.data());
        if (rc != ZGPU_OK) {
            // stream mode: input that stops inside a block is not an error, nothing of it is taken (one workgroup cannot hand a window on)
            if (stream_mode && rc == ZGPU_DATA_ERROR && res->error_msg == kMsgTruncated) { res->incomplete = 1; res->in_used = 0; res->out_bytes = 0; res->stream_end = 0; return ZGPU_OK; }
            return rc;
        }
    }
    if (out && res->out_bytes) ZGPU_HIP_CHECK(hipMemcpy(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost));
    if (offsets_out) *offsets_out = b;
    return ZGPU_OK;
}

extern "C" {
#pragma GCC visibility push(default)
uint64_t zgpu_inflate_spec_count(int which) { return which == 0 ? g_spec_done.load() : which == 1 ? g_whole_done.load() : (which == 2 || which == 3) ? batch_pieces_count(which - 2) : (which == 4 || which == 5) ? batch_pieces_sizes_count(which - 4) : (which == 6 || which == 7) ? batch_pieces_verify_count(which - 6) : 0; }
int zgpu_inflate_find_chunks_host(zgpu_engine *e, const void *in, uint64_t in_bytes, uint32_t chunk_size, uint64_t *offsets, uint64_t max_chunks,
                                  uint64_t *nchunks)
{
    (void)chunk_size;
    if (!offsets || !nchunks) return ZGPU_STREAM_ERROR;
    std::vector<uint64_t> b;
    zgpu_inflate_result res{};
    // the staging output is sized from the data (four times the input, more when the decode asks for it), not from the capacity of the
    // caller's table: max_chunks * 64 KiB is 15 GB for the default table of a 1 MiB body
    uint64_t cap = in_bytes * 4 + 65536;
    const uint64_t cap_max = max_chunks * (uint64_t)kChunkMax;
    if (cap > cap_max) cap = cap_max;
    int rc;
    for (;;) {
        rc = inflate_stream_host(e, in, in_bytes, 0, nullptr, cap, &res, &b);
        if (rc != ZGPU_BUF_ERROR || cap >= cap_max) break;
        cap = res.out_bytes > cap ? res.out_bytes : cap * 4;
        if (cap > cap_max) cap = cap_max;
    }
    if (rc) return rc;
    if (b.size() - 1 > max_chunks) return fail(e, ZGPU_BUF_ERROR, "offset table too small");
    for (size_t i = 0; i < b.size(); i++) offsets[i] = b[i];
    *nchunks = b.size() - 1;
    return ZGPU_OK;
}
int zgpu_inflate_stream_host(zgpu_engine *e, const void *in, uint64_t in_bytes, void *out, uint64_t out_cap, zgpu_inflate_result *res)
{
    if (!out) return ZGPU_STREAM_ERROR;
    return inflate_stream_host(e, in, in_bytes, 0, out, out_cap, res, nullptr);
}
int zgpu_inflate_stream_host2(zgpu_engine *e, const void *in, uint64_t in_bytes, uint32_t flags, void *out, uint64_t out_cap, zgpu_inflate_result *res)
{
    if (!out) return ZGPU_STREAM_ERROR;
    return inflate_stream_host(e, in, in_bytes, flags, out, out_cap, res, nullptr);
}
int zgpu_inflate_stream_host3(zgpu_engine *e, const void *in, uint64_t in_bytes, uint32_t start_bit, uint32_t flags, void *out, uint64_t out_cap, zgpu_inflate_result *res)
{
    if (!out) return ZGPU_STREAM_ERROR;
    return inflate_stream_host(e, in, in_bytes, flags, out, out_cap, res, nullptr, start_bit);
}
#pragma GCC visibility pop
}
