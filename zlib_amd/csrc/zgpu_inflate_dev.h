// zgpu_inflate_dev.h -- internal, device side: what more than one inflate kernel uses -- the decoder (zgpu_inflate.hip) and the block finder
// (zgpu_inflate_stream.hip).  The LDS layouts, the wave-uniform bit reader, the decoding tables and the header of a dynamic block.
#pragma once
#include "zgpu_common.h"

namespace zgpu {

constexpr uint32_t kLBits = 9, kDBits = 9, kStageDwords = 256;
#ifndef ZGPU_INF_RING
#define ZGPU_INF_RING 32768
#endif
#ifndef ZGPU_INF_PARCOPY
#define ZGPU_INF_PARCOPY 1 // the independent matches of a pass copied together (0: one after the other, A/B builds)
#endif
#ifndef ZGPU_INF_RING_DEFAULT_KB
#define ZGPU_INF_RING_DEFAULT_KB 8 // the ring of chunks decoded straight into place (zgpu_inflate_device); ZGPU_INF_RING_KB at run time
#endif
#ifndef ZGPU_INF_SIZES_WAVES
#define ZGPU_INF_SIZES_WAVES 6 // waves per SIMD the sizing pass is compiled for: its LDS lets 24 one-wave workgroups share a CU, six per SIMD (80 registers)
#endif
constexpr uint32_t kOutRing = ZGPU_INF_RING, kOutHalf = kOutRing / 2; // the last 32 KiB of output live in LDS (the farthest a distance reaches)

// Decoding table entries of the literal/length and distance codes carry everything the symbol loop needs:
//   bits 0-3 code length, 4-7 extra bits, 8 literal, 9 end of block, 10 length/distance, 11 invalid symbol, 16-31 byte / base value
constexpr uint32_t kEntLit = 1u << 8, kEntEob = 1u << 9, kEntLen = 1u << 10, kEntBad = 1u << 11;

// RingT: uint8_t, or uint16_t for the speculative decode of a stream's middle (spec_*, zgpu_inflate_stream.hip): values >= 0x8000 are markers, "the byte
// at index v & 0x7fff of the 32 KiB in front of this segment", which nobody knows yet
template <typename RingT, uint32_t kRing = kOutRing> struct InflateLdsT {
    RingT out[kRing];
    uint32_t ltab[1 << kLBits]; // 0 = code longer than kLBits (or unassigned)
    uint32_t dtab[1 << kDBits];
    uint32_t stage[kStageDwords]; // ring of input dwords
    uint32_t tok[128];            // token ring, reader -> writer, handed over in halves of 64
    uint32_t abort_flag, end_bits; // writer -> reader: stop, the output is void; reader -> writer: bits of the segment used when it ended
    uint16_t lens[320];
    uint16_t lsym[288], dsym[32]; // symbols sorted by (length, symbol) for the long-code walk
    uint16_t lcount[16], dcount[16];
    uint16_t work_offs[16], work_first[16], work_start[16];
    uint32_t build_rc, build_n;
    uint32_t end_final, pad1;     // reader -> writer: the segment ended with a final block
};
using InflateLds = InflateLdsT<uint8_t>;
// The sizing pass (inflate_kernel_t<..., SIZES>) keeps what the reader needs and nothing else: no output ring, and no token ring either, because the
// one wave that decodes the tokens also counts them
struct InflateLdsSizes {
    uint32_t ltab[1 << kLBits];
    uint32_t dtab[1 << kDBits];
    uint32_t stage[kStageDwords];
    uint32_t abort_flag, end_bits;
    uint16_t lens[320];
    uint16_t lsym[288], dsym[32];
    uint16_t lcount[16], dcount[16];
    uint16_t work_offs[16], work_first[16], work_start[16];
    uint32_t build_rc, build_n;
    uint32_t end_final, pad1;
};
// The integrity test (inflate_kernel_t<..., VERIFY>): the decoder's layout with the 32 KiB ring, unchanged, and behind it the writer wave's CRC lookup
struct InflateLdsVerify : InflateLdsT<uint8_t, 32768> {
    uint32_t crc_nib[kCrcNibWords]; // eight nibble tables of 16 words (crc_nib_entry, zgpu_common.h)
};
// The fused batch decode (inflate_kernel_t<..., FOLD>): the decoder's layout with the ring the call picks -- the rings BATCH serves -- and the CRC lookup behind it
template <uint32_t kRing> struct InflateLdsFoldT : InflateLdsT<uint8_t, kRing> {
    uint32_t crc_nib[kCrcNibWords];
};
using InflateLdsSpec = InflateLdsT<uint16_t>;
constexpr uint32_t kScanBytes = 4096; // the block finder reads the input through LDS in pieces of this size (+ the 16 bytes a bit offset at the end reaches into)
constexpr uint32_t kFindList = 1024; // candidates listed between two rounds of the second sieve (a group of 2048 offsets yields 683 at most: one in three)
using InflateLdsFind = InflateLdsT<uint8_t, kScanBytes + 64 + kFindList * 2>;
static_assert(sizeof(InflateLdsFind) <= 14336, "eleven finder waves per CU");
static_assert(sizeof(InflateLds) <= 40448, "four segments per CU");
static_assert(sizeof(InflateLdsVerify) <= 40448 && 4 * sizeof(InflateLdsVerify) <= 160 * 1024, "the integrity test: four workgroups per CU, as the decoder it is");
static_assert(sizeof(InflateLdsFoldT<32768>) <= 40448 && 4 * sizeof(InflateLdsFoldT<32768>) <= 160 * 1024, "the fused batch decode, 32 KiB ring: four workgroups per CU");
static_assert(6 * sizeof(InflateLdsFoldT<16384>) <= 160 * 1024, "the fused batch decode, 16 KiB ring: six workgroups per CU, as the decoder with that ring");
static_assert(10 * sizeof(InflateLdsFoldT<8192>) <= 160 * 1024, "the fused batch decode, 8 KiB ring: ten workgroups per CU, as the decoder with that ring (five waves per SIMD)");
static_assert(10 * sizeof(InflateLdsT<uint8_t, 8192>) <= 160 * 1024, "ten segments per CU with the 8 KiB ring (five waves per SIMD: 96 registers)");
static_assert(sizeof(InflateLdsSpec) <= 81920, "two workgroups per CU");
static_assert(24 * sizeof(InflateLdsSizes) <= 160 * 1024, "the sizing pass: twenty-four one-wave workgroups per CU (six waves per SIMD)");

// Wave-uniform bit reader over a ring of input dwords in LDS.
struct BitSrc {
    const uint32_t *g32; // aligned global dwords
    uint64_t gdwords;    // dwords that may be read from g32 (bounds the whole input buffer)
    uint64_t d0;         // index of the first dword of the segment inside g32
    uint32_t filled;     // dwords of the segment staged so far
    uint32_t rd;         // dwords consumed into hold
    uint64_t hold;
    uint32_t bits;
    uint32_t nx;         // stage[rd]: read one refill ahead so that a refill never waits for LDS
    uint32_t seg_bits;   // size of the segment in bits (from its first dword, including the leading byte offset)
};

// The bit reader's state is the same in all lanes; values that come back from LDS are declared so (v_readfirstlane), which
// moves the whole decode loop -- shifts, masks, compares, branches -- from the vector pipe to scalar instructions.
__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ inline void settle(BitSrc &b) // (the compiler cannot see that loop-carried reader state is wave-uniform: tell it once per symbol)
{
    b.hold = (uint64_t)uni((uint32_t)b.hold) | ((uint64_t)uni((uint32_t)(b.hold >> 32)) << 32);
    b.bits = uni(b.bits); b.rd = uni(b.rd); b.filled = uni(b.filled); b.seg_bits = uni(b.seg_bits);
}

__device__ inline void stage_fill(BitSrc &b, uint32_t *stage, uint32_t lane)
{
    // keep at least 120 dwords ahead of the reader; each call loads 128 dwords (8 bytes per lane).  The ring holds 256: the
    // scalar reader's rd runs two dwords ahead of the position it will be set back to (reposition, the lane-parallel decode),
    // so a fill must leave room behind rd as well: 119 + 128 ahead at most, 9 behind at least.
    while (b.filled - b.rd < 120) {
        const uint64_t i = b.d0 + b.filled + lane * 2;
        uint32_t v[2];
#pragma unroll
        for (int k = 0; k < 2; k++) v[k] = (i + k < b.gdwords) ? b.g32[i + k] : 0u;
        const uint32_t s = (b.filled + lane * 2) & (kStageDwords - 1);
#pragma unroll
        for (int k = 0; k < 2; k++) stage[s + k] = v[k];
        b.filled += 128;
    }
}
__device__ inline void refill(BitSrc &b, const uint32_t *stage)
{
    if (b.bits <= 32) { b.hold |= (uint64_t)uni(b.nx) << b.bits; b.rd++; b.bits += 32; b.nx = stage[b.rd & (kStageDwords - 1)]; } // nx stays a vector register: the wait for it belongs to its use
}
__device__ inline void prime(BitSrc &b, const uint32_t *stage) { b.nx = stage[b.rd & (kStageDwords - 1)]; } // after (re)positioning the reader
__device__ inline uint32_t peek(const BitSrc &b, uint32_t n) { return (uint32_t)b.hold & ((1u << n) - 1); }
__device__ inline void drop(BitSrc &b, uint32_t n) { b.hold >>= n; b.bits -= n; }
__device__ inline uint32_t consumed_bits(const BitSrc &b) { return b.rd * 32 - b.bits; }

// one wave's LDS operations complete in order: ordering its own writes and reads needs the compiler held back, no barrier
__device__ inline void wave_sync() { __builtin_amdgcn_wave_barrier(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// set bit i of a wave-uniform mask (one scalar instruction; the shift-and-or the compiler emits is two in the walk's chain)
__device__ inline void mark_bit(uint64_t &m, uint32_t i) { asm("s_bitset1_b64 %0, %1" : "+s"(m) : "s"(i)); }

// v = the lane's bit of a wave mask ? a : b
__device__ inline uint32_t sel_mask(uint64_t m, uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
    return r;
}
// inclusive prefix sum over the 64 lanes (DPP: shifts inside the rows of 16, then the row totals passed on)
template <int CTRL, int ROWS> __device__ inline uint32_t dpp_or_zero(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false); }
__device__ inline uint32_t wave_prefix_sum(uint32_t v)
{
    v += dpp_or_zero<0x111, 0xf>(v); // row_shr:1
    v += dpp_or_zero<0x112, 0xf>(v); // row_shr:2
    v += dpp_or_zero<0x114, 0xf>(v); // row_shr:4
    v += dpp_or_zero<0x118, 0xf>(v); // row_shr:8
    v += dpp_or_zero<0x142, 0xa>(v); // row_bcast:15 into rows 1 and 3
    v += dpp_or_zero<0x143, 0xc>(v); // row_bcast:31 into rows 2 and 3
    return v;
}

// Build one decoding table from code lengths lens[0..n).  kind: 0 code-length code, 1 literal/length, 2 distance.
// Acceptance rules of inflate_table (inftrees.c:106-138).  Returns 0 ok, 1 rejected.  Lane 0 does the serial part
// (its small work arrays live in LDS: dynamically indexed private arrays would go to scratch memory).
// base value and extra bits of length symbol 257 + k and of distance symbol s (inflate_table's lbase/lext/dbase/dext,
// inftrees.c:46-60, in closed form: no table in memory to wait for)
__device__ inline uint32_t len_extra(uint32_t k) { return (k < 8 || k == 28) ? 0u : (k >> 2) - 1; }
__device__ inline uint32_t len_base(uint32_t k) { return k < 8 ? 3 + k : k == 28 ? 258u : 3 + ((4 + (k & 3)) << ((k >> 2) - 1)); }
__device__ inline uint32_t dist_extra(uint32_t s) { return s < 4 ? 0u : (s >> 1) - 1; }
__device__ inline uint32_t dist_base(uint32_t s) { return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s >> 1) - 1)); }
__constant__ const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// table entry of symbol s with code length l.  kind: 0 code-length code (plain sym << 8 | len), 1 literal/length, 2 distance
__device__ inline uint32_t make_entry(uint32_t kind, uint32_t s, uint32_t l)
{
    if (kind == 0) return (s << 8) | l;
    if (kind == 1) {
        if (s < 256) return l | kEntLit | (s << 16);
        if (s == 256) return l | kEntEob;
        if (s > 285) return l | kEntBad;
        return l | (len_extra(s - 257) << 4) | kEntLen | (len_base(s - 257) << 16);
    }
    if (s > 29) return l | kEntBad;
    return l | (dist_extra(s) << 4) | kEntLen | (dist_base(s) << 16);
}

template <class LDS> __device__ __noinline__ uint32_t build_table(LDS &L, const uint16_t *lens, uint32_t n, uint32_t kind, uint32_t tbits, uint32_t *tab,
                                             uint16_t *sorted, uint16_t *count, uint32_t lane)
{
    // All lanes together (round 2; one lane walking 286 lengths twice was four fifths of a dynamic block's header): a lane holds the lengths of
    // symbols lane, 64 + lane, ...; counts per length and a symbol's place among those of its length are ballots.
    wave_sync();
    for (uint32_t i = lane; i < (1u << tbits); i += 64) tab[i] = 0;
    constexpr uint32_t kGroups = 5; // 320 lengths at most
    const uint32_t ng = (n + 63) >> 6;
    uint32_t ml[kGroups];
#pragma unroll
    for (uint32_t g = 0; g < kGroups; g++) { const uint32_t s2 = g * 64 + lane; ml[g] = s2 < n ? lens[s2] : 0u; }
    uint32_t cnt[16];
    cnt[0] = 0;
#pragma unroll
    for (uint32_t l = 1; l <= 15; l++) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t g = 0; g < kGroups; g++) if (g < ng) c += (uint32_t)__builtin_popcountll(__ballot(ml[g] == l));
        cnt[l] = c;
    }
    uint32_t maxl = 0;
#pragma unroll
    for (uint32_t l = 1; l <= 15; l++) maxl = cnt[l] ? l : maxl;
    uint32_t rc = 0;
    if (maxl > 0) { // inflate_table's rules, inftrees.c:106-138
        int left = 1;
#pragma unroll
        for (uint32_t l = 1; l <= 15; l++) { left <<= 1; left -= (int)cnt[l]; if (left < 0) rc = 1; }
        if (!rc && left > 0 && (kind == 0 || maxl != 1)) rc = 1; // incomplete set
    }
    uint32_t first[16], start[16], c = 0, o = 0;
    first[0] = 0; start[0] = 0;
#pragma unroll
    for (uint32_t l = 1; l <= 15; l++) { c = (c + cnt[l - 1]) << 1; first[l] = c; start[l] = o; o += cnt[l]; }
    // the per-length rows where the long-code walk and the fill below look for them
    {
        uint32_t mc = 0, mf = 0, ms = 0;
#pragma unroll
        for (uint32_t l = 1; l <= 15; l++) { mc = lane == l ? cnt[l] : mc; mf = lane == l ? first[l] : mf; ms = lane == l ? start[l] : ms; }
        if (lane < 16) { count[lane] = (uint16_t)mc; L.work_first[lane] = (uint16_t)mf; L.work_start[lane] = (uint16_t)ms; }
        if (lane == 0) { L.build_n = o; L.build_rc = rc; }
    }
    if (rc == 0) {
#pragma unroll
        for (uint32_t l = 1; l <= 15; l++) {
            if (cnt[l] == 0) continue;
            uint32_t base = start[l];
#pragma unroll
            for (uint32_t g = 0; g < kGroups; g++) {
                if (g >= ng) continue;
                const uint64_t m = __ballot(ml[g] == l);
                if (ml[g] == l) sorted[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)(g * 64 + lane);
                base += (uint32_t)__builtin_popcountll(m);
            }
        }
    }
    wave_sync();
    if (rc == 0) {
        // symbol number j in (length, symbol) order has the canonical code first[l] + (j - start[l])
        for (uint32_t j = lane; j < o; j += 64) {
            const uint32_t s2 = sorted[j], l = lens[s2];
            if (l <= tbits) {
                const uint32_t code = (uint32_t)L.work_first[l] + (j - L.work_start[l]), rev = __brev(code) >> (32 - l), e = make_entry(kind, s2, l);
                for (uint32_t i = rev; i < (1u << tbits); i += 1u << l) tab[i] = e;
            }
        }
    }
    wave_sync();
    return rc;
}

// A code longer than the table, canonical first-code method with one code length per lane: lane l (1..15) holds, for its
// table, the first code of length l, the number of codes of that length and where they start in the (length, symbol) order
// (CodeRows, loaded after build_table); the pattern decodes at the one length whose code range holds its first l bits.
// Returns symbol | length << 16, or 0xFFFF when the bit pattern is not assigned (incomplete / empty code).
struct CodeRows { uint32_t first, count, start; };
template <class LDS> __device__ inline CodeRows load_rows(const LDS &L, const uint16_t *count, uint32_t lane)
{
    CodeRows r;
    r.first = L.work_first[lane & 15]; r.start = L.work_start[lane & 15]; r.count = (lane >= 1 && lane < 16) ? count[lane] : 0u;
    return r;
}
__device__ inline uint32_t long_code(uint32_t hbits, const CodeRows &r, const uint16_t *sorted, uint32_t lane)
{
    const uint32_t l = (lane & 15) ? (lane & 15) : 1, d = (__brev(hbits) >> (32 - l)) - r.first;
    const bool hit = d < r.count; // (count is zero in the lanes that hold no length)
    uint32_t sym = 0;
    if (hit) sym = sorted[r.start + d];
    const uint64_t m = __ballot(hit);
    if (!m) return 0xFFFFu;
    const uint32_t at = (uint32_t)__builtin_ctzll(m);
    return (uint32_t)__builtin_amdgcn_readlane((int)sym, (int)at) | (at << 16);
}

// decode one symbol of the code-length code (plain entries sym << 8 | len; its codes all fit the 7-bit table); 0xFFFF when
// the bit pattern is not assigned
__device__ inline uint32_t decode_sym(BitSrc &b, const uint32_t *tab, uint32_t tbits)
{
    const uint32_t e = uni(tab[peek(b, tbits)]);
    if (!e) return 0xFFFFu;
    drop(b, e & 255);
    return e >> 8;
}

// The header of a dynamic block behind its three type bits (inflate.c:811-880): the counts, the code-length code, the code lengths, the
// two decoding tables.  Returns 0 or the message of the first rule broken.  Wave-uniform; shared by the reader and the block finder.
// QUICK (the block finder, which only wants yes or no): the lengths' sums are kept while they are read, and a literal/length or distance code that is
// over-subscribed already ends the parse -- a header that is none usually is within a few dozen lengths, not after three hundred.  (The decoder proper
// reads them all first: an invalid repeat further on is the error zlib reports, inflate.c:838-866 before :870-885.)
template <bool QUICK, class LDS> __device__ inline uint32_t dynamic_header(LDS &L, BitSrc &b, uint32_t lane, CodeRows &lrows, CodeRows &drows)
{
    refill(b, L.stage);
    const uint32_t nlen = peek(b, 5) + 257; drop(b, 5);
    const uint32_t ndist = peek(b, 5) + 1; drop(b, 5);
    const uint32_t ncode = peek(b, 4) + 4; drop(b, 4);
    if (nlen > 286 || ndist > 30) return kMsgTooMany;
    // The code-length code (19 symbols, codes of at most 7 bits) is built in registers: lane s holds the length of symbol s, the canonical codes come
    // from ballots, and the 128-entry decoding table lives in two registers per lane (entry `lane` and entry `64 + lane`: a look-up is a
    // v_readlane, not a round trip to LDS).  inflate_table's rules for this code (inftrees.c:106-138): over-subscribed or incomplete is an error.
    uint64_t y;
    {
        refill(b, L.stage);
        const uint32_t n0 = ncode < 10 ? ncode : 10;
        const uint64_t lo = peek(b, 3 * n0); drop(b, 3 * n0);
        refill(b, L.stage);
        const uint32_t n1 = ncode - n0;
        const uint64_t hi = n1 ? peek(b, 3 * n1) : 0u; drop(b, 3 * n1);
        y = lo | (hi << 30);
    }
    // where symbol s stands in the order the lengths are sent in (16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15): five bits each
    constexpr uint64_t kInvLo = 3ull | (17ull << 5) | (15ull << 10) | (13ull << 15) | (11ull << 20) | (9ull << 25) | (7ull << 30) | (5ull << 35) | (4ull << 40) | (6ull << 45) | (8ull << 50) | (10ull << 55);
    constexpr uint64_t kInvHi = 12ull | (14ull << 5) | (16ull << 10) | (18ull << 15) | (0ull << 20) | (1ull << 25) | (2ull << 30);
    const uint32_t where = lane < 12 ? (uint32_t)(kInvLo >> (5 * lane)) & 31u : lane < 19 ? (uint32_t)(kInvHi >> (5 * (lane - 12))) & 31u : 31u;
    const uint32_t cl_len = where < ncode ? (uint32_t)(y >> (3 * where)) & 7u : 0u;
    uint32_t cl_first[8], cl_rank = 0, kraft = 0, code = 0, prev_count = 0;
#pragma unroll
    for (uint32_t l = 1; l <= 7; l++) {
        const uint64_t m = __ballot(cl_len == l);
        const uint32_t cnt = (uint32_t)__builtin_popcountll(m), below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        code = (code + prev_count) << 1; cl_first[l] = code; prev_count = cnt;
        kraft += cnt * (128u >> l);
        if (cl_len == l) cl_rank = cl_first[l] + below;
    }
    if (kraft != 128u && kraft != 0u) return kMsgCodeLens; // (no code at all: every look-up below fails, as the reference's empty table does)
    const uint32_t cl_rev = cl_len ? __brev(cl_rank) >> (32 - cl_len) : 0u;
    uint32_t cl0 = 0, cl1 = 0;
    for (uint32_t sy = 0; sy < 19; sy++) {
        const uint32_t ls = (uint32_t)__builtin_amdgcn_readlane((int)cl_len, (int)sy);
        if (!ls) continue;
        const uint32_t rs = (uint32_t)__builtin_amdgcn_readlane((int)cl_rev, (int)sy), mk = (1u << ls) - 1, e = (sy << 8) | ls;
        if ((lane & mk) == rs) cl0 = e;
        if (((lane + 64) & mk) == rs) cl1 = e;
    }
    wave_sync();
    for (uint32_t s = lane; s < 320; s += 64) L.lens[s] = 0;
    uint32_t have = 0, prev = 0, qkl = 0, qkd = 0;
    while (have < nlen + ndist) {
        stage_fill(b, L.stage, lane);
        refill(b, L.stage);
        const uint32_t ci = peek(b, 7);
        const uint32_t ce = ci < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)cl0, (int)ci) : (uint32_t)__builtin_amdgcn_readlane((int)cl1, (int)(ci - 64));
        if (!ce) return kMsgCodeLens;
        drop(b, ce & 255u);
        const uint32_t s = ce >> 8;
        if (s < 16) {
            if (lane == 0) L.lens[have] = (uint16_t)s;
            if (QUICK && s) { if (have < nlen) qkl += 32768u >> s; else qkd += 32768u >> s; if (qkl > 32768u || qkd > 32768u) return kMsgLitLens; }
            prev = s; have++; continue;
        }
        uint32_t rep, val = 0;
        refill(b, L.stage);
        if (s == 16) { if (have == 0) return kMsgRepeat; val = prev; rep = 3 + peek(b, 2); drop(b, 2); }
        else if (s == 17) { rep = 3 + peek(b, 3); drop(b, 3); }
        else { rep = 11 + peek(b, 7); drop(b, 7); }
        if (have + rep > nlen + ndist) return kMsgRepeat;
        if (QUICK && val) { // (a run of equal lengths may straddle the two codes)
            const uint32_t inl = have >= nlen ? 0u : (have + rep <= nlen ? rep : nlen - have);
            qkl += inl * (32768u >> val); qkd += (rep - inl) * (32768u >> val);
            if (qkl > 32768u || qkd > 32768u) return kMsgLitLens;
        }
        if (lane < rep) L.lens[have + lane] = (uint16_t)val;
        if (lane + 64 < rep) L.lens[have + lane + 64] = (uint16_t)val;
        if (lane + 128 < rep) L.lens[have + lane + 128] = (uint16_t)val;
        prev = val; have += rep;
    }
    wave_sync();
    // inflate_table's verdict on the two sets of lengths (inftrees.c:106-138: over-subscribed, or incomplete with more than a single one-bit
    // code), taken by all lanes together before lane 0 builds anything: the block finder comes here with thousands of headers that are none
    {
        uint32_t kl = 0, kd = 0, ml = 0, md = 0;
        for (uint32_t i = lane; i < nlen + ndist; i += 64) {
            const uint32_t l = L.lens[i], k = l ? (32768u >> l) : 0u;
            if (i < nlen) { kl += k; ml = l > ml ? l : ml; } else { kd += k; md = l > md ? l : md; }
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            kl += (uint32_t)__shfl_xor((int)kl, sh); kd += (uint32_t)__shfl_xor((int)kd, sh);
            const uint32_t a = (uint32_t)__shfl_xor((int)ml, sh), c = (uint32_t)__shfl_xor((int)md, sh);
            ml = a > ml ? a : ml; md = c > md ? c : md;
        }
        kl = uni(kl); kd = uni(kd); ml = uni(ml); md = uni(md);
        if (ml && (kl > 32768u || (kl < 32768u && ml != 1))) return kMsgLitLens;
        if (md && (kd > 32768u || (kd < 32768u && md != 1))) return kMsgDists;
    }
    if (build_table(L, L.lens, nlen, 1, kLBits, L.ltab, L.lsym, L.lcount, lane)) return kMsgLitLens;
    lrows = load_rows(L, L.lcount, lane);
    wave_sync();
    if (build_table(L, L.lens + nlen, ndist, 2, kDBits, L.dtab, L.dsym, L.dcount, lane)) return kMsgDists;
    drows = load_rows(L, L.dcount, lane);
    return kMsgNone;
}

} // namespace zgpu
