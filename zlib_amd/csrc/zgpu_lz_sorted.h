// zgpu_lz_sorted.h -- what the files of the sorted-bucket LZ77 stage share (zgpu_lz_sorted.hip has the map of them): the workspace of a batch of
// chunks and the launchers zgpu_lz_sorted.hip calls (host), and the device helpers that more than one kernel's file uses.  Internal to those files.
#pragma once
#include "zgpu_common.h"
#include "zgpu_engine.h"
#include "zgpu_deflate_batch_plan.h"

namespace zgpu {

constexpr uint32_t kHeadWords = kChunkMax / 32;                  // dwords of bucket-head bits per chunk ...
constexpr uint32_t kHeadStride = kHeadWords + kChunkMax / 64 / 2; // ... followed by one u16 per 64 S indices (dwords per chunk)
constexpr uint32_t kGPad = 32, kGStride = kChunkMax + 2 * kGPad;  // fast_kernel's flag bytes per chunk, room in front for the group reads

// The workspace of a batch of chunks (host side): the one place that says where its arrays lie and how large it is.
//   header (fault: the word the sort's self-check raises) | S (u16; kSStride per chunk, zgpu_common.h) | rk: sort_kernel's ranks by position (u16) |
//   heads: bucket-head bits, heads_below | recs: match3's records (uint2 by position) | ir: idx | rank << 16 by position (u32; what the walkers
//   and the levels 1-3 kernels look a position up with)
// The records' memory serves whichever search runs: match3's records, the walkers' games gm (u32 by position) with the bitmaps gs (a bit by
// position) behind them (tiles), the logs a chunk's walkers hand their games to the fused parse in (lrec: u32, lpos: u16 behind them; kP2Win
// entries per window, zgpu_lz_parse.h), or fast_kernel's flag bytes G.
struct SortedWs {
    static constexpr size_t kHeaderBytes = 256, kSBytes = kSStride * 2, kRkBytes = kChunkMax * 2, kHeadBytes = kHeadStride * 4, kRecBytes = kChunkMax * 8, kIrBytes = kChunkMax * 4;
    static constexpr size_t kSlack = 1024; // S's end is rounded up to 256 bytes; the rest is margin
    static_assert(kChunkMax * 4 + kChunkMax / 8 <= kRecBytes && kGStride <= kRecBytes, "gm + gs, and G, lie in the records' memory");
    static_assert(kChunkMax * (4 + 2) <= kRecBytes, "and so do the logs: the workspace, and with it the batch a device holds, is what it was");
    static constexpr size_t bytes(size_t nchunks) { return kHeaderBytes + nchunks * (kSBytes + kRkBytes + kHeadBytes + kRecBytes + kIrBytes) + kSlack; }

    size_t nch;
    uint32_t *fault; uint16_t *S, *rk; uint32_t *heads; uint2 *recs; uint32_t *ir;
    SortedWs(void *workspace, size_t nchunks) : nch(nchunks)
    {
        uint8_t *p = static_cast<uint8_t *>(workspace);
        auto take = [&p](size_t n) { uint8_t *at = p; p += n; return at; };
        fault = reinterpret_cast<uint32_t *>(take(kHeaderBytes));
        S = reinterpret_cast<uint16_t *>(take((nch * kSBytes + 255) & ~(size_t)255));
        rk = reinterpret_cast<uint16_t *>(take(nch * kRkBytes));
        heads = reinterpret_cast<uint32_t *>(take(nch * kHeadBytes));
        recs = reinterpret_cast<uint2 *>(take(nch * kRecBytes));
        ir = reinterpret_cast<uint32_t *>(take(nch * kIrBytes));
    }
    uint32_t *gm() const { return reinterpret_cast<uint32_t *>(recs); }
    uint32_t *gs() const { return gm() + nch * kChunkMax; }
    uint32_t *lrec() const { return reinterpret_cast<uint32_t *>(recs); }
    uint16_t *lpos() const { return reinterpret_cast<uint16_t *>(lrec() + nch * kChunkMax); }
    uint8_t *G() const { return reinterpret_cast<uint8_t *>(recs); }
};

static_assert(SortedWs::kHeaderBytes == kDwsSortedHeader && SortedWs::kSlack == kDwsSortedSlack && SortedWs::bytes(1) == kDwsSortedHeader + kDwsSortedChunk + kDwsSortedSlack &&
              SortedWs::bytes(3) - SortedWs::bytes(2) == kDwsSortedChunk, "zgpu_deflate_batch_plan.h states the workspace of a chunk as numbers");

// The kernels' launchers, one file each; zgpu_lz_sorted.hip puts them in order on the stream.
bool launch_sort(const ChunkGeom &g, const SortedWs &ws, ChunkMeta *meta, hipStream_t st, zgpu_engine *prof, int exact_sort);                  // zgpu_lz_sort.hip
void launch_match3(const ChunkGeom &g, LevelCfg cfg, const SortedWs &ws, hipStream_t st);                                                     // zgpu_lz_match3.hip
void launch_walk_chunks(const ChunkGeom &g, LevelCfg cfg, const SortedWs &ws, uint32_t *tokens, ChunkMeta *meta, hipStream_t st);              // zgpu_lz_walk.hip, walk_kernel<1>
void launch_walk_tiles(const ChunkGeom &g, const TileGeom &tg, LevelCfg cfg, const SortedWs &ws, ChunkMeta *meta, hipStream_t st);             // zgpu_lz_walk.hip, walk_kernel<2>
void launch_fast(const ChunkGeom &g, LevelCfg cfg, const SortedWs &ws, uint32_t *tokens, ChunkMeta *meta, hipStream_t st);                     // zgpu_lz_fast.hip

// ---- device helpers ----
__device__ inline uint32_t lds_off(const void *p) { return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p; }
// wave-private LDS words by byte offset (plain C++ volatile accesses through a generic pointer compile to flat_* memory instructions)
__device__ inline void lds_st32(uint32_t a, uint32_t v) { asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(v) : "memory"); }
__device__ inline void lds_st16(uint32_t a, uint32_t v) { asm volatile("ds_write_b16 %0, %1" ::"v"(a), "v"(v) : "memory"); }
__device__ inline void lds_max32(uint32_t a, uint32_t v) { asm volatile("ds_max_u32 %0, %1" ::"v"(a), "v"(v) : "memory"); }
__device__ inline uint32_t lds_ld32(uint32_t a) { uint32_t v; asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory"); return v; }
__device__ inline uint32_t lds_ld16(uint32_t a) { uint32_t v; asm volatile("ds_read_u16 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory"); return v; }

__device__ inline void lds_st8(uint32_t a, uint32_t v) { asm volatile("ds_write_b8 %0, %1" ::"v"(a), "v"(v) : "memory"); }
__device__ inline uint32_t lds_ld8(uint32_t a) { uint32_t v; asm volatile("ds_read_u8 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory"); return v; }

__device__ inline uint32_t lds_ld32u(uint32_t a) // 4 bytes at any LDS byte offset: aligned ds_read2_b32 + v_alignbyte
{
    uint64_t v; const uint32_t al = a & ~3u;
    asm volatile("ds_read2_b32 %0, %1 offset1:1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(al) : "memory");
    return __builtin_amdgcn_alignbyte((uint32_t)(v >> 32), (uint32_t)v, a & 3);
}
// xa, xb = the first and the second four bytes of (8 bytes at LDS offset a) ^ (8 bytes at LDS offset b), any alignment: three aligned
// dwords of each string in flight together, one wait
__device__ inline void lds_cmp8(uint32_t a, uint32_t b, uint32_t &xa, uint32_t &xb)
{
    uint64_t va, vb; uint32_t va2, vb2;
    const uint32_t aa = a & ~3u, ba = b & ~3u;
    asm volatile("ds_read2_b32 %0, %4 offset1:1\n\tds_read_b32 %1, %4 offset:8\n\tds_read2_b32 %2, %5 offset1:1\n\tds_read_b32 %3, %5 offset:8\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(va), "=&v"(va2), "=&v"(vb), "=&v"(vb2) : "v"(aa), "v"(ba) : "memory");
    const uint32_t a0 = __builtin_amdgcn_alignbyte((uint32_t)(va >> 32), (uint32_t)va, a & 3), a1 = __builtin_amdgcn_alignbyte(va2, (uint32_t)(va >> 32), a & 3);
    const uint32_t b0 = __builtin_amdgcn_alignbyte((uint32_t)(vb >> 32), (uint32_t)vb, b & 3), b1 = __builtin_amdgcn_alignbyte(vb2, (uint32_t)(vb >> 32), b & 3);
    xa = a0 ^ b0; xb = a1 ^ b1;
}
__device__ inline void lds_ld2bytes(uint32_t a, uint32_t &b0, uint32_t &b1)
{
    asm volatile("ds_read_u8 %0, %2\n\tds_read_u8 %1, %2 offset:1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(b0), "=&v"(b1) : "v"(a) : "memory");
}
struct __attribute__((packed, aligned(2))) U64u { uint64_t v; };
struct __attribute__((packed, aligned(2))) U128u { uint4 v; }; // 8 bytes at 2-byte alignment: one global_load_dwordx2 on gfx950 (scripts/micro/global_unaligned.hip)

// chunk bytes -> LDS (zero padded to kChunkMax + 64), by all T lanes of the workgroup
template <uint32_t T> __device__ inline void stage_chunk(const uint8_t *src, uint32_t n, uint32_t *d32, uint32_t tid)
{
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const uint4 *s128 = reinterpret_cast<const uint4 *>(src);
        uint4 *d128 = reinterpret_cast<uint4 *>(d32);
        const uint32_t nv = n >> 4;
        for (uint32_t i = tid; i < (kChunkMax + 64) / 16; i += T) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (i < nv) v = s128[i];
            else if (i == nv) {
                uint32_t w[4] = {0, 0, 0, 0};
                for (uint32_t k = 0; k < (n & 15); k++) w[k >> 2] |= (uint32_t)src[(nv << 4) + k] << (8 * (k & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            d128[i] = v;
        }
    } else {
        for (uint32_t i = tid; i < (kChunkMax + 64) / 4; i += T) {
            uint32_t v = 0;
            for (uint32_t k = 0; k < 4; k++) { uint32_t a = (i << 2) + k; if (a < n) v |= (uint32_t)src[a] << (8 * (k & 3)); }
            d32[i] = v;
        }
    }
}

// Lane masks straight from a vector compare (SGPR pair).  `__ballot(a && b)` of two conditions goes through
// v_cndmask + v_cmp_ne to rebuild a mask the compares had already produced; the walk step below keeps the set of lanes
// still walking as such a mask and combines compare results with scalar ANDs.
__device__ inline unsigned long long mask_eq_u32(uint32_t a, uint32_t b) { unsigned long long m; asm volatile("v_cmp_eq_u32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(b)); return m; }
__device__ inline unsigned long long mask_le_i32(int a, int b) { unsigned long long m; asm volatile("v_cmp_le_i32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(b)); return m; }
__device__ inline unsigned long long mask_gt_u32(uint32_t a, uint32_t b) { unsigned long long m; asm volatile("v_cmp_gt_u32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(b)); return m; }
__device__ inline unsigned long long mask_lt_i32(int a, int b) { unsigned long long m; asm volatile("v_cmp_lt_i32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(b)); return m; }
// the lanes of m append `entry` to the wave's stack at LDS byte offset rt, in lane order; the other lanes store to a dummy
// word instead (narrowing exec for the store costs more than the select: writes to exec stall the vector pipe)
__device__ inline void stack_push(unsigned long long m, uint32_t rt, uint32_t dummy, uint32_t entry)
{
    uint32_t t;
    asm volatile("v_mbcnt_lo_u32_b32 %0, %2, 0\n\tv_mbcnt_hi_u32_b32 %0, %3, %0\n\tv_lshl_add_u32 %0, %0, 2, %4\n\t"
                 "v_cndmask_b32_e64 %0, %5, %0, %1\n\tds_write_b32 %0, %6"
                 : "=&v"(t) : "s"(m), "s"((uint32_t)m), "s"((uint32_t)(m >> 32)), "s"(rt), "v"(dummy), "v"(entry) : "memory");
}

// LDS byte offset of the slot the lanes of m append to a stack whose top is at byte offset rt, in lane order (the other lanes get a slot they must not use)
__device__ inline uint32_t stack_slot(unsigned long long m, uint32_t rt)
{
    uint32_t t;
    asm volatile("v_mbcnt_lo_u32_b32 %0, %1, 0\n\tv_mbcnt_hi_u32_b32 %0, %2, %0\n\tv_lshl_add_u32 %0, %0, 2, %3" : "=&v"(t) : "s"((uint32_t)m), "s"((uint32_t)(m >> 32)), "s"(rt));
    return t;
}

// The LDS of a searching workgroup, match3_kernel's and (in front of its own arrays) walk_kernel's: the chunk's bytes, then a stack and 64 slots per wave
constexpr uint32_t kRing = 128;                                  // parked candidates per wave: q | owner<<16 | (k&1023)<<22
constexpr uint32_t kM3WaveLds = kRing * 4 + 64 * 4 + 64 * 2;     // ring + slots + owners' positions
constexpr uint32_t kM3DataLds = kChunkMax + 64 + 320;            // chunk bytes + zero pad + slack for reads past a garbage candidate

} // namespace zgpu
