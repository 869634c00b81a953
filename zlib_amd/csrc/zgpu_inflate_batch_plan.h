// zgpu_inflate_batch_plan.h -- internal (not installed): the workspace of a stream-ordered batch inflate call (zgpu_inflate_batch_*_enqueue) as a function
// of plain numbers.  The caller owns the workspace; a call carves it up as this header says and touches no device memory of the engine's.  Host only:
// no HIP type, no include but <cstdint>, so that tests/tools/inflate_batch_plan_model.cpp prints the same layouts on a machine without a GPU.  The record
// sizes are written out as numbers here; zgpu_inflate_batch.hip asserts that they are the sizeof of the structs they stand for.
#pragma once
#include <cstdint>

namespace zgpu {

// the four jobs (include/zamd_gpu.h: ZGPU_BATCH_JOB_*)
constexpr int kBatchJobDecode = 0, kBatchJobSizes = 1, kBatchJobVerify = 2, kBatchJobPacked = 3, kBatchJobCount = 4;

// bytes of one record of each region, and what its type wants for alignment
constexpr uint64_t kWsSegBytes = 32;     // four uint64_t: body start, input end, output start, output end
constexpr uint64_t kWsStateBytes = 64;   // BatchItemState
constexpr uint64_t kWsStatusBytes = 16;  // InfStatus
constexpr uint64_t kWsCntBytes = 256;    // the counters: 32 uint64_t, one region whatever n is
constexpr uint64_t kWsMetaBytes = 32;    // ChunkMeta: the item's folded check values
constexpr uint64_t kWsHiBytes = 8;       // packed: where every item's range ends, n + 1 entries
constexpr uint64_t kWsItemBytes = 32;    // packed: zgpu_inflate_item, the decoder's records until they are merged with the sizing pass's
constexpr uint64_t kWsAlign = 256;       // every region starts at a multiple of this (the workspace itself must too)
constexpr uint64_t kWsMaxItems = 1ull << 32; // a call serves fewer items than this

// the counters of a call (uint64_t each, zeroed by the call's one memset)
constexpr uint32_t kCntTotal = 0;      // packed: the layout's total
constexpr uint32_t kCntFailed = 1;     // items whose record is not ZGPU_OK (packed: of the sizing pass)
constexpr uint32_t kCntBadOffsets = 2; // items whose offsets run backwards or leave their buffer
constexpr uint32_t kCntMerged = 3;     // packed: failed items after the merge
constexpr uint32_t kCntHeaderFlag = 4; // what the header kernel ors its bad-table bit into (not read)
constexpr uint32_t kCntDecodeFailed = 5; // packed: the decode stage's own count (not read)

struct BatchWsRegion { uint64_t off, bytes, align; };
struct BatchWsPlan {
    BatchWsRegion seg, states, status, cnt, meta, hi, items2; // a region the job does not have: bytes == 0, off == total
    uint64_t total; // bytes of the whole workspace; 0: no such job, or n >= kWsMaxItems
};
constexpr int kBatchWsRegions = 7;
inline const BatchWsRegion &batch_ws_region(const BatchWsPlan &p, int i)
{
    return i == 0 ? p.seg : i == 1 ? p.states : i == 2 ? p.status : i == 3 ? p.cnt : i == 4 ? p.meta : i == 5 ? p.hi : p.items2;
}
inline const char *batch_ws_region_name(int i)
{
    static const char *const names[kBatchWsRegions] = {"seg", "states", "status", "cnt", "meta", "hi", "items2"};
    return i >= 0 && i < kBatchWsRegions ? names[i] : "";
}

// The layout of job `job` for n items.  It grows with n only: no region depends on what the items decode to -- the fused decoder keeps no piece table.
// n < 2^32 and the largest record has 64 bytes: the total stays below 2^40, no sum here can wrap.
inline BatchWsPlan inflate_batch_ws_plan(int job, uint64_t n)
{
    BatchWsPlan p{};
    if (job < 0 || job >= kBatchJobCount || n >= kWsMaxItems) return p;
    uint64_t off = 0;
    auto carve = [&](uint64_t bytes, uint64_t align) {
        BatchWsRegion r{off, bytes, align};
        off = (off + bytes + kWsAlign - 1) & ~(kWsAlign - 1);
        return r;
    };
    p.seg = carve(n * kWsSegBytes, 8);
    p.states = carve(n * kWsStateBytes, 8);
    p.status = carve(n * kWsStatusBytes, 4);
    p.cnt = carve(kWsCntBytes, 8);
    const bool folds = job != kBatchJobSizes, packed = job == kBatchJobPacked;
    // (a region the job does not have is empty and lies where the workspace ends)
    p.meta = folds ? carve(n * kWsMetaBytes, 4) : BatchWsRegion{off, 0, 4};
    p.hi = packed ? carve((n + 1) * kWsHiBytes, 8) : BatchWsRegion{off, 0, 8};
    p.items2 = packed ? carve(n * kWsItemBytes, 8) : BatchWsRegion{off, 0, 8};
    p.total = off;
    return p;
}

inline uint64_t inflate_batch_ws_bytes(int job, uint64_t n) { return inflate_batch_ws_plan(job, n).total; }

} // namespace zgpu
