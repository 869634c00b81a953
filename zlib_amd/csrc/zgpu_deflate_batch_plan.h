// zgpu_deflate_batch_plan.h -- internal (not installed): the workspace of a stream-ordered batch deflate call (zgpu_deflate_batch_*_enqueue) as a function
// of plain numbers.  The caller owns the workspace; a call carves it up as this header says and touches no device memory of the engine's.  Host only:
// no HIP type, no include but <cstdint>, so that tests/tools/deflate_batch_plan_model.cpp prints the same layouts on a machine without a GPU.  What a
// round's item costs is written out as numbers here; zgpu_lz_sorted.h and zgpu_deflate_batch.hip assert that they are the structs and constants they
// stand for.
#pragma once
#include <cstdint>

namespace zgpu {

// per item of a ROUND (min(n, batch_items) of them; nothing here is per item of the call): where its bytes lie, the sanitized table, the item's state, the
// staging buffer the served items are gathered into, and what the existing launchers work in
constexpr uint64_t kDwsLoBytes = 8;       // uint64_t: where the item's input begins in the caller's buffer
constexpr uint64_t kDwsPreBytes = 8;      // uint64_t: where the item begins in the staging buffer -- the exclusive sum of the lengths of the round's served items,
                                          // a failed item counting nothing; one entry more, the round's end
constexpr uint64_t kDwsStateBytes = 4;    // uint32_t: 0 served, 1 failed by the table check
constexpr uint64_t kDwsStageBytes = 65536;      // kChunkMax: no item is longer
constexpr uint64_t kDwsStageSlack = 256;        // once, behind the last item
constexpr uint64_t kDwsSortedHeader = 256;      // SortedWs: the header with the sort's fault word, once
constexpr uint64_t kDwsSortedChunk = 1058832;   // SortedWs: S 131088, rk 131072, heads 10240, recs 524288, ir 262144
constexpr uint64_t kDwsSortedSlack = 1024;      // SortedWs: margin behind the last array, once
constexpr uint64_t kDwsTokenBytes = 262144;     // kChunkMax tokens of four bytes
constexpr uint64_t kDwsSlotBytes = 65792;       // kSlotStride
constexpr uint64_t kDwsMetaBytes = 32;          // ChunkMeta
constexpr uint64_t kDwsCntBytes = 256;          // the counters: 32 uint64_t, one region whatever n is
constexpr uint64_t kDwsAlign = 256;             // every region starts at a multiple of this (the workspace itself must too)
constexpr uint64_t kDwsMaxItems = 1ull << 32;   // a call serves fewer items than this
constexpr uint32_t kDwsDefaultRound = 4096;     // batch_items == 0

// the counters of a call (uint64_t each, zeroed by the call's first launch)
constexpr uint32_t kDcntTotal = 0;      // packed: bytes laid out so far, carried from round to round
constexpr uint32_t kDcntFailed = 1;     // records that are not ZGPU_OK
constexpr uint32_t kDcntBadOffsets = 2; // items whose offsets (or range) run backwards or leave their buffer
constexpr uint32_t kDcntTooLong = 3;    // items over the length limit

struct DeflateWsRegion { uint64_t off, bytes, align; };
struct DeflateWsPlan {
    DeflateWsRegion cnt, lo, pre, state, stage, sorted, tokens, slots, meta;
    uint64_t round; // items of a full round: min(n, batch_items), batch_items == 0 standing for 4096
    uint64_t total; // bytes of the whole workspace; 0: n >= kDwsMaxItems
};
constexpr int kDeflateWsRegions = 9;
inline const DeflateWsRegion &deflate_ws_region(const DeflateWsPlan &p, int i)
{
    return i == 0 ? p.cnt : i == 1 ? p.lo : i == 2 ? p.pre : i == 3 ? p.state : i == 4 ? p.stage : i == 5 ? p.sorted : i == 6 ? p.tokens : i == 7 ? p.slots : p.meta;
}
inline const char *deflate_ws_region_name(int i)
{
    static const char *const names[kDeflateWsRegions] = {"cnt", "lo", "pre", "state", "stage", "sorted", "tokens", "slots", "meta"};
    return i >= 0 && i < kDeflateWsRegions ? names[i] : "";
}

inline uint64_t deflate_batch_round(uint64_t n, uint32_t batch_items)
{
    const uint64_t b = batch_items ? batch_items : kDwsDefaultRound;
    return n < b ? n : b;
}

// The layout for n items in rounds of batch_items.  A function of min(n, batch_items) and n alone: nothing depends on the items' bytes, on the level or on
// the wrapper.  n < 2^32 and a round's item costs 1 452 356 bytes: the total stays below 2^53, no sum here can wrap.
inline DeflateWsPlan deflate_batch_ws_plan(uint64_t n, uint32_t batch_items)
{
    DeflateWsPlan p{};
    if (n >= kDwsMaxItems) return p;
    const uint64_t b = deflate_batch_round(n, batch_items);
    uint64_t off = 0;
    auto carve = [&](uint64_t bytes, uint64_t align) {
        DeflateWsRegion r{off, bytes, align};
        off = (off + bytes + kDwsAlign - 1) & ~(kDwsAlign - 1);
        return r;
    };
    p.cnt = carve(kDwsCntBytes, 8);
    p.lo = carve(b * kDwsLoBytes, 8);
    p.pre = carve((b + 1) * kDwsPreBytes, 8);
    p.state = carve(b * kDwsStateBytes, 4);
    p.stage = carve(b * kDwsStageBytes + kDwsStageSlack, 256);
    p.sorted = carve(kDwsSortedHeader + b * kDwsSortedChunk + kDwsSortedSlack, 256);
    p.tokens = carve(b * kDwsTokenBytes, 4);
    p.slots = carve(b * kDwsSlotBytes, 4);
    p.meta = carve(b * kDwsMetaBytes, 4);
    p.round = b;
    p.total = off;
    return p;
}

inline uint64_t deflate_batch_ws_bytes(uint64_t n, uint32_t batch_items) { return deflate_batch_ws_plan(n, batch_items).total; }

} // namespace zgpu
