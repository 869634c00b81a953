// zgpu_inflate_pieces_plan.h -- internal (not installed): what the piece path of the blocking batch decode (zgpu_inflate_batch_pieces.hip) decides from
// plain numbers: which items are long, how far apart their pieces and their block finders stand, which of the finders' hits become piece starts,
// how a call's long items are split into rounds and how a round's scratch is laid out.  No HIP type and no include but <cstdint>: tests/tools/
// inflate_pieces_plan_model.cpp runs the same code on a machine without a GPU.  The functions the device runs too carry ZGPU_PIECES_HD, which is
// `__host__ __device__` under hipcc and nothing elsewhere.
// The spacing formulas are those of inflate_spec_run (zgpu_inflate_stream.hip) for one stream of the same length.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ZGPU_PIECES_HD __host__ __device__
#else
#define ZGPU_PIECES_HD
#endif

namespace zgpu {

constexpr uint64_t kPiecesMinBytesDefault = 131072;       // ZGPU_BATCH_PIECES_MIN_BYTES: a deflate body of at least this many bytes is a long item (0: none is)
constexpr uint64_t kPiecesRoundBytesDefault = 512ull << 20; // ZGPU_BATCH_PIECES_ROUND_BYTES: bytes of output room one round serves
constexpr uint64_t kPiecesScratchCap = (2ull << 30) - 1;  // ... and a round ends before its scratch would pass this, whatever the knob says
constexpr uint64_t kPiecesBodyMax = 1ull << 29;           // the one-workgroup decoder's own limit of an item: a longer body is its to refuse
constexpr uint64_t kPiecesStoredFlag = 1ull << 62;        // a start that is the (byte-aligned) LEN of a stored block (inflate_kernel_t<SPEC>)
constexpr uint64_t kPiecesNone = ~0ull;                   // a finder that found nothing
constexpr uint32_t kPiecesRing = 32768, kPiecesHalf = 16384; // kOutRing, kOutHalf of the decoder in pieces (zgpu_inflate_batch_pieces.hip asserts it)

// spacing: bytes between two piece starts the selection aims at (starts are kept 6 * spacing BITS, three quarters of it, apart or more);
// fspacing: bytes between two finders; ntargets: finders of a body (finder t scans [t * fspacing, (t + 1) * fspacing), t = 1 .. ntargets);
// piece_cap: pieces the selection can make of it at most -- the first, and one per 6 * spacing bits that end more than 2 * spacing bits before the end
struct PiecesGeom { uint64_t spacing, fspacing; uint32_t ntargets, piece_cap; };
ZGPU_PIECES_HD inline PiecesGeom pieces_geom(uint64_t body)
{
    PiecesGeom g{};
    g.spacing = (body / 4096 + 4095) & ~4095ull;
    if (g.spacing < 32768) g.spacing = 32768;
    g.fspacing = g.spacing / 4 < 16384 ? 16384 : (g.spacing / 4 + 4095) & ~4095ull;
    g.ntargets = body ? (uint32_t)((body - 1) / g.fspacing) : 0u;
    g.piece_cap = (uint32_t)(body * 8 / (g.spacing * 6)) + 1;
    return g;
}
// three finders at least, as inflate_spec_run asks (a threshold set far below the default can name bodies that have fewer)
ZGPU_PIECES_HD inline bool pieces_long(uint64_t body, uint64_t min_bytes)
{
    return min_bytes != 0 && body >= min_bytes && body < kPiecesBodyMax && pieces_geom(body).ntargets >= 3;
}

// Finder t (1 .. ntargets) of a body that begins at byte body_lo of the buffer and ends at byte end: bits [lo, hi) of the buffer.  Every inner border is
// rounded down to 16 bytes of the BUFFER (the finder stages its bytes in 16-byte vectors from there): the regions still tile the body behind the first.
ZGPU_PIECES_HD inline uint64_t pieces_target_lo(uint64_t body_lo, uint64_t fspacing, uint32_t t) { return ((body_lo + (uint64_t)t * fspacing) & ~15ull) * 8; }
ZGPU_PIECES_HD inline uint64_t pieces_target_hi(uint64_t body_lo, uint64_t end, uint64_t fspacing, uint32_t ntargets, uint32_t t)
{
    return t >= ntargets ? end * 8 : pieces_target_lo(body_lo, fspacing, t + 1);
}

// The selection (the rules of inflate_spec_run, in one pass over what the finders report in target order).
//   dyn[i]  bit position of the first dynamic block header finder i + 1 believes in, sto[i] byte position of the LEN of the first stored block it
//           vouches for (both in the buffer; kPiecesNone: nothing).  Both ascend with i, the finders' regions being disjoint and in order.
//   in      the buffer (the LEN of a vouched stored block is read from it); first_bit: the body's first bit; end: the byte behind the item.
//   starts  receives the piece starts, ascending, a stored start with kPiecesStoredFlag; starts[0] = first_bit always.  Returns their number, <= cap.
// Rules: a dynamic start inside the bytes of a stored block the finders vouch for is struck (the eight vouched blocks in front of it are looked at, as on
// the host: a block has 64 KiB at most and the finders stand 16 KiB apart or more); a start is kept when it lies 6 * spacing bits or more behind the one
// kept before it and more than 2 * spacing bits before the item's end; at the same position a dynamic start goes first (the host sorts pairs).
// Termination: one pass over i < ntargets, each step an inner loop of eight entries at most.
ZGPU_PIECES_HD inline uint32_t pieces_select(const uint64_t *dyn, const uint64_t *sto, uint32_t ntargets, const uint8_t *in, uint64_t first_bit, uint64_t end, uint64_t spacing,
                                             uint64_t *starts, uint32_t cap)
{
    uint32_t n = 0;
    if (cap == 0) return 0;
    starts[n++] = first_bit;
    uint64_t last = first_bit;
    auto take = [&](uint64_t pos, bool stored) {
        if (n < cap && pos >= last + spacing * 6 && pos + spacing * 2 < end * 8) { starts[n++] = stored ? pos | kPiecesStoredFlag : pos; last = pos; }
    };
    auto vouched = [&](uint32_t i) { return sto[i] != kPiecesNone && sto[i] + 4 <= end; };
    for (uint32_t i = 0; i < ntargets; i++) {
        const uint64_t d = dyn[i], B = sto[i];
        bool keep_d = d != kPiecesNone;
        if (keep_d) {
            uint32_t seen = 0;
            for (uint32_t j = i + 1; j-- > 0 && seen < 8;) {
                if (!vouched(j) || sto[j] * 8 > d) continue;
                seen++;
                const uint64_t b = sto[j], stop = (b + 4 + ((uint64_t)in[b] | ((uint64_t)in[b + 1] << 8))) * 8;
                if (d < stop) { keep_d = false; break; }
            }
        }
        // (both lie in finder i + 1's region: in position order, the dynamic one first on a tie)
        if (keep_d && (B == kPiecesNone || d <= B * 8)) { take(d, false); keep_d = false; }
        if (B != kPiecesNone) take(B * 8, true);
        if (keep_d) take(d, false);
    }
    return n;
}

// ---- rounds ----
// What a long item costs a round: its output room, and the scratch of its pieces.
struct PiecesItemCost { uint64_t room; uint32_t ntargets, piece_cap; };
// per piece: its tail (a ring of 16-bit symbols), its window (bytes), the page it may leave half empty, its row, end record, status and output start
constexpr uint64_t kPiecesPerPieceBytes = 2ull * kPiecesRing + kPiecesRing + 2ull * kPiecesHalf + 32 + 16 + 16 + 8;
constexpr uint64_t kPiecesPerTargetBytes = 24 + 16; // a finder's row and its two results
ZGPU_PIECES_HD inline uint64_t pieces_item_scratch(const PiecesItemCost &c)
{
    return c.room * 2 + (c.room / kPiecesHalf) * 8 + (uint64_t)c.piece_cap * kPiecesPerPieceBytes + (uint64_t)c.ntargets * kPiecesPerTargetBytes + 16;
}
// The round that begins with long item `first` of `nlong`: it ends behind item *last - 1.  Items are taken in order while their rooms stay within
// round_bytes and their scratch within kPiecesScratchCap; an item that alone passes either makes a round of its own (whether its scratch can be had is
// found out when it is reserved).  Every long item is in exactly one round.
// Termination: *last grows by one per step and stops at nlong.
inline uint64_t pieces_round_end(const PiecesItemCost *c, uint64_t nlong, uint64_t first, uint64_t round_bytes)
{
    uint64_t room = 0, scratch = 0, k = first;
    while (k < nlong) {
        const uint64_t s = pieces_item_scratch(c[k]);
        if (k > first && (room + c[k].room > round_bytes || scratch + s > kPiecesScratchCap)) break;
        room += c[k].room; scratch += s; k++;
    }
    return k;
}

// ---- the scratch of a round ----
// nitems long items with ntargets finders, npieces piece slots (the sum of the items' piece_cap) and `room` bytes of output room together.
struct PiecesRegion { uint64_t off, bytes; };
struct PiecesRoundPlan {
    PiecesRegion targets, found, rows, ends, status, ostart, ranges, cnt, owner, windows, entry, tails, mid; // in this order
    uint64_t page_cap; // pages of kPiecesHalf symbols: what the rooms can hold and one a piece may leave half empty
    uint64_t total;    // 0: the round cannot be had (more than 2^32 - 2 slots or pages)
};
constexpr int kPiecesRegions = 13;
constexpr uint64_t kPiecesAlign = 256;
inline const PiecesRegion &pieces_region(const PiecesRoundPlan &p, int i)
{
    const PiecesRegion *r[kPiecesRegions] = {&p.targets, &p.found, &p.rows, &p.ends, &p.status, &p.ostart, &p.ranges, &p.cnt, &p.owner, &p.windows, &p.entry, &p.tails, &p.mid};
    return *r[i];
}
inline const char *pieces_region_name(int i)
{
    static const char *const names[kPiecesRegions] = {"targets", "found", "rows", "ends", "status", "ostart", "ranges", "cnt", "owner", "windows", "entry", "tails", "mid"};
    return i >= 0 && i < kPiecesRegions ? names[i] : "";
}
// nitems, ntargets and npieces stay below 2^32 and room below 2^44 (a call's out_cap): the largest term, npieces * 64 KiB, stays below 2^48.
inline PiecesRoundPlan pieces_round_plan(uint64_t nitems, uint64_t ntargets, uint64_t npieces, uint64_t room)
{
    PiecesRoundPlan p{};
    const uint64_t pages = room / kPiecesHalf + npieces + 2;
    if (nitems >= 0xFFFFFFFFull || ntargets >= 0xFFFFFFFFull || npieces >= 0xFFFFFFFFull || pages >= 0xFFFFFFFFull || room >= (1ull << 44)) return p;
    uint64_t off = 0;
    auto carve = [&](uint64_t bytes) { PiecesRegion r{off, bytes}; off = (off + bytes + kPiecesAlign - 1) & ~(kPiecesAlign - 1); return r; };
    p.targets = carve(ntargets * 24);        // PieceTarget
    p.found = carve(ntargets * 16);          // dynamic hits, then stored hits
    p.rows = carve(npieces * 32);            // PieceRow
    p.ends = carve(npieces * 16);            // SpecEnd
    p.status = carve(npieces * 16);          // InfStatus: the decoder writes one per segment
    p.ostart = carve(npieces * 8);           // where a piece's output starts inside its item
    p.ranges = carve(nitems * 8);            // the chained pieces of every item, for the window composition
    p.cnt = carve(64);                       // [0] pages taken
    p.owner = carve(pages * 8);
    p.windows = carve(npieces * kPiecesRing);
    p.entry = carve(kPiecesRing);            // zeros: what lies in front of an item's first piece
    p.tails = carve(npieces * kPiecesRing * 2);
    p.mid = carve(pages * kPiecesHalf * 2);
    p.page_cap = pages;
    p.total = off;
    return p;
}

} // namespace zgpu
