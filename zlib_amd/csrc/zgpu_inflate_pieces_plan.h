// zgpu_inflate_pieces_plan.h -- internal (not installed): what the piece path of the blocking batch decode (zgpu_inflate_batch_pieces.hip) decides from
// plain numbers: which items are long, how far apart their pieces and their block finders stand, which of the finders' hits become piece starts,
// how a call's long items are split into rounds and how a round's scratch is laid out; and, for the sizing form of the path (at the end), the verdict
// over an item's counted pieces and the sizing round's plan; and, for the verify form (behind that), the verdict over an item's tails records, the slot
// cap and the verify round's plan.  No HIP type and no include but <cstdint>: tests/tools/inflate_pieces_plan_model.cpp,
// tests/tools/inflate_sizes_pieces_model.cpp and tests/tools/inflate_verify_pieces_model.cpp run the same code on a machine without a GPU.  The functions the device runs too carry ZGPU_PIECES_HD, which is
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
constexpr uint64_t kPiecesRoundBytesDefault = 512ull << 20; // ZGPU_BATCH_PIECES_ROUND_BYTES: bytes of output room one round of the DECODE serves (no meaning for sizing, which has no rooms)
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

// ---- the sizing form (the sizing pass of the sizes and the packed call, batch_pieces_sizes_run) ----
// The decoded size of a stream is a function of its symbols alone: a piece that starts at a block boundary is COUNTED with no knowledge of the 32 KiB in
// front of it.  What a piece cannot settle alone is settled by the chain below from plain numbers per piece: where it ended, how many bytes it counted,
// whether it saw the final block, and `need` -- how far its matches reach in front of its own first byte.
constexpr uint64_t kPiecesItemLimit = 0xFFFF0000ull; // the one-workgroup decoder's limit of an item's decoded size (a piece's count stops there too)

// does a piece that ended at bit eb hand over to this start?  A plain start: exactly there.  A stored start (the LEN of a stored block): 3 header bits and
// up to 7 of padding lie between, all zeros -- BFINAL 0, type stored, padding.  Termination: ten bits at most.
ZGPU_PIECES_HD inline bool pieces_links(const uint8_t *in, uint64_t eb, uint64_t start)
{
    if (!(start & kPiecesStoredFlag)) return eb == start;
    const uint64_t s = start & ~kPiecesStoredFlag;
    if (eb + 3 > s || eb + 10 < s) return false;
    for (uint64_t q = eb; q < s; q++) if ((in[q >> 3] >> (q & 7)) & 1u) return false;
    return true;
}

// The verdict over one item's pieces.  ends[i]: .end_bit, .out_bytes, .flags (bit 0 the final block, bits 8.. an error; all ones: never written);
// need[i]: the largest (distance - bytes the piece had counted in front of that token) over piece i's matches, floored at 0 (piece 0's reach is its own
// error); rows[i].start: the piece's start as selected; the item's body begins at byte body_lo and the item ends in front of byte in_hi of `in`.
// Clean: every piece up to the one that saw the final block ended without error and linked to the next start, the final block ends inside the item, the
// total is within the item limit, and no piece i > 0 needs more than pieces 0 .. i - 1 counted -- the sizing form of "no back-reference reaches in
// front of the item's first byte", which the decode learns in its resolve pass.  `used`: pieces up to the final one (meaningful when clean).
// Termination: one step per piece, pieces_links in each.
struct PiecesSizesVerdict { uint64_t total, end_bit; uint32_t used, clean; };
template <class End, class Row>
ZGPU_PIECES_HD inline PiecesSizesVerdict pieces_sizes_chain(const End *ends, const uint32_t *need, const Row *rows, uint32_t npieces, const uint8_t *in, uint64_t body_lo,
                                                            uint64_t in_hi)
{
    PiecesSizesVerdict v{};
    bool ended = false, reach = false;
    for (uint32_t i = 0; i < npieces; i++) {
        if (ends[i].flags >> 8) break; // an error (a count that would pass the item limit is one), or never written
        if (i > 0 && need[i] > v.total) { reach = true; break; }
        v.total += ends[i].out_bytes; v.used = i + 1;
        if (ends[i].flags & 1u) { ended = true; v.end_bit = ends[i].end_bit; break; }
        if (i + 1 == npieces || !pieces_links(in, ends[i].end_bit, rows[i + 1].start)) break;
    }
    v.clean = (ended && !reach && v.total <= kPiecesItemLimit && v.end_bit >= body_lo * 8 && v.end_bit <= in_hi * 8) ? 1u : 0u;
    return v;
}

// A sizing round's scratch: per finder its row and its two results, per piece slot its row, end record, status, output start (the selection's list of
// starts stands there first) and need.  There is no term in the room: there is no room.
constexpr uint64_t kPiecesSizesPerPieceBytes = 32 + 16 + 16 + 8 + 4;
struct PiecesSizesRoundPlan {
    PiecesRegion targets, found, rows, ends, status, ostart, need; // in this order
    uint64_t total; // 0: the round cannot be had (2^32 - 1 items, finders or slots, or more)
};
constexpr int kPiecesSizesRegions = 7;
inline const PiecesRegion &pieces_sizes_region(const PiecesSizesRoundPlan &p, int i)
{
    const PiecesRegion *r[kPiecesSizesRegions] = {&p.targets, &p.found, &p.rows, &p.ends, &p.status, &p.ostart, &p.need};
    return *r[i];
}
inline const char *pieces_sizes_region_name(int i)
{
    static const char *const names[kPiecesSizesRegions] = {"targets", "found", "rows", "ends", "status", "ostart", "need"};
    return i >= 0 && i < kPiecesSizesRegions ? names[i] : "";
}
inline PiecesSizesRoundPlan pieces_sizes_round_plan(uint64_t nitems, uint64_t ntargets, uint64_t npieces)
{
    PiecesSizesRoundPlan p{};
    if (nitems >= 0xFFFFFFFFull || ntargets >= 0xFFFFFFFFull || npieces >= 0xFFFFFFFFull) return p;
    uint64_t off = 0;
    auto carve = [&](uint64_t bytes) { PiecesRegion r{off, bytes}; off = (off + bytes + kPiecesAlign - 1) & ~(kPiecesAlign - 1); return r; };
    p.targets = carve(ntargets * 24);
    p.found = carve(ntargets * 16);
    p.rows = carve(npieces * 32);
    p.ends = carve(npieces * 16);
    p.status = carve(npieces * 16);
    p.ostart = carve(npieces * 8);
    p.need = carve(npieces * 4);
    p.total = off;
    return p;
}
// what a long item adds to a sizing round's scratch (its room does not count)
ZGPU_PIECES_HD inline uint64_t pieces_sizes_item_scratch(const PiecesItemCost &c)
{
    return (uint64_t)c.piece_cap * kPiecesSizesPerPieceBytes + (uint64_t)c.ntargets * kPiecesPerTargetBytes;
}
// The sizing round that begins with long item `first` of `nlong`: it ends behind item (return value) - 1.  Items are taken in order while their scratch
// (with the regions' alignment) stays within kPiecesScratchCap, their slots and finders below 2^32 - 1, and -- slot_cap, ZGPU_BATCH_PIECES_SIZES_ROUND_SLOTS,
// 0: no cap -- their slots within the cap; an item that alone passes a limit makes a round of its own.  ZGPU_BATCH_PIECES_ROUND_BYTES has no meaning
// here.  Every long item is in exactly one round.  Termination: k grows by one per step and stops at nlong.
inline uint64_t pieces_sizes_round_end(const PiecesItemCost *c, uint64_t nlong, uint64_t first, uint64_t slot_cap)
{
    uint64_t scratch = kPiecesSizesRegions * kPiecesAlign, slots = 0, targets = 0, k = first;
    while (k < nlong) {
        const uint64_t s = pieces_sizes_item_scratch(c[k]);
        if (k > first && (scratch + s > kPiecesScratchCap || slots + c[k].piece_cap >= 0xFFFFFFFFull || targets + c[k].ntargets >= 0xFFFFFFFFull || k - first + 1 >= 0xFFFFFFFFull ||
                          (slot_cap && slots + c[k].piece_cap > slot_cap)))
            break;
        scratch += s; slots += c[k].piece_cap; targets += c[k].ntargets; k++;
    }
    return k;
}

// ---- the verify form (the blocking integrity test, batch_pieces_verify_run) ----
// Check values need every byte, in order, with the real 32 KiB in front of every piece -- and the integrity test allocates no room for a decoded byte.  So
// the pieces are decoded twice, both times into LDS alone: the tails pass (the rowed SPEC decode with no pages) leaves per slot its tail -- the last
// 32 Ki symbols, markers included -- and its end record; the chain below and the window kernels turn the tails into per-slot byte windows; the check pass
// decodes every chained piece again behind the window of the slot in front and folds its bytes.  A slot costs its tail, its window and its records:
// nothing is proportional to an item's decoded size or to the number of items.
// ZGPU_BATCH_PIECES_VERIFY_MIN_BYTES when neither it nor ZGPU_BATCH_PIECES_MIN_BYTES is set: decided by profiles/r14_batch_verify_long_table.txt.  Two passes
// over every piece lose to the one-workgroup verifier on 256 items with bodies of 318 KB (46.6 ms against 18.9 ms) and win on 16 items with bodies of
// 20,481,854 bytes (381 ms against 986 ms): the smallest measured body at which the path wins, rounded down.  Nothing between the two has been measured.
constexpr uint64_t kPiecesVerifyMinBytesDefault = 20000000;
constexpr uint64_t kPiecesVerifyRoundSlotsDefault = 1024; // ZGPU_BATCH_PIECES_VERIFY_ROUND_SLOTS: one residency of the check kernel, four workgroups on each of 256 CUs
// per piece slot: its tail (16-bit symbols), its window (bytes), its row, end record, status, output start and check record
constexpr uint64_t kPiecesVerifyPerPieceBytes = 2ull * kPiecesRing + kPiecesRing + 32 + 16 + 16 + 8 + 32;
// the slot cap rounds are made under: the knob (0: the default), and never so many slots that a round of items within the cap would pass kPiecesScratchCap
ZGPU_PIECES_HD inline uint64_t pieces_verify_slot_cap(uint64_t knob)
{
    const uint64_t most = (kPiecesScratchCap / 2) / kPiecesVerifyPerPieceBytes, cap = knob ? knob : kPiecesVerifyRoundSlotsDefault;
    return cap < most ? cap : most;
}

// The verdict over one item's tails records: pieces_sizes_chain without its `need` term (a reach in front of the item is the check pass's to find, exactly:
// it knows where every piece starts).  ostart[i] receives where piece i's output starts inside its item, for every piece up to the final one.
// Termination: one step per piece, pieces_links in each.
template <class End, class Row>
ZGPU_PIECES_HD inline PiecesSizesVerdict pieces_verify_chain(const End *ends, const Row *rows, uint32_t npieces, const uint8_t *in, uint64_t body_lo, uint64_t in_hi, uint64_t *ostart)
{
    PiecesSizesVerdict v{};
    bool ended = false;
    for (uint32_t i = 0; i < npieces; i++) {
        if (ends[i].flags >> 8) break; // an error, or never written
        ostart[i] = v.total;
        v.total += ends[i].out_bytes; v.used = i + 1;
        if (ends[i].flags & 1u) { ended = true; v.end_bit = ends[i].end_bit; break; }
        if (i + 1 == npieces || !pieces_links(in, ends[i].end_bit, rows[i + 1].start)) break;
    }
    v.clean = (ended && v.total <= kPiecesItemLimit && v.end_bit >= body_lo * 8 && v.end_bit <= in_hi * 8) ? 1u : 0u;
    return v;
}

// A verify round's scratch.  The small records first, then one entry of zeros (what lies in front of an item's first piece, for the window composition),
// the windows and the tails.  There is no term in an item's decoded size: there is no room and there are no pages.
struct PiecesVerifyRoundPlan {
    PiecesRegion targets, found, rows, ends, status, ostart, checks, ranges, entry, windows, tails; // in this order
    uint64_t total; // 0: the round cannot be had (2^32 - 1 items, finders or slots, or more)
};
constexpr int kPiecesVerifyRegions = 11;
inline const PiecesRegion &pieces_verify_region(const PiecesVerifyRoundPlan &p, int i)
{
    const PiecesRegion *r[kPiecesVerifyRegions] = {&p.targets, &p.found, &p.rows, &p.ends, &p.status, &p.ostart, &p.checks, &p.ranges, &p.entry, &p.windows, &p.tails};
    return *r[i];
}
inline const char *pieces_verify_region_name(int i)
{
    static const char *const names[kPiecesVerifyRegions] = {"targets", "found", "rows", "ends", "status", "ostart", "checks", "ranges", "entry", "windows", "tails"};
    return i >= 0 && i < kPiecesVerifyRegions ? names[i] : "";
}
inline PiecesVerifyRoundPlan pieces_verify_round_plan(uint64_t nitems, uint64_t ntargets, uint64_t npieces)
{
    PiecesVerifyRoundPlan p{};
    if (nitems >= 0xFFFFFFFFull || ntargets >= 0xFFFFFFFFull || npieces >= 0xFFFFFFFFull) return p;
    uint64_t off = 0;
    auto carve = [&](uint64_t bytes) { PiecesRegion r{off, bytes}; off = (off + bytes + kPiecesAlign - 1) & ~(kPiecesAlign - 1); return r; };
    p.targets = carve(ntargets * 24);
    p.found = carve(ntargets * 16);
    p.rows = carve(npieces * 32);
    p.ends = carve(npieces * 16);
    p.status = carve(npieces * 16);
    p.ostart = carve(npieces * 8);
    p.checks = carve(npieces * 32);          // PieceCheck
    p.ranges = carve(nitems * 8);            // the chained pieces of every item, for the window composition
    p.entry = carve(kPiecesRing);            // zeros
    p.windows = carve(npieces * kPiecesRing);
    p.tails = carve(npieces * kPiecesRing * 2);
    p.total = off;
    return p;
}
// what a long item adds to a verify round's scratch (its room and its decoded size do not count)
ZGPU_PIECES_HD inline uint64_t pieces_verify_item_scratch(const PiecesItemCost &c)
{
    return (uint64_t)c.piece_cap * kPiecesVerifyPerPieceBytes + (uint64_t)c.ntargets * kPiecesPerTargetBytes + 8;
}
// Rounds are made by pieces_sizes_round_end under pieces_verify_slot_cap: a round of more than one item has `cap` slots at most, so its piece scratch is
// bounded by max(cap, the largest item's piece_cap) * kPiecesVerifyPerPieceBytes whatever the call holds.

} // namespace zgpu
