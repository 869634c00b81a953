// zgpu_inflate_batch_pieces.hip -- the long items of a blocking batch decode (inflate_batch_run_ranges, zgpu_inflate_batch.hip), decoded in pieces.
// One workgroup per item leaves the chip idle when the items are few and large.  A deflate body of min_bytes or more is a LONG item: it is cut into pieces
// at block starts found by search, as zgpu_inflate_stream.hip cuts one foreign stream, and the pieces of ALL long items of a call share the launches:
//   classify  (batch_header_kernel) which items are long; they leave the segment table for a list of their own, so the one-workgroup decoder skips them
//   round     (one workgroup)      where the finders and the piece slots of every item of the round begin (an exclusive scan)
//   targets   (a workgroup / item) the finders' table: bit range and the ITEM's end
//   find      spec_find_kernel in its table form
//   select    (a lane / item)      pieces_select (zgpu_inflate_pieces_plan.h) over what the item's finders report: the piece rows
//   decode    inflate_kernel_t<SPEC> over the rows: a first piece has nothing in front of it, every read ends with the item
//   chain     (a lane / item)      every piece must end where the next starts, the last with the final block, the total within the room: clean, or fall back
//   windows, resolve               spec_window_rel / abs and spec_resolve_kernel, item by item
//   status    (a lane / item)      a clean item gets the record the one-workgroup decoder would write; the others are gathered
//   fallback                       ONE kInfBatch launch over the gathered items, their records scattered back: the verdict of anything that is not clean
//                                  (damage, a false start, a room too small, a page that was missing) is the one-workgroup decoder's by construction
// There are no repair rounds and no retry.  The number of long items and their sums come home with the caller's own round trip behind the decoder's
// launch (a call without long items pays no synchronize for asking), their costs only when they pass one round's room, the counters at the end; nothing
// else crosses: no kernel waits on another workgroup, the stages are ordered by the stream.
// Two more forms of the path follow the decode's: the sizing form (batch_pieces_sizes_run: the pieces counted, no bytes at all) and the verify form
// (batch_pieces_verify_run: the pieces decoded twice inside LDS, check values joined, scratch bounded by a slot cap).
#include "zgpu_common.h"
#include "zgpu_engine.h"
#include "zgpu_inflate_dev.h"
#include "zgpu_inflate_pieces_plan.h"
#include <atomic>
#include <cstdlib>
#include <vector>

static std::atomic<uint64_t> g_pieces_done{0}, g_pieces_fell{0};
static std::atomic<uint64_t> g_sizes_done{0}, g_sizes_fell{0}; // the sizing form (batch_pieces_sizes_run): counted apart, also inside a packed call
static std::atomic<uint64_t> g_verify_done{0}, g_verify_fell{0}; // the verify form (batch_pieces_verify_run): counted apart again

namespace zgpu {
static_assert(kPiecesRing == kOutRing && kPiecesHalf == kOutHalf && kPiecesStoredFlag == (1ull << 62), "zgpu_inflate_pieces_plan.h states the decoder's ring as numbers");
static_assert(sizeof(PieceTarget) == 24 && sizeof(PieceRow) == 32 && sizeof(SpecEnd) == 16 && sizeof(InfStatus) == 16 && sizeof(PiecesItemCost) == 16,
              "zgpu_inflate_pieces_plan.h states the record sizes as numbers");

// what the piece path keeps for the whole call (the round's scratch is the engine's inf_slots): the long items, and the fallback's compact segment table,
// item numbers and records
// (fbmeta, the verify form only: the fallback's compact check records, behind the rest, so that the list lies where it lies in the other two forms)
struct PiecesCall { PieceItem *items; uint64_t *fbseg; uint32_t *fbmap; InfStatus *fbstatus; ChunkMeta *fbmeta; };
static PiecesCall pieces_call(uint8_t *scr, uint64_t max_long, size_t *total, bool verify = false)
{
    Carve at;
    const size_t o_items = at(max_long * sizeof(PieceItem)), o_seg = at(max_long * 32), o_map = at(max_long * 4), o_st = at(max_long * sizeof(InfStatus));
    const size_t o_meta = verify ? at(max_long * sizeof(ChunkMeta)) : 0;
    if (total) *total = at.off;
    PiecesCall c{};
    if (scr) {
        c.items = reinterpret_cast<PieceItem *>(scr + o_items); c.fbseg = reinterpret_cast<uint64_t *>(scr + o_seg); c.fbmap = reinterpret_cast<uint32_t *>(scr + o_map);
        c.fbstatus = reinterpret_cast<InfStatus *>(scr + o_st);
        if (verify) c.fbmeta = reinterpret_cast<ChunkMeta *>(scr + o_meta);
    }
    return c;
}

// One workgroup: target0 and slot0 of the round's items, exclusive scans of ntargets and piece_cap (their totals are the host's already)
// Termination: two passes over the thread's items, a scan of ten steps (the pattern of batch_piece_scan_kernel).
__global__ void __launch_bounds__(1024) pieces_round_kernel(PieceItem *items, uint32_t nitems)
{
    __shared__ unsigned long long pt[1024], ps[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = ((uint64_t)nitems + 1023) / 1024, a = tid * per < nitems ? tid * per : nitems, z = (tid + 1) * per < nitems ? (tid + 1) * per : nitems;
    unsigned long long st = 0, ss = 0;
    for (uint64_t i = a; i < z; i++) { st += items[i].ntargets; ss += items[i].piece_cap; }
    pt[tid] = st; ps[tid] = ss;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long at = tid >= d ? pt[tid - d] : 0, as = tid >= d ? ps[tid - d] : 0;
        __syncthreads();
        pt[tid] += at; ps[tid] += as;
        __syncthreads();
    }
    unsigned long long ot = pt[tid] - st, os = ps[tid] - ss;
    for (uint64_t i = a; i < z; i++) { items[i].target0 = (uint32_t)ot; items[i].slot0 = (uint32_t)os; ot += items[i].ntargets; os += items[i].piece_cap; }
}

// one workgroup per item: the rows of its finders.  Termination: ntargets / 256 steps a thread.
__global__ void __launch_bounds__(256) pieces_targets_kernel(const PieceItem *__restrict__ items, uint32_t nitems, PieceTarget *table)
{
    if (blockIdx.x >= nitems) return;
    const PieceItem it = items[blockIdx.x];
    const uint64_t fsp = pieces_geom(it.in_hi - it.body_lo).fspacing;
    for (uint32_t t = threadIdx.x; t < it.ntargets; t += 256)
        table[it.target0 + t] = PieceTarget{pieces_target_lo(it.body_lo, fsp, t + 1), pieces_target_hi(it.body_lo, it.in_hi, fsp, it.ntargets, t + 1), it.in_hi};
}

// one lane per item: the selection, and the item's rows -- piece i from its start to the next one's (the last: to the bit behind the item), every read
// bounded by the item's end; the slots the item does not use are marked.  The starts stand in the rows' own `start` fields while they are selected.
// Termination: pieces_select's, then two passes over the item's piece_cap slots.
__global__ void __launch_bounds__(64) pieces_select_kernel(PieceItem *items, uint32_t nitems, const uint8_t *__restrict__ in, const uint64_t *__restrict__ found, uint32_t ntargets,
                                                           PieceRow *rows, uint64_t *scratch_starts)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nitems) return;
    const PieceItem it = items[j];
    uint64_t *starts = scratch_starts + it.slot0; // (the round's ostart region: the chain kernel writes it later)
    const uint32_t np = pieces_select(found + it.target0, found + ntargets + it.target0, it.ntargets, in, it.body_lo * 8, it.in_hi, pieces_geom(it.in_hi - it.body_lo).spacing, starts,
                                      it.piece_cap);
    for (uint32_t i = 0; i < it.piece_cap; i++) {
        PieceRow r{};
        r.item = kPieceNoItem;
        if (i < np) { r.start = starts[i]; r.stop = i + 1 < np ? starts[i + 1] : it.in_hi * 8; r.in_end = it.in_hi; r.item = j; r.first = i == 0 ? 1u : 0u; }
        rows[it.slot0 + i] = r;
    }
    items[j].npieces = np;
}

// one lane per item: the chain (what inflate_spec_run checks on the host, the input read here).  ostart[slot]: where the piece's output starts inside its
// item.  Clean: every piece up to the one that saw the final block ended where the next one starts, the total is within the item's room, no piece went
// without a page and the final block ends inside the item.  Anything else -- an error in any piece, a false start, a broken chain -- is "fall back".
// Termination: one step per piece in use (npieces <= piece_cap); pieces_links looks at ten bits at most.
__global__ void __launch_bounds__(64) pieces_chain_kernel(PieceItem *items, uint32_t nitems, const uint8_t *__restrict__ in, const PieceRow *__restrict__ rows,
                                                          const SpecEnd *__restrict__ ends, uint64_t *ostart, uint2 *ranges)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nitems) return;
    const PieceItem it = items[j];
    uint64_t total = 0, end_bit = 0;
    uint32_t used = 0;
    bool ended = false, dry = false;
    for (uint32_t i = 0; i < it.npieces; i++) {
        const SpecEnd e = ends[it.slot0 + i];
        if (e.flags >> 8) break; // an error (or never written)
        ostart[it.slot0 + i] = total;
        total += e.out_bytes; used = i + 1; dry = dry || (e.flags & 2u);
        if (e.flags & 1u) { ended = true; end_bit = e.end_bit; break; }
        if (i + 1 == it.npieces || !pieces_links(in, e.end_bit, rows[it.slot0 + i + 1].start)) break;
    }
    const bool clean = ended && !dry && total <= it.out_hi - it.out_lo && end_bit >= it.body_lo * 8 && end_bit <= it.in_hi * 8;
    items[j].total = total; items[j].end_bit = end_bit; items[j].npieces = clean ? used : 0u; items[j].clean = clean ? 1u : 0u; items[j].bad = 0;
    ranges[j] = clean ? make_uint2(it.slot0, it.slot0 + used) : make_uint2(0u, 0u);
}

// one lane per item, behind the resolve pass (or, for a round that got no scratch, behind nothing: clean is 0 then): the item's state goes back to the
// header's verdict (the caller's first merge has put the verdict of the empty segment there), and a clean item's record is written, as the
// one-workgroup decoder writes it for an item that fits its range; every other item into the fallback's compact segment table
__global__ void __launch_bounds__(256) pieces_status_kernel(const PieceItem *__restrict__ items, uint32_t nitems, BatchItemState *states, InfStatus *status, uint64_t *fbseg,
                                                            uint32_t *fbmap, unsigned long long *hdr)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nitems) return;
    const PieceItem it = items[j];
    states[it.k].code = ZGPU_OK; states[it.k].msg = kMsgNone; // (a long item's header was fine: the merge that follows takes the decoder's record)
    if (it.clean && !it.bad) {
        const uint64_t bits = it.end_bit - it.body_lo * 8;
        InfStatus s{};
        s.code = ZGPU_OK; s.msg = (uint32_t)(bits & 7u) << 24; s.out_bytes = (uint32_t)it.total; s.used = (uint32_t)((bits + 7) >> 3) | (1u << 31);
        status[it.k] = s;
        atomicAdd(&hdr[kHdrClean], 1ull);
        return;
    }
    const uint64_t at = atomicAdd(&hdr[kHdrGathered], 1ull);
    fbseg[4 * at] = it.body_lo; fbseg[4 * at + 1] = it.in_hi; fbseg[4 * at + 2] = it.out_lo; fbseg[4 * at + 3] = it.out_hi;
    fbmap[at] = it.k;
    atomicAdd(&hdr[kHdrFell], 1ull);
}

__global__ void __launch_bounds__(256) pieces_scatter_kernel(const InfStatus *__restrict__ fbstatus, const uint32_t *__restrict__ fbmap, const unsigned long long *__restrict__ hdr,
                                                             uint32_t nitems, InfStatus *status, const ChunkMeta *__restrict__ fbmeta = nullptr, ChunkMeta *meta = nullptr)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nitems || j >= hdr[kHdrGathered]) return;
    status[fbmap[j]] = fbstatus[j];
    if (fbmeta) meta[fbmap[j]] = fbmeta[j]; // (the verify form: the fallback's check values go with its record)
}

BatchPiecesKnobs batch_pieces_knobs()
{
    BatchPiecesKnobs k{kPiecesMinBytesDefault, kPiecesRoundBytesDefault};
    if (const char *v = getenv("ZGPU_BATCH_PIECES_MIN_BYTES")) k.min_bytes = strtoull(v, nullptr, 10);
    if (const char *v = getenv("ZGPU_BATCH_PIECES_ROUND_BYTES")) { const uint64_t r = strtoull(v, nullptr, 10); if (r) k.round_bytes = r; }
    return k;
}
uint64_t batch_pieces_count(int which) { return which == 0 ? g_pieces_done.load() : which == 1 ? g_pieces_fell.load() : 0; }
size_t batch_pieces_scratch_bytes(uint64_t max_long) { size_t total = 0; pieces_call(nullptr, max_long, &total); return total; }

PieceItem *batch_pieces_items(uint8_t *scr) { return pieces_call(scr, 0, nullptr).items; }

int batch_pieces_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, uint8_t *d_out, uint64_t out_cap, uint64_t max_long, uint8_t *scr, unsigned long long *d_hdr,
                     const unsigned long long *hdr, BatchItemState *states, InfStatus *status, uint64_t round_bytes, int ring_kb, hipStream_t st)
{
    const PiecesCall c = pieces_call(scr, max_long, nullptr);
    unsigned long long h[8] = {};
    for (int i = 0; i < 8; i++) h[i] = hdr[i];
    const uint64_t nlong = h[kHdrLong];
    if (nlong == 0) return ZGPU_OK;
    // one round serves everything, or the list of long items comes home (80 bytes each) and pieces_round_end cuts it
    std::vector<PiecesItemCost> cost;
    const PiecesItemCost all{h[kHdrRoom], 0, 0};
    const bool one = h[kHdrRoom] <= round_bytes && nlong < 0xFFFFFFFFull && h[kHdrTargets] < 0xFFFFFFFFull && h[kHdrSlots] < 0xFFFFFFFFull &&
                     pieces_item_scratch(all) + h[kHdrSlots] * kPiecesPerPieceBytes + h[kHdrTargets] * kPiecesPerTargetBytes <= kPiecesScratchCap;
    if (!one) {
        std::vector<PieceItem> list(nlong);
        ZGPU_HIP_CHECK(hipMemcpyAsync(list.data(), c.items, nlong * sizeof(PieceItem), hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        cost.resize(nlong);
        for (uint64_t j = 0; j < nlong; j++) cost[j] = PiecesItemCost{list[j].out_hi - list[j].out_lo, list[j].ntargets, list[j].piece_cap};
    }
    for (uint64_t j0 = 0; j0 < nlong;) {
        uint64_t j1 = nlong, targets = h[kHdrTargets], slots = h[kHdrSlots], room = h[kHdrRoom];
        if (!one) {
            j1 = pieces_round_end(cost.data(), nlong, j0, round_bytes);
            targets = slots = room = 0;
            for (uint64_t j = j0; j < j1; j++) { targets += cost[j].ntargets; slots += cost[j].piece_cap; room += cost[j].room; }
        }
        const uint32_t ni = (uint32_t)(j1 - j0), igrid = (ni + 255) / 256;
        PieceItem *items = c.items + j0;
        const PiecesRoundPlan p = pieces_round_plan(ni, targets, slots, room);
        // Declining is no error: the round's items go to the one-workgroup decoder, which needs no scratch.  A hipMalloc that failed stays the thread's last
        // error until it is fetched: it is fetched here, so that the check behind the round's launches sees the launches alone.
        // (ZGPU_BATCH_PIECES_NO_SCRATCH=1, tests: every round is declined as if its scratch could not be had)
        uint8_t *base = nullptr;
        if (p.total != 0 && !getenv("ZGPU_BATCH_PIECES_NO_SCRATCH")) {
            if (e->inf_slots.reserve(nullptr, p.total)) (void)hipGetLastError();
            else base = e->inf_slots.p;
        }
        ZGPU_HIP_CHECK(hipMemsetAsync(d_hdr + kHdrGathered, 0, 8, st));
        ZGPU_HIP_CHECK(hipMemsetAsync(c.fbseg + 4 * j0, 0, (size_t)ni * 32, st));
        if (base) {
            const uint32_t nt = (uint32_t)targets, ns = (uint32_t)slots;
            PieceTarget *table = reinterpret_cast<PieceTarget *>(base + p.targets.off);
            uint64_t *found = reinterpret_cast<uint64_t *>(base + p.found.off), *ostart = reinterpret_cast<uint64_t *>(base + p.ostart.off);
            PieceRow *rows = reinterpret_cast<PieceRow *>(base + p.rows.off);
            uint2 *ranges = reinterpret_cast<uint2 *>(base + p.ranges.off);
            SpecArgs sp{};
            sp.mid = reinterpret_cast<uint16_t *>(base + p.mid.off); sp.page_owner = reinterpret_cast<uint64_t *>(base + p.owner.off);
            sp.page_count = reinterpret_cast<uint32_t *>(base + p.cnt.off); sp.page_cap = (uint32_t)p.page_cap;
            sp.tails = reinterpret_cast<uint16_t *>(base + p.tails.off); sp.ends = reinterpret_cast<SpecEnd *>(base + p.ends.off); sp.rows = rows;
            ZGPU_HIP_CHECK(hipMemsetAsync(sp.page_count, 0, 64, st));
            ZGPU_HIP_CHECK(hipMemsetAsync(sp.ends, 0xFF, (size_t)ns * sizeof(SpecEnd), st));
            ZGPU_HIP_CHECK(hipMemsetAsync(base + p.entry.off, 0, kOutRing, st));
            hipLaunchKernelGGL(pieces_round_kernel, dim3(1), dim3(1024), 0, st, items, ni);
            hipLaunchKernelGGL(pieces_targets_kernel, dim3(ni), dim3(256), 0, st, items, ni, table);
            launch_spec_find_table(d_in, in_bytes, table, nt, found, st);
            hipLaunchKernelGGL(pieces_select_kernel, dim3((ni + 63) / 64), dim3(64), 0, st, items, ni, d_in, found, nt, rows, ostart);
            for (uint32_t c0 = 0; c0 < ns; c0 += 65536) {
                const uint32_t nb = ns - c0 < 65536 ? ns - c0 : 65536;
                InfLaunch a{d_in, in_bytes, nullptr, c0, nb, d_out, out_cap, reinterpret_cast<InfStatus *>(base + p.status.off) + c0};
                launch_inflate_decode(kInfPieces, kInfNoRing, a, sp, st);
            }
            hipLaunchKernelGGL(pieces_chain_kernel, dim3((ni + 63) / 64), dim3(64), 0, st, items, ni, d_in, rows, sp.ends, ostart, ranges);
            launch_spec_resolve_items(sp, ns, ni, ranges, base + p.entry.off, base + p.windows.off, ostart, items, d_out, st);
        }
        hipLaunchKernelGGL(pieces_status_kernel, dim3(igrid), dim3(256), 0, st, items, ni, states, status, c.fbseg + 4 * j0, c.fbmap + j0, d_hdr);
        // the fallback: the gathered items lead the round's compact table, the entries behind them are empty
        for (uint32_t c0 = 0; c0 < ni; c0 += 65536) {
            const uint32_t nb = ni - c0 < 65536 ? ni - c0 : 65536;
            launch_inflate_decode(kInfBatch, ring_kb, InfLaunch{d_in, in_bytes, c.fbseg + 4 * j0, c0, nb, d_out, out_cap, c.fbstatus + j0 + c0}, SpecArgs{}, st);
        }
        hipLaunchKernelGGL(pieces_scatter_kernel, dim3(igrid), dim3(256), 0, st, c.fbstatus + j0, c.fbmap + j0, d_hdr, ni, status);
        ZGPU_HIP_CHECK(hipGetLastError());
        j0 = j1;
    }
    ZGPU_HIP_CHECK(hipMemcpyAsync(h, d_hdr, sizeof h, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    g_pieces_done += h[kHdrClean]; g_pieces_fell += h[kHdrFell];
    return ZGPU_OK;
}

// ---- the sizing form: the long items of a sizing pass (inflate_batch_sizes_launch, zgpu_inflate_batch.hip), counted in pieces ----
// classify, round, targets, find and select are the decode's, kernel for kernel; then
//   count     inflate_kernel_t<SPEC, SIZES> over the rows: one wave per slot, an end record and a need per slot
//   chain     (a lane / item)      pieces_sizes_chain (zgpu_inflate_pieces_plan.h): clean, or fall back
//   status    pieces_status_kernel: a clean item gets the record the one-wave sizing kernel would write, the others are gathered
//   fallback  ONE kInfSizes launch over the gathered items, their records scattered back: the verdict of anything that is not clean (damage, a cut item, a
//             false start, a reach in front of the item, an item over the limit) is the one-wave sizing kernel's by construction
// No pages, no windows, no resolve pass, no destination; no repair rounds, no retry, no kernel that waits on another workgroup: the stream orders the stages.

// one lane per item: the verdict.  Termination: pieces_sizes_chain's, one step per piece in use.
__global__ void __launch_bounds__(64) pieces_sizes_chain_kernel(PieceItem *items, uint32_t nitems, const uint8_t *__restrict__ in, const PieceRow *__restrict__ rows,
                                                                const SpecEnd *__restrict__ ends, const uint32_t *__restrict__ need)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nitems) return;
    const PieceItem it = items[j];
    const PiecesSizesVerdict v = pieces_sizes_chain(ends + it.slot0, need + it.slot0, rows + it.slot0, it.npieces, in, it.body_lo, it.in_hi);
    items[j].total = v.total; items[j].end_bit = v.end_bit; items[j].npieces = v.clean ? v.used : 0u; items[j].clean = v.clean; items[j].bad = 0;
}

BatchPiecesSizesKnobs batch_pieces_sizes_knobs()
{
    BatchPiecesSizesKnobs k{batch_pieces_knobs().min_bytes, 0};
    if (const char *v = getenv("ZGPU_BATCH_PIECES_SIZES_MIN_BYTES")) k.min_bytes = strtoull(v, nullptr, 10);
    if (const char *v = getenv("ZGPU_BATCH_PIECES_SIZES_ROUND_SLOTS")) k.round_slots = strtoull(v, nullptr, 10);
    return k;
}
uint64_t batch_pieces_sizes_count(int which) { return which == 0 ? g_sizes_done.load() : which == 1 ? g_sizes_fell.load() : 0; }

int batch_pieces_sizes_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, uint64_t max_long, uint8_t *scr, unsigned long long *d_hdr, const unsigned long long *hdr,
                           BatchItemState *states, InfStatus *status, uint64_t round_slots, hipStream_t st)
{
    const PiecesCall c = pieces_call(scr, max_long, nullptr);
    unsigned long long h[8] = {};
    for (int i = 0; i < 8; i++) h[i] = hdr[i];
    const uint64_t nlong = h[kHdrLong];
    if (nlong == 0) return ZGPU_OK;
    // one round serves everything, or the list of long items comes home and pieces_sizes_round_end cuts it
    std::vector<PiecesItemCost> cost;
    const bool one = nlong < 0xFFFFFFFFull && h[kHdrTargets] < 0xFFFFFFFFull && h[kHdrSlots] < 0xFFFFFFFFull && (round_slots == 0 || h[kHdrSlots] <= round_slots) &&
                     pieces_sizes_round_plan(nlong, h[kHdrTargets], h[kHdrSlots]).total <= kPiecesScratchCap;
    if (!one) {
        std::vector<PieceItem> list(nlong);
        ZGPU_HIP_CHECK(hipMemcpyAsync(list.data(), c.items, nlong * sizeof(PieceItem), hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        cost.resize(nlong);
        for (uint64_t j = 0; j < nlong; j++) cost[j] = PiecesItemCost{0, list[j].ntargets, list[j].piece_cap};
    }
    for (uint64_t j0 = 0; j0 < nlong;) {
        uint64_t j1 = nlong, targets = h[kHdrTargets], slots = h[kHdrSlots];
        if (!one) {
            j1 = pieces_sizes_round_end(cost.data(), nlong, j0, round_slots);
            targets = slots = 0;
            for (uint64_t j = j0; j < j1; j++) { targets += cost[j].ntargets; slots += cost[j].piece_cap; }
        }
        const uint32_t ni = (uint32_t)(j1 - j0), igrid = (ni + 255) / 256;
        PieceItem *items = c.items + j0;
        const PiecesSizesRoundPlan p = pieces_sizes_round_plan(ni, targets, slots);
        // declining is no error, as in batch_pieces_run: the round's items go to the one-wave sizing kernel (ZGPU_BATCH_PIECES_NO_SCRATCH=1: every round)
        uint8_t *base = nullptr;
        if (p.total != 0 && p.total <= kPiecesScratchCap && !getenv("ZGPU_BATCH_PIECES_NO_SCRATCH")) {
            if (e->inf_slots.reserve(nullptr, p.total)) (void)hipGetLastError();
            else base = e->inf_slots.p;
        }
        ZGPU_HIP_CHECK(hipMemsetAsync(d_hdr + kHdrGathered, 0, 8, st));
        ZGPU_HIP_CHECK(hipMemsetAsync(c.fbseg + 4 * j0, 0, (size_t)ni * 32, st));
        if (base) {
            const uint32_t nt = (uint32_t)targets, ns = (uint32_t)slots;
            PieceTarget *table = reinterpret_cast<PieceTarget *>(base + p.targets.off);
            uint64_t *found = reinterpret_cast<uint64_t *>(base + p.found.off), *ostart = reinterpret_cast<uint64_t *>(base + p.ostart.off);
            PieceRow *rows = reinterpret_cast<PieceRow *>(base + p.rows.off);
            SpecArgs sp{};
            sp.ends = reinterpret_cast<SpecEnd *>(base + p.ends.off); sp.rows = rows; sp.need = reinterpret_cast<uint32_t *>(base + p.need.off);
            ZGPU_HIP_CHECK(hipMemsetAsync(sp.ends, 0xFF, (size_t)ns * sizeof(SpecEnd), st));
            ZGPU_HIP_CHECK(hipMemsetAsync(sp.need, 0, (size_t)ns * 4, st));
            hipLaunchKernelGGL(pieces_round_kernel, dim3(1), dim3(1024), 0, st, items, ni);
            hipLaunchKernelGGL(pieces_targets_kernel, dim3(ni), dim3(256), 0, st, items, ni, table);
            launch_spec_find_table(d_in, in_bytes, table, nt, found, st);
            hipLaunchKernelGGL(pieces_select_kernel, dim3((ni + 63) / 64), dim3(64), 0, st, items, ni, d_in, found, nt, rows, ostart);
            for (uint32_t c0 = 0; c0 < ns; c0 += 65536) {
                const uint32_t nb = ns - c0 < 65536 ? ns - c0 : 65536;
                InfLaunch a{d_in, in_bytes, nullptr, c0, nb, nullptr, 0, reinterpret_cast<InfStatus *>(base + p.status.off) + c0};
                launch_inflate_decode(kInfPieceSizes, kInfNoRing, a, sp, st);
            }
            hipLaunchKernelGGL(pieces_sizes_chain_kernel, dim3((ni + 63) / 64), dim3(64), 0, st, items, ni, d_in, rows, sp.ends, sp.need);
        }
        // (a round that got no scratch: the items' clean fields are the zeros the header kernel wrote)
        hipLaunchKernelGGL(pieces_status_kernel, dim3(igrid), dim3(256), 0, st, items, ni, states, status, c.fbseg + 4 * j0, c.fbmap + j0, d_hdr);
        for (uint32_t c0 = 0; c0 < ni; c0 += 65536) {
            const uint32_t nb = ni - c0 < 65536 ? ni - c0 : 65536;
            launch_inflate_decode(kInfSizes, kInfNoRing, InfLaunch{d_in, in_bytes, c.fbseg + 4 * j0, c0, nb, nullptr, 0, c.fbstatus + j0 + c0}, SpecArgs{}, st);
        }
        hipLaunchKernelGGL(pieces_scatter_kernel, dim3(igrid), dim3(256), 0, st, c.fbstatus + j0, c.fbmap + j0, d_hdr, ni, status);
        ZGPU_HIP_CHECK(hipGetLastError());
        j0 = j1;
    }
    ZGPU_HIP_CHECK(hipMemcpyAsync(h, d_hdr, sizeof h, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    g_sizes_done += h[kHdrClean]; g_sizes_fell += h[kHdrFell];
    return ZGPU_OK;
}

// ---- the verify form: the long items of a blocking integrity test (inflate_batch_verify_run, zgpu_inflate_batch.hip), checked in pieces ----
// Check values need every byte, in order, with the real 32 KiB in front of every piece; the integrity test has no room for a decoded byte.  classify, round,
// targets, find and select are the decode's, kernel for kernel; then
//   tails     inflate_kernel_t<SPEC> over the rows, no pages: per slot its tail (the last 32 Ki symbols, markers included) and its end record
//   chain     (a lane / item)      pieces_verify_chain (zgpu_inflate_pieces_plan.h): ostart[slot] and the item's range, or fall back; the slots no clean
//                                  chain uses are struck from the rows, so the check pass skips them
//   windows   spec_window_rel / abs, as they are: tails into per-slot byte windows.  No resolve pass: there is nothing to resolve into
//   check     inflate_kernel_t<SPEC, .., VERIFY> over the rows: every chained piece again, behind the window of the slot in front, folded: one PieceCheck a slot
//   confirm   (a lane / item)      pieces_verify_confirm (zgpu_common.h): every check ended where its tails record says, then the joined values into meta[k]
//   status    pieces_status_kernel: a clean item gets the record the one-workgroup verifier would write, the others are gathered
//   fallback  ONE kInfVerify launch over the gathered items, records and check values scattered back: the verdict of anything that is not clean (damage, a
//             cut item, a false start, a broken chain, a reach in front of the item, an item over the limit) is the one-workgroup verifier's by construction
// The caller's merge and finish kernels then run unchanged: the item is one piece of all its bytes, and its trailer is compared by the code that compares
// every trailer.  A slot costs its tail, its window and its records (kPiecesVerifyPerPieceBytes); rounds are cut under a slot cap, so the scratch depends
// neither on what the items decode to nor on how many there are.  No repair rounds, no retry, no kernel that waits on another workgroup.

// one lane per item: the verdict over the tails records.  Termination: pieces_verify_chain's, then one pass over the item's piece_cap slots.
__global__ void __launch_bounds__(64) pieces_verify_chain_kernel(PieceItem *items, uint32_t nitems, const uint8_t *__restrict__ in, PieceRow *rows, const SpecEnd *__restrict__ ends,
                                                                 uint64_t *ostart, uint2 *ranges)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nitems) return;
    const PieceItem it = items[j];
    const PiecesSizesVerdict v = pieces_verify_chain(ends + it.slot0, rows + it.slot0, it.npieces, in, it.body_lo, it.in_hi, ostart + it.slot0);
    const uint32_t used = v.clean ? v.used : 0u;
    for (uint32_t i = used; i < it.piece_cap; i++) rows[it.slot0 + i].item = kPieceNoItem;
    items[j].total = v.total; items[j].end_bit = v.end_bit; items[j].npieces = used; items[j].clean = v.clean; items[j].bad = 0;
    ranges[j] = v.clean ? make_uint2(it.slot0, it.slot0 + used) : make_uint2(0u, 0u);
}

// one lane per item, behind the check pass: confirm and join.  Termination: pieces_verify_confirm's, one step per chained piece.
__global__ void __launch_bounds__(64) pieces_verify_confirm_kernel(PieceItem *items, uint32_t nitems, const SpecEnd *__restrict__ ends, const PieceCheck *__restrict__ checks,
                                                                   uint32_t do_adler, uint32_t do_crc, ChunkMeta *meta)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nitems) return;
    const PieceItem it = items[j];
    if (!it.clean) return;
    PiecesJoined v{};
    if (!pieces_verify_confirm(ends + it.slot0, checks + it.slot0, it.npieces, do_adler, do_crc, &v)) { items[j].clean = 0; items[j].npieces = 0; return; }
    ChunkMeta m{}; // (what the one-workgroup verifier leaves of an item)
    m.out_bytes = (uint32_t)it.total; m.adler_a = v.a; m.adler_b = v.b; m.crc = v.crc;
    meta[it.k] = m;
}

BatchPiecesVerifyKnobs batch_pieces_verify_knobs()
{
    // the threshold: the verify knob; not set, the shared knob where the caller has set one (0 switches every form off); neither set, the default the
    // rate table decided for this form -- two passes over every piece pay only for items far longer than the decode's 128 KiB
    BatchPiecesVerifyKnobs k{getenv("ZGPU_BATCH_PIECES_MIN_BYTES") ? batch_pieces_knobs().min_bytes : kPiecesVerifyMinBytesDefault, 0};
    if (const char *v = getenv("ZGPU_BATCH_PIECES_VERIFY_MIN_BYTES")) k.min_bytes = strtoull(v, nullptr, 10);
    if (const char *v = getenv("ZGPU_BATCH_PIECES_VERIFY_ROUND_SLOTS")) k.round_slots = strtoull(v, nullptr, 10);
    k.round_slots = pieces_verify_slot_cap(k.round_slots);
    return k;
}
uint64_t batch_pieces_verify_count(int which) { return which == 0 ? g_verify_done.load() : which == 1 ? g_verify_fell.load() : 0; }
size_t batch_pieces_verify_scratch_bytes(uint64_t max_long) { size_t total = 0; pieces_call(nullptr, max_long, &total, true); return total; }

int batch_pieces_verify_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, uint32_t checks, uint64_t max_long, uint8_t *scr, unsigned long long *d_hdr,
                            const unsigned long long *hdr, BatchItemState *states, InfStatus *status, ChunkMeta *meta, uint64_t round_slots, hipStream_t st)
{
    const PiecesCall c = pieces_call(scr, max_long, nullptr, true);
    unsigned long long h[8] = {};
    for (int i = 0; i < 8; i++) h[i] = hdr[i];
    const uint64_t nlong = h[kHdrLong];
    if (nlong == 0) return ZGPU_OK;
    const uint32_t do_adler = checks & 1u, do_crc = (checks >> 1) & 1u;
    // one round serves everything, or the list of long items comes home and pieces_sizes_round_end cuts it under the slot cap
    std::vector<PiecesItemCost> cost;
    const bool one = nlong < 0xFFFFFFFFull && h[kHdrTargets] < 0xFFFFFFFFull && h[kHdrSlots] <= round_slots;
    if (!one) {
        std::vector<PieceItem> list(nlong);
        ZGPU_HIP_CHECK(hipMemcpyAsync(list.data(), c.items, nlong * sizeof(PieceItem), hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        cost.resize(nlong);
        for (uint64_t j = 0; j < nlong; j++) cost[j] = PiecesItemCost{0, list[j].ntargets, list[j].piece_cap};
    }
    for (uint64_t j0 = 0; j0 < nlong;) {
        uint64_t j1 = nlong, targets = h[kHdrTargets], slots = h[kHdrSlots];
        if (!one) {
            j1 = pieces_sizes_round_end(cost.data(), nlong, j0, round_slots);
            targets = slots = 0;
            for (uint64_t j = j0; j < j1; j++) { targets += cost[j].ntargets; slots += cost[j].piece_cap; }
        }
        const uint32_t ni = (uint32_t)(j1 - j0), igrid = (ni + 255) / 256;
        PieceItem *items = c.items + j0;
        const PiecesVerifyRoundPlan p = pieces_verify_round_plan(ni, targets, slots);
        // declining is no error, as in batch_pieces_run: the round's items go to the one-workgroup verifier (ZGPU_BATCH_PIECES_NO_SCRATCH=1: every round)
        uint8_t *base = nullptr;
        if (p.total != 0 && p.total <= kPiecesScratchCap && !getenv("ZGPU_BATCH_PIECES_NO_SCRATCH")) {
            if (e->inf_slots.reserve(nullptr, p.total)) (void)hipGetLastError();
            else base = e->inf_slots.p;
        }
        ZGPU_HIP_CHECK(hipMemsetAsync(d_hdr + kHdrGathered, 0, 8, st));
        ZGPU_HIP_CHECK(hipMemsetAsync(c.fbseg + 4 * j0, 0, (size_t)ni * 32, st));
        if (base) {
            const uint32_t nt = (uint32_t)targets, ns = (uint32_t)slots;
            PieceTarget *table = reinterpret_cast<PieceTarget *>(base + p.targets.off);
            uint64_t *found = reinterpret_cast<uint64_t *>(base + p.found.off), *ostart = reinterpret_cast<uint64_t *>(base + p.ostart.off);
            PieceRow *rows = reinterpret_cast<PieceRow *>(base + p.rows.off);
            uint2 *ranges = reinterpret_cast<uint2 *>(base + p.ranges.off);
            InfStatus *slot_status = reinterpret_cast<InfStatus *>(base + p.status.off);
            SpecArgs sp{}; // (no pages: mid, page_owner and page_count stay null)
            sp.tails = reinterpret_cast<uint16_t *>(base + p.tails.off); sp.ends = reinterpret_cast<SpecEnd *>(base + p.ends.off); sp.rows = rows;
            sp.windows = base + p.windows.off; sp.ostart = ostart; sp.checks = reinterpret_cast<PieceCheck *>(base + p.checks.off);
            ZGPU_HIP_CHECK(hipMemsetAsync(sp.ends, 0xFF, (size_t)ns * sizeof(SpecEnd), st));
            ZGPU_HIP_CHECK(hipMemsetAsync(sp.checks, 0xFF, (size_t)ns * sizeof(PieceCheck), st));
            ZGPU_HIP_CHECK(hipMemsetAsync(base + p.entry.off, 0, kOutRing, st));
            hipLaunchKernelGGL(pieces_round_kernel, dim3(1), dim3(1024), 0, st, items, ni);
            hipLaunchKernelGGL(pieces_targets_kernel, dim3(ni), dim3(256), 0, st, items, ni, table);
            launch_spec_find_table(d_in, in_bytes, table, nt, found, st);
            hipLaunchKernelGGL(pieces_select_kernel, dim3((ni + 63) / 64), dim3(64), 0, st, items, ni, d_in, found, nt, rows, ostart);
            for (uint32_t c0 = 0; c0 < ns; c0 += 65536) {
                const uint32_t nb = ns - c0 < 65536 ? ns - c0 : 65536;
                launch_inflate_decode(kInfPieces, kInfNoRing, InfLaunch{d_in, in_bytes, nullptr, c0, nb, nullptr, 0, slot_status + c0}, sp, st);
            }
            hipLaunchKernelGGL(pieces_verify_chain_kernel, dim3((ni + 63) / 64), dim3(64), 0, st, items, ni, d_in, rows, sp.ends, ostart, ranges);
            launch_spec_windows_items(sp.tails, ns, ni, ranges, base + p.entry.off, base + p.windows.off, st);
            for (uint32_t c0 = 0; c0 < ns; c0 += 65536) {
                const uint32_t nb = ns - c0 < 65536 ? ns - c0 : 65536;
                launch_inflate_decode(kInfPieceVerify, kInfNoRing, InfLaunch{d_in, in_bytes, nullptr, c0, nb, nullptr, (uint64_t)checks, slot_status + c0}, sp, st);
            }
            hipLaunchKernelGGL(pieces_verify_confirm_kernel, dim3((ni + 63) / 64), dim3(64), 0, st, items, ni, sp.ends, sp.checks, do_adler, do_crc, meta);
        }
        // (a round that got no scratch: the items' clean fields are the zeros the header kernel wrote)
        hipLaunchKernelGGL(pieces_status_kernel, dim3(igrid), dim3(256), 0, st, items, ni, states, status, c.fbseg + 4 * j0, c.fbmap + j0, d_hdr);
        for (uint32_t c0 = 0; c0 < ni; c0 += 65536) {
            const uint32_t nb = ni - c0 < 65536 ? ni - c0 : 65536;
            InfLaunch a{d_in, in_bytes, c.fbseg + 4 * j0, c0, nb, nullptr, (uint64_t)checks, c.fbstatus + j0 + c0};
            a.meta = c.fbmeta + j0 + c0;
            launch_inflate_decode(kInfVerify, kInfNoRing, a, SpecArgs{}, st);
        }
        hipLaunchKernelGGL(pieces_scatter_kernel, dim3(igrid), dim3(256), 0, st, c.fbstatus + j0, c.fbmap + j0, d_hdr, ni, status, c.fbmeta + j0, meta);
        ZGPU_HIP_CHECK(hipGetLastError());
        j0 = j1;
    }
    ZGPU_HIP_CHECK(hipMemcpyAsync(h, d_hdr, sizeof h, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    g_verify_done += h[kHdrClean]; g_verify_fell += h[kHdrFell];
    return ZGPU_OK;
}
} // namespace zgpu
