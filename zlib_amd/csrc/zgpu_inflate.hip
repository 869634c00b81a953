// zgpu_inflate.hip -- decode path: the decoder kernel, one workgroup per segment, its one launcher, the chunk path (inflate_run) and its C entry points.  The batch of
// independent streams is zgpu_inflate_batch.hip, a stream that was not produced in chunks zgpu_inflate_stream.hip; what the kernels share, zgpu_inflate_dev.h.
//
// Restates (file:line under /root/reference):
//   block header / stored / dynamic-table states of inflate()   qcsrc/inflate.c:773-949
//   code-length validation of inflate_table                     qcsrc/inftrees.c:106-138
//   symbol decode + match copy (inflate_fast and the slow path) qcsrc/inffast.c:67-302, qcsrc/inflate.c:950-1076
//   length / distance bases and extra bits                      qcsrc/inftrees.c:60-73
// The reference decodes through 2-level tables of `code` structs; only the produced bytes and the error class are
// observable, so the table layout here is the engine's own: a 9-bit literal/length and a 9-bit distance direct
// table in LDS, codes longer than that resolved by a canonical first-code walk.
//
// Work split: the bit reader and symbol decode are wave-uniform (every lane computes the same values: the decode of one
// deflate stream is sequential); lanes cooperate on table fill, input staging (512 bytes per refill, 8 bytes per lane),
// match copies (64 bytes per step) and the flushes to the destination (16 bytes per lane).  The last RING bytes of output
// -- 32 KiB, or 8 / 16 KiB for chunks placed directly -- live in a ring in LDS that is flushed half by half: back-references
// inside the ring never touch global memory, those of a small ring that reach farther read the flushed bytes back.
#include "zgpu_common.h"
#include "zgpu_engine.h"
#include "zgpu_inflate_dev.h"
#include <type_traits>
#include "../../include/zamd_gpu.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace zgpu {

static const char *const kInfMessages[kMsgCount] = {
    "", "invalid block type", "invalid stored block lengths", "too many length or distance symbols", "invalid code lengths set",
    "invalid bit length repeat", "invalid literal/lengths set", "invalid distances set", "invalid literal/length code", "invalid distance code",
    "invalid distance too far back", "segment ends inside a block", "segment decodes to more than chunk_size bytes",
    "segment holds data after its last block", "segment decodes to fewer than chunk_size bytes", "segment table out of range",
    "incorrect header check", "unknown compression method", "invalid window size", "unknown header flags set", "header crc mismatch",
    "incorrect data check", "incorrect length check", "invalid BGZF block chain"};

#ifdef ZGPU_INF_TIME // debug build only (scripts/inf_time.py): clock per phase, summed over chunks
__device__ unsigned long long inf_time[16];
extern "C" __attribute__((visibility("default"))) void zgpu_debug_inf_time(unsigned long long *out, int reset)
{
    unsigned long long z[16] = {};
    hipMemcpyFromSymbol(out, HIP_SYMBOL(inf_time), sizeof z);
    if (reset) hipMemcpyToSymbol(HIP_SYMBOL(inf_time), z, sizeof z);
}
#define INF_T(i) do { const unsigned long long t_ = wall_clock64(); t_acc[i] += t_ - t_prev; t_prev = t_; } while (0)
#define INF_T0() unsigned long long t_prev = wall_clock64(); unsigned long long t_acc[16] = {}; unsigned long long n_lit = 0, n_mat = 0, n_slow = 0
#define INF_N(x) x++
#else
#define INF_T(i) do { } while (0)
#define INF_T0() do { } while (0)
#define INF_N(x) do { } while (0)
#endif

// VERIFY's fold of one piece (see inflate_kernel_t): p[0, n), n <= kFoldMax, into the running Adler-32 halves and CRC-32.  The writer wave, all 64 lanes;
// one copy of the code for the kernel's three flushes.  Every loop is bounded by n / 64 or is one of six steps across the lanes.
struct FoldRun { uint32_t a, b, crc; }; // (by value both ways: the running values stay in registers)
__device__ __noinline__ FoldRun verify_fold(const uint8_t *p, uint32_t n, const uint32_t *crc_nib, uint32_t lane, uint32_t do_adler, uint32_t do_crc, FoldRun run)
{
    if (do_adler) {
        uint64_t s1, s2;
        fold_adler_lane(p, n, lane, s1, s2);
        for (int sh = 32; sh > 0; sh >>= 1) { s1 += __shfl_xor(s1, sh); s2 += __shfl_xor(s2, sh); }
        fold_adler_join(run.a, run.b, s1, s2, n);
    }
    if (do_crc) {
        uint32_t lg, slo, shi;
        fold_slice(n, lane, lg, slo, shi);
        uint32_t crc = crc_nib_span(crc_nib, p + slo, shi - slo);
#pragma unroll 1
        for (uint32_t st = 0; st < 6; st++) crc = fold_crc_step(crc, (uint32_t)__shfl_down((int)crc, 1u << st), lane, 1u << st, lg, st);
        run.crc = crc_join(run.crc, (uint32_t)__builtin_amdgcn_readfirstlane((int)crc), fold_xpow8n(n));
    }
    return run;
}

// One workgroup of two waves per segment.  Wave 0 (the reader) owns the bit stream: block headers, code tables and the
// token decode; it never needs to know how many bytes came out so far.  Wave 1 (the writer) owns the output: the 32 KiB
// ring in LDS, match copies, flushes to the destination, and the limits that depend on the output position (distance too
// far back, chunk size).  Tokens travel through a ring of 128 words in LDS, handed over in halves of 64 with one workgroup
// barrier per half: while the writer executes half k the reader fills half k + 1.
// token word: bits 0-1 kind (0 nothing, 1 literal, 2 match, 3 command)
//   literal: bits 2-9 byte;  match: bits 2-10 length, 11-25 distance - 1
//   command: bits 2-3 which (1 stored bytes: bits 4-20 count, the next two words = offset of the bytes in the input;
//            2 end of the segment: bits 4-11 the reader's verdict)
enum : uint32_t { kCmdStored = 1, kCmdEnd = 2 };

__device__ inline void block_sync() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }

// SPEC (speculative decode of one stream in pieces, zgpu_inflate_stream.hip): segment gc starts at BIT offsets[gc] of the input -- a block start
// the finder believes in -- and ends at the first block boundary at or behind bit offsets[gc + 1], or with the final block; nothing is known about
// the 32 KiB in front of it, so the ring holds 16-bit symbols (byte, or marker = index into that unknown window) and goes to pages of
// kOutHalf symbols taken from a pool as it fills, the segment's place in the output being unknown too.
// SPEC with sp.rows (the pieces of MANY streams, zgpu_inflate_batch_pieces.hip): segment gc is rows[gc] -- its start and stop bits, the byte behind ITS
// stream (no read and no stop bit lies behind it, where the next stream's bytes are) and whether it is its stream's first piece (then nothing lies in
// front of it: reach is the dictionary's, which a batch does not have).  A row that belongs to no item ends its workgroup before the first barrier.
// RING: bytes of output the workgroup keeps in LDS.  32768 is the farthest a distance reaches: every match copies from the ring.  A smaller ring
// (chunks placed directly at their offset of the destination only) lets more segments share a CU; a match that reaches farther back than RING reads its
// source from the destination itself, where every byte older than the ring has been flushed: the lanes that hold such matches ask for their first 32 bytes
// when their half of the token ring is handed over, all at once, and the copy takes them from registers when its turn comes.
// BATCH (zgpu_inflate_batch_*): segment gc is one independent stream, offsets[4 gc ..] = {body start, input end, output start, output end}; it must
// reach its final block, whatever follows is its trailer (stream_mode), and it goes straight to its own range of the destination with no dictionary.
// SIZES (zgpu_inflate_batch_sizes_*, BATCH only): the sizing pass.  The decoded size of a deflate stream is a function of its symbols alone, so the workgroup is
// the reader wave and nothing else: where the reader would hand tokens to the writer it takes their lengths itself (a prefix sum per hand-over) and applies
// the limits that depend on the output position -- distance too far back, the 4 GiB item limit -- in the order the writer does.  There is no output ring, no
// token ring, no barrier, no match copy and no access to the destination: `out`, the output half of the segment table and `dict` are never touched.
// status[] is what the BATCH decoder writes for the same item into a range of exactly its size.  What this pass cannot say: it computes no Adler-32 or
// CRC-32 and compares no ISIZE, so its verdict is the decoder's verdict minus the trailer checks.
// Termination: SIZES adds no loop.  The block loop and the token loop are the reader's, and every iteration of either consumes input bits or ends with
// an error (or with `stop`, which the counting sets together with its error); the counting itself is straight-line code.
// SPEC with SIZES (kInfPieceSizes, sp.rows only: the sizing pass over the pieces of many streams, batch_pieces_sizes_run): the reader of the rowed SPEC decode --
// start and stop bits, a start at a stored block's LEN, in_end and `first` from the row, a slot with kPieceNoItem returns at the top -- that counts as SIZES
// counts, from its start to the first block boundary at or behind its stop, or to the final block.  One wave per slot, InflateLdsSizes, no token ring,
// no output ring, no barrier; `out`, the page pool and the tails are never touched.  It writes one SpecEnd per slot (end_bit, out_bytes, bit 0 = the
// final block, bits 8.. the error, as the SPEC decode sets them) and sp.need[slot].  Two things differ from SIZES.  Reach: a first piece keeps SIZES' rule
// (reach 0: a distance beyond the bytes counted so far is its error); every other piece cannot know what lies in front of it, never fails for reach and
// records need = the largest (distance - bytes counted in front of that token) over its matches, floored at 0, which pieces_sizes_chain holds against
// what the pieces in front of it counted.  Overflow: the count stops at the item limit 0xFFFF0000 with kMsgOutput instead of wrapping (a piece whose
// finders found nothing can be a body of 2^29 bytes, and deflate expands 1032 to 1): SIZES' own `over` rule, chunk_size being that limit here.
// Occupancy: compiled for ZGPU_INF_SIZES_WAVES like SIZES, the same LDS: twenty-four slots a CU, six waves a SIMD (registers: profiles/sizes_pieces_isa.txt).
// Termination: it adds no loop to the reader's; `need` is straight-line code (a maximum over the lanes, six steps) in the hand-overs of a piece's first 32 KiB.
// VERIFY (zgpu_inflate_batch_verify_*, BATCH only, the 32 KiB ring): the integrity test.  The reader is the decoder's, and so is everything the writer does
// inside the ring -- literals, match copies, stored blocks half by half; every match finds its source there.  What it does not have is a destination: where
// the decoder would flush ring bytes [flushed, upto) to memory (half a ring, or the tail at the end, never wrapping) the writer wave folds them into the
// running Adler-32 and CRC-32 it keeps in registers (zgpu_common.h, "the fold"), whichever of the two `out_cap` asks for (bit 0 Adler-32, bit 1 CRC-32:
// there is no capacity to pass).  No byte of output goes to global memory or comes from it, `out` and the output half of the segment table are never
// touched, and the only limit on the output position is the 4 GiB of an item.  status[] is the BATCH decoder's for a range of exactly the item's size;
// meta[c] (one record per ITEM here) takes the two check values.
// The CRC lookup: eight 16-word nibble tables in LDS behind the decoder's own layout (512 bytes, built by the writer wave before its first token), so
// the workgroup stays within the 40448 bytes that let four share a CU.  A lookup's 64 lanes go to one table, 16 consecutive words: no two entries share
// a bank.  The alternatives -- a table in lane registers read by cross-lane shuffles, a 1 KiB byte table (three workgroups a CU), the 4 KiB
// slicing-by-4 table of zgpu_checksum.hip (three as well) -- have not been measured against it.
// Termination: VERIFY adds the fold's loops, each bounded by the bytes of one flush (16 KiB), and a table build of two words per lane.
// SPEC with sp.rows and NOPAGES (the launcher picks it where sp.mid == nullptr: the tails pass of the verify form of the piece path, batch_pieces_verify_run): the rowed SPEC decode whose
// flushes go nowhere.  The same reader, the same 16-bit ring with markers; no page is taken from a pool and nothing goes to `mid`.  It leaves what the window
// kernels read -- the slot's tail and its SpecEnd.  A deflate distance reaches 32 KiB at most, so the ring alone carries the decode.
// SPEC with VERIFY (kInfPieceVerify, sp.rows only: the check pass of the same path): the rowed reader paired with VERIFY's writer.  Start bit, stop bit, a start at
// a stored block's LEN, in_end and `first` come from the row as in the rowed SPEC decode; a slot with kPieceNoItem returns at the top.  The writer keeps
// VERIFY's byte ring of 32 KiB (InflateLdsVerify, the CRC nibble tables behind it: four workgroups a CU, as VERIFY) and folds where the decoder would flush.
// Before its first token the ring is preloaded with the window of the slot in front (sp.windows[gc - 1], bytes), as the dictionary preload does: its last
// `reach` = min(32768, sp.ostart[gc]) bytes, the bytes of the item in front of this piece; an item's first piece preloads nothing and has reach 0.  A distance
// beyond reach is the decoder's own "invalid distance too far back" -- exact here, where the tails pass could not know it.  Each slot writes one record
// (sp.checks[gc]): end bit, bytes produced, the final-block bit or the error, and the Adler-32 halves and CRC-32 of its own bytes started from (1, 0) and 0,
// whichever `out_cap` asks for.  It touches neither `out` nor a destination, takes no page and writes no tail; `meta` is not used.
// Termination: the mode adds no loop beyond the preload (2048 vectors over 64 lanes at most); the reader's loops are the rowed SPEC decode's, the fold's VERIFY's.
// Registers, LDS and scratch of the instantiation: profiles/verify_pieces_isa.txt.
// FOLD (zgpu_inflate_batch_*_enqueue, BATCH only, the rings BATCH has): the fused decode.  BATCH as it stands -- the same destination, the same dst_room / nofit
// rules, the same status[] -- whose writer wave, in flush_to, first folds ring bytes [flushed, upto) into the running check values as VERIFY does and then
// stores them as BATCH does.  The bytes are folded out of LDS in the flush that carries them to memory, so the output is never read again: no piece table, no
// second pass, and no count the host would have to fetch to size one.  Which checks: `fold_checks` (bit 0 Adler-32, bit 1 CRC-32), an argument of its
// own, since `out_cap` is the destination's here.  meta[c] takes what VERIFY writes.  An item that does not fit its range (nofit) goes on folding the
// bytes that are not stored: its status is ZGPU_BUF_ERROR and nobody reads its check values.  With the 32 KiB ring every match finds its source in LDS
// and the destination is write-only; with a small ring the far matches read the destination back as in BATCH, behind the wait that follows the flush's
// stores (the fold stands in front of the stores and reads LDS only, so it changes nothing about what is in memory when).  The CRC lookup lies behind the
// layout (InflateLdsFoldT): 512 bytes that leave the workgroups per CU of every ring as they are -- four, six, ten.
// Termination: FOLD adds to BATCH exactly what VERIFY adds -- the fold's loops, each bounded by the bytes of one flush (half a ring, 16 KiB at most), and the table build --
// and the flush's store loops stay BATCH's, bounded by the same bytes.
template <bool SPEC, uint32_t RING = ZGPU_INF_RING, bool BATCH = false, bool SIZES = false, bool VERIFY = false, bool FOLD = false, bool NOPAGES = false>
__global__ void __launch_bounds__(SIZES ? 64 : 128, SIZES ? ZGPU_INF_SIZES_WAVES : (!SPEC && RING <= 8192) ? 5 : 4) inflate_kernel_t(const uint8_t *__restrict__ in, uint64_t in_bytes, const uint64_t *__restrict__ offsets,
                                                        uint64_t chunk0, uint32_t nchunks, uint64_t last_chunk, uint32_t chunk_size_arg,
                                                        uint8_t *__restrict__ out, uint64_t out_cap, InfStatus *status, ChunkMeta *meta,
                                                        const uint8_t *__restrict__ dict, uint32_t dict_len, uint32_t stream_mode, SpecArgs sp, uint32_t fold_checks)
{
    typedef typename std::conditional<SPEC && !VERIFY, uint16_t, uint8_t>::type ring_t; // (the check pass knows the window in front: bytes, no markers)
    typedef typename std::conditional<SIZES, InflateLdsSizes, typename std::conditional<VERIFY, InflateLdsVerify, typename std::conditional<FOLD, InflateLdsFoldT<RING>, InflateLdsT<ring_t, RING>>::type>::type>::type Lds;
    static_assert(!SIZES || (BATCH != SPEC), "the sizing pass serves batch items, whole (BATCH) or by the rows of their pieces (SPEC)");
    static_assert(!VERIFY || ((BATCH != SPEC) && !SIZES && !FOLD && RING == 32768), "the integrity test serves batch items, whole (BATCH) or by the rows of their pieces (SPEC), every match from the ring");
    static_assert(!FOLD || (BATCH && !SPEC && !SIZES && !VERIFY), "the fused decode serves batch items");
    static_assert(!NOPAGES || (SPEC && !BATCH && !SIZES && !VERIFY && !FOLD), "the no-pages form is the 16-bit decode in pieces, its flushes dropped");
    constexpr uint32_t kOutRing = RING, kOutHalf = RING / 2; // (this kernel's ring, not the file's default)
    constexpr bool FAR = RING < 32768;
    static_assert(!(SPEC && FAR) && RING >= 4096 && (RING & (RING - 1)) == 0, "ring size");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    Lds &L = *reinterpret_cast<Lds *>(lds_raw);
    const uint32_t c = blockIdx.x, lane = threadIdx.x & 63u;
    const uint32_t role = uni(threadIdx.x >> 6); // 0 reader, 1 writer
    if (c >= nchunks) return;
    const uint64_t gc = chunk0 + c;
    const uint32_t start_bits = stream_mode >> 8; // (a whole-stream call: the stream begins at that bit of its first byte)
    stream_mode &= 255u;
    // SPEC, the pieces of many streams (sp.rows): the segment's two starts, the end of its own stream and whether anything lies in front of it come from
    // its row; a slot that is not in use ends here, before the first barrier
    const bool rowed = SPEC && sp.rows != nullptr;
    if (rowed && sp.rows[gc].item == kPieceNoItem) return;
    if (SPEC && (SIZES || VERIFY) && !rowed) return; // (the sizing form and the verify form have rows only)
    uint64_t seg_lo = rowed ? sp.rows[gc].start : BATCH ? offsets[4 * gc] : offsets[gc], seg_hi = rowed ? sp.rows[gc].stop : BATCH ? offsets[4 * gc + 1] : offsets[gc + 1];
    const uint64_t spec_end = rowed ? sp.rows[gc].in_end : in_bytes; // SPEC: the byte behind the stream the segment belongs to
    const bool spec_first = rowed ? sp.rows[gc].first != 0 : gc == 0; // SPEC: the stream's first segment
    uint32_t bit_lead = 0, stop_bits = 0xFFFFFFFFu; // SPEC: bits of the first byte in front of the start; where the next segment starts, in bits from seg_lo
    bool bad_table;
    bool at_len = false; // SPEC: the piece starts at the LEN field of a stored block (its header bits lie in front, the piece before checks them)
    if (SPEC) {
        // bit 62 of a start: the position is the (byte-aligned) LEN of a stored block; the piece in front of such a start stops at the first block
        // boundary that can be that block's: 3 header bits and up to 7 of padding in front of LEN
        at_len = (seg_lo >> 62) & 1u;
        const uint64_t s0 = seg_lo & ~(3ull << 62), s1 = ((seg_hi >> 62) & 1u) ? (seg_hi & ~(3ull << 62)) - 10 : seg_hi;
        bad_table = s0 >= s1 || s1 > spec_end * 8 || spec_end > in_bytes || s1 - (s0 & ~7ull) >= (1ull << 31);
        seg_lo = s0 >> 3; seg_hi = spec_end - seg_lo < (1ull << 28) ? spec_end : seg_lo + (1ull << 28);
        bit_lead = (uint32_t)(s0 & 7u); stop_bits = bad_table ? 0u : (uint32_t)(s1 - seg_lo * 8);
    } else {
        // the table may arrive next to the data from anywhere: an entry that does not lie inside the input, runs backwards or is longer than
        // a 32-bit bit count can express is an error of that segment, decoded as an empty one (nothing outside the input is ever read)
        bad_table = seg_lo > seg_hi || seg_hi > in_bytes || seg_hi - seg_lo >= (1ull << 29);
        bit_lead = start_bits;
    }
    if (bad_table) { seg_lo = 0; seg_hi = 0; }
    const bool must_be_final = !SPEC && (BATCH || gc == last_chunk);
    // chunk_size_arg == 0: "compact" mode, segments of any size up to 64 KiB are decoded into per-chunk slots and
    // concatenated afterwards (used for streams whose chunks are not all full, e.g. flushed mid-chunk)
    const bool compact = chunk_size_arg == 0;
    // chunk_size_arg == kWholeStream: one segment of any size (a stream that was not produced in chunks): decoded from end to
    // end by this one workgroup straight into the destination, limited only by the destination's capacity (a destination
    // that is too small still gets the size that would have been needed)
    const bool whole = SPEC || BATCH || chunk_size_arg == kWholeStream;
    const uint32_t chunk_size = compact ? kChunkMax : whole ? 0xFFFF0000u : chunk_size_arg;
    // a preset dictionary (inflateSetDictionary, inflate.c:1200-1236) is what the window holds before the first byte: in the ring it
    // sits right below position 0, and the first segment may reach that much farther back
    // (the check pass of the verify form knows where its piece starts inside its item: what lies in front of it, 32 KiB at most, is all a distance may reach)
    const uint32_t reach = (SPEC && VERIFY) ? (spec_first ? 0u : (uint32_t)(sp.ostart[gc] < kOutRing ? sp.ostart[gc] : kOutRing))
                                            : BATCH ? 0u : (SPEC ? spec_first : gc == 0) ? dict_len : SPEC ? kOutRing : 0u;
    if (threadIdx.x == 0) { L.abort_flag = 0; L.end_bits = 0; L.end_final = 0; }
    INF_T0();

    if (role == 0) {
        // =========================================== reader ===========================================
        uint32_t err = bad_table ? (uint32_t)kMsgTable : (uint32_t)kMsgNone;
        uint32_t wr = 0;   // tokens put into the ring so far
        bool stop = false; // the writer gave up (its error comes first in stream order)
        uint32_t size_o = 0, size_err = kMsgNone; // SIZES: bytes the tokens so far stand for; the error of the first token that breaks a limit of the output position
        uint32_t size_need = 0;                   // SIZES of a piece that is not its item's first: how far its matches reach in front of its first byte
        auto publish = [&]() { // the current half is complete: hand it over, the other half is free from here on
            INF_T(9);
            block_sync();
            INF_T(13);
            stop = uni(L.abort_flag) != 0;
        };
        // the marked lanes' token words, in lane order
        auto emit_tokens = [&](uint64_t marks, uint32_t word) {
            if constexpr (SIZES) { // what the writer does with a run of tokens, minus the bytes (the marked lanes are in stream order)
                const uint32_t k2 = sel_mask(marks, word & 3u, 0u), len = (word >> 2) & 511u, ol = k2 == 1 ? 1u : k2 == 2 ? len : 0u;
                const uint32_t incl = wave_prefix_sum(ol), offv = size_o + incl - ol;
                // (SPEC: only a first piece knows what lies in front of it -- nothing; the others record how far they reach instead)
                const bool far = k2 == 2 && (!SPEC || spec_first) && (word >> 11) >= offv + reach, over = offv + ol > chunk_size; // (size_o <= 0xFFFF0000 and a run adds 64 * 258 at most: no wrap)
                if constexpr (SPEC) {
                    if (!spec_first && !stop && size_o < 32768u) { // (behind 32 KiB of its own no distance reaches in front of the piece)
                        uint32_t nd = (k2 == 2 && (word >> 11) >= offv) ? (word >> 11) + 1 - offv : 0u;
#pragma unroll
                        for (int sh = 32; sh >= 1; sh >>= 1) { const uint32_t o2 = (uint32_t)__shfl_xor((int)nd, sh); nd = o2 > nd ? o2 : nd; }
                        nd = uni(nd);
                        size_need = nd > size_need ? nd : size_need;
                    }
                }
                const uint64_t bad = __ballot(far || over);
                if (stop) { } // (the second window of a step whose first one broke a limit: the first error stands, as the writer takes no token behind its error)
                else if (bad) { size_err = ((__ballot(far) >> (uint32_t)__builtin_ctzll(bad)) & 1) ? kMsgTooFar : kMsgOutput; stop = true; }
                else size_o += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            } else {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(marks >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)marks, 0u));
            const uint32_t t = (uint32_t)__builtin_popcountll(marks), bound = (wr | 63u) + 1, at = wr + rank;
            const bool mine = sel_mask(marks, 1u, 0u) != 0;
            if (mine && at < bound) L.tok[at & 127u] = word;
            if (wr + t >= bound) {
                publish();
                if (mine && at >= bound) L.tok[at & 127u] = word;
            }
            wr += t;
            }
        };
        // n <= 3 words that must sit in one half (lane i holds word i); `final`: pad the half and hand it over
        auto emit_command = [&](uint32_t word, uint32_t n, bool final) {
            if constexpr (SIZES) { // a stored block counts its bytes (lane 0 holds the command word); the end command has nobody to go to
                if (!final) {
                    const uint32_t slen = (uni(word) >> 4) & 0x1FFFFu;
                    if (size_o + slen > chunk_size) { size_err = kMsgOutput; stop = true; }
                    else size_o += slen;
                }
            } else {
            if ((wr & 63u) + n > 64u) { // no room: pad this half with nothing-tokens
                const uint32_t bound = (wr | 63u) + 1;
                if (wr + lane < bound) L.tok[(wr + lane) & 127u] = 0u;
                wr = bound;
                publish();
            }
            if (lane < n) L.tok[(wr + lane) & 127u] = word;
            wr += n;
            if (final) {
                const uint32_t bound = ((wr - 1) | 63u) + 1;
                if (wr + lane < bound) L.tok[(wr + lane) & 127u] = 0u;
                wr = bound;
                publish();
            } else if ((wr & 63u) == 0) publish();
            }
        };
        BitSrc b;
        const uint64_t in_addr = reinterpret_cast<uint64_t>(in);
        const uint64_t abs_lo = in_addr + seg_lo, abs_al = abs_lo & ~3ull;
        b.g32 = reinterpret_cast<const uint32_t *>(abs_al);
        b.gdwords = (in_addr + in_bytes - abs_al + 3) >> 2; // reads past the input buffer are replaced by zeros, see stage_fill
        // the dword holding the last input bytes may extend past the buffer by up to 3 bytes inside the same aligned dword
        b.d0 = 0; b.filled = 0; b.rd = 0; b.hold = 0; b.bits = 0;
        const uint32_t lead = (uint32_t)(abs_lo - abs_al);
        b.seg_bits = (uint32_t)(seg_hi - seg_lo + lead) * 8;
        stage_fill(b, L.stage, lane);
        wave_sync();
        prime(b, L.stage);
        refill(b, L.stage); refill(b, L.stage);
        drop(b, lead * 8);
        drop(b, bit_lead);
        auto reposition = [&](uint32_t pos) { // the scalar reader at bit `pos` of the staged dwords
            b.rd = pos >> 5; b.hold = 0; b.bits = 0;
            prime(b, L.stage); refill(b, L.stage); refill(b, L.stage);
            drop(b, pos & 31);
        };
        bool last = false, seen_final = false;
        uint32_t org_bits = 0; // bits between the segment's (aligned) start and the bit reader's origin: stored blocks move the origin
        CodeRows lrows{}, drows{}; // per-length rows of the two codes of the current block (lanes 1..15)
        INF_T(0);
        while (!err && !last && !stop) {
            if (consumed_bits(b) >= b.seg_bits) break; // segment exhausted at a block boundary (normal end of a non-final segment)
            if (SPEC && org_bits + consumed_bits(b) - lead * 8 >= stop_bits) break; // a block boundary at or behind the next segment's start
            stage_fill(b, L.stage, lane); wave_sync();
            refill(b, L.stage);
            uint32_t type = 0;
            if (SPEC && at_len) at_len = false; // (the first block of this piece: stored, not the last, the reader stands at its LEN)
            else {
                const uint32_t hdr = peek(b, 3); drop(b, 3);
                last = hdr & 1; seen_final = seen_final || last;
                type = hdr >> 1;
            }
            if (type == 3) { err = kMsgBlockType; break; }
            if (type == 0) {
                drop(b, b.bits & 7);
                refill(b, L.stage);
                const uint32_t len = peek(b, 16); drop(b, 16);
                refill(b, L.stage);
                const uint32_t nlen = peek(b, 16); drop(b, 16);
                if (len != (nlen ^ 0xFFFFu)) { err = kMsgStoredLen; break; }
                const uint32_t bytepos = consumed_bits(b) >> 3; // from the reader's current origin (dword b.d0 of the segment)
                if ((uint64_t)bytepos + len > (b.seg_bits >> 3)) { err = kMsgTruncated; break; }
                const uint64_t src = reinterpret_cast<uint64_t>(b.g32 + b.d0) + bytepos - in_addr; // the writer copies the bytes from the input
                emit_command(lane == 0 ? (3u | (kCmdStored << 2) | (len << 4)) : lane == 1 ? (uint32_t)src : (uint32_t)(src >> 32), 3, false);
                // reposition the reader right after the stored bytes: new origin = the dword holding that byte
                const uint32_t np = bytepos + len;
                b.d0 += np >> 2; b.filled = 0; b.rd = 0; b.hold = 0; b.bits = 0;
                b.seg_bits -= (np & ~3u) * 8; // seg_bits stays relative to the origin
                org_bits += (np & ~3u) * 8;   // ... and this is where the origin stands in the segment
                wave_sync();
                stage_fill(b, L.stage, lane); wave_sync();
                prime(b, L.stage);
                refill(b, L.stage); refill(b, L.stage);
                drop(b, (np & 3) * 8);
                continue;
            }
            // ---- tables ----
            if (type == 1) {
                for (uint32_t s = lane; s < 288; s += 64) L.lens[s] = (uint16_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                wave_sync();
                build_table(L, L.lens, 288, 1, kLBits, L.ltab, L.lsym, L.lcount, lane);
                lrows = load_rows(L, L.lcount, lane);
                wave_sync();
                for (uint32_t s = lane; s < 32; s += 64) L.lens[s] = 5;
                wave_sync();
                build_table(L, L.lens, 32, 2, kDBits, L.dtab, L.dsym, L.dcount, lane);
                drows = load_rows(L, L.dcount, lane);
            } else {
                err = dynamic_header<false>(L, b, lane, lrows, drows);
                if (err) break;
            }
            wave_sync();
            INF_T(1);
            // ---- symbols ----
            // Every lane decodes the token that would start at its own bit offset behind the reader (both table lookups, extra
            // bits included); a scalar walk from offset 0 then picks the lanes that really are token starts (each token says
            // where the next one begins).  A token the tables do not resolve (code longer than the table, end of block, invalid
            // code, the end of the segment) ends the walk and goes through the one-symbol path below.
            uint32_t pos = consumed_bits(b); // the reader's position in bits from the segment's origin dword
            bool eob = false;
            while (!eob && !stop) {
                pos = uni(pos); wr = uni(wr);
                b.rd = pos >> 5; b.filled = uni(b.filled); b.seg_bits = uni(b.seg_bits);
                stage_fill(b, L.stage, lane);
                if (pos > b.seg_bits) { err = kMsgTruncated; break; }
                // two windows of 64 bit offsets per step: lane i looks at offsets i and 64 + i
                uint32_t info0, word0, info1, word1; // info: token length in bits (64 = not a token the walk may take)
                {
                    const uint32_t p = pos + lane, wi = p >> 5, sh = p & 31;
                    uint32_t w[5];
#pragma unroll
                    for (int k = 0; k < 5; k++) w[k] = L.stage[(wi + k) & (kStageDwords - 1)];
                    // (both windows side by side, so that their table lookups are in flight together)
                    const uint32_t lo[2] = {__builtin_amdgcn_alignbit(w[1], w[0], sh), __builtin_amdgcn_alignbit(w[3], w[2], sh)};
                    const uint32_t hi[2] = {__builtin_amdgcn_alignbit(w[2], w[1], sh), __builtin_amdgcn_alignbit(w[4], w[3], sh)};
                    uint32_t e[2], ed[2], h2[2], t[2], len[2];
#pragma unroll
                    for (int k = 0; k < 2; k++) e[k] = L.ltab[lo[k] & ((1u << kLBits) - 1)];
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const uint32_t l1 = e[k] & 15u, xl = (e[k] >> 4) & 15u;
                        t[k] = l1 + xl;
                        len[k] = (e[k] >> 16) + __builtin_amdgcn_ubfe(lo[k] >> l1, 0, xl);
                        h2[k] = (uint32_t)((((uint64_t)hi[k] << 32) | lo[k]) >> t[k]);
                    }
#pragma unroll
                    for (int k = 0; k < 2; k++) ed[k] = L.dtab[h2[k] & ((1u << kDBits) - 1)];
                    uint32_t info[2], word[2];
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const uint32_t l2 = ed[k] & 15u, xd = (ed[k] >> 4) & 15u;
                        const uint32_t dist = (ed[k] >> 16) + __builtin_amdgcn_ubfe(h2[k] >> l2, 0, xd);
                        // (selects by mask arithmetic: written as ?: the compiler turns the two token kinds into branches on exec)
                        const uint32_t litm = 0u - ((e[k] >> 8) & 1u), l1 = e[k] & 15u;
                        const uint32_t tokm = litm | (0u - ((e[k] & ed[k] & kEntLen) >> 10));
                        const uint32_t nb = l1 + ((t[k] - l1 + l2 + xd) & ~litm);
                        const uint32_t as_lit = 1u | ((e[k] >> 16) << 2), as_match = 2u | (len[k] << 2) | ((dist - 1) << 11);
                        word[k] = (as_lit & litm) | (as_match & ~litm);
                        info[k] = (tokm != 0 && p + 64 * k + nb <= b.seg_bits) ? nb : 64u;
                    }
                    info0 = info[0]; word0 = word[0]; info1 = info[1]; word1 = word[1];
                }
                INF_T(8);
                // the walk: token starts from offset 0 on (a lane that is not a token is marked too and ends it)
                uint64_t marks0 = 0, marks1 = 0;
                uint32_t cur = 0;
                do { mark_bit(marks0, cur); cur += (uint32_t)__builtin_amdgcn_readlane((int)info0, (int)cur); } while (cur < 64);
                const uint64_t bad0 = __ballot(info0 == 64u) & marks0;
                if (bad0) { cur = (uint32_t)__builtin_ctzll(bad0); marks0 &= (1ull << cur) - 1; }
                else {
                    uint32_t c1 = cur - 64;
                    do { mark_bit(marks1, c1); c1 += (uint32_t)__builtin_amdgcn_readlane((int)info1, (int)c1); } while (c1 < 64);
                    const uint64_t bad1 = __ballot(info1 == 64u) & marks1;
                    if (bad1) { c1 = (uint32_t)__builtin_ctzll(bad1); marks1 &= (1ull << c1) - 1; }
                    cur = 64 + c1;
                }
                if (cur != 0) {
                    emit_tokens(marks0, word0);
                    if (marks1) emit_tokens(marks1, word1);
                    INF_N(n_lit); // (steps)
                    INF_T(9);
                    pos += cur;
                    continue;
                }
                // ---- one symbol through the scalar reader ----
                INF_N(n_slow);
                reposition(pos);
                uint32_t e = uni(L.ltab[(uint32_t)b.hold & ((1u << kLBits) - 1)]);
                if (e) drop(b, e & 15u);
                else { // a code longer than the table, or no code at all
                    const uint32_t s2 = long_code((uint32_t)b.hold, lrows, L.lsym, lane);
                    if (s2 == 0xFFFFu) { err = kMsgLitCode; break; }
                    drop(b, s2 >> 16);
                    e = make_entry(1, s2 & 0xFFFFu, 0);
                }
                uint32_t tokw;
                if (e & kEntLit) tokw = 1u | ((e >> 16) << 2);
                else {
                    if (e & kEntEob) { eob = true; pos = consumed_bits(b); if (pos > b.seg_bits) err = kMsgTruncated; break; }
                    if (e & kEntBad) { err = kMsgLitCode; break; }
                    const uint32_t xl = (e >> 4) & 15u, len = (e >> 16) + peek(b, xl);
                    drop(b, xl);
                    refill(b, L.stage);
                    uint32_t ed = uni(L.dtab[(uint32_t)b.hold & ((1u << kDBits) - 1)]);
                    if (ed) drop(b, ed & 15u);
                    else {
                        const uint32_t d2 = long_code((uint32_t)b.hold, drows, L.dsym, lane);
                        if (d2 == 0xFFFFu) { err = kMsgDistCode; break; }
                        drop(b, d2 >> 16);
                        ed = make_entry(2, d2 & 0xFFFFu, 0);
                    }
                    if (ed & kEntBad) { err = kMsgDistCode; break; }
                    const uint32_t xd = (ed >> 4) & 15u, dist = (ed >> 16) + peek(b, xd);
                    drop(b, xd);
                    tokw = 2u | (len << 2) | ((dist - 1) << 11);
                }
                pos = consumed_bits(b);
                if (pos > b.seg_bits) { err = kMsgTruncated; break; } // the token runs past the end of the segment
                emit_tokens(1ull, tokw);
                INF_T(12);
            }
            // the scalar reader takes over again at the block boundary
            if (eob && !err) reposition(pos);
            else if (err == kMsgTruncated && !eob) reposition(pos);
        }
        // an error found in bits that lie past the end of the segment is the zero padding talking: the segment is truncated
        if (err && consumed_bits(b) > b.seg_bits) err = kMsgTruncated;
        if (!err && !stop) {
            const uint32_t used = consumed_bits(b);
            if (used > b.seg_bits) err = kMsgTruncated;                       // decoded past the end of the segment
            else if (SPEC) { if (!seen_final && org_bits + used - lead * 8 < stop_bits) err = kMsgTruncated; } // the input ended first
            else if (must_be_final && !seen_final) err = kMsgTruncated;       // the stream never ends
            else if (stream_mode && seen_final) { }                           // stream mode: the stream ends where its final block ends, whatever follows
            else if (!must_be_final && seen_final) err = kMsgTrailing;        // a final block before the last segment
            else if (((b.seg_bits - used) >> 3) != 0) err = kMsgTrailing;     // whole bytes left over
            if (!err && lane == 0) { L.end_bits = org_bits + used - lead * 8; L.end_final = seen_final ? 1u : 0u; } // counted from the segment's first byte
        }
        emit_command(3u | (kCmdEnd << 2) | (err << 4), 1, true);
        if constexpr (SIZES) { // the record the writer ends with: an error of the counting lies in front of whatever the reader found behind it
            if (size_err) err = size_err;
            wave_sync(); // (lane 0's end_bits / end_final)
            if (lane == 0) {
                status[c].code = err ? ZGPU_DATA_ERROR : ZGPU_OK;
                status[c].msg = err ? err : ((L.end_bits & 7u) << 24); status[c].out_bytes = err ? 0 : size_o;
                status[c].used = err ? 0u : (((L.end_bits + 7u) >> 3) | (L.end_final << 31));
                if constexpr (SPEC) { // the piece's end record, as the SPEC decode's writer forms it (no page pool: bit 1 stays clear), and its reach
                    sp.ends[gc].end_bit = seg_lo * 8 + L.end_bits; sp.ends[gc].out_bytes = err ? 0 : size_o; sp.ends[gc].flags = err ? (err << 8) : L.end_final;
                    sp.need[gc] = size_need;
                }
            }
        }
#ifdef ZGPU_INF_TIME
        if (lane == 0) { t_acc[5] = n_lit; t_acc[7] = n_slow; for (int i_ = 0; i_ < 16; i_++) if (t_acc[i_]) atomicAdd(&inf_time[i_], t_acc[i_]); }
#endif
        return;
    }

    // =========================================== writer ===========================================
    if constexpr (!SIZES) {
    uint32_t err = kMsgNone;
    uint32_t o = 0;       // bytes produced
    if constexpr (SPEC && VERIFY) {
        // the window of the slot in front, as bytes: its last `reach` bytes lie right below position 0 of the ring (whole 16-byte vectors: what a vector
        // brings in front of them is never read -- a distance beyond reach is an error).  A piece that is not its item's first has a slot in front: gc >= 1.
        if (reach) {
            const uint4 *w = reinterpret_cast<const uint4 *>(sp.windows + (gc - 1) * kOutRing);
            for (uint32_t i = ((kOutRing - reach) >> 4) + lane; i < kOutRing / 16; i += 64) reinterpret_cast<uint4 *>(L.out)[i] = w[i];
        }
    } else if (SPEC) {
        for (uint32_t i = lane; i < kOutRing; i += 64) L.out[i] = (ring_t)(0x8000u | i); // slot i, never written, is byte i of the window in front
        if (spec_first) for (uint32_t i = lane; i < dict_len; i += 64) L.out[(kOutRing - dict_len + i) & (kOutRing - 1)] = dict[i];
    } else
    for (uint32_t i = lane; i < reach; i += 64) L.out[(kOutRing - reach + i) & (kOutRing - 1)] = dict[i];
    uint32_t flushed = 0; // bytes already copied from the LDS ring to the destination (a multiple of kOutHalf until the end)
    bool nofit = false;   // direct placement: the destination ended before the chunk did
    FoldRun run{1, 0, 0}; // VERIFY, FOLD: Adler-32 (halves) and CRC-32 of output bytes [0, flushed)
    const uint32_t want = VERIFY ? (uint32_t)out_cap : FOLD ? fold_checks : 0u, do_adler = want & 1u, do_crc = want & 2u;
    if constexpr (VERIFY || FOLD) {
        if (do_crc) for (uint32_t i = lane; i < kCrcNibWords; i += 64) L.crc_nib[i] = crc_nib_entry(i);
    }
    uint8_t *dst = VERIFY ? nullptr : BATCH ? out + offsets[4 * gc + 2] : compact ? out + (uint64_t)c * kChunkMax : whole ? out : out + gc * (uint64_t)chunk_size;
    const uint64_t dst_room = VERIFY ? ~0ull : BATCH ? offsets[4 * gc + 3] - offsets[4 * gc + 2] : SPEC ? ~0ull : compact ? kChunkMax : whole ? out_cap : (out_cap > gc * (uint64_t)chunk_size ? out_cap - gc * (uint64_t)chunk_size : 0);
    // copy a match of `len` bytes at distance `dist` to output position `at`; a distance shorter than the length repeats its
    // pattern (byte-sequential semantics of inffast.c:246-259).  The ring holds the last 32 KiB: a read at the full distance
    // 32768 hits the slot its own lane is about to write.
    auto copy_match = [&](uint32_t at, uint32_t len, uint32_t dist) {
        __builtin_amdgcn_wave_barrier();
        if (len <= 64 && dist >= len) { // the common case
            if (lane < len) { const ring_t v = L.out[(at - dist + lane) & (kOutRing - 1)]; L.out[(at + lane) & (kOutRing - 1)] = v; }
        } else if (dist >= len || dist >= 64) {
            for (uint32_t i0 = 0; i0 < len; i0 += (dist < 64 ? dist : 64)) {
                const uint32_t span = dist < 64 ? dist : 64, i = i0 + lane;
                ring_t v = 0;
                if (lane < span && i < len) v = L.out[(at - dist + i) & (kOutRing - 1)];
                if (lane < span && i < len) L.out[(at + i) & (kOutRing - 1)] = v;
                __builtin_amdgcn_wave_barrier();
            }
        } else {
            const uint32_t recip = 0xFFFFFFFFu / dist + 1;
            for (uint32_t i = lane; i < len; i += 64) {
                const uint32_t qd = dist == 1 ? i : __umulhi(i, recip), r = i - qd * dist; // recip overflows for dist 1
                L.out[(at + i) & (kOutRing - 1)] = L.out[(at - dist + r) & (kOutRing - 1)];
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    // copy bytes [flushed, upto) of the output to the destination; the range never wraps in the ring
    auto flush_to = [&](uint32_t upto) {
        INF_T(11);
        wave_sync();
        uint32_t nbytes = upto - flushed;
        if constexpr (VERIFY) { // the fold: ring bytes [flushed, upto) into the running check values (flushed is a multiple of kOutHalf: 16-byte aligned)
            run = verify_fold(reinterpret_cast<const uint8_t *>(L.out) + (flushed & (kOutRing - 1)), nbytes, L.crc_nib, lane, do_adler, do_crc, run);
            flushed = upto;
            return;
        }
        if (SPEC) { // the next page of the pool (flushed is a multiple of kOutHalf: the page's index within the segment)
            if constexpr (NOPAGES) { flushed = upto; return; } // (no pages: the tails pass of the verify form keeps the ring and nothing else)
            uint32_t page = 0;
            if (lane == 0) page = atomicAdd(sp.page_count, 1u);
            page = uni(page);
            if (page >= sp.page_cap) nofit = true;
            else {
                if (lane == 0) sp.page_owner[page] = (gc << 32) | (flushed / kOutHalf);
                const uint4 *s128 = reinterpret_cast<const uint4 *>(L.out + (flushed & (kOutRing - 1)));
                uint4 *d128 = reinterpret_cast<uint4 *>(sp.mid + (uint64_t)page * kOutHalf);
                for (uint32_t i = lane; i < (nbytes + 7) / 8; i += 64) d128[i] = s128[i]; // (whole vectors: the page and the ring half have the room)
            }
            flushed = upto;
            return;
        }
        if constexpr (FOLD) // the fold in front of the store, out of the ring (flushed is a multiple of kOutHalf: 16-byte aligned; nbytes <= kOutHalf = kFoldMax)
            run = verify_fold(reinterpret_cast<const uint8_t *>(L.out) + (flushed & (kOutRing - 1)), nbytes, L.crc_nib, lane, do_adler, do_crc, run);
        if ((uint64_t)flushed + nbytes > dst_room) { nofit = true; nbytes = dst_room > flushed ? (uint32_t)(dst_room - flushed) : 0; }
        const uint8_t *src_r = reinterpret_cast<const uint8_t *>(L.out) + (flushed & (kOutRing - 1)); // (the byte ring; SPEC has returned above)
        uint8_t *d = dst + flushed;
        if ((reinterpret_cast<uintptr_t>(d) & 15) == 0) {
            const uint4 *s128 = reinterpret_cast<const uint4 *>(src_r);
            for (uint32_t i = lane; i < (nbytes >> 4); i += 64) reinterpret_cast<uint4 *>(d)[i] = s128[i];
            for (uint32_t i = (nbytes & ~15u) + lane; i < nbytes; i += 64) d[i] = src_r[i];
        } else {
            for (uint32_t i = lane; i < nbytes; i += 64) d[i] = src_r[i];
        }
        flushed = upto;
        if (FAR) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // what has been flushed IS in memory: matches read it back from there
        INF_T(3);
    };
    uint32_t reader_err = kMsgNone;
    INF_T(0);
    for (uint32_t half = 0;; half++) {
        block_sync(); // the reader has completed this half of the ring
        INF_T(14);
        const uint32_t tw = L.tok[(half & 1) * 64 + lane];
        const uint32_t kind = tw & 3u;
        uint64_t cmds = __ballot(kind == 3);
        uint32_t from = 0; // lanes below are done
        bool ended = false;
        for (;;) { // runs of tokens between the commands of this half; after an error only the commands are followed
            const uint32_t upto = cmds ? (uint32_t)__builtin_ctzll(cmds) : 64u;
            if (!err) { // ---- the tokens in lanes [from, upto) ----
                o = uni(o); flushed = uni(flushed);
                const bool inr = lane >= from && lane < upto;
                const uint32_t k2 = inr ? kind : 0u, len = (tw >> 2) & 511u, ol = k2 == 1 ? 1u : k2 == 2 ? len : 0u;
                const uint32_t incl = wave_prefix_sum(ol), offv = o + incl - ol, o_end = o + (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                // limits that depend on the output position, in the order inffast.c checks them for one token
                const bool far = k2 == 2 && (tw >> 11) >= offv + reach, over = offv + ol > chunk_size;
                const uint64_t bad = __ballot(far || over);
                if (bad) err = ((__ballot(far) >> (uint32_t)__builtin_ctzll(bad)) & 1) ? kMsgTooFar : kMsgOutput;
                uint64_t todo = bad ? 0ull : __ballot(ol != 0);
                // FAR: matches whose source is no longer in the ring (the ring holds the RING bytes in front of a token when its turn comes)
                uint64_t farm = 0, pfm = 0;
                uint32_t p0, p1, p2, p3, p4, p5, p6, p7; // (written by the loads below when they arrive, read after the wait in front of their first use: nothing else may touch them in between)
                if (FAR) {
                    const bool isfar = k2 == 2 && (tw >> 11) >= kOutRing;
                    farm = todo & __ballot(isfar);
                    if (farm && dst_room >= 32) {
                        // the source ends below flushed - RING / 2 + 516: flushed, and in memory (flush_to waits for its stores).  32 bytes at once when
                        // the match is that short and the 32 bytes lie inside what is flushed (and inside the destination: one that is too small gets no
                        // reads past its end).  Every lane loads -- the others the destination's first bytes -- so that the registers have one writer;
                        // sc0 sc1: from memory, not from a line this CU's cache took in when only a part of it had been flushed.
                        const uint32_t s0 = offv - (tw >> 11) - 1;
                        const bool rdy = isfar && len <= 32 && s0 + 32 <= flushed && (uint64_t)s0 + 32 <= dst_room;
                        pfm = farm & __ballot(rdy);
                        const uint8_t *ps = dst + (rdy ? s0 : 0u);
                        if (pfm) // (uniform; every such run waits for these loads when the first of its lanes' matches is copied)
                        asm volatile("global_load_dword %0, %8, off sc0 sc1\n\tglobal_load_dword %1, %8, off offset:4 sc0 sc1\n\t"
                                     "global_load_dword %2, %8, off offset:8 sc0 sc1\n\tglobal_load_dword %3, %8, off offset:12 sc0 sc1\n\t"
                                     "global_load_dword %4, %8, off offset:16 sc0 sc1\n\tglobal_load_dword %5, %8, off offset:20 sc0 sc1\n\t"
                                     "global_load_dword %6, %8, off offset:24 sc0 sc1\n\tglobal_load_dword %7, %8, off offset:28 sc0 sc1"
                                     : "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3), "=&v"(p4), "=&v"(p5), "=&v"(p6), "=&v"(p7) : "v"(ps) : "memory");
                    }
                }
                // Literals are stored by their lanes ahead of the match copies of the same pass.  The ring is exactly as long as
                // the farthest distance, so a store that far ahead may hit what an earlier match still has to read: position
                // q lands on the slot of q - 32768.  A pass therefore ends with the first match whose source would be reached
                // by the pass's last byte (and with the half of the ring that is flushed next).
                while (todo) {
                    const uint32_t lim = flushed + kOutHalf;
                    uint64_t take = todo & __ballot(offv < lim), rest = todo & ~take;
                    uint32_t pend = rest ? (uint32_t)__builtin_amdgcn_readlane((int)offv, (int)__builtin_ctzll(rest)) : o_end;
                    const uint64_t hz = take & ~farm & __ballot(k2 == 2 && offv + (kOutRing - 1) - (tw >> 11) < pend);
                    if (hz) {
                        take &= (2ull << (uint32_t)__builtin_ctzll(hz)) - 1; rest = todo & ~take;
                        pend = rest ? (uint32_t)__builtin_amdgcn_readlane((int)offv, (int)__builtin_ctzll(rest)) : o_end;
                    }
                    if (sel_mask(take, k2, 0u) == 1) L.out[offv & (kOutRing - 1)] = (ring_t)(uint8_t)(tw >> 2);
                    INF_T(10);
                    uint64_t mm = take & __ballot(k2 == 2);
                    if (ZGPU_INF_PARCOPY) {
                        // The matches whose source ends in front of what this pass produces do not depend on each other or on the pass's literals: they are copied together, 64 bytes of
                        // their concatenation a step -- byte b belongs to the first match whose running length exceeds b (a search over the lanes' prefix sums by shuffles) --
                        // instead of one match after the other (most are under ten bytes: six lanes of 64 at work, 215 ns each at ten segments a CU).  The others -- a source inside the
                        // pass's own output, a distance shorter than the length, a source that is read back from the destination -- follow in order as before.
                        const uint32_t dist = (tw >> 11) + 1;
                        const bool ind = ((take >> lane) & 1ull) && k2 == 2 && !(FAR && ((farm >> lane) & 1ull)) && dist >= (offv - o) + len;
                        const uint64_t pm = __ballot(ind);
                        if (__builtin_popcountll(pm) >= 2) {
                            const uint32_t li = ind ? len : 0u, incl = wave_prefix_sum(li), T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                            __builtin_amdgcn_wave_barrier();
                            for (uint32_t it = 0; it < T; it += 64) {
                                const uint32_t b = it + lane;
                                uint32_t lo = 0, hi = 63;
#pragma unroll
                                for (int st = 0; st < 6; st++) { const uint32_t mid = (lo + hi) >> 1, v = (uint32_t)__shfl((int)incl, (int)mid); if (v > b) hi = mid; else lo = mid + 1; }
                                const uint32_t im = (uint32_t)__shfl((int)incl, (int)lo), lm = (uint32_t)__shfl((int)li, (int)lo), om = (uint32_t)__shfl((int)offv, (int)lo), dm = (uint32_t)__shfl((int)dist, (int)lo);
                                const uint32_t j = b - (im - lm);
                                if (b < T) { const ring_t v = L.out[(om - dm + j) & (kOutRing - 1)]; L.out[(om + j) & (kOutRing - 1)] = v; }
                            }
                            __builtin_amdgcn_wave_barrier();
                            mm &= ~pm;
                        }
                    }
                    while (mm) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(mm); mm &= mm - 1;
                        const uint32_t t2 = (uint32_t)__builtin_amdgcn_readlane((int)tw, (int)l), mo = (uint32_t)__builtin_amdgcn_readlane((int)offv, (int)l);
                        if (FAR && ((farm >> l) & 1ull)) {
                            const uint32_t flen = (t2 >> 2) & 511u, fs = mo - (t2 >> 11) - 1;
                            __builtin_amdgcn_wave_barrier();
                            if ((pfm >> l) & 1ull) { // the 32 bytes lane l asked for: byte i to lane i
                                // (the wait and the reads of the loaded registers in ONE statement: the compiler must not read -- copy -- them before the loads have landed)
                                uint32_t d0, d1, d2, d3, d4, d5, d6, d7;
                                asm volatile("s_waitcnt vmcnt(0)\n\t"
                                             "v_readlane_b32 %0, %8, %16\n\tv_readlane_b32 %1, %9, %16\n\tv_readlane_b32 %2, %10, %16\n\tv_readlane_b32 %3, %11, %16\n\t"
                                             "v_readlane_b32 %4, %12, %16\n\tv_readlane_b32 %5, %13, %16\n\tv_readlane_b32 %6, %14, %16\n\tv_readlane_b32 %7, %15, %16"
                                             : "=&s"(d0), "=&s"(d1), "=&s"(d2), "=&s"(d3), "=&s"(d4), "=&s"(d5), "=&s"(d6), "=&s"(d7)
                                             : "v"(p0), "v"(p1), "v"(p2), "v"(p3), "v"(p4), "v"(p5), "v"(p6), "v"(p7), "s"(l) : "memory");
                                const uint32_t ws = (lane >> 2) & 7u;
                                const uint32_t wv = ws == 0 ? d0 : ws == 1 ? d1 : ws == 2 ? d2 : ws == 3 ? d3 : ws == 4 ? d4 : ws == 5 ? d5 : ws == 6 ? d6 : d7;
                                if (lane < flen) L.out[(mo + lane) & (kOutRing - 1)] = (ring_t)(uint8_t)(wv >> (8 * (lane & 3u)));
                            } else { // longer than 32 bytes, or asked for too early: from memory now
                                for (uint32_t i = lane; i < flen; i += 64) {
                                    uint8_t v = 0;
                                    if ((uint64_t)fs + i < dst_room) v = __hip_atomic_load(dst + fs + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    L.out[(mo + i) & (kOutRing - 1)] = (ring_t)v;
                                }
                            }
                            __builtin_amdgcn_wave_barrier();
                        } else
                        copy_match(mo, (t2 >> 2) & 511u, (t2 >> 11) + 1);
                        INF_N(n_mat);
                    }
                    todo = rest; o = pend;
                    if (o >= lim) flush_to(lim);
                    INF_T(11);
                }
            }
            if (upto == 64) break;
            // ---- the command in lane upto ----
            const uint32_t cw = (uint32_t)__builtin_amdgcn_readlane((int)tw, (int)upto);
            if (((cw >> 2) & 3u) == kCmdEnd) { reader_err = (cw >> 4) & 255u; ended = true; break; }
            if (!err) {
                const uint64_t soff = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)tw, (int)((upto + 2) & 63u)) << 32) |
                                      (uint32_t)__builtin_amdgcn_readlane((int)tw, (int)((upto + 1) & 63u));
                const uint8_t *src = in + soff;
                const uint32_t slen = (cw >> 4) & 0x1FFFFu;
                if (o + slen > chunk_size) err = kMsgOutput;
                else for (uint32_t done = 0; done < slen;) { // through the ring, half by half
                    const uint32_t room = flushed + kOutHalf - o, part = slen - done < room ? slen - done : room;
                    for (uint32_t i = lane; i < part; i += 64) L.out[(o + i) & (kOutRing - 1)] = src[done + i];
                    o += part; done += part;
                    if (o == flushed + kOutHalf) flush_to(o);
                }
            }
            from = upto + 3;
            cmds &= ~(7ull << upto);
        }
        if (ended) break;
        if (err && lane == 0) L.abort_flag = 1; // void output: the reader stops at its next hand-over and sends its end command
    }
    if (!err) err = reader_err;
    if (!err && !compact && !SPEC && !must_be_final && o != chunk_size) err = kMsgShort; // direct placement assumes full chunks
    // the rest of the chunk (an error leaves what was flushed before it was found; the status says the chunk is void)
    if (!err && (!SPEC || o != flushed)) flush_to(o);
    if (SPEC && !VERIFY && !err) // the ring is the last 32 KiB of what this segment knows: slots it never wrote still name the window in front
        for (uint32_t j = lane; j < kOutRing; j += 64) sp.tails[gc * kOutRing + j] = L.out[(o + j) & (kOutRing - 1)];
    const bool fits = !nofit;
    INF_T(4);
    if (lane == 0) {
        status[c].code = err ? ZGPU_DATA_ERROR : (fits ? ZGPU_OK : ZGPU_BUF_ERROR);
        status[c].msg = err ? err : ((L.end_bits & 7u) << 24); status[c].out_bytes = err ? 0 : o; // (a segment that decoded: the bits of its last byte that are its own, for a stream taken up at a bit offset)
        status[c].used = err ? 0u : (((L.end_bits + 7u) >> 3) | (L.end_final << 31));
        if constexpr (SPEC && VERIFY) { // the check's record: the end as the tails pass forms it, and the piece's own check values
            PieceCheck r{};
            r.end_bit = seg_lo * 8 + L.end_bits; r.out_bytes = err ? 0 : o; r.flags = err ? (err << 8) : L.end_final; r.adler_a = run.a; r.adler_b = run.b; r.crc = run.crc;
            sp.checks[gc] = r;
        } else if (SPEC) { sp.ends[gc].end_bit = seg_lo * 8 + L.end_bits; sp.ends[gc].out_bytes = err ? 0 : o; sp.ends[gc].flags = err ? (err << 8) : (L.end_final | (nofit ? 2u : 0u)); }
#ifdef ZGPU_INF_TIME
        t_acc[6] = n_mat;
        for (int i_ = 0; i_ < 16; i_++) if (t_acc[i_]) atomicAdd(&inf_time[i_], t_acc[i_]);
#endif
        if constexpr (SPEC && VERIFY) { } // (the check pass: its values stand in the record above)
        else if constexpr (VERIFY || FOLD) { meta[c].out_bytes = err ? 0 : o; meta[c].adler_a = run.a; meta[c].adler_b = run.b; meta[c].crc = run.crc; }
        else if (meta) { meta[c].out_bytes = err ? 0 : o; meta[c].ntok = 0; meta[c].adler_a = 1; meta[c].adler_b = 0; meta[c].in_bytes = 0; meta[c].data_type = 2; }
    }
    } // !SIZES
}

// first failing chunk + total bytes (one workgroup; chunk order matters for "first")
// stream_mode: the segments are candidate pieces of ONE stream that ends where its first final block ends.  Segments behind that
// one are not part of it (whatever they decoded to is dropped: their meta.out_bytes is cleared for the scan and the stitcher);
// and when the only failure is the last segment stopping inside a block, the segments before it stand as a partial result.
__global__ void __launch_bounds__(1024) inflate_reduce_kernel(const InfStatus *st, uint32_t nchunks, uint64_t chunk0, uint32_t chunk_size, uint64_t *acc,
                                                              uint32_t stream_mode, uint64_t last_chunk, ChunkMeta *meta, uint32_t trunc_msg)
{
    // acc[0] total bytes, acc[1] first bad chunk (+1, 0 = none), acc[2] its code, acc[3] its msg, acc[4] "short chunk before the end" flag,
    // acc[5] chunk that ends the stream (+1), acc[6] input bytes of that chunk used, acc[7] chunk at which a partial result stops (+1)
    __shared__ unsigned long long bad_min, fin_min;
    __shared__ unsigned long long total;
    if (threadIdx.x == 0) { bad_min = ~0ull; fin_min = ~0ull; total = 0; }
    __syncthreads();
    if (acc[5] != 0 || acc[7] != 0) { // an earlier batch ended the stream (or the partial result): nothing of this batch counts
        if (meta) for (uint32_t i = threadIdx.x; i < nchunks; i += 1024) meta[i].out_bytes = 0;
        return;
    }
    unsigned long long bad = ~0ull, fin = ~0ull;
    for (uint32_t i = threadIdx.x; i < nchunks; i += 1024) {
        if (st[i].code != 0 && bad == ~0ull) bad = chunk0 + i;
        if (stream_mode && st[i].code == 0 && (st[i].used >> 31) && fin == ~0ull) fin = chunk0 + i;
    }
    atomicMin(&bad_min, bad);
    atomicMin(&fin_min, fin);
    __syncthreads();
    unsigned long long upto = chunk0 + nchunks; // chunks [chunk0, upto) count
    if (stream_mode) {
        if (fin_min != ~0ull && fin_min < bad_min) upto = fin_min + 1;                       // the stream ends in chunk fin_min
        else if (bad_min != ~0ull && bad_min == last_chunk && st[bad_min - chunk0].msg == trunc_msg) upto = bad_min; // incomplete tail
    }
    unsigned long long t = 0;
    for (uint32_t i = threadIdx.x; i < nchunks; i += 1024) {
        if (chunk0 + i < upto) t += st[i].out_bytes;
        else if (meta) meta[i].out_bytes = 0;
    }
    atomicAdd(&total, t);
    __syncthreads();
    if (threadIdx.x == 0) {
        acc[0] += total;
        if (stream_mode && upto != chunk0 + nchunks) {
            if (fin_min != ~0ull && fin_min < bad_min) { acc[5] = fin_min + 1; acc[6] = (st[fin_min - chunk0].used & 0x7fffffffu) | ((unsigned long long)((st[fin_min - chunk0].msg >> 24) & 7u) << 56); }
            else acc[7] = bad_min + 1;
        } else if (acc[1] == 0 && bad_min != ~0ull) { acc[1] = bad_min + 1; acc[2] = (uint64_t)(int64_t)st[bad_min - chunk0].code; acc[3] = st[bad_min - chunk0].msg; }
        else if (stream_mode && fin_min != ~0ull) { acc[5] = fin_min + 1; acc[6] = (st[fin_min - chunk0].used & 0x7fffffffu) | ((unsigned long long)((st[fin_min - chunk0].msg >> 24) & 7u) << 56); } // (the final block ends the last chunk)
    }
}

int inflate_ring_kb()
{
    int ring_kb = ZGPU_INF_RING_DEFAULT_KB;
    if (const char *v = getenv("ZGPU_INF_RING_KB")) ring_kb = atoi(v);
    return (ring_kb == 8 || ring_kb == 16) ? ring_kb : 32;
}

// Every launch of the decoder: one launch per call (the batch loops are the callers'), the instantiation, block size and LDS size picked here.
// ring_kb counts for chunks and batch items only: whether a small ring may serve a call is the caller's to say (inflate_run).
void launch_inflate_decode(InfKind kind, int ring_kb, const InfLaunch &a, const SpecArgs &sp, hipStream_t st)
{
    constexpr size_t kLds8 = sizeof(InflateLdsT<uint8_t, 8192>), kLds16 = sizeof(InflateLdsT<uint8_t, 16384>);
    static bool opt_in = false;
    if (!opt_in) {
        hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel_t<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InflateLds));
        hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel_t<false, 16384>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds16);
        hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel_t<false, 8192>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds8);
        hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel_t<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InflateLdsSpec));
        hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel_t<true, ZGPU_INF_RING, false, false, false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InflateLdsSpec));
        hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel_t<false, 32768, true, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InflateLdsVerify));
        hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel_t<true, 32768, false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InflateLdsVerify));
        hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel_t<false, 32768, true, false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InflateLdsFoldT<32768>));
        hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel_t<false, 16384, true, false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InflateLdsFoldT<16384>));
        hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel_t<false, 8192, true, false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InflateLdsFoldT<8192>));
        opt_in = true;
    }
    // (one pointer type for all instantiations: __launch_bounds__ is no part of the type, so the 64-thread sizing kernel goes through it on purpose; `threads` counts)
    auto go = [&](decltype(&inflate_kernel_t<false>) kern, uint32_t threads, size_t lds) {
        hipLaunchKernelGGL(kern, dim3(a.nchunks), dim3(threads), lds, st, a.in, a.in_bytes, a.offsets, a.chunk0, a.nchunks, a.last_chunk, a.chunk_size, a.out, a.out_cap,
                           a.status, a.meta, a.dict, a.dict_len, a.stream_mode, sp, a.checks);
    };
    if (kind == kInfPieces && sp.mid == nullptr) go(inflate_kernel_t<true, ZGPU_INF_RING, false, false, false, false, true>, 128, sizeof(InflateLdsSpec)); // (the no-pages form: an instantiation of its own, so the decode in pieces is the code it was)
    else if (kind == kInfPieces) go(inflate_kernel_t<true>, 128, sizeof(InflateLdsSpec));
    else if (kind == kInfSizes) go(inflate_kernel_t<false, ZGPU_INF_RING, true, true>, 64, sizeof(InflateLdsSizes));
    else if (kind == kInfPieceSizes) go(inflate_kernel_t<true, ZGPU_INF_RING, false, true>, 64, sizeof(InflateLdsSizes));
    else if (kind == kInfPieceVerify) go(inflate_kernel_t<true, 32768, false, false, true>, 128, sizeof(InflateLdsVerify));
    else if (kind == kInfVerify) go(inflate_kernel_t<false, 32768, true, false, true>, 128, sizeof(InflateLdsVerify));
    else if (kind == kInfBatchFold) {
        if (ring_kb == 8) go(inflate_kernel_t<false, 8192, true, false, false, true>, 128, sizeof(InflateLdsFoldT<8192>));
        else if (ring_kb == 16) go(inflate_kernel_t<false, 16384, true, false, false, true>, 128, sizeof(InflateLdsFoldT<16384>));
        else go(inflate_kernel_t<false, 32768, true, false, false, true>, 128, sizeof(InflateLdsFoldT<32768>));
    }
    else if (kind == kInfBatch) {
        if (ring_kb == 8) go(inflate_kernel_t<false, 8192, true>, 128, kLds8);
        else if (ring_kb == 16) go(inflate_kernel_t<false, 16384, true>, 128, kLds16);
        else go(inflate_kernel_t<false, ZGPU_INF_RING, true>, 128, sizeof(InflateLds));
    } else {
        if (ring_kb == 8) go(inflate_kernel_t<false, 8192>, 128, kLds8);
        else if (ring_kb == 16) go(inflate_kernel_t<false, 16384>, 128, kLds16);
        else go(inflate_kernel_t<false>, 128, sizeof(InflateLds));
    }
}

// Adler-32 and CRC-32 of the produced bytes, as far as zgpu_inflate_set_checks asks for them, over 64 KiB pieces of the output (checksum_pass, zgpu_engine.hip)
int output_checksums(zgpu_engine *e, const uint8_t *d_out, uint64_t nbytes, uint64_t out_cap, zgpu_inflate_result *res, hipStream_t st)
{
    const uint64_t max_pieces = (out_cap >> 16) + 2;
    int rc = ZGPU_OK;
    res->adler32 = 1; res->crc32 = 0;
    if (e->inf_checks) rc = checksum_pass(e, d_out, nbytes, e->inf_checks, (uint32_t)(max_pieces < 65536 ? max_pieces : 65536), e->inf_meta, st, &res->adler32, &res->crc32);
    collect_spans(e);
    return rc;
}

// stream_mode (compact or whole-stream calls): see inflate_reduce_kernel; h_offsets = the offsets table on the host (for res->in_used);
// open_end: the last segment ends with a flush marker like the others, no segment has to hold the final block
// h_dst (direct placement only): the caller's host buffer of h_cap bytes; every batch's output is copied there on the engine's copy stream while
// the next batch is being decoded.  out_cap is the DEVICE buffer's room (whole chunks); no copy to the host reaches beyond h_cap, and a result that
// does not fit h_cap is an error before anything that was not served batch by batch is copied
int inflate_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_offsets, uint64_t nchunks, uint32_t chunk_size,
                uint8_t *d_out, uint64_t out_cap, zgpu_inflate_result *res, hipStream_t st, uint32_t stream_mode, const uint64_t *h_offsets, bool open_end,
                uint8_t *h_dst, uint64_t h_cap)
{
    // stream_mode bits 8-10: the one segment of a whole-stream call begins at that bit of its first byte (inflate_stream_host's decoder of a stream
    // taken up at a bit offset); only the decoding kernels see them
    const uint32_t kern_mode = chunk_size == kWholeStream ? stream_mode : (stream_mode & 255u);
    stream_mode &= 255u;
    const uint64_t host_cap = h_dst ? (h_cap < out_cap ? h_cap : out_cap) : 0;
    const uint64_t last_chunk = open_end ? ~0ull : nchunks - 1;
    if (!e || !res || !d_in || !d_out || !d_offsets || nchunks == 0 || (chunk_size > kChunkMax && !(chunk_size == kWholeStream && nchunks == 1)) ||
        (chunk_size == kWholeStream && in_bytes >= (1ull << 29)))
        return fail(e, ZGPU_STREAM_ERROR, "bad inflate arguments");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const bool compact = chunk_size == 0; // segments of any size: decode into slots, then concatenate
    // (one batch has nothing to overlap with.  Until round 3 these copies were bounded by the device buffer's size, not by the caller's: a buffer of
    // exactly the decoded length was overrun by up to a chunk -- which is what "threw inside the runtime" on small calls)
    static long tohost_min = -1;
    if (tohost_min < 0) { const char *v = getenv("ZGPU_TOHOST_MIN_CHUNKS"); tohost_min = v ? atol(v) : 4097; }
    const bool to_host = h_dst && chunk_size != 0 && chunk_size <= kChunkMax && (long)nchunks >= tohost_min;
    const uint32_t batch_cap = to_host ? 4096u : 65536u; // (host output: batches small enough for copies and kernels to take turns)
    const uint32_t batch = (uint32_t)(nchunks < batch_cap ? nchunks : batch_cap);
    if (e->inf_status.reserve(e, (size_t)batch * sizeof(InfStatus) + 64)) return ZGPU_MEM_ERROR;
    InfStatus *status = reinterpret_cast<InfStatus *>(e->inf_status.p);
    uint64_t *acc = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(status) + (((size_t)batch * sizeof(InfStatus) + 15) & ~(size_t)15));
    const uint64_t max_pieces = (out_cap >> 16) + 2;
    const uint32_t cbatch_cap = (uint32_t)(max_pieces < 65536 ? max_pieces : 65536); // the checksum pass works on 64 KiB pieces of the OUTPUT
    // meta and the offsets scratch (below) are sized here for the decode AND for the checksum pass behind it, so that the pass never regrows a buffer
    // the decode kernels were given
    if (e->inf_meta.reserve(e, batch > cbatch_cap ? batch : cbatch_cap)) return ZGPU_MEM_ERROR;
    ChunkMeta *meta = e->inf_meta;
    uint8_t *slots = nullptr;
    if (compact) { if (e->inf_slots.reserve(e, (size_t)batch * kChunkMax + 256)) return ZGPU_MEM_ERROR; slots = e->inf_slots; }
    res->adler32 = 1; res->crc32 = 0; res->first_bad_chunk = -1; res->error_code = 0; res->error_msg = 0; res->out_bytes = 0;
    res->in_used = in_bytes; res->in_used_bits = 0; res->stream_end = 0; res->incomplete = 0;
    ZGPU_HIP_CHECK(hipMemsetAsync(acc, 0, 8 * sizeof(uint64_t), st));
    RunState rs{}; rs.adler_a = 1;
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->run, &rs, sizeof rs, hipMemcpyHostToDevice, st));
    // the ring: 32 KiB (every distance inside it), or -- chunks that go straight to their place in the destination, no dictionary in front, not a whole
    // stream -- a smaller one with the far matches read back from the destination (more segments per CU).  ZGPU_INF_RING_KB=8|16|32 picks it.
    const int ring_here = (!compact && chunk_size != kWholeStream && e->inf_dict_len == 0) ? inflate_ring_kb() : 32;
    // (one argument set for all three rings: a small ring implies !compact and inf_dict_len == 0, so it gets d_out, no meta and a dictionary of 0 bytes)
    InfLaunch a{d_in, in_bytes, d_offsets, 0, 0, compact ? slots : d_out, out_cap, status, last_chunk, chunk_size, compact ? meta : nullptr, e->inf_dict.p, e->inf_dict_len, kern_mode};
    hipEvent_t ev{};
    int rc_sum = 0;
    prof_span_begin(e, st, &ev);
    if (e->inf_offs.reserve(e, nchunks + 1 + (out_cap >> 16) + 2)) return ZGPU_MEM_ERROR;
    uint64_t *oscr = e->inf_offs;
    for (uint64_t c0 = 0; c0 < nchunks; c0 += batch) {
        const uint32_t nb = (uint32_t)(nchunks - c0 < batch ? nchunks - c0 : batch);
        a.chunk0 = c0; a.nchunks = nb;
        launch_inflate_decode(kInfChunks, ring_here, a, SpecArgs{}, st);
        hipLaunchKernelGGL(inflate_reduce_kernel, dim3(1), dim3(1024), 0, st, status, nb, c0, chunk_size, acc, stream_mode, last_chunk, compact ? meta : nullptr, (uint32_t)kMsgTruncated);
        if (compact) {
            launch_scan(meta, nb, c0, oscr, e->run, out_cap, st); // out_bytes -> byte offsets, continuing across batches
            launch_stitch(slots, meta, oscr, c0, nb, d_out, out_cap, kChunkMax, st);
        }
        ZGPU_HIP_CHECK(hipGetLastError());
        if (to_host) { // the batch before this one goes to the host while this one is being decoded (a copy to pageable memory holds the host)
            const size_t b = (size_t)(c0 / batch);
            ZGPU_HIP_CHECK(hipEventRecord(engine_copy_event(e, b), st));
            if (b > 0) {
                const uint64_t lo = (c0 - batch) * chunk_size, hi = c0 * (uint64_t)chunk_size < host_cap ? c0 * (uint64_t)chunk_size : host_cap;
                ZGPU_HIP_CHECK(hipStreamWaitEvent(e->copy_stream, engine_copy_event(e, b - 1), 0));
                if (hi > lo) ZGPU_HIP_CHECK(hipMemcpyAsync(h_dst + lo, d_out + lo, hi - lo, hipMemcpyDeviceToHost, e->copy_stream));
            }
        }
    }
    if (to_host) {
        const size_t b = (size_t)((nchunks - 1) / batch);
        const uint64_t lo = b * (uint64_t)batch * chunk_size, hi = nchunks * (uint64_t)chunk_size < host_cap ? nchunks * (uint64_t)chunk_size : host_cap;
        ZGPU_HIP_CHECK(hipStreamWaitEvent(e->copy_stream, engine_copy_event(e, b), 0));
        if (hi > lo) ZGPU_HIP_CHECK(hipMemcpyAsync(h_dst + lo, d_out + lo, hi - lo, hipMemcpyDeviceToHost, e->copy_stream));
        ZGPU_HIP_CHECK(hipStreamSynchronize(e->copy_stream));
    }
    prof_span_end(e, st, ZGPU_STAGE_INFLATE, ev);
    uint64_t h[8];
    ZGPU_HIP_CHECK(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (stream_mode) {
        if (h[5]) { res->stream_end = 1; res->in_used = (h_offsets ? h_offsets[h[5] - 1] : 0) + (h[6] & 0xffffffffffffffull); }
        else if (h[7]) { res->incomplete = 1; res->in_used = h_offsets ? h_offsets[h[7] - 1] : 0; }
    }
    res->out_bytes = h[0]; res->first_bad_chunk = h[1] ? (int32_t)(h[1] - 1) : -1; res->error_code = (int32_t)(int64_t)h[2]; res->error_msg = (uint32_t)h[3];
    if (h[1]) { collect_spans(e); return fail(e, res->error_code, kInfMessages[res->error_msg < kMsgCount ? res->error_msg : 0]); }
    if (h[0] > out_cap || (h_dst && h[0] > host_cap)) { collect_spans(e); return fail(e, ZGPU_BUF_ERROR, "output capacity too small"); }
    rc_sum = output_checksums(e, d_out, h[0], out_cap, res, st);
    if (rc_sum) return rc_sum;
    if (h_dst && !to_host && h[0]) { // a host destination that was not served batch by batch
        ZGPU_HIP_CHECK(hipMemcpyAsync(h_dst, d_out, h[0], hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    }
    return ZGPU_OK;
}
} // namespace zgpu

extern "C" __attribute__((visibility("default"))) const char *zgpu_inflate_message(uint32_t index) { return index < zgpu::kMsgCount ? zgpu::kInfMessages[index] : ""; }

// ---- the C entry points of the chunked decoder (include/zamd_gpu.h): all they call is inflate_run ----
using namespace zgpu;

extern "C" {
#pragma GCC visibility push(default)

int zgpu_inflate_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_chunk_offsets, uint64_t nchunks,
                        uint32_t chunk_size, void *d_out, uint64_t out_cap, zgpu_inflate_result *res, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    return inflate_run(e, static_cast<const uint8_t *>(d_in), in_bytes, d_chunk_offsets, nchunks, chunk_size, static_cast<uint8_t *>(d_out), out_cap, res, st);
}

int zgpu_inflate_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *chunk_offsets, uint64_t nchunks, uint32_t chunk_size,
                      void *out, uint64_t out_cap, zgpu_inflate_result *res)
{
    if (!e || !res || !in || !out || !chunk_offsets || nchunks == 0) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const uint64_t need_out = nchunks * (uint64_t)(chunk_size ? chunk_size : kChunkMax);
    int rc = ensure_stage(e, in_bytes + 64, need_out);
    if (rc) return rc;
    if ((rc = e->offsets.reserve(e, nchunks + 1))) return rc;
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, in, in_bytes, hipMemcpyHostToDevice, e->stream));
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->offsets, chunk_offsets, (nchunks + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
    // direct placement with room for every chunk: the output goes to the caller's buffer batch by batch, under the decoding of the next batch
    // (the device buffer has room for nchunks whole chunks; the caller's buffer has out_cap bytes, and no copy into it goes beyond them)
    const bool stream_out = chunk_size != 0 && chunk_size <= kChunkMax;
    rc = inflate_run(e, e->stage_in, in_bytes, e->offsets, nchunks, chunk_size, e->stage_out, need_out, res, e->stream, 0, nullptr, false,
                     stream_out ? static_cast<uint8_t *>(out) : nullptr, out_cap);
    if (rc) return rc;
    if (res->out_bytes > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    if (!stream_out) ZGPU_HIP_CHECK(hipMemcpyAsync(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost, e->stream));
    ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream));
    return ZGPU_OK;
}

int zgpu_inflate_set_dictionary(zgpu_engine *e, const void *dict, uint32_t len)
{
    if (!e || (!dict && len)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    if (len > kWSize) { dict = static_cast<const uint8_t *>(dict) + (len - kWSize); len = kWSize; } // the window keeps the tail (inflate.c:1222-1226)
    if (len) { const int rc = e->inf_dict.reserve(e, kWSize); if (rc) return rc; }
    if (len) { ZGPU_HIP_CHECK(hipMemcpyAsync(e->inf_dict, dict, len, hipMemcpyHostToDevice, e->stream)); ZGPU_HIP_CHECK(hipStreamSynchronize(e->stream)); }
    e->inf_dict_len = len;
    return ZGPU_OK;
}

int zgpu_inflate_set_checks(zgpu_engine *e, uint32_t mask)
{
    if (!e || mask > 3u) return fail(e, ZGPU_STREAM_ERROR, "checks: a mask of ZGPU_CHECK_ADLER32 | ZGPU_CHECK_CRC32");
    e->inf_checks = mask;
    return ZGPU_OK;
}

#pragma GCC visibility pop
} // extern "C"
