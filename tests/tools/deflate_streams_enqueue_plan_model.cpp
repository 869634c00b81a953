// deflate_streams_enqueue_plan_model.cpp -- the device-side plan of the stream-ordered batch compress of items of any length on the CPU: the very functions the
// kernels of zlib_amd/csrc/zgpu_streams_batch.hip and the batched block layer of zgpu_cont.hip call (zlib_amd/csrc/zgpu_deflate_streams_plan.h), in plain loops.
// Usage: deflate_streams_enqueue_plan_model ROW...; every ROW is one argument and gives one line on stdout:
//   "ntiles L0 L1 ..."            per length: streams_ntiles(L) and the bound L / kTileStride + 1
//   "ws N IN_BYTES BATCH"         the workspace: ntiles_max, batch, rounds, total and every region as name=off,bytes; then what a round of `batch` one-tile streams
//                                 needs: parts, tokoff, blk_item, T, blk, pos, slots (bytes)
//   "rooms FLAGS IN_BYTES L0 .."  senq_rooms_bound(n, IN_BYTES, FLAGS) and streams_layout's total for items of these lengths
//   "scan IN_BYTES OUT_CAP IO0 .. / OO0 .."   senq_tile_scan of an explicit table: states, tile0, piece0
//   "plan BATCH SEED COUNT"       COUNT random good tables (empty items, one-tile items, long ones): the device's judgement of the tables against the host's -- senq_tile_scan
//                                 against streams_tile_scan, senq_tile_row against streams_tile_row (and padding rows behind) -- and the round plan both calls share
//                                 (streams_round_plan, streams_part_args) against a derivation by brute force written out here: the round's tiles one by one, each tile's
//                                 item by a linear walk, runs of one item grouped into parts, the caps as numbers; prints what was compared and the mismatches
//   "overlap SEED COUNT"          COUNT random tables whose ranges overlap or run backwards, rooms bad here and there: the tiles and pieces of the served stay within
//                                 ntiles_max, a failed item has none, the states are senq_item_state's or bad by the list's cap
// Built for the host only (tests/test_deflate_streams_enqueue_plan_cpu.py); no HIP call is made.
#include "../../zlib_amd/csrc/zgpu_deflate_streams_plan.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

using namespace zgpu;
typedef unsigned long long ull;

static uint64_t rng_state;
static uint64_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return rng_state >> 33; }

static uint64_t random_len()
{
    static const uint64_t edges[] = {0, 1, 65024, 65025, 97536, 97537, 65536, 130048, 130049};
    switch (rnd() % 6) {
    case 0: return 0;
    case 1: return rnd() % 5000;
    case 2: return edges[rnd() % 9];
    case 3: return 60000 + rnd() % 80000;
    case 4: return rnd() % 1000000;
    default: return 1 + rnd() % 65024;
    }
}

static bool row_eq(const TileRow &a, const TileRow &b) { return a.lo == b.lo && a.n == b.n && a.h0 == b.h0 && a.h1 == b.h1 && a.nent == b.nent && a.base == b.base && a.nil_local == b.nil_local; }

// the round plan by brute force, with nothing of the header's round plan in it
struct BrutePart { uint64_t item, a, b; }; // tiles [a, b) of the list belong to `item`
static uint64_t brute_item_of(const std::vector<uint64_t> &tile0, uint64_t n, uint64_t t)
{
    for (uint64_t k = 0; k < n; k++) if (tile0[k] <= t && t < tile0[k + 1]) return k;
    return n;
}
static uint64_t brute_tok_cap(uint64_t nt) { return (16384 + 32512 * (nt + 1) + 512 + 3) & ~3ull; }
static uint64_t brute_blk_cap(uint64_t nt) { return brute_tok_cap(nt) / 16383 + 2; }

static void plan(uint32_t batch, uint64_t seed, uint64_t count)
{
    rng_state = seed;
    ull tables = 0, tiles = 0, rounds = 0, parts = 0, bad = 0, mid = 0, pads = 0;
    for (uint64_t it = 0; it < count; it++) {
        const uint64_t n = 1 + rnd() % 24;
        std::vector<uint64_t> io(n + 1), oo(n + 1), h_tile0(n + 1), tile0(n + 1), piece0(n + 1);
        std::vector<uint32_t> state(n);
        io[0] = rnd() % 3 ? 0 : rnd() % 1000;
        for (uint64_t k = 0; k < n; k++) io[k + 1] = io[k] + random_len();
        const uint64_t in_bytes = io[n] + (rnd() % 2 ? 0 : rnd() % 100000);
        uint64_t out_cap = 0;
        streams_layout(io.data(), n, ZGPU_F_ZLIB_WRAP, oo.data(), &out_cap);
        if (!streams_tile_scan(io.data(), n, h_tile0.data())) { bad++; continue; }
        const uint64_t nt = senq_tile_scan(io.data(), oo.data(), n, in_bytes, out_cap, state.data(), tile0.data(), piece0.data());
        tables++; tiles += nt;
        if (nt != h_tile0[n] || nt > senq_ntiles_max(n, in_bytes) || piece0[n] > nt) bad++;
        for (uint64_t k = 0; k <= n; k++) if (tile0[k] != h_tile0[k]) bad++;
        for (uint64_t k = 0; k < n; k++) if (state[k] != kSenqServed) bad++;
        // the rows of the padded list
        const uint64_t b = senq_batch(n, in_bytes, batch), nr = senq_rounds(n, in_bytes, batch);
        if (nr * b < senq_ntiles_max(n, in_bytes)) bad++;
        for (uint64_t k = 0; k < n; k++)
            for (uint64_t ti = 0; ti < tile0[k + 1] - tile0[k]; ti++)
                if (!row_eq(senq_tile_row(io.data(), tile0.data(), n, tile0[k] + ti), streams_tile_row(io[k], io[k + 1] - io[k], ti))) bad++;
        for (uint64_t t = nt; t < nr * b; t++) { const TileRow r = senq_tile_row(io.data(), tile0.data(), n, t); pads++; if (!streams_row_is_pad(r) || r.h0 != r.h1) bad++; }
        for (uint64_t t = 0; t < nt; t++) if (streams_row_is_pad(senq_tile_row(io.data(), tile0.data(), n, t))) bad++;
        // the rounds
        std::vector<StreamsRoundPart> rp(b);
        for (uint64_t r = 0; r < nr; r++) {
            const uint64_t t0 = r * b;
            const StreamsRound rd = streams_round_plan(tile0.data(), n, t0, (uint32_t)b, rp.data());
            rounds++;
            const uint32_t nb = (uint32_t)(nt <= t0 ? 0 : nt - t0 < b ? nt - t0 : b);
            if (rd.nreal != nb) bad++;
            if (nb == 0) { if (rd.nparts || rd.nslots || rd.ntok) bad++; continue; }
            std::vector<BrutePart> bp;
            for (uint64_t t = t0; t < t0 + nb; t++) {
                const uint64_t k = brute_item_of(h_tile0, n, t);
                if (!bp.empty() && bp.back().item == k) bp.back().b = t + 1; else bp.push_back(BrutePart{k, t, t + 1});
            }
            uint64_t t = 0, bl = 0;
            for (const BrutePart &pt : bp) { t += brute_tok_cap(pt.b - pt.a); bl += brute_blk_cap(pt.b - pt.a); }
            if (bp.size() != rd.nparts || t != rd.ntok || bl != rd.nslots) bad++;
            if (rd.nslots > (uint64_t)kSenqBlkPerTile * nb || rd.ntok > (uint64_t)kSenqTokPerTile * nb || rd.nparts > nb) bad++;
            uint32_t j = 0; uint64_t toff = 0, boff = 0;
            for (const BrutePart &pt : bp) {
                if (j >= rd.nparts) { bad++; break; }
                const uint64_t k = pt.item;
                const bool ends = pt.b == h_tile0[k + 1];
                const StreamsRoundPart &p = rp[j];
                const uint32_t pnt = (uint32_t)(pt.b - pt.a);
                parts++;
                if (!ends) mid++;
                if (p.item != k || p.c0 != pt.a - t0 || p.nt != pnt || (p.ends != 0) != ends || p.boff != boff || p.toff != toff || p.j != j || p.nblk_cap != brute_blk_cap(pnt)) bad++;
                // what a one-stream launch gets from the host: L, the segment's end, the stream's own number of the part's first tile, the special position
                const uint64_t L = io[k + 1] - io[k];
                const StreamsPartArgs a = streams_part_args(p, L, tile0[k], t0);
                uint64_t sp = ~0ull;
                if (ends && L >= 65274u) { const uint64_t q = (L - 65274u) / 32768u * 32768u + 65274u; if (q + 261u >= L) sp = q; } // the position 32768 k + 65274 in [L - 261, L]
                if (a.L != L || a.seg_end != (ends ? L : ~0ull) || a.chunk0 != pt.a - h_tile0[k] || a.final_block != (ends ? 1u : 0u) || a.sp != sp) bad++;
                toff += brute_tok_cap(pnt); boff += brute_blk_cap(pnt); j++;
            }
            if (j != rd.nparts) bad++;
        }
    }
    printf("plan batch=%u tables=%llu tiles=%llu rounds=%llu parts=%llu open_parts=%llu pad_rows=%llu mismatches=%llu\n", batch, tables, tiles, rounds, parts, mid, pads, bad);
}

static void overlap(uint64_t seed, uint64_t count)
{
    rng_state = seed;
    ull tables = 0, capped = 0, failed = 0, bad = 0;
    for (uint64_t it = 0; it < count; it++) {
        const uint64_t n = 1 + rnd() % 16, in_bytes = 1 + rnd() % 600000, out_cap = 1 << 20;
        std::vector<uint64_t> io(n + 1), oo(n + 1), tile0(n + 1), piece0(n + 1);
        std::vector<uint32_t> state(n);
        for (uint64_t k = 0; k <= n; k++) { io[k] = rnd() % 8 == 0 ? in_bytes + rnd() % 10 : rnd() % (in_bytes + 1); oo[k] = 4 * k * 1000 + (rnd() % 10 == 0 ? 2 : 0); }
        if (rnd() % 4 == 0) oo[n] = out_cap + 4;
        const uint64_t m = senq_ntiles_max(n, in_bytes);
        const uint64_t nt = senq_tile_scan(io.data(), oo.data(), n, in_bytes, out_cap, state.data(), tile0.data(), piece0.data());
        tables++;
        if (nt > m || piece0[n] > m || tile0[n] != nt) bad++;
        uint64_t asked = 0;
        for (uint64_t k = 0; k < n; k++) {
            const uint32_t s0 = senq_item_state(io[k], io[k + 1], in_bytes, oo[k], oo[k + 1], out_cap);
            const uint64_t want = senq_item_tiles(s0, io[k], io[k + 1]);
            asked += want;
            const bool cut = want != 0 && asked > m;
            if (cut) capped++;
            if (state[k] != (cut ? kSenqBad : s0)) bad++;
            if (state[k] != kSenqServed) { failed++; if (tile0[k + 1] != tile0[k] || piece0[k + 1] != piece0[k]) bad++; }
            else if (tile0[k + 1] - tile0[k] != streams_ntiles(io[k + 1] - io[k])) bad++;
        }
    }
    printf("overlap tables=%llu capped_items=%llu failed_items=%llu mismatches=%llu\n", tables, capped, failed, bad);
}

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; i++) {
        std::istringstream in(argv[i]);
        std::string what;
        in >> what;
        std::vector<uint64_t> v;
        std::vector<uint64_t> w;
        std::string tok;
        bool second = false;
        while (in >> tok) { if (tok == "/") { second = true; continue; } (second ? w : v).push_back(strtoull(tok.c_str(), nullptr, 10)); }
        if (what == "ntiles") {
            printf("ntiles");
            for (uint64_t L : v) printf(" %llu=%llu,%llu", (ull)L, (ull)streams_ntiles(L), (ull)(L / kTileStride + 1));
            printf("\n");
        } else if (what == "ws" && v.size() == 3) {
            const SenqWsPlan p = senq_ws_plan(v[0], v[1], (uint32_t)v[2]);
            printf("ws ntiles_max=%llu batch=%u rounds=%llu total=%llu", (ull)p.ntiles_max, p.batch, (ull)p.rounds, (ull)p.total);
            for (int r = 0; r < kSwRegions && p.total; r++) printf(" %s=%llu,%llu", senq_region_name(r), (ull)p.r[r].off, (ull)p.r[r].bytes);
            const uint64_t b = p.batch; // every tile of a round a stream of its own
            printf(" need_parts=%llu need_tokoff=%llu need_blk_item=%llu need_T=%llu need_blk=%llu need_pos=%llu need_slots=%llu\n", (ull)(b * sizeof(StreamsRoundPart)), (ull)((2 * b) * 4),
                   (ull)(b * streams_blk_cap(1) * 4), (ull)(b * streams_tok_cap(1) * 4ull), (ull)(b * streams_blk_cap(1) * sizeof(ContBlk)), (ull)((b * streams_blk_cap(1) + b) * 8),
                   (ull)(b * streams_blk_cap(1) * (uint64_t)kSlotStride));
        } else if (what == "rooms" && v.size() >= 2) {
            std::vector<uint64_t> io(1, 0), oo(v.size() - 1);
            for (size_t k = 2; k < v.size(); k++) io.push_back(io.back() + v[k]);
            uint64_t total = 0;
            streams_layout(io.data(), io.size() - 1, (uint32_t)v[0], oo.data(), &total);
            printf("rooms bound=%llu total=%llu\n", (ull)senq_rooms_bound(io.size() - 1, v[1], (uint32_t)v[0]), (ull)total);
        } else if (what == "scan" && v.size() >= 3 && w.size() + 2 == v.size()) {
            const uint64_t n = w.size() - 1;
            std::vector<uint64_t> tile0(n + 1), piece0(n + 1);
            std::vector<uint32_t> state(n);
            senq_tile_scan(v.data() + 2, w.data(), n, v[0], v[1], state.data(), tile0.data(), piece0.data());
            printf("scan states=");
            for (uint64_t k = 0; k < n; k++) printf("%s%u", k ? "," : "", state[k]);
            printf(" tile0=");
            for (uint64_t k = 0; k <= n; k++) printf("%s%llu", k ? "," : "", (ull)tile0[k]);
            printf(" piece0=");
            for (uint64_t k = 0; k <= n; k++) printf("%s%llu", k ? "," : "", (ull)piece0[k]);
            printf("\n");
        } else if (what == "plan" && v.size() == 3) plan((uint32_t)v[0], v[1], v[2]);
        else if (what == "overlap" && v.size() == 2) overlap(v[0], v[1]);
        else { fprintf(stderr, "bad row: %s\n", argv[i]); return 2; }
    }
    return 0;
}
