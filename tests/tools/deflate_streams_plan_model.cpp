// deflate_streams_plan_model.cpp -- what the batch compress of many streams decides from plain numbers (zlib_amd/csrc/zgpu_deflate_streams_plan.h) on the CPU.
// Usage: deflate_streams_plan_model ROW...; every ROW is one argument and gives one line on stdout:
//   "rows L"                    a stream of L bytes: its tile count by streams_ntiles and by plan_cont (a fresh stream's one FINISH feed), the tiles whose row
//                               (streams_tile_row at buffer offset 1000) differs from what tile_span gives that feed's tile -- window start, window length, h0,
//                               h1, entries -- or whose base / nil_local differ from the walkers' own arithmetic, and the first and the last row
//   "layout FLAGS L0 L1 ..."    the rooms of items of these lengths: out_offsets, the total, the bound of each item
//   "batches BATCH L0 L1 ..."   the tiles of these items in batches of BATCH, by the round plan (streams_round_plan): per batch the parts item:a-b in tiles of
//                               the list (a '.' behind a part whose stream ends there) and the block layer's needs parts/tokens/block slots
// Built for the host only (tests/test_deflate_streams_plan_cpu.py); no HIP call is made.
#include "../../zlib_amd/csrc/zgpu_deflate_streams_plan.h"
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

using namespace zgpu;

static void print_row(const char *name, const TileRow &r)
{
    printf(" %s=%llu,%u,%u,%u,%u,%u,%lld", name, (unsigned long long)r.lo, r.n, r.h0, r.h1, r.nent, r.base, r.nil_local == ~0u ? -1ll : (long long)r.nil_local);
}

static void rows(uint64_t L)
{
    const uint64_t off = 1000;
    const uint64_t nt = streams_ntiles(L);
    const LevelCfg cfg = level_cfg_tuned(6, 0, false, nullptr);
    const ContPlan pl = plan_cont(cfg, 0, 0, L, ZGPU_CONT_FINISH, PlanEngine{}, ContKnobs{});
    ChunkGeom g{}; TileGeom tg{};
    g.in_bytes = L; g.tile_w0 = pl.w0; g.tile_stride = kTileStride; g.chunk0 = 0;
    tg.abs0 = 0; tg.e0 = pl.e0; tg.end = pl.end; tg.abs0_nil = 1;
    // deflate_cont's nil_pos of a stream that ends at L
    uint64_t sp = ~0ull;
    if (L >= 65274u) { const uint64_t s = (L - 65274u) / 32768u * 32768u + 65274u; if (s + 261u >= L) sp = s; }
    tg.nil_pos = (sp != ~0ull && sp < L) ? sp : ~0ull;
    uint64_t bad = 0;
    for (uint64_t t = 0; t < nt && t < pl.ntiles; t++) {
        uint64_t wb; uint32_t nloc, h0, h1, nent;
        tile_span<false>(g, tg, (uint32_t)t, wb, nloc, h0, h1, nent);
        const uint32_t base = (tg.abs0_nil && tg.abs0 + wb == 0) ? 0u : 1u;                                                   // walk_kernel<2>'s
        const uint32_t nil_local = (tg.nil_pos >= wb && tg.nil_pos - wb < kChunkMax) ? (uint32_t)(tg.nil_pos - wb) : ~0u;
        const TileRow r = streams_tile_row(off, L, t);
        if (r.lo != off + wb || r.n != nloc || r.h0 != h0 || r.h1 != h1 || r.nent != nent || r.base != base || r.nil_local != nil_local) bad++;
    }
    printf("L=%llu ntiles=%llu plan_ntiles=%llu mismatches=%llu", (unsigned long long)L, (unsigned long long)nt, (unsigned long long)pl.ntiles, (unsigned long long)bad);
    if (nt) { print_row("first", streams_tile_row(off, L, 0)); print_row("last", streams_tile_row(off, L, nt - 1)); }
    printf("\n");
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        std::istringstream in(argv[a]);
        std::string kind;
        in >> kind;
        std::vector<uint64_t> v;
        for (std::string w; in >> w;) v.push_back(strtoull(w.c_str(), nullptr, 0));
        if (kind == "rows" && v.size() == 1) rows(v[0]);
        else if (kind == "layout" && v.size() >= 1) {
            const uint32_t flags = (uint32_t)v[0];
            const uint64_t n = v.size() - 1;
            std::vector<uint64_t> off(n + 1, 0), oo(n + 1, 0);
            for (uint64_t k = 0; k < n; k++) off[k + 1] = off[k] + v[k + 1];
            uint64_t total = 0;
            const bool ok = streams_layout(off.data(), n, flags, oo.data(), &total);
            printf("ok=%d total=%llu oo=", ok ? 1 : 0, (unsigned long long)total);
            for (uint64_t k = 0; k <= n; k++) printf("%s%llu", k ? "," : "", (unsigned long long)oo[k]);
            printf(" bound=");
            for (uint64_t k = 0; k < n; k++) printf("%s%llu", k ? "," : "", (unsigned long long)streams_bound(v[k + 1], flags));
            printf(" cap=");
            for (uint64_t k = 0; k < n; k++) printf("%s%llu", k ? "," : "", (unsigned long long)streams_room_cap(oo[k + 1] - oo[k], flags));
            printf("\n");
        } else if (kind == "batches" && v.size() >= 1) {
            const uint32_t batch = (uint32_t)v[0];
            const uint64_t n = v.size() - 1;
            std::vector<uint64_t> off(n + 1, 0), tile0(n + 1, 0);
            for (uint64_t k = 0; k < n; k++) off[k + 1] = off[k] + v[k + 1];
            const bool ok = streams_tile_scan(off.data(), n, tile0.data());
            printf("ok=%d ntiles=%llu", ok ? 1 : 0, (unsigned long long)tile0[n]);
            std::vector<StreamsRoundPart> parts((size_t)(tile0[n] < batch ? tile0[n] : batch) + 1); // (a part per tile at the most)
            for (uint64_t t0 = 0; ok && batch && t0 < tile0[n]; t0 += batch) {
                const StreamsRound rd = streams_round_plan(tile0.data(), n, t0, batch, parts.data());
                printf(" |");
                for (uint32_t j = 0; j < rd.nparts; j++)
                    printf(" %u:%llu-%llu%s", parts[j].item, (unsigned long long)(t0 + parts[j].c0), (unsigned long long)(t0 + parts[j].c0 + parts[j].nt), parts[j].ends ? "." : "");
                printf(" needs=%u/%u/%u", rd.nparts, rd.ntok, rd.nslots);
            }
            printf("\n");
        } else { fprintf(stderr, "bad row: %s\n", argv[a]); return 2; }
    }
    return 0;
}
