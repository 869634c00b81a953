// deflate_plan_model.cpp -- the compress calls' decisions (zlib_amd/csrc/zgpu_deflate_plan.h) on the CPU: plan_deflate with its batch steps, plan_cont and
// plan_fast_phases, called exactly as zgpu_deflate.hip and zgpu_deflate_cont.hip call them, with the engine's state, the environment knobs and the free device
// memory given as numbers.  Usage: deflate_plan_model ROW...; every ROW is one argument, "KIND key=value key=value ...", KIND = deflate | cont | phases, and
// gives one line "key=value ..." on stdout.  Keys that are left out have the value of a fresh engine, no knob set, memory not known.  Built for the host only
// (tests/test_deflate_plan_cpu.py); no HIP call is made.
#include "../../zlib_amd/csrc/zgpu_deflate_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

using namespace zgpu;

struct Row {
    std::string kind;
    std::map<std::string, std::string> kv;
    bool has(const char *k) const { return kv.count(k) != 0; }
    uint64_t u(const char *k, uint64_t dflt = 0) const { auto it = kv.find(k); return it == kv.end() ? dflt : strtoull(it->second.c_str(), nullptr, 0); }
    int i(const char *k, int dflt = 0) const { auto it = kv.find(k); return it == kv.end() ? dflt : atoi(it->second.c_str()); }
};

static Row parse(const char *arg)
{
    Row r;
    std::istringstream in(arg);
    in >> r.kind;
    for (std::string w; in >> w;) {
        const size_t eq = w.find('=');
        if (eq == std::string::npos) { fprintf(stderr, "not key=value: %s\n", w.c_str()); exit(2); }
        r.kv[w.substr(0, eq)] = w.substr(eq + 1);
    }
    return r;
}

static PlanEngine engine_of(const Row &r)
{
    PlanEngine pe;
    pe.geo_w = r.i("geo_w", 15); pe.geo_m = r.i("geo_m", 8);
    pe.tuned = r.has("tune_good");
    pe.tune[0] = (uint32_t)r.u("tune_good"); pe.tune[1] = (uint32_t)r.u("tune_lazy"); pe.tune[2] = (uint32_t)r.u("tune_nice"); pe.tune[3] = (uint32_t)r.u("tune_chain");
    pe.exact_sort = r.i("exact_sort") != 0;
    pe.lz_parallel = r.i("lz_parallel", 1) != 0;
    const int level = r.i("level", 6);
    // (what lz_fastwin_serves says: of the level's own parameters, or of deflateTune's)
    pe.fastwin_serves = r.i("fastwin", level >= 1 && level <= 9 && fastwin_row_serves(level_cfg_tuned(level, r.i("strategy"), pe.tuned, pe.tune))) != 0;
    pe.sorted_ws_chunk = r.u("sws", 1245184);
    pe.batch_cap = (uint32_t)r.u("batch_cap"); pe.par_cap = (uint32_t)r.u("par_cap"); pe.ct_tiles = (uint32_t)r.u("ct_tiles");
    pe.free_bytes = r.u("free");
    return pe;
}

static const char *impl_name(int impl)
{
    static const char *names[] = {"AUTO", "SERIAL", "PARALLEL", "SORTED", "WALK", "FAST", "FASTWIN"};
    return impl >= 0 && impl <= 6 ? names[impl] : "?";
}

static void deflate_row(const Row &r)
{
    PlanCall c;
    c.args = r.i("args", 1) != 0;
    c.level = r.i("level", 6); c.strategy = r.i("strategy"); c.lz_impl = r.i("lz_impl", ZGPU_LZ_AUTO);
    c.chunk_size = (uint32_t)r.u("chunk_size"); c.flags = (uint32_t)r.u("flags"); c.prime = (uint32_t)r.u("prime");
    c.in_bytes = r.has("in_bytes") ? r.u("in_bytes") : r.u("nchunks", 1) * kChunkMax;
    c.seg = r.i("seg") != 0; c.nseg = r.u("nseg"); c.skip0 = (uint32_t)r.u("skip0"); c.host_in = r.i("host") != 0;
    DeflateKnobs kn;
    kn.lz_default = r.i("lz_default");
    if (r.has("hand_on")) kn.hand_on = r.kv.at("hand_on")[0];
    kn.batch_chunks = (uint32_t)r.u("batch_chunks"); kn.host_batch = (uint32_t)r.u("host_batch"); kn.first_batch = (uint32_t)r.u("first_batch");
    const DeflatePlan pl = plan_deflate(c, engine_of(r), kn);
    if (pl.rc) { printf("rc=%d msg=%s\n", pl.rc, pl.msg); return; }
    printf("rc=0 impl=%s serial=%d hand_on=%d geo=%d check_sort=%d with_crc=%d seg_wrap=%d head=%u tail=%u nchunks=%llu batch=%u hand_piece=%u first=%u", impl_name(pl.impl), pl.serial,
           pl.hand_on, pl.geo, pl.check_sort, pl.with_crc, pl.seg_wrap, pl.head_bytes, pl.tail_bytes, (unsigned long long)pl.nchunks, pl.batch, pl.hand_piece, pl.first);
    printf(" good=%u lazy=%u nice=%u chain=%u slow=%u w_bits=%u hash_bits=%u block_tokens=%u nbatches=%zu", pl.cfg.good, pl.cfg.lazy, pl.cfg.nice, pl.cfg.chain, pl.cfg.slow, pl.cfg.w_bits,
           pl.cfg.hash_bits, pl.block_tokens, plan_nbatches(pl));
    if (r.i("steps")) { // the chunks of every batch, as deflate_device's loop takes them
        printf(" steps=");
        for (BatchSteps s(pl); s.more(); s.next()) printf("%s%u", s.k ? "," : "", s.nb());
    }
    printf("\n");
}

static void cont_row(const Row &r)
{
    ContKnobs kn;
    kn.batch_tiles = (uint32_t)r.u("batch_tiles"); kn.batch_tiles_set = r.has("batch_tiles");
    kn.pipe = r.i("pipe");
    const uint32_t zero[4] = {0, 0, 0, 0};
    const LevelCfg cfg = level_cfg_tuned(r.i("level", 6), r.i("strategy"), false, zero);
    const ContPlan pl = plan_cont(cfg, r.u("entry"), r.u("abs0"), r.u("buf"), r.i("mode", ZGPU_CONT_FINISH), engine_of(r), kn);
    printf("fast_lz=%d e0=%llu w0=%llu end=%llu ntiles=%llu pipe=%d batch=%u nbatches=%llu\n", pl.fast_lz, (unsigned long long)pl.e0, (unsigned long long)pl.w0, (unsigned long long)pl.end,
           (unsigned long long)pl.ntiles, pl.pipe, pl.batch, (unsigned long long)((pl.ntiles + pl.batch - 1) / pl.batch));
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        const Row r = parse(argv[a]);
        if (r.kind == "deflate") deflate_row(r);
        else if (r.kind == "cont") cont_row(r);
        else if (r.kind == "phases") printf("K=%u\n", plan_fast_phases((uint32_t)r.u("nb"), (uint32_t)r.u("fast_run")));
        else { fprintf(stderr, "unknown row kind: %s\n", r.kind.c_str()); return 2; }
    }
    return 0;
}
