// zgpu_lz_sorted.hip -- LZ77 stage for levels 4-9, second parallel form: hash buckets as sorted arrays.
//
// Same mathematics as zgpu_lz_parallel.hip (static chains, all-position search with two budgets, record-driven lazy
// parse -- SURVEY.md 8a A4/A5), different data structure.  Instead of walking `link(p)` pointers through an LDS ring, the
// positions of a chunk are counting-sorted by their 3-byte hash:
//
//     S[start(h) .. start(h)+count(h))  = the positions with hash h, ascending
//     idx(p)   = index of p in S,   rank(p) = number of earlier positions with the same hash
//
// so the hash chain of p, nearest candidate first, is simply S[idx-1], S[idx-2], ... S[idx-rank]: no dependent pointer
// hop per candidate (the next candidates are known in advance and are fetched four at a time with one 8-byte load), no
// link ring in LDS (the match kernel needs only the 64 KiB chunk there, so two 1024-lane workgroups fit a CU instead
// of one), no tiles and no per-tile barriers (any position can be searched at any time).
//
// This file is the launch side: the workspace's size and the order of the kernels on the stream.  The kernels, one file each behind zgpu_lz_sorted.h:
//   K1c  sort4_kernel   zgpu_lz_sort.hip: the sort: ranks by ordered LDS atomics under a wave token, kept in registers, scatter staged through LDS,
//                       self-check; output S (u16 positions), ir (idx | rank << 16 by position), one bit per S index marking
//                       bucket heads, heads_below per 64 indices
//   K1'  sort_kernel    zgpu_lz_sort.hip: the same result with ballots only (6x slower): fallback when sort4's self-check fails, ZGPU_SORT=1
//   K2'' match3_kernel  zgpu_lz_match3.hip: one 1024-lane workgroup per chunk, a wave per 64 consecutive S entries, all lanes on their k-th
//                       candidate in the same step, full compares deferred to a per-wave stack and folded with atomic max
//   K3                  parse2_kernel (zgpu_lz_parse.hip), or parse_kernel of zgpu_lz_parallel.hip with ZGPU_PARSE=1
//   K2w  walk_kernel    zgpu_lz_walk.hip: the default at levels 4-9: parse-driven search with the rest of the parse behind it (replaces K2'' + K3)
//        fast_kernel    zgpu_lz_fast.hip: levels 1-3 (ZGPU_LZ_FAST): deflate_fast on the sorted buckets, one lane per chunk
#include "zgpu_lz_sorted.h"

namespace zgpu {

size_t lz_sorted_workspace_bytes(uint32_t batch) { return SortedWs::bytes(batch); }
uint32_t *lz_sorted_fault_word(void *workspace) { return SortedWs(workspace, 0).fault; }

// A batch of chunks: the sort, then the search and parse `impl` names -- ZGPU_LZ_WALK: walk_kernel<1>; ZGPU_LZ_SORTED: the all-position search
// (match3_kernel + parse2_kernel); levels 1-3: ZGPU_LZ_FAST, fast_kernel, or ZGPU_LZ_FASTWIN, a wave per chunk (zgpu_lz_fastwin.hip).
// Returns what launch_sort returns.
bool launch_lz_sorted(const ChunkGeom &g, LevelCfg cfg, void *workspace, uint32_t *tokens, ChunkMeta *meta, hipStream_t st, zgpu_engine *prof, int exact_sort, int impl)
{
    const SortedWs ws(workspace, g.nchunks);
    const bool adler_done = launch_sort(g, ws, meta, st, prof, exact_sort);
    hipEvent_t ev{};
    prof_span_begin(prof, st, &ev);
    if (impl == ZGPU_LZ_FASTWIN) launch_lz_fastwin(g, cfg, ws.S, ws.ir, tokens, meta, st);
    else if (impl == ZGPU_LZ_FAST) launch_fast(g, cfg, ws, tokens, meta, st);
    else if (impl == ZGPU_LZ_WALK) launch_walk_chunks(g, cfg, ws, tokens, meta, st);
    else { // ZGPU_LZ_SORTED
        launch_match3(g, cfg, ws, st);
        prof_span_end(prof, st, ZGPU_STAGE_MATCH, ev);
        prof_span_begin(prof, st, &ev);
        launch_parse(g, cfg, ws.recs, tokens, meta, st);
        prof_span_end(prof, st, ZGPU_STAGE_PARSE, ev);
        return adler_done;
    }
    prof_span_end(prof, st, ZGPU_STAGE_MATCH, ev);
    return adler_done;
}

// A batch of tiles of a continuous stream (zgpu_cont.hip): sort, walkers + exit functions, the chain of entries, the tiles' tokens.

// the sort alone (levels 1-3 go on with fastwin_tile_kernel's rounds, zgpu_deflate_cont.hip lz_tiles_fast): where S and ir of the batch's tiles are
void launch_sort_tiles(const ChunkGeom &g, void *workspace, ChunkMeta *meta, hipStream_t st, zgpu_engine *prof, int exact_sort, const uint16_t **S_out, const uint32_t **ir_out)
{
    const SortedWs ws(workspace, g.nchunks);
    launch_sort(g, ws, meta, st, prof, exact_sort);
    *S_out = ws.S; *ir_out = ws.ir;
}
void launch_lz_tiles(const ChunkGeom &g, const TileGeom &tg, LevelCfg cfg, void *workspace, ChunkMeta *meta, uint16_t *comp, uint16_t *gentry, hipStream_t st, zgpu_engine *prof,
                     int exact_sort)
{
    const SortedWs ws(workspace, g.nchunks);
    launch_sort(g, ws, meta, st, prof, exact_sort);
    hipEvent_t ev{};
    prof_span_begin(prof, st, &ev);
    launch_walk_tiles(g, tg, cfg, ws, meta, st);
    prof_span_end(prof, st, ZGPU_STAGE_MATCH, ev);
    prof_span_begin(prof, st, &ev);
    launch_chain(tg.exits, g.nchunks, comp, gentry, tg.entry + g.chunk0, st);
    prof_span_end(prof, st, ZGPU_STAGE_PARSE, ev);
}
// ... and the tiles' tokens from their true entries: a launch of its own, so that it can run on another stream under the next batch's walkers (it is all
// latency -- a window at a time, one wave threading the path -- and they are bound by the vector units: what the chunk path gets by fusing the two)
void launch_lz_tiles_parse(const ChunkGeom &g, const TileGeom &tg, LevelCfg cfg, void *workspace, uint32_t *tokens, ChunkMeta *meta, hipStream_t st, zgpu_engine *prof)
{
    const SortedWs ws(workspace, g.nchunks);
    hipEvent_t ev{};
    prof_span_begin(prof, st, &ev);
    launch_parse_tile(g, cfg, ws.gm(), ws.gs(), tokens, meta, tg, st);
    prof_span_end(prof, st, ZGPU_STAGE_PARSE, ev);
}

} // namespace zgpu
