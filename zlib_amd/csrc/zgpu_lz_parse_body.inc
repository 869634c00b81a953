// zgpu_lz_parse_body.inc -- the body of the parallel parse (see zgpu_lz_parse.h for what it does), included where it runs:
//   parse2_kernel (zgpu_lz_parse.hip)   a kernel of its own, the arrays below static __shared__
//   walk_kernel   (zgpu_lz_walk.hip)    behind its walkers, the arrays carved out of the LDS the chunk bytes lived in
// The includer defines: the arrays J, HAS, MARK, COV, MAT, wbase, VIS, EXITS, wave_tot and the word sh_entry (LDS); g, c, cfg, recs,
// gmv_all, gsv_all, tokens, meta; the compile-time constants LITE, FUSED, TILE, ROWS (the tiles come row by row, TileRow), LOG, kP2Threads; the LDS word sh_exit and the TileGeom tg (used when TILE);
// the chunk's logs lpos, lrec (global), their counts lcnt and the array END (LDS) -- used when LOG (zgpu_lz_parse.h), which implies LITE and not TILE.
// TILE (continuous stream, zgpu_cont.hip): the chunk is a tile's 64 KiB; the path starts at the tile's entry (tg.entry, found by the chain over the tiles'
// exit functions), the tokens are the positions from the entry to the end of the last game that starts below h1 (at most 512 behind it), and the block
// cuts are not the tile's business (blocks are counted from the start of the stream).
{
    constexpr uint32_t kP2Own = kP2Win / kP2Threads;
    static_assert(kP2Own % kP2Batch == 0 && kP2Threads >= kP2Win / 32 && kP2Threads / 64 <= 16, "workgroup size");
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t lo; uint32_t n;
    chunk_span<ROWS>(g, c, lo, n);
    if constexpr (ROWS) { if (n == 0) return; } // a padding row (zgpu_deflate_streams_plan.h, streams_pad_row): a tile that parses nothing; no barrier, no LDS use above
    ParseCtx cx;
    cx.rec = LITE ? nullptr : recs + (size_t)c * kChunkMax;
    const uint32_t *gmv = LITE ? gmv_all + (size_t)c * kChunkMax : nullptr, *gsv = LITE ? gsv_all + (size_t)c * kP2Words : nullptr;
    cx.n = n; cx.base = chunk_base(g, c); cx.good = cfg.good; cx.lazy = cfg.lazy; cx.strategy = cfg.strategy;
    {
        // deflate.c:1278-1310 as a function of the position: the first check of "lookahead < MIN_LOOKAHEAD" happens at the first
        // visited p > buffered0 - 262, later ones at p > n - 262; the slide needs p + base >= WSIZE + MAX_DIST on top
        const int room = (int)(2 * kWSize - cx.base), b0 = (int)n < room ? (int)n : room;
        const int a = b0 - (int)kMinLookahead + 1, b = (int)(kWSize + kMaxDist) - (int)cx.base;
        cx.slide_at = a > b ? a : b;
    }
    uint32_t *tok = tokens + (size_t)c * kChunkMax;
    const uint8_t *src = g.in + lo;
    const uint32_t nwords = (n + 31) >> 5;
    uint32_t t_h1 = n, t_e = 0; // TILE: the end of the tile's range, the entry (local positions)
    if (TILE) {
        uint64_t wb_; uint32_t nl_, h0_, ne_;
        tile_span<ROWS>(g, tg, c, wb_, nl_, h0_, t_h1, ne_);
        t_e = h0_ + tg.entry[g.chunk0 + c];
    }

    static_assert(!LOG || (LITE && !TILE), "the logs are what a chunk's walkers leave");
    P2_T0();
    // ---- 1. has(p) ----
    for (uint32_t i = tid; i < kP2Words; i += kP2Threads) { MARK[i] = 0; COV[i] = 0; MAT[i] = 0; if (LOG) HAS[i] = 0; else if (LITE) HAS[i] = p2_ld<FUSED>(gsv + i); }
    // (the logs' positions are read two to a dword, and nothing is done to a loaded value before every load of its batch is out: a 16-bit load is
    // widened, and so waited for, where it stands)
    const uint32_t *lpos2 = reinterpret_cast<const uint32_t *>(lpos);
    // The logs' loads depend on nothing the tail computes -- the counts are final when the walkers are done -- so none of them stands on the tail's
    // critical path by itself: stage 1 issues the position loads of all windows before it waits (a load, a wait and the atomics per window were
    // eight round trips in a row), and the entries of window w + 1 (nq, nv) are asked for in window w and taken over at the top of w + 1.
    uint32_t nq[kP2Own], nv[kP2Own]; // LOG: the log entries of the next window (positions two to a dword, records)
    auto log_fetch = [&](uint32_t w0n, uint32_t tid) { // (w0n < n, uniform; tid: the window's, see the loop)
        const uint32_t cw = (uint32_t)__builtin_amdgcn_readfirstlane((int)lcnt[w0n / kP2Win]);
        const uint32_t *lp2 = lpos2 + w0n / 2, *lr = lrec + w0n; // (w0n / kP2Win * kP2Win == w0n)
#pragma unroll
        for (uint32_t i = 0; i < kP2Own; i++) {
            nq[i] = 0; nv[i] = 0;
            if (i * kP2Threads < cw) { const uint32_t e = i * kP2Threads + tid; nq[i] = p2_ld<FUSED>(lp2 + (e >> 1)); nv[i] = p2_ld<FUSED>(lr + e); } // (e < kP2Win: inside the log, whatever the count)
        }
    };
    if (LOG) { // a bit per logged game start: the logs' positions, read once and densely
        constexpr uint32_t kRounds = kP2Win / 2 / kP2Threads;
        __syncthreads();
        log_fetch(0, tid); // (behind the position loads of stage 1 in the queue; taken over at the top of window 0)
        uint32_t pv[kP2Wins][kRounds], cw[kP2Wins];
#pragma unroll
        for (uint32_t a = 0; a < kP2Wins; a++) {
            cw[a] = (uint32_t)__builtin_amdgcn_readfirstlane((int)lcnt[a]); // (uniform: the rounds are cut off by scalar branches)
#pragma unroll
            for (uint32_t r = 0; r < kRounds; r++) { pv[a][r] = 0; if (r * kP2Threads * 2 < cw[a]) pv[a][r] = p2_ld<FUSED>(lpos2 + a * (kP2Win / 2) + r * kP2Threads + tid); }
        }
#pragma unroll
        for (uint32_t a = 0; a < kP2Wins; a++) {
#pragma unroll
            for (uint32_t r = 0; r < kRounds; r++) {
                const uint32_t e = (r * kP2Threads + tid) * 2, p0 = pv[a][r] & 0xffffu, p1 = pv[a][r] >> 16;
                if (e < cw[a]) atomicOr(&HAS[p0 >> 5], 1u << (p0 & 31u));
                if (e + 1 < cw[a]) atomicOr(&HAS[p1 >> 5], 1u << (p1 & 31u));
            }
        }
    }
    if (!LITE) for (uint32_t p0 = 0; p0 < kChunkMax; p0 += kP2Threads * kP2Batch) {
        uint2 rv[kP2Batch];
#pragma unroll
        for (uint32_t u = 0; u < kP2Batch; u++) { const uint32_t p = p0 + u * kP2Threads + tid; rv[u] = p < n ? cx.rec[p] : make_uint2(0, 0); }
#pragma unroll
        for (uint32_t u = 0; u < kP2Batch; u++) {
            const uint32_t pw = p0 + u * kP2Threads, p = pw + tid;
            uint32_t d;
            const bool h = p < n && cx.take(p, kMinMatch - 1, rv[u], d) >= kMinMatch;
            const unsigned long long b = __builtin_amdgcn_ballot_w64(h);
            if (lane == 0) { HAS[(pw >> 5) + 2 * wave] = (uint32_t)b; HAS[(pw >> 5) + 2 * wave + 1] = (uint32_t)(b >> 32); }
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t x0 = (!TILE || t_e < t_h1) ? next_bit(HAS, t_e, nwords) : kNone;
        if (TILE && x0 != kNone && x0 >= t_h1) x0 = kNone;
        sh_entry = x0;
        if (TILE) sh_exit = t_e;
    }
    __syncthreads();
    P2_T(0);

    const uint32_t *TOK = COV; // a window's COV words turn into its token words in step C
    auto index_of = [&](uint32_t p) { return wbase[p >> 5] + (uint32_t)__builtin_popcount(TOK[p >> 5] & ~(~0u << (p & 31u))); };
    uint32_t tokbase = 0;                   // tokens in front of the window (uniform)
    uint32_t def_m = kNone, def_tok = 0;    // a match token whose position lies in the next window

    // ---- 2. window by window: path, matches, token indices, tokens ----
    const uint32_t w_first = TILE ? t_e / kP2Win * kP2Win : 0u, w_lim = TILE ? (t_h1 + kTileSlack < n ? t_h1 + kTileSlack : n) : n;
    const uint32_t tid_all = tid;
    for (uint32_t w0 = w_first; w0 < w_lim; w0 += kP2Win) {
        const uint32_t wend = w0 + kP2Win;
        // LOG: the lane's number is opaque inside a window.  Everything a window derives from it alone -- the offsets of its sixteen log entries and of its
        // sixteen bytes, the shuffles' lanes -- the compiler otherwise computes once in front of the loop and keeps: forty registers that the loads in
        // flight across the window's stages need (it spilled instead).  They are a few instructions a window to compute again.
        uint32_t tid = tid_all;
        if (LOG) asm volatile("" : "+v"(tid));
        const uint32_t entry = sh_entry;
        uint32_t gm[kP2Own]; // the game of this lane's has-positions: (m - p) << 24 | len << 15 | dist; 0: none
        uint32_t gp[kP2Own / 2]; // LOG: where the game gm[i] starts, two to a register (otherwise a lane's positions follow from i)
        uint32_t onp = 0;    // bit i: gm[i] is a game on the path (stage B)
#pragma unroll
        for (uint32_t i = 0; i < kP2Own; i++) { gm[i] = 0; gp[i >> 1] = 0; }
        auto pos_of = [&](uint32_t i) { return LOG ? (gp[i >> 1] >> ((i & 1u) << 4)) & 0xffffu : w0 + i * kP2Threads + tid; };
        // LOG: what this window takes from memory besides its log -- the bytes of its positions, for stage D's literals (lane = position, as D stores) --
        // and the next window's log are asked for as soon as this window's log has left nq / nv (stage A1), in front of every barrier of the window.
        // D then only selects and stores.
        uint32_t litw[kP2Own];
        auto win_fetch = [&]() {
#pragma unroll
            for (uint32_t i = 0; i < kP2Own; i++) { const uint32_t p = w0 + i * kP2Threads + tid; litw[i] = 0; if (p < n) litw[i] = src[p]; }
            if (wend < n) log_fetch(wend, tid);
        };
        const bool has_path = entry != kNone && entry < wend; // (uniform) the path has nodes in this window
        if (has_path) {
            // A1. successors of all has-positions of the window.  A lane's game reads the records of the positions right behind
            // its own: those are its neighbours' records (lanes = consecutive positions), fetched with lane shuffles; the first
            // kP2Over positions behind the wave's 64 are loaded by lanes 0..kP2Over-1 as well.  (A dependent global load per step of
            // the game -- some lane of the wave always needs one -- was 45% of this kernel.)
            if (LOG) {
                // the window's log entries are shared out, entry e to lane e % kP2Threads (log_fetch, a window ago: nq, nv; zero from the count on),
                // and nothing but the games is looked at -- J and END are written, and later read, at game starts only
                const uint32_t cw = (uint32_t)__builtin_amdgcn_readfirstlane((int)lcnt[w0 / kP2Win]);
#pragma unroll
                for (uint32_t i = 0; i < kP2Own; i++) {
                    const bool v = i * kP2Threads + tid < cw;
                    const uint32_t p = (nq[i] >> ((tid & 1u) << 4)) & 0xffffu; // (kP2Threads is even: entry e's half is lane's)
                    const uint32_t gvi = nv[i];
                    gm[i] = v ? gvi : 0u; gp[i >> 1] |= (v ? p : 0u) << ((i & 1u) << 4);
                    if (v) {
                        const uint32_t end = p + (gvi >> 24) + ((gvi >> 15) & 511u), t = next_bit(HAS, end, nwords);
                        J[p - w0] = (uint16_t)(t < wend ? t - w0 : 0xffffu);
                        END[p - w0] = (uint16_t)(end - w0);
                    }
                }
            } else if (LITE) {
                uint32_t gv[kP2Own];
#pragma unroll
                for (uint32_t i = 0; i < kP2Own; i++) {
                    const uint32_t p = w0 + i * kP2Threads + tid;
#if defined(ZGPU_P2_EXP) && ZGPU_P2_EXP == 1
                    gv[i] = 0x00018001u; // timing experiment: no loads (results are wrong)
#else
                    gv[i] = p < n ? p2_ld<FUSED>(gmv + p) : 0; // (all positions, whatever the words of the others hold: loads under a per-lane condition are waited for one by one)
#endif
                }
#pragma unroll
                for (uint32_t i = 0; i < kP2Own; i++) {
                    const uint32_t p = w0 + i * kP2Threads + tid;
                    if (!(p < n && ((HAS[p >> 5] >> (p & 31u)) & 1u))) gv[i] = 0;
                }
#pragma unroll
                for (uint32_t i = 0; i < kP2Own; i++) {
                    const uint32_t xw = i * kP2Threads + tid, p = w0 + xw;
                    uint32_t succ = 0xffffu;
                    gm[i] = gv[i];
                    if (gv[i]) {
                        const uint32_t t = next_bit(HAS, p + (gv[i] >> 24) + ((gv[i] >> 15) & 511u), nwords);
                        if (t < wend) succ = t - w0;
                    }
                    J[xw] = (uint16_t)succ;
                }
            } else {
#pragma unroll
            for (uint32_t ib = 0; ib < kP2Own; ib += kP2Pair) {
                uint2 ra[kP2Pair], rx[kP2Pair];
#pragma unroll
                for (uint32_t u = 0; u < kP2Pair; u++) {
                    const uint32_t p = w0 + (ib + u) * kP2Threads + tid, px = p + 64; // the overhang: positions 64.. behind the wave's first, one per low lane
                    ra[u] = p < n ? cx.rec[p] : make_uint2(0, 0);
                    rx[u] = (lane < kP2Over && px < n) ? cx.rec[px] : make_uint2(0, 0);
                }
#pragma unroll
                for (uint32_t u = 0; u < kP2Pair; u++) {
                    const uint32_t x = (ib + u) * kP2Threads + tid, p = w0 + x;
                    const bool hs = p < n && ((HAS[p >> 5] >> (p & 31u)) & 1u);
                    uint32_t L = kMinMatch - 1, D = 0, j = 1; // the match in hand starts at p + j - 1
                    if (hs) L = cx.take(p, kMinMatch - 1, ra[u], D);
                    bool live = hs;
                    // the games of a wave advance in step (j is the same in every lane that is still playing), so the records
                    // they need next are the wave's records rotated by one more lane each time: a DPP rotate per register, the
                    // overhang entering at lane 63 (a lane shuffle through the LDS crossbar per step was the cost of this loop)
                    uint32_t qx = ra[u].x, qy = ra[u].y, ox = rx[u].x, oy = rx[u].y;
                    while (__builtin_amdgcn_ballot_w64(live)) {
                        const uint32_t sl = lane + j;
                        const uint32_t tx = wave_rol1(qx), ty = wave_rol1(qy);
                        ox = wave_rol1(ox); oy = wave_rol1(oy);
                        qx = lane == 63 ? ox : tx; qy = lane == 63 ? oy : ty;
                        uint2 rn;
                        rn.x = qx; rn.y = qy;
                        const bool far = live && sl >= 64 + kP2Over;
                        if (__builtin_amdgcn_ballot_w64(far)) { if (far) rn = cx.rec[p + j]; } // a game that long is rare
                        uint32_t D2 = D;
                        const uint32_t L2 = cx.take(p + j, L, rn, D2); // (pure arithmetic: every lane evaluates it, the ones in a game use it)
                        live = live && L2 > L;
                        L = live ? L2 : L; D = live ? D2 : D; j += live ? 1u : 0u;
                    }
                    uint32_t succ = 0xffffu;
                    if (hs) {
                        const uint32_t m = p + j - 1;
                        gm[ib + u] = ((m - p) << 24) | (L << 15) | D;
                        const uint32_t t = next_bit(HAS, m + L, nwords);
                        if (t < wend) succ = t - w0;
                    }
                    J[x] = (uint16_t)succ;
                }
            }
            }
        }
        if (LOG) win_fetch(); // (ONE place for all of a window's loads, whether the path passes the window by or not: asked for in two branches, the registers
                              // they arrive in were merged by copies behind the branches, and a copy waits for its load)
        if (has_path) {
            __syncthreads();
            P2_T(1);
            // A2. The path through the window, without walking it end to end: parses started at different positions fall into
            // step with each other after a match or two, so every block of 256 positions is walked speculatively from its first
            // has-position (64 lanes, ~30 dependent hops each), and the true path is then threaded through the blocks: it is
            // walked from where it enters a block until it meets the block's speculative walk; from there on that walk IS the path.
            if (wave == 0) {
                const uint32_t bs = w0 + lane * kP2Blk, be = bs + kP2Blk;
                uint32_t v8[kP2Blk / 32];
#pragma unroll
                for (uint32_t j = 0; j < kP2Blk / 32; j++) v8[j] = 0;
                uint32_t x = next_bit(HAS, bs, nwords); // (an empty block's exit: the first node behind it)
                if (x != kNone && x >= wend) x = kNone;
                while (x != kNone && x < be) {
                    const uint32_t wi = (x - bs) >> 5, bit = 1u << (x & 31u);
#pragma unroll
                    for (uint32_t j = 0; j < kP2Blk / 32; j++) v8[j] |= wi == j ? bit : 0u;
                    const uint32_t a2 = J[x - w0];
                    x = a2 == 0xffffu ? kNone : w0 + a2;
                }
#pragma unroll
                for (uint32_t j = 0; j < kP2Blk / 32; j++) VIS[lane * (kP2Blk / 32) + j] = v8[j];
                EXITS[lane] = x; // where the block's walk leaves the block (kNone: leaves the window)
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // other lanes' VIS and EXITS (LDS, same wave: in order)
                __builtin_amdgcn_wave_barrier();
                // Threading, optimistic form: assume the path meets every block's speculative walk inside the block.  Then the blocks
                // it visits follow from the exits alone (a walk over at most 64 lanes' registers), every visited block finds its
                // meeting point on its own lane, and the assumption is checked block by block.
                uint32_t last = entry;
                bool ok;
                {
                    const uint32_t myexit = x;
                    uint32_t myentry = kNone;              // where the path enters this lane's block
                    uint32_t cb = (entry - w0) / kP2Blk, ce = entry, lastb = cb;
                    for (;;) {                             // wave-uniform, no memory
                        if (lane == cb) myentry = ce;
                        lastb = cb;
                        ce = (uint32_t)__builtin_amdgcn_readlane((int)myexit, (int)cb);
                        if (ce == kNone) break;
                        cb = (ce - w0) / kP2Blk;
                    }
                    // each visited block: from its entry to the meeting point
                    uint32_t m8[kP2Blk / 32];
#pragma unroll
                    for (uint32_t j = 0; j < kP2Blk / 32; j++) m8[j] = 0;
                    uint32_t x2 = myentry;
                    bool met = false;
                    while (x2 != kNone && x2 < be) {
                        const uint32_t wi = (x2 - bs) >> 5, bit = 1u << (x2 & 31u);
                        uint32_t vw = 0;
#pragma unroll
                        for (uint32_t j = 0; j < kP2Blk / 32; j++) vw = wi == j ? v8[j] : vw;
                        if (vw & bit) { // met: the rest of the speculative walk is the path
#pragma unroll
                            for (uint32_t j = 0; j < kP2Blk / 32; j++) m8[j] |= j > wi ? v8[j] : j == wi ? v8[j] & (~0u << (x2 & 31u)) : 0u;
                            met = true;
                            break;
                        }
#pragma unroll
                        for (uint32_t j = 0; j < kP2Blk / 32; j++) m8[j] |= wi == j ? bit : 0u;
                        const uint32_t a2 = J[x2 - w0];
                        x2 = a2 == 0xffffu ? kNone : w0 + a2;
                    }
                    // a block the path ran through without meeting the walk must at least leave it where the walk does
                    const bool bad = myentry != kNone && !met && x2 != myexit;
                    ok = __builtin_amdgcn_ballot_w64(bad) == 0;
                    if (ok) {
#pragma unroll
                        for (uint32_t j = 0; j < kP2Blk / 32; j++) if (m8[j]) atomicOr(&MARK[(w0 >> 5) + lane * (kP2Blk / 32) + j], m8[j]);
                        uint32_t hi = 0; // 1 + the last path node of this block (window-relative)
#pragma unroll
                        for (uint32_t j = 0; j < kP2Blk / 32; j++) if (m8[j]) hi = ((lane * (kP2Blk / 32) + j) << 5) + 32u - (uint32_t)__builtin_clz(m8[j]);
                        last = w0 + (uint32_t)__builtin_amdgcn_readlane((int)hi, (int)lastb) - 1;
                    }
                }
                if (!ok) { // (rare) thread the path block by block, walking until it meets the block's speculative walk
                    uint32_t cur = entry, met_blk = kNone; // wave-uniform
                    last = entry;
                    while (cur != kNone) {
                        const uint32_t blk = (cur - w0) / kP2Blk, be2 = w0 + (blk + 1) * kP2Blk;
                        uint32_t x2 = cur;
                        met_blk = kNone;
                        while (x2 != kNone && x2 < be2 && !((VIS[(x2 - w0) >> 5] >> (x2 & 31u)) & 1u)) {
                            last = x2;
                            if (lane == 0) atomicOr(&MARK[x2 >> 5], 1u << (x2 & 31u));
                            const uint32_t a2 = J[x2 - w0];
                            x2 = a2 == 0xffffu ? kNone : w0 + a2;
                        }
                        if (x2 != kNone && x2 < be2) { // met at x2
                            const uint32_t cw = (x2 - w0) >> 5;
                            if (lane < kP2Blk / 32) {
                                const uint32_t wd = blk * (kP2Blk / 32) + lane;
                                uint32_t v = VIS[wd];
                                if (wd < cw) v = 0; else if (wd == cw) v &= ~0u << (x2 & 31u);
                                if (v) atomicOr(&MARK[(w0 >> 5) + wd], v);
                            }
                            met_blk = blk;
                            x2 = EXITS[blk];
                        }
                        cur = (uint32_t)__builtin_amdgcn_readfirstlane(x2);
                        last = (uint32_t)__builtin_amdgcn_readfirstlane(last);
                        met_blk = (uint32_t)__builtin_amdgcn_readfirstlane(met_blk);
                    }
                    if (met_blk != kNone) { // the path ended inside a speculative walk: its last node is that block's last visited one
                        uint32_t hi = 0;
                        for (uint32_t j = 0; j < kP2Blk / 32; j++) { const uint32_t v = VIS[met_blk * (kP2Blk / 32) + j]; if (v) hi = ((met_blk * (kP2Blk / 32) + j) << 5) + 32u - (uint32_t)__builtin_clz(v); }
                        last = w0 + hi - 1;
                    }
                }
                if (lane == 0) { // the last path node of the window leads to the entry of the next one
                    uint32_t m, L, D;
                    if (LOG) { m = w0 + END[last - w0]; L = 0; } // (the end of the game, from stage A1: no trip to memory)
                    else if (LITE) { const uint32_t gv = p2_ld<FUSED>(gmv + last); m = last + (gv >> 24); L = (gv >> 15) & 511u; D = gv & 32767u; }
                    else cx.game(last, cx.rec[last], cx.rec[last + 1], m, L, D);
                    sh_entry = next_bit(HAS, m + L, nwords);
                    if (TILE) sh_exit = m + L;
                }
            }
            __syncthreads();
            P2_T(2);
            // B. matches of the path: MAT bit at the match start, COV bits on the bytes behind it (they may reach into the next window)
#pragma unroll
            for (uint32_t i = 0; i < kP2Own; i++) {
                const uint32_t p = pos_of(i);
                // (gm[] is not touched here: `if (on the path) {...} else gm[i] = 0` made hipcc of ROCm 7.2 keep two copies of the array and, in some register
                // allocations of this kernel, copy gm[6] and gm[7] back as ONE 64-bit pair (v_mov_b64 v[10:11], v[18:19]) behind the zeroing of gm[7]:
                // games that are not on the path then wrote match tokens in stage D -- round 2's "wrong tokens" whenever this file was touched,
                // DESIGN.md section 4.  Which games are on the path is a bit mask of its own instead.)
                const bool on_path = gm[i] != 0 && ((MARK[p >> 5] >> (p & 31u)) & 1u);
                onp |= on_path ? 1u << i : 0u;
                if (on_path) {
                    const uint32_t m = p + (gm[i] >> 24), L = (gm[i] >> 15) & 511u;
                    atomicOr(&MAT[m >> 5], 1u << (m & 31u));
                    const uint32_t a = m + 1, z = m + L; // [a, z)
                    for (uint32_t wd = a >> 5; wd <= (z - 1) >> 5; wd++) {
                        const uint32_t lo_b = wd == (a >> 5) ? (a & 31u) : 0u, hi_b = wd == ((z - 1) >> 5) ? ((z - 1) & 31u) : 31u;
                        atomicOr(&COV[wd], (~0u << lo_b) & (~0u >> (31u - hi_b)));
                    }
                }
            }
        }
        __syncthreads();
        P2_T(3);
        // C. token positions of the window = positions not inside a match; exclusive prefix counts per word (512 words: lanes 0..511)
        {
            const uint32_t wd = (w0 >> 5) + tid;
            uint32_t tw = 0;
            if (tid < kP2Win / 32 && wd < nwords) {
                tw = ~COV[wd];
                if (wd == nwords - 1 && (n & 31u)) tw &= ~0u >> (32u - (n & 31u));
                if (TILE) { // tokens: from the entry to the exit.  A window that reaches h1 is threaded after every game start of the tile: sh_exit is final there.
                    const uint32_t xl = wend > t_h1 ? (sh_exit > t_h1 ? sh_exit : t_h1) : wend, p0 = wd << 5;
                    tw &= p0 + 32 <= t_e ? 0u : p0 >= t_e ? ~0u : ~0u << (t_e & 31u);
                    tw &= p0 >= xl ? 0u : p0 + 32 <= xl ? ~0u : ~0u >> (32u - (xl & 31u));
                }
            }
            const uint32_t cnt = (uint32_t)__builtin_popcount(tw);
            uint32_t x = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if ((int)lane >= d) x += y; }
            if (lane == 63) wave_tot[wave] = x;
            __syncthreads();
            uint32_t b = tokbase + x - cnt, tot = 0;
            for (uint32_t w = 0; w < kP2Win / 32 / 64; w++) { const uint32_t t = wave_tot[w]; tot += t; if (w < wave) b += t; }
            if (tid < kP2Win / 32) { wbase[wd] = b; COV[wd] = tw; } // (wd < kP2Words always; words past nwords hold no tokens)
            tokbase += tot;
            __syncthreads();
        }
        P2_T(4);
        // D. tokens of the window
        // LOG: a batch's token indices first, then its stores in one run, each a 32-bit offset from `tok`, and the loaded bytes and the indices are
        // pinned in front of the run (an empty asm that uses them: the compiler otherwise moves whatever a store alone needs under that store's
        // condition).  A byte that is first used under a lane's own condition is waited for under that condition, and again under the next one, since
        // the wave may have skipped the first -- s_waitcnt vmcnt(0) in front of every store, which waits for the store before it as well: sixteen
        // literal stores a lane and window, each acknowledged before the next was issued.
        auto tok_put = [&](uint32_t idx, uint32_t v) { *reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(tok) + (idx << 2)) = v; }; // (idx < kChunkMax)
        if (def_m != kNone) { tok[index_of(def_m)] = def_tok; def_m = kNone; }
#pragma unroll
        for (uint32_t ib = 0; ib < kP2Own; ib += kP2Batch) {
            uint32_t lit[kP2Batch], ix[kP2Batch];
            bool li[kP2Batch];
#pragma unroll
            for (uint32_t u = 0; u < kP2Batch; u++) {
                const uint32_t p = w0 + (ib + u) * kP2Threads + tid, bit = 1u << (p & 31u);
                li[u] = p < n && (TOK[p >> 5] & bit) && !(MAT[p >> 5] & bit);
                lit[u] = 0;
                // (every position's byte is asked for, literal or not: eight loads in flight instead of eight waits one after the other.  Round 2 kept
                // conditional loads in the all-position form because "the toolchain produced wrong tokens the other way": that was stage B's miscompiled
                // `else gm[i] = 0`, see there)
                if (LOG) lit[u] = litw[ib + u];
                else if (p < n) lit[u] = src[p];
                ix[u] = LOG ? index_of(p) : 0u; // (p < kChunkMax: a word of the arrays, token or not)
            }
            if (LOG) {
#pragma unroll
                for (uint32_t u = 0; u < kP2Batch; u++) asm volatile("" : "+v"(lit[u]), "+v"(ix[u]));
            }
#pragma unroll
            for (uint32_t u = 0; u < kP2Batch; u++) {
                const uint32_t p = w0 + (ib + u) * kP2Threads + tid;
                if (LOG) { if (li[u]) tok_put(ix[u], tok_lit(lit[u])); }
                else if (li[u]) tok[index_of(p)] = tok_lit(lit[u]);
                const uint32_t gv = (!LOG && ((onp >> (ib + u)) & 1u)) ? gm[ib + u] : 0u;
                if (gv) {
                    const uint32_t m = p + (gv >> 24), t = tok_match(gv & 32767u, ((gv >> 15) & 511u) - kMinMatch);
                    if (m < wend) tok[index_of(m)] = t; else { def_m = m; def_tok = t; } // (at most one per lane: m - p < 1024)
                }
            }
        }
        if (LOG) { // the match tokens, by game.  A lane's games lie anywhere in the window, but a game on the path whose match starts at or behind wend
                   // is the path's last in this window (the next node lies behind the match): one per window, so one deferred token per lane is enough
#pragma unroll
                for (uint32_t ib = 0; ib < kP2Own; ib += kP2Batch) {
                    uint32_t mx[kP2Batch], mt[kP2Batch];
#pragma unroll
                    for (uint32_t u = 0; u < kP2Batch; u++) {
                        const uint32_t gv = ((onp >> (ib + u)) & 1u) ? gm[ib + u] : 0u, m = pos_of(ib + u) + (gv >> 24);
                        mt[u] = gv ? tok_match(gv & 32767u, ((gv >> 15) & 511u) - kMinMatch) : 0u;
                        mx[u] = kNone;
                        if (gv) { if (m < wend) mx[u] = index_of(m); else { def_m = m; def_tok = mt[u]; } }
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kP2Batch; u++) asm volatile("" : "+v"(mx[u]), "+v"(mt[u]));
#pragma unroll
                    for (uint32_t u = 0; u < kP2Batch; u++) if (mx[u] != kNone) tok_put(mx[u], mt[u]);
                }
        }
        P2_T(5);
    }
    const uint32_t ntok = tokbase, nw_done = ((n + kP2Win - 1) / kP2Win) * (kP2Win / 32); // words that have a wbase entry
    __syncthreads();

    // ---- 3. block cuts (deflate.c:1620-1626, 1651-1656: after the 16383rd token of a block) and the stored-block veto ----
    if (TILE) { if (tid == 0) { meta[c].ntok = ntok; meta[c].in_bytes = (sh_exit > t_h1 ? sh_exit : t_h1) - t_e; } } // (in_bytes: the bytes the tile's tokens cover)
    else if (tid == 0) parse_block_cuts(cx.slide_at, cx.base, TOK, MAT, wbase, n, nwords, nw_done, ntok, meta[c]);
    P2_T(6);
    P2_TEND();
}
