// zgpu_cont_compact_body.inc -- the body of cont_compact_kernel (zgpu_cont.hip), included where it runs: in the one-stream kernel with the host's arguments and in
// cont_compact_batch_kernel with the arguments of the part the tile belongs to.  The includer defines g, tg (ChunkGeom, TileGeom), c (the tile of the launch),
// tokens, tmeta, tokoff, T and blk.
{
    __shared__ unsigned long long sums[kMaxCuts];
    __shared__ uint32_t lastlen[kMaxCuts];
    const uint32_t tid = threadIdx.x, n = tmeta[c].ntok, off = tokoff[c];
    const uint32_t *tok = tokens + (size_t)c * kChunkMax;
    uint32_t ncut = 0, istar[kMaxCuts];
    for (uint32_t B = (off / kBlockTokens + 1) * kBlockTokens; B <= off + n && ncut < kMaxCuts; B += kBlockTokens) istar[ncut++] = B - 1 - off;
    if (tid < kMaxCuts) { sums[tid] = 0; lastlen[tid] = 0; }
    __syncthreads();
    unsigned long long s[kMaxCuts] = {0, 0, 0, 0, 0, 0};
    for (uint32_t j = tid; j < n; j += 256) {
        const uint32_t t = tok[j], len = (t >> 8) ? (t & 255u) + kMinMatch : 1u;
        T[off + j] = t;
        for (uint32_t q = 0; q < ncut; q++) { if (j <= istar[q]) s[q] += len; if (j == istar[q]) lastlen[q] = len; }
    }
    if (ncut == 0) return; // (uniform)
    for (uint32_t q = 0; q < ncut; q++) {
        unsigned long long v = s[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if ((tid & 63) == 0 && v) atomicAdd(&sums[q], v);
    }
    __syncthreads();
    if (tid < ncut) {
        uint64_t wb; uint32_t nloc, h0, h1, ne;
        tile_span(g, tg, c, wb, nloc, h0, h1, ne);
        const uint64_t e_abs = tg.abs0 + wb + h0 + tg.entry[g.chunk0 + c];
        ContBlk &b = blk[(off + istar[tid] + 1) / kBlockTokens - 1];
        b.end_pos = e_abs + sums[tid]; b.last_len = lastlen[tid];
    }
}
