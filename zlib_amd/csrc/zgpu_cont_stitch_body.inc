// zgpu_cont_stitch_body.inc -- the body of cont_stitch_kernel (zgpu_cont.hip), included where it runs: in the one-stream kernel with the host's arguments and in
// cont_stitch_batch_kernel with the arguments of the part the block slot belongs to.  The includer defines b (the stream's block), blk, st, pos, slots, slot_stride,
// in, abs0, out and out_words; a `return` leaves the kernel.
{
    const uint32_t tid = threadIdx.x;
    if (b >= st->nblk) return;
    const ContBlk &k = blk[b];
    const uint64_t D = pos[b], E = pos[b + 1];
    if (E == D) return;
    const uint64_t wf = D >> 5, wl = (E - 1) >> 5;
    if (k.btype) { // a coded block: its bits, from bit 0 of the slot, shifted to D
        const uint32_t *S = reinterpret_cast<const uint32_t *>(slots + (size_t)b * slot_stride);
        const uint32_t nsw = (k.nbits + 31) >> 5;
        for (uint64_t w = wf + tid; w <= wl; w += 256) {
            if (w >= out_words) break;
            uint32_t v;
            if (32 * w < D) v = S[0] << (uint32_t)(D - 32 * w);
            else {
                const uint64_t o = 32 * w - D;
                const uint32_t sw = (uint32_t)(o >> 5), sh = (uint32_t)(o & 31), lo = S[sw], hi = sw + 1 < nsw ? S[sw + 1] : 0u;
                v = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
            }
            if (32 * w + 32 > E) v &= (1u << (uint32_t)(E - 32 * w)) - 1u;
            if (word_is_inner(w, D, E)) out[w] = v; else atomicOr(&out[w], v);
        }
    } else { // a stored block (trees.c:867-879, 1197-1219): three header bits at D, zeros up to the byte boundary, LEN, ~LEN, the bytes of the input
        const uint32_t ph = (uint32_t)(D & 7), hb = (ph + 3 + 7) >> 3, len = k.stored_len, hdr = k.eof << ph;
        const uint64_t db0 = D >> 3, nb = hb + 4 + (uint64_t)len;
        const uint8_t *src = in + (k.start_pos - abs0);
        for (uint64_t w = wf + tid; w <= wl; w += 256) {
            if (w >= out_words) break;
            uint32_t v = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint64_t a = 4 * w + j;
                if (a < db0 || a - db0 >= nb) continue;
                const uint64_t i = a - db0;
                uint32_t byte;
                if (i < hb) byte = (hdr >> (8 * (uint32_t)i)) & 255u;
                else if (i < hb + 4) { const uint32_t f = (uint32_t)(i - hb), l16 = f < 2 ? len : ~len; byte = (l16 >> (8 * (f & 1))) & 255u; }
                else byte = src[i - hb - 4];
                v |= byte << (8 * j);
            }
            if (word_is_inner(w, D, E)) out[w] = v; else atomicOr(&out[w], v);
        }
    }
}
