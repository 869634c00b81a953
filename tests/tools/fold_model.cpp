// fold_model.cpp -- the verifying decoder's fold (zlib_amd/csrc/zgpu_common.h, "the fold") on the CPU, through the very helpers the kernel calls:
// crc_nib_entry / crc_nib_span (the nibble tables), fold_slice, fold_crc_step, fold_xpow8n, fold_adler_lane, fold_adler_join and crc_join.  What is
// restated here is only what the device does with cross-lane shuffles: the sum of the lanes' Adler parts and the order of the six join steps, over
// arrays of 64 values.  Usage: fold_model FILE -> "adler32 crc32" (decimal) of the file folded in pieces of kFoldMax bytes and a ragged tail, each
// piece at a 16-byte boundary as a half of the ring is.  Built for the host only (tests/test_batch_verify_cpu.py); no HIP call is made.
#include "../../zlib_amd/csrc/zgpu_common.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace zgpu;

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + got);
    fclose(f);
    uint32_t tab[kCrcNibWords];
    for (uint32_t i = 0; i < kCrcNibWords; i++) tab[i] = crc_nib_entry(i);
    uint8_t *piece = static_cast<uint8_t *>(aligned_alloc(16, kFoldMax));
    uint32_t a = 1, b = 0, crc = 0;
    for (size_t at = 0; at < data.size(); at += kFoldMax) {
        const uint32_t n = (uint32_t)(data.size() - at < kFoldMax ? data.size() - at : kFoldMax);
        memcpy(piece, data.data() + at, n);
        uint64_t s1 = 0, s2 = 0;
        uint32_t v[kFoldLanes], w[kFoldLanes], lg = 0;
        for (uint32_t t = 0; t < kFoldLanes; t++) {
            uint64_t l1, l2;
            fold_adler_lane(piece, n, t, l1, l2);
            s1 += l1; s2 += l2;
            uint32_t lo, hi;
            fold_slice(n, t, lg, lo, hi);
            v[t] = crc_nib_span(tab, piece + lo, hi - lo);
        }
        fold_adler_join(a, b, s1, s2, n);
        for (uint32_t st = 0; st < 6; st++) {
            const uint32_t s = 1u << st;
            for (uint32_t t = 0; t < kFoldLanes; t++) w[t] = fold_crc_step(v[t], v[t + s < kFoldLanes ? t + s : t], t, s, lg, st);
            memcpy(v, w, sizeof v);
        }
        crc = crc_join(crc, v[0], fold_xpow8n(n));
    }
    free(piece);
    printf("%u %u\n", a | (b << 16), crc);
    return 0;
}
