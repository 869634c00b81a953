/* zamd_bgzf.c -- BGZF files, zlib style (include/zamd_bgzf.h): all blocks of a file through one call of the engine.
 *
 * Compress and uncompress are zgpu_bgzf_deflate_host / zgpu_bgzf_inflate_host with zlib's codes.  The index is a walk over the headers on the host
 * (the file is in host memory: one dependent read per block costs nothing here) with the rules of the device's finder (zgpu_bgzf.hip); a range is
 * the blocks that cover it as one zgpu_inflate_batch_host call into scratch, and the slice copied out.  Engines come from the library's pool. */
#include "../../include/zamd_bgzf.h"
#include "../../include/zamd_gpu.h"
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define EXPORT __attribute__((visibility("default")))
#define BGZF_BLOCK 65280u
#define BGZF_ISIZE_MAX 65536u

zgpu_engine *zamd_engine_checkout(void); /* zamd_zlib.c */
void zamd_engine_checkin(zgpu_engine *e);

static const unsigned char kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static int z_code(int rc)
{
    return rc == ZGPU_OK ? Z_OK : rc == ZGPU_BUF_ERROR ? Z_BUF_ERROR : rc == ZGPU_DATA_ERROR ? Z_DATA_ERROR : rc == ZGPU_STREAM_ERROR ? Z_STREAM_ERROR : Z_MEM_ERROR;
}

EXPORT uLong zamd_bgzf_bound(uLong sourceLen) { return (uLong)zgpu_bgzf_bound(sourceLen, 0); }

EXPORT int zamd_bgzf_compress(Bytef *dest, uLongf *destLen, const Bytef *source, uLong sourceLen, int level)
{
    if (!dest || !destLen || (!source && sourceLen)) return Z_STREAM_ERROR;
    if (level == Z_DEFAULT_COMPRESSION) level = 6;
    if (level < 1 || level > 9) return Z_STREAM_ERROR;
    zgpu_engine *e = zamd_engine_checkout();
    if (!e) return Z_MEM_ERROR;
    zgpu_deflate_result res;
    memset(&res, 0, sizeof res);
    const int rc = zgpu_bgzf_deflate_host(e, source, sourceLen, level, Z_DEFAULT_STRATEGY, 0, dest, *destLen, NULL, &res);
    zamd_engine_checkin(e);
    if (rc == ZGPU_OK) *destLen = (uLongf)res.out_bytes;
    return z_code(rc);
}

EXPORT int zamd_bgzf_uncompress(Bytef *dest, uLongf *destLen, const Bytef *source, uLong sourceLen)
{
    if (!destLen || (!dest && *destLen) || (!source && sourceLen)) return Z_STREAM_ERROR;
    zgpu_engine *e = zamd_engine_checkout();
    if (!e) return Z_MEM_ERROR;
    zgpu_inflate_result res;
    memset(&res, 0, sizeof res);
    const int rc = zgpu_bgzf_inflate_host(e, source, sourceLen, dest, *destLen, NULL, &res);
    zamd_engine_checkin(e);
    if (rc == ZGPU_OK || rc == ZGPU_BUF_ERROR) *destLen = (uLongf)res.out_bytes; /* (the size needed) */
    return z_code(rc);
}

EXPORT int zamd_bgzf_test(const Bytef *source, uLong sourceLen, uLongf *decodedLen)
{
    if (!source && sourceLen) return Z_STREAM_ERROR;
    if (sourceLen == 0) { if (decodedLen) *decodedLen = 0; return Z_OK; } /* (a file of no blocks: nothing to ask an engine) */
    zgpu_engine *e = zamd_engine_checkout();
    if (!e) return Z_MEM_ERROR;
    zgpu_inflate_result res;
    memset(&res, 0, sizeof res);
    const int rc = zgpu_bgzf_verify_host(e, source, sourceLen, NULL, &res);
    zamd_engine_checkin(e);
    if (rc == ZGPU_OK && decodedLen) *decodedLen = (uLongf)res.out_bytes;
    return z_code(rc);
}

/* the block at `pos`: its length and ISIZE; 0 when there is no valid block (the rules of bgzf_candidate in zgpu_bgzf.hip) */
static uint64_t block_at(const unsigned char *s, uint64_t n, uint64_t pos, uint32_t *isize)
{
    if (n - pos < 12) return 0;
    const unsigned char *p = s + pos;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
    const uint32_t xlen = p[10] | (uint32_t)p[11] << 8, xend = 12 + xlen;
    if (n - pos - 12 < xlen) return 0;
    uint32_t q = 12, bsize = 0;
    int found = 0;
    while (q + 4 <= xend) {
        const uint32_t slen = p[q + 2] | (uint32_t)p[q + 3] << 8;
        if (p[q] == 66 && p[q + 1] == 67 && slen == 2) {
            if (q + 6 <= xend) { bsize = p[q + 4] | (uint32_t)p[q + 5] << 8; found = 1; }
            break;
        }
        q += 4 + slen;
    }
    if (!found) return 0;
    const uint64_t len = (uint64_t)bsize + 1;
    if (len < (uint64_t)xend + 2 + 8 || len > n - pos) return 0; /* the header, a deflate body (never under 2 bytes), CRC-32 and ISIZE */
    const unsigned char *t = p + len - 4;
    *isize = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    return *isize <= BGZF_ISIZE_MAX ? len : 0;
}

EXPORT int zamd_bgzf_index(const Bytef *source, uLong sourceLen, zamd_bgzf_block *blocks, size_t cap, size_t *n, int *has_eof)
{
    if (!n || (!source && sourceLen)) return Z_STREAM_ERROR;
    for (int pass = 0; pass < 2; pass++) { /* count, then fill */
        uint64_t pos = 0, upos = 0, last = 0;
        size_t k = 0;
        while (pos < sourceLen) {
            uint32_t isize = 0;
            const uint64_t len = block_at(source, sourceLen, pos, &isize);
            if (!len) return Z_DATA_ERROR;
            if (pass) { blocks[k].coffset = pos; blocks[k].uoffset = upos; }
            k++; last = pos; pos += len; upos += isize;
        }
        if (!pass) {
            *n = k;
            if (has_eof) *has_eof = k && sourceLen - last == sizeof kEof && !memcmp(source + last, kEof, sizeof kEof);
            if (k + 1 > cap || !blocks) return Z_BUF_ERROR;
        } else { blocks[k].coffset = sourceLen; blocks[k].uoffset = upos; }
    }
    return Z_OK;
}

EXPORT int zamd_bgzf_uncompress_range(Bytef *dest, const Bytef *source, uLong sourceLen, const zamd_bgzf_block *blocks, size_t n, unsigned long long uoffset,
                                      uLong len)
{
    if (!blocks || (!source && sourceLen) || (!dest && len)) return Z_STREAM_ERROR;
    if (blocks[n].coffset != sourceLen) return Z_STREAM_ERROR;
    const uint64_t total = blocks[n].uoffset;
    if (uoffset > total || len > total - uoffset) return Z_BUF_ERROR;
    if (len == 0) return Z_OK;
    /* the first block that holds uoffset: the last one whose uoffset is not above it (empty blocks in front of it share that offset) */
    size_t lo = 0, hi = n;
    while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (blocks[mid + 1].uoffset <= uoffset) lo = mid + 1; else hi = mid; }
    const size_t b0 = lo;
    size_t b1 = b0; /* one behind the last block of the range */
    while (b1 < n && blocks[b1].uoffset < uoffset + len) b1++;
    const size_t nb = b1 - b0;
    const uint64_t cin = blocks[b0].coffset, ubase = blocks[b0].uoffset, ubytes = blocks[b1].uoffset - ubase;
    uint64_t *ioff = malloc((nb + 1) * sizeof *ioff), *ooff = malloc((nb + 1) * sizeof *ooff);
    zgpu_inflate_item *items = malloc(nb * sizeof *items);
    unsigned char *scratch = malloc(ubytes + 1);
    int ret = ioff && ooff && items && scratch ? Z_OK : Z_MEM_ERROR;
    if (ret == Z_OK) {
        for (size_t k = 0; k <= nb; k++) {
            if (blocks[b0 + k].coffset < cin || blocks[b0 + k].coffset > sourceLen || blocks[b0 + k].uoffset < ubase) { ret = Z_STREAM_ERROR; break; }
            ioff[k] = blocks[b0 + k].coffset - cin; ooff[k] = blocks[b0 + k].uoffset - ubase;
        }
    }
    if (ret == Z_OK) {
        zgpu_engine *e = zamd_engine_checkout();
        if (!e) ret = Z_MEM_ERROR;
        else {
            uint64_t nfailed = 0;
            const int rc = zgpu_inflate_batch_host(e, source + cin, ioff[nb], ioff, nb, ZGPU_WRAP_GZIP, 0, scratch, ubytes, ooff, items, &nfailed);
            zamd_engine_checkin(e);
            ret = rc != ZGPU_OK ? z_code(rc) : nfailed ? Z_DATA_ERROR : Z_OK;
            for (size_t k = 0; ret == Z_OK && k < nb; k++)
                if (items[k].out_bytes != ooff[k + 1] - ooff[k] || items[k].in_used != ioff[k + 1] - ioff[k])
                    ret = Z_DATA_ERROR; /* (a block shorter than the index says, or deflate data that ends in front of the trailer: as the whole-file decode) */
        }
    }
    if (ret == Z_OK) memcpy(dest, scratch + (uoffset - ubase), len);
    free(ioff); free(ooff); free(items); free(scratch);
    return ret;
}
