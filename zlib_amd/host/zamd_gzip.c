/* zamd_gzip.c -- zamd_gunzip (include/zamd_gzip.h): a multi-member gzip file through one call of the engine, zgpu_gzip_inflate_host, with zlib's
 * codes.  The engine is the batch calls' (zamd_batch.c); gzread() and inflate() keep their own member-by-member path. */
#include "../../include/zamd_gzip.h"
#include "../../include/zamd_gpu.h"
#include "zamd_host.h"
#include <string.h>

#define EXPORT __attribute__((visibility("default")))

EXPORT int zamd_gunzip(Bytef *dest, uLongf *destLen, const Bytef *source, uLong sourceLen, uLong *sourceUsed, uLong *members)
{
    if (sourceUsed) *sourceUsed = 0;
    if (members) *members = 0;
    if (sourceLen == 0) { /* a file of no members */
        if (destLen) *destLen = 0;
        return Z_OK;
    }
    if (!dest || !destLen || !source) return Z_STREAM_ERROR;
    zgpu_engine *e = zamd_batch_engine_lock();
    if (!e) return Z_MEM_ERROR;
    zgpu_inflate_result res;
    memset(&res, 0, sizeof res);
    uint64_t n = 0;
    const int rc = zgpu_gzip_inflate_host(e, source, sourceLen, dest, *destLen, NULL, NULL, NULL, 0, &n, &res);
    zamd_batch_engine_unlock();
    if (rc == ZGPU_OK || rc == ZGPU_BUF_ERROR || rc == ZGPU_DATA_ERROR) *destLen = (uLongf)res.out_bytes;
    if (rc == ZGPU_OK || rc == ZGPU_DATA_ERROR) {
        if (sourceUsed) *sourceUsed = (uLong)res.in_used;
        if (members) *members = (uLong)n;
    }
    return rc == ZGPU_OK ? Z_OK : rc == ZGPU_BUF_ERROR ? Z_BUF_ERROR : rc == ZGPU_DATA_ERROR ? Z_DATA_ERROR : rc == ZGPU_STREAM_ERROR ? Z_STREAM_ERROR : Z_MEM_ERROR;
}
