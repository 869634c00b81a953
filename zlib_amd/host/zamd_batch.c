/* zamd_batch.c -- zamd_compress2_batch / zamd_uncompress_batch (include/zamd_batch.h): many small independent streams in one engine call,
 * each with the verdict compress2() / uncompress() (qcsrc/compress.c:22-58, qcsrc/uncompr.c:26-61) give it alone.
 *
 * Compress: the items of at most 64 KiB at levels 1-9 go to zgpu_deflate_segments_host with ZGPU_F_FINAL and the wrapper (every segment one
 * complete stream, byte for byte what compress2() of it emits); larger items at levels 4-9 go to zgpu_deflate_streams_host, many continuous
 * streams whose tiles share the launches, in calls of at most STREAMS_IN_MAX bytes of input; level 0, larger items at levels 1-3 and items of
 * 4 GiB or more take the one-item path.  Uncompress: every item of
 * less than 512 MiB of input goes to zgpu_inflate_batch_host, the per-item codes are mapped the way uncompress() maps inflate()'s.
 * The batch calls use an engine of their own (created on first use, on the device ZAMD_DEVICE names, like the stream API's). */
#include "../../include/zamd_batch.h"
#include "../../include/zamd_gpu.h"
#include "zamd_host.h"
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define EXPORT __attribute__((visibility("default")))
#define SEG_MAX 65536u
#define STREAMS_IN_MAX (1ull << 30) /* input bytes of one zgpu_deflate_streams_host call (an item larger than that is a call of its own) */
#define BATCH_IN_MAX (1ull << 29) /* the decoder's limit of compressed bytes per item */

static pthread_mutex_t g_batch_lock = PTHREAD_MUTEX_INITIALIZER; /* one call at a time on the engine (one stream, one workspace) */
static zgpu_engine *g_batch_engine;

zgpu_engine *zamd_batch_engine_lock(void)
{
    pthread_mutex_lock(&g_batch_lock);
    if (!g_batch_engine) {
        const char *dev = getenv("ZAMD_DEVICE");
        if (zgpu_engine_create(dev ? atoi(dev) : 0, &g_batch_engine) != ZGPU_OK) g_batch_engine = NULL;
    }
    if (!g_batch_engine) pthread_mutex_unlock(&g_batch_lock);
    return g_batch_engine;
}
void zamd_batch_engine_unlock(void) { pthread_mutex_unlock(&g_batch_lock); }

static int first_failure(const int *status, size_t n)
{
    for (size_t k = 0; k < n; k++)
        if (status[k] != Z_OK) return status[k];
    return Z_OK;
}

/* one item the way compress2() (windowBits 15) or deflateInit2() + deflate(Z_FINISH) serve it */
static int compress_one(Bytef *dest, uLongf *destLen, const Bytef *src, uLong len, int level, int wbits)
{
    if (wbits == 15) return compress2(dest, destLen, src, len, level);
    if (len > 0xFFFFFFFFul) return Z_STREAM_ERROR;
    z_stream st;
    memset(&st, 0, sizeof st);
    int err = deflateInit2_(&st, level, Z_DEFLATED, wbits, 8, Z_DEFAULT_STRATEGY, ZLIB_VERSION, (int)sizeof st);
    if (err != Z_OK) return err;
    st.next_in = (Bytef *)src; st.avail_in = (uInt)len;
    st.next_out = dest; st.avail_out = *destLen > 0xFFFFFFFFul ? 0xFFFFFFFFu : (uInt)*destLen;
    err = deflate(&st, Z_FINISH);
    if (err != Z_STREAM_END) { deflateEnd(&st); return err == Z_OK ? Z_BUF_ERROR : err; }
    *destLen = st.total_out;
    return deflateEnd(&st);
}

/* one item the way uncompress() serves it (windowBits 15), or inflateInit2() + inflate(Z_FINISH) with uncompress()'s mapping of the codes */
static int uncompress_one(Bytef *dest, uLongf *destLen, const Bytef *src, uLong len, int wbits)
{
    if (wbits == 15) return uncompress(dest, destLen, src, len);
    if (len > 0xFFFFFFFFul || *destLen > 0xFFFFFFFFul) return Z_BUF_ERROR; /* uncompr.c:36-38 */
    z_stream st;
    memset(&st, 0, sizeof st);
    st.next_in = (Bytef *)src; st.avail_in = (uInt)len;
    st.next_out = dest; st.avail_out = (uInt)*destLen;
    int err = inflateInit2_(&st, wbits, ZLIB_VERSION, (int)sizeof st);
    if (err != Z_OK) return err;
    err = inflate(&st, Z_FINISH);
    if (err != Z_STREAM_END) {
        const int full = st.avail_out == 0; /* (this inflate() takes all input: what ran out is the room, or the stream) */
        inflateEnd(&st);
        if (err == Z_NEED_DICT || (err == Z_BUF_ERROR && !full)) return Z_DATA_ERROR;
        return err == Z_OK ? Z_BUF_ERROR : err;
    }
    *destLen = st.total_out;
    return inflateEnd(&st);
}

static uint64_t g_streams_calls, g_one_by_one; /* (diagnostic) */
EXPORT unsigned long long zamd_compress2_batch_count(int which) { return which == 0 ? g_streams_calls : which == 1 ? g_one_by_one : 0; }

static int engine_code(int rc);
/* is item k of a compress batch one of the large items that go through zgpu_deflate_streams_host? */
static int streams_item(uLong len, int level) { return level >= 4 && len > SEG_MAX && len <= 0xFFFFFFFFul; }

/* the large items idx[0 .. m) as one zgpu_deflate_streams_host call; status and destLen of each as compress2() leaves them */
static void compress_streams_call(Bytef *const *dest, uLongf *destLen, const Bytef *const *source, const uLong *sourceLen, const size_t *idx, size_t m, int level,
                                  int windowBits, int *status)
{
    const uint32_t flags = ZGPU_F_FINAL | (windowBits == 15 ? ZGPU_F_ZLIB_WRAP : windowBits == 31 ? ZGPU_F_GZIP_WRAP : 0u);
    uint64_t *ioff = malloc((m + 1) * sizeof *ioff), *ooff = malloc((m + 1) * sizeof *ooff);
    zgpu_deflate_batch_item *items = malloc(m * sizeof *items);
    uint8_t *in = NULL, *out = NULL;
    uint64_t at = 0, cap = 0;
    int rc = ioff && ooff && items ? ZGPU_OK : ZGPU_MEM_ERROR;
    if (rc == ZGPU_OK) {
        for (size_t i = 0; i < m; i++) { ioff[i] = at; at += sourceLen[idx[i]]; }
        ioff[m] = at;
        rc = zgpu_deflate_streams_layout(ioff, m, flags, ooff, &cap);
    }
    if (rc == ZGPU_OK) {
        in = malloc(at + 1); out = malloc(cap + 1);
        if (!in || !out) rc = ZGPU_MEM_ERROR;
    }
    if (rc == ZGPU_OK) {
        for (size_t i = 0; i < m; i++) memcpy(in + ioff[i], source[idx[i]], sourceLen[idx[i]]);
        zgpu_deflate_params p;
        memset(&p, 0, sizeof p);
        p.level = level; p.flags = flags; p.lz_impl = ZGPU_LZ_AUTO;
        zgpu_deflate_result res;
        memset(&res, 0, sizeof res);
        zgpu_engine *e = zamd_batch_engine_lock();
        if (!e) rc = ZGPU_ERRNO;
        else {
            rc = zgpu_deflate_streams_host(e, in, ioff, m, &p, out, cap, ooff, items, &res);
            g_streams_calls++;
            zamd_batch_engine_unlock();
        }
    }
    for (size_t i = 0; i < m; i++) {
        const size_t k = idx[i];
        if (rc != ZGPU_OK) { status[k] = rc == ZGPU_MEM_ERROR ? Z_MEM_ERROR : engine_code(rc); continue; }
        if (items[i].code != ZGPU_OK) { status[k] = items[i].code == ZGPU_BUF_ERROR ? Z_BUF_ERROR : Z_ERRNO; continue; }
        if (items[i].out_bytes > destLen[k]) { status[k] = Z_BUF_ERROR; continue; }
        memcpy(dest[k], out + ooff[i], items[i].out_bytes);
        destLen[k] = items[i].out_bytes;
        status[k] = Z_OK;
    }
    free(ioff); free(ooff); free(items); free(in); free(out);
}

static int engine_code(int rc) { return rc == ZGPU_MEM_ERROR ? Z_MEM_ERROR : rc == ZGPU_STREAM_ERROR ? Z_STREAM_ERROR : Z_ERRNO; }

EXPORT int zamd_compress2_batch(Bytef *const *dest, uLongf *destLen, const Bytef *const *source, const uLong *sourceLen, size_t n, int level,
                                int windowBits, int *status)
{
    if (n && (!dest || !destLen || !source || !sourceLen || !status)) return Z_STREAM_ERROR;
    if (level == Z_DEFAULT_COMPRESSION) level = 6;
    if (level < 0 || level > 9 || (windowBits != 15 && windowBits != 31 && windowBits != -15)) return Z_STREAM_ERROR;
    for (size_t k = 0; k < n; k++)
        if ((!source[k] && sourceLen[k]) || !dest[k]) return Z_STREAM_ERROR;
    uint64_t nb = 0, in_total = 0;
    for (size_t k = 0; k < n; k++)
        if (level > 0 && sourceLen[k] <= SEG_MAX) { nb++; in_total += sourceLen[k]; }
    if (nb) {
        const uint32_t flags = ZGPU_F_FINAL | (windowBits == 15 ? ZGPU_F_ZLIB_WRAP : windowBits == 31 ? ZGPU_F_GZIP_WRAP : 0u);
        const uint64_t cap = zgpu_deflate_segments_bound(nb, in_total, flags);
        uint8_t *in = malloc(in_total + 1), *out = malloc(cap);
        uint64_t *seg = malloc((nb + 1) * sizeof *seg), *ooff = malloc((nb + 1) * sizeof *ooff);
        size_t *idx = malloc(nb * sizeof *idx);
        int rc = in && out && seg && ooff && idx ? ZGPU_OK : ZGPU_MEM_ERROR;
        if (rc == ZGPU_OK) {
            uint64_t j = 0, at = 0;
            for (size_t k = 0; k < n; k++)
                if (level > 0 && sourceLen[k] <= SEG_MAX) {
                    seg[j] = at; idx[j++] = k;
                    if (sourceLen[k]) memcpy(in + at, source[k], sourceLen[k]);
                    at += sourceLen[k];
                }
            seg[nb] = at;
            zgpu_deflate_params p;
            memset(&p, 0, sizeof p);
            p.level = level; p.flags = flags; p.lz_impl = ZGPU_LZ_AUTO;
            zgpu_deflate_result res;
            memset(&res, 0, sizeof res);
            zgpu_engine *e = zamd_batch_engine_lock();
            if (!e) rc = ZGPU_ERRNO;
            else {
                rc = zgpu_deflate_segments_host(e, in, seg, nb, &p, out, cap, ooff, &res);
                zamd_batch_engine_unlock();
            }
            for (uint64_t i = 0; i < nb; i++) {
                const size_t k = idx[i];
                if (rc != ZGPU_OK) { status[k] = engine_code(rc); continue; }
                const uint64_t len = ooff[i + 1] - ooff[i];
                if (len > destLen[k]) { status[k] = Z_BUF_ERROR; continue; }
                memcpy(dest[k], out + ooff[i], len);
                destLen[k] = len;
                status[k] = Z_OK;
            }
        } else {
            for (size_t k = 0; k < n; k++)
                if (level > 0 && sourceLen[k] <= SEG_MAX) status[k] = Z_MEM_ERROR;
        }
        free(in); free(out); free(seg); free(ooff); free(idx);
    }
    { /* the large items at levels 4-9: many streams a call, at most STREAMS_IN_MAX bytes of input each */
        size_t nl = 0;
        for (size_t k = 0; k < n; k++) nl += streams_item(sourceLen[k], level) ? 1 : 0;
        size_t *idx = nl ? malloc(nl * sizeof *idx) : NULL;
        if (nl && !idx) {
            for (size_t k = 0; k < n; k++)
                if (streams_item(sourceLen[k], level)) status[k] = Z_MEM_ERROR;
        } else if (nl) {
            size_t m = 0;
            uint64_t bytes = 0;
            for (size_t k = 0; k < n; k++) {
                if (!streams_item(sourceLen[k], level)) continue;
                if (m && bytes + sourceLen[k] > STREAMS_IN_MAX) { compress_streams_call(dest, destLen, source, sourceLen, idx, m, level, windowBits, status); m = 0; bytes = 0; }
                idx[m++] = k; bytes += sourceLen[k];
            }
            if (m) compress_streams_call(dest, destLen, source, sourceLen, idx, m, level, windowBits, status);
        }
        free(idx);
    }
    for (size_t k = 0; k < n; k++)
        if (!(level > 0 && sourceLen[k] <= SEG_MAX) && !streams_item(sourceLen[k], level)) {
            status[k] = compress_one(dest[k], &destLen[k], source[k], sourceLen[k], level, windowBits);
            g_one_by_one++;
        }
    return first_failure(status, n);
}

EXPORT int zamd_uncompress_batch(Bytef *const *dest, uLongf *destLen, const Bytef *const *source, const uLong *sourceLen, size_t n, int windowBits,
                                 int *status)
{
    if (n && (!dest || !destLen || !source || !sourceLen || !status)) return Z_STREAM_ERROR;
    const int wrap = windowBits == 15 ? ZGPU_WRAP_ZLIB : windowBits == 31 ? ZGPU_WRAP_GZIP : windowBits == 47 ? ZGPU_WRAP_AUTO : windowBits == -15 ? ZGPU_WRAP_RAW : -1;
    if (wrap < 0) return Z_STREAM_ERROR;
    for (size_t k = 0; k < n; k++)
        if ((!source[k] && sourceLen[k]) || (!dest[k] && destLen[k])) return Z_STREAM_ERROR;
    uint64_t nb = 0, in_total = 0, out_total = 0;
    for (size_t k = 0; k < n; k++)
        if (sourceLen[k] < BATCH_IN_MAX) { nb++; in_total += sourceLen[k]; out_total += destLen[k]; }
    if (nb) {
        uint8_t *in = malloc(in_total + 1), *out = malloc(out_total + 1);
        uint64_t *ioff = malloc((nb + 1) * sizeof *ioff), *ooff = malloc((nb + 1) * sizeof *ooff);
        zgpu_inflate_item *items = malloc(nb * sizeof *items);
        size_t *idx = malloc(nb * sizeof *idx);
        int rc = in && out && ioff && ooff && items && idx ? ZGPU_OK : ZGPU_MEM_ERROR;
        if (rc == ZGPU_OK) {
            uint64_t j = 0, ai = 0, ao = 0;
            for (size_t k = 0; k < n; k++)
                if (sourceLen[k] < BATCH_IN_MAX) {
                    ioff[j] = ai; ooff[j] = ao; idx[j++] = k;
                    if (sourceLen[k]) memcpy(in + ai, source[k], sourceLen[k]);
                    ai += sourceLen[k]; ao += destLen[k];
                }
            ioff[nb] = ai; ooff[nb] = ao;
            zgpu_engine *e = zamd_batch_engine_lock();
            if (!e) rc = ZGPU_ERRNO;
            else {
                rc = zgpu_inflate_batch_host(e, in, in_total, ioff, nb, wrap, 0, out, out_total, ooff, items, NULL);
                zamd_batch_engine_unlock();
            }
            for (uint64_t i = 0; i < nb; i++) {
                const size_t k = idx[i];
                if (rc != ZGPU_OK) { status[k] = engine_code(rc); continue; }
                const zgpu_inflate_item *it = &items[i];
                if (it->code == ZGPU_OK) {
                    if (it->out_bytes) memcpy(dest[k], out + ooff[i], it->out_bytes);
                    destLen[k] = it->out_bytes;
                    status[k] = Z_OK;
                } else status[k] = it->code == ZGPU_BUF_ERROR ? Z_BUF_ERROR : Z_DATA_ERROR; /* Z_NEED_DICT, truncation: uncompr.c:50-56 */
            }
        } else {
            for (size_t k = 0; k < n; k++)
                if (sourceLen[k] < BATCH_IN_MAX) status[k] = Z_MEM_ERROR;
        }
        free(in); free(out); free(ioff); free(ooff); free(items); free(idx);
    }
    for (size_t k = 0; k < n; k++)
        if (sourceLen[k] >= BATCH_IN_MAX) status[k] = uncompress_one(dest[k], &destLen[k], source[k], sourceLen[k], windowBits);
    return first_failure(status, n);
}

static int window_wrap(int windowBits)
{
    return windowBits == 15 ? ZGPU_WRAP_ZLIB : windowBits == 31 ? ZGPU_WRAP_GZIP : windowBits == 47 ? ZGPU_WRAP_AUTO : windowBits == -15 ? ZGPU_WRAP_RAW : -1;
}

/* the decoded size of one item through inflate(), the output discarded piece by piece (items too large for the engine's batch).  Every round of
 * the loop takes input in, delivers output or ends it: a round that does neither is the stream having stopped short. */
static int size_one(uLongf *size, const Bytef *src, uLong len, int wbits)
{
    enum { ROOM = 1 << 20 };
    z_stream st;
    memset(&st, 0, sizeof st);
    int err = inflateInit2_(&st, wbits, ZLIB_VERSION, (int)sizeof st);
    if (err != Z_OK) return err;
    Bytef *room = malloc(ROOM);
    if (!room) { inflateEnd(&st); return Z_MEM_ERROR; }
    st.next_in = (Bytef *)src;
    uLong left = len, total = 0;
    for (;;) {
        uInt fed = 0;
        if (st.avail_in == 0 && left) { fed = left > 0x40000000ul ? 0x40000000u : (uInt)left; st.avail_in = fed; left -= fed; }
        st.next_out = room; st.avail_out = ROOM;
        err = inflate(&st, left ? Z_NO_FLUSH : Z_FINISH);
        const uInt got = ROOM - st.avail_out;
        total += got;
        if (err == Z_OK || (err == Z_BUF_ERROR && (got || fed))) continue;
        break;
    }
    free(room);
    inflateEnd(&st);
    if (err != Z_STREAM_END) return err == Z_MEM_ERROR ? Z_MEM_ERROR : Z_DATA_ERROR; /* damaged, stopped short, or in need of a dictionary */
    *size = total;
    return Z_OK;
}

/* the items the engine's batch takes (less than 512 MiB of input), packed into one buffer: in, ioff[0..nb], idx[j] = the item's index in the call */
struct packed_in { uint8_t *in; uint64_t *ioff; size_t *idx; zgpu_inflate_item *items; uint64_t nb, in_total; };
static void packed_in_free(struct packed_in *p) { free(p->in); free(p->ioff); free(p->idx); free(p->items); }
static int packed_in_make(struct packed_in *p, const Bytef *const *source, const uLong *sourceLen, size_t n)
{
    memset(p, 0, sizeof *p);
    for (size_t k = 0; k < n; k++)
        if (sourceLen[k] < BATCH_IN_MAX) { p->nb++; p->in_total += sourceLen[k]; }
    if (!p->nb) return ZGPU_OK;
    p->in = malloc(p->in_total + 1); p->ioff = malloc((p->nb + 1) * sizeof *p->ioff); p->idx = malloc(p->nb * sizeof *p->idx); p->items = malloc(p->nb * sizeof *p->items);
    if (!p->in || !p->ioff || !p->idx || !p->items) return ZGPU_MEM_ERROR;
    uint64_t j = 0, at = 0;
    for (size_t k = 0; k < n; k++)
        if (sourceLen[k] < BATCH_IN_MAX) {
            p->ioff[j] = at; p->idx[j++] = k;
            if (sourceLen[k]) memcpy(p->in + at, source[k], sourceLen[k]);
            at += sourceLen[k];
        }
    p->ioff[p->nb] = at;
    return ZGPU_OK;
}

/* sizes of all items: the engine's sizing pass for those it takes, size_one for the others.  size[k] = 0 where status[k] is not Z_OK.
 * verify: the integrity test in the sizing pass's place -- the trailers are checked too (size_one checks them as it is); size may be NULL then */
static void sizes_all(struct packed_in *p, int rc, uLongf *size, const Bytef *const *source, const uLong *sourceLen, size_t n, int windowBits, int *status, int verify)
{
    if (p->nb && rc == ZGPU_OK) {
        zgpu_engine *e = zamd_batch_engine_lock();
        if (!e) rc = ZGPU_ERRNO;
        else {
            if (verify) rc = zgpu_inflate_batch_verify_host(e, p->in, p->in_total, p->ioff, p->nb, window_wrap(windowBits), 0, p->items, NULL);
            else rc = zgpu_inflate_batch_sizes_host(e, p->in, p->in_total, p->ioff, p->nb, window_wrap(windowBits), p->items, NULL);
            zamd_batch_engine_unlock();
        }
    }
    for (uint64_t i = 0; i < p->nb; i++) {
        const size_t k = p->idx[i];
        if (rc != ZGPU_OK) status[k] = rc == ZGPU_MEM_ERROR ? Z_MEM_ERROR : engine_code(rc);
        else status[k] = p->items[i].code == ZGPU_OK ? Z_OK : Z_DATA_ERROR;
        if (size) size[k] = status[k] == Z_OK ? (uLongf)p->items[i].out_bytes : 0;
    }
    for (size_t k = 0; k < n; k++)
        if (sourceLen[k] >= BATCH_IN_MAX) {
            uLongf got = 0;
            status[k] = size_one(&got, source[k], sourceLen[k], windowBits);
            if (size) size[k] = got;
        }
}

EXPORT int zamd_uncompress_sizes_batch(uLongf *destLen, const Bytef *const *source, const uLong *sourceLen, size_t n, int windowBits, int *status)
{
    if (n && (!destLen || !source || !sourceLen || !status)) return Z_STREAM_ERROR;
    if (window_wrap(windowBits) < 0) return Z_STREAM_ERROR;
    for (size_t k = 0; k < n; k++)
        if (!source[k] && sourceLen[k]) return Z_STREAM_ERROR;
    if (n == 0) return Z_OK;
    struct packed_in p;
    const int rc = packed_in_make(&p, source, sourceLen, n);
    sizes_all(&p, rc, destLen, source, sourceLen, n, windowBits, status, 0);
    packed_in_free(&p);
    return first_failure(status, n);
}

EXPORT int zamd_uncompress_verify_batch(uLongf *destLen, const Bytef *const *source, const uLong *sourceLen, size_t n, int windowBits, int *status)
{
    if (n && (!source || !sourceLen || !status)) return Z_STREAM_ERROR;
    if (window_wrap(windowBits) < 0) return Z_STREAM_ERROR;
    for (size_t k = 0; k < n; k++)
        if (!source[k] && sourceLen[k]) return Z_STREAM_ERROR;
    if (n == 0) return Z_OK;
    struct packed_in p;
    const int rc = packed_in_make(&p, source, sourceLen, n);
    sizes_all(&p, rc, destLen, source, sourceLen, n, windowBits, status, 1);
    packed_in_free(&p);
    return first_failure(status, n);
}

EXPORT int zamd_uncompress_batch_packed(Bytef *dest, uLongf *destCap, uLong *destOffsets, const Bytef *const *source, const uLong *sourceLen, size_t n,
                                        int windowBits, int *status)
{
    if (!destCap || (n && (!destOffsets || !source || !sourceLen || !status)) || (n && !dest && *destCap)) return Z_STREAM_ERROR;
    const int wrap = window_wrap(windowBits);
    if (wrap < 0) return Z_STREAM_ERROR;
    for (size_t k = 0; k < n; k++)
        if (!source[k] && sourceLen[k]) return Z_STREAM_ERROR;
    if (n == 0) { *destCap = 0; return Z_OK; }
    struct packed_in p;
    int rc = packed_in_make(&p, source, sourceLen, n);
    int ret;
    if (rc == ZGPU_OK && p.nb == n) {
        /* the usual case, every item in the engine's reach: sizing pass, layout and decode in one engine call, one upload (idx is the identity) */
        uint64_t *ooff = malloc((n + 1) * sizeof *ooff), total = 0;
        zgpu_engine *e = ooff ? zamd_batch_engine_lock() : NULL;
        if (!ooff) rc = ZGPU_MEM_ERROR;
        else if (!e) rc = ZGPU_ERRNO;
        else {
            rc = zgpu_inflate_batch_packed_host(e, p.in, p.in_total, p.ioff, n, wrap, 0, 1, dest, *destCap, ooff, p.items, &total, NULL);
            zamd_batch_engine_unlock();
        }
        if (rc == ZGPU_OK || rc == ZGPU_BUF_ERROR) {
            for (size_t k = 0; k < n; k++) { destOffsets[k] = (uLong)ooff[k]; status[k] = p.items[k].code == ZGPU_OK ? Z_OK : Z_DATA_ERROR; }
            destOffsets[n] = (uLong)ooff[n];
            *destCap = (uLongf)total;
            ret = rc == ZGPU_BUF_ERROR ? Z_BUF_ERROR : first_failure(status, n);
        } else {
            for (size_t k = 0; k < n; k++) status[k] = rc == ZGPU_MEM_ERROR ? Z_MEM_ERROR : engine_code(rc);
            ret = status[0];
        }
        free(ooff);
        packed_in_free(&p);
        return ret;
    }
    /* items the batch does not take among them: sizes first, then the layout, then the batch decode of the small ones into their places and the
     * large ones one by one */
    uLongf *size = malloc(n * sizeof *size);
    uint64_t *ooff = malloc((p.nb + 1) * sizeof *ooff);
    if (!size || !ooff) rc = ZGPU_MEM_ERROR;
    if (rc != ZGPU_OK) {
        for (size_t k = 0; k < n; k++) status[k] = Z_MEM_ERROR;
        free(size); free(ooff); packed_in_free(&p);
        return Z_MEM_ERROR;
    }
    sizes_all(&p, rc, size, source, sourceLen, n, windowBits, status, 0);
    uint64_t total = 0;
    for (size_t k = 0; k < n; k++) { destOffsets[k] = (uLong)total; total += size[k]; }
    destOffsets[n] = (uLong)total;
    const int too_small = total > *destCap;
    *destCap = (uLongf)total;
    if (!too_small) {
        for (uint64_t i = 0; i < p.nb; i++) ooff[i] = destOffsets[p.idx[i]];
        ooff[p.nb] = total;
        if (p.nb) {
            zgpu_engine *e = zamd_batch_engine_lock();
            if (!e) rc = ZGPU_ERRNO;
            else {
                rc = zgpu_inflate_batch_host(e, p.in, p.in_total, p.ioff, p.nb, wrap, 0, dest, total, ooff, p.items, NULL);
                zamd_batch_engine_unlock();
            }
            for (uint64_t i = 0; i < p.nb; i++) {
                const size_t k = p.idx[i];
                if (status[k] != Z_OK) continue; /* (its range is empty: the sizing pass's verdict stands) */
                status[k] = rc != ZGPU_OK ? engine_code(rc) : p.items[i].code == ZGPU_OK ? Z_OK : Z_DATA_ERROR;
            }
        }
        for (size_t k = 0; k < n; k++)
            if (sourceLen[k] >= BATCH_IN_MAX && status[k] == Z_OK) {
                uLongf len = size[k];
                status[k] = uncompress_one(dest + destOffsets[k], &len, source[k], sourceLen[k], windowBits);
            }
    }
    free(size); free(ooff); packed_in_free(&p);
    return too_small ? Z_BUF_ERROR : first_failure(status, n);
}

/* crc32() / adler32() of many buffers: the items' own checksums from one zgpu_checksum_batch_host, the caller's running values folded in here */
static int checksum_batch(uLong *val, const Bytef *const *buf, const uLong *len, size_t n, int want_crc)
{
    if (n && (!val || !buf || !len)) return Z_STREAM_ERROR;
    uint64_t total = 0;
    for (size_t k = 0; k < n; k++) {
        if ((!buf[k] && len[k]) || len[k] >= 0xFFFFFFFFul) return Z_STREAM_ERROR;
        total += len[k];
    }
    if (n == 0) return Z_OK;
    uint8_t *in = malloc(total + 1);
    uint64_t *off = malloc((n + 1) * sizeof *off);
    zgpu_check_item *items = malloc(n * sizeof *items);
    int rc = in && off && items ? ZGPU_OK : ZGPU_MEM_ERROR;
    if (rc == ZGPU_OK) {
        uint64_t at = 0;
        for (size_t k = 0; k < n; k++) {
            off[k] = at;
            if (len[k]) memcpy(in + at, buf[k], len[k]);
            at += len[k];
        }
        off[n] = at;
        zgpu_engine *e = zamd_batch_engine_lock();
        if (!e) rc = ZGPU_MEM_ERROR;
        else {
            rc = zgpu_checksum_batch_host(e, in, total, off, n, want_crc ? ZGPU_CHECK_CRC32 : ZGPU_CHECK_ADLER32, items);
            zamd_batch_engine_unlock();
        }
    }
    if (rc == ZGPU_OK)
        for (size_t k = 0; k < n; k++)
            val[k] = want_crc ? crc32_combine(val[k], items[k].crc32, (z_off_t)len[k]) : adler32_combine(val[k], items[k].adler32, (z_off_t)len[k]);
    free(in); free(off); free(items);
    return rc == ZGPU_OK ? Z_OK : rc == ZGPU_STREAM_ERROR ? Z_STREAM_ERROR : Z_MEM_ERROR;
}

EXPORT int zamd_crc32_batch(uLong *crc, const Bytef *const *buf, const uLong *len, size_t n) { return checksum_batch(crc, buf, len, n, 1); }
EXPORT int zamd_adler32_batch(uLong *adler, const Bytef *const *buf, const uLong *len, size_t n) { return checksum_batch(adler, buf, len, n, 0); }
