// zgpu_engine.hip -- the engine itself behind the C ABI in include/zamd_gpu.h: its lifetime, error text, per-stage HIP-event timing, the staging buffers
// of the *_host entry points and the checksum pass.  The compress calls are zgpu_deflate.hip's and zgpu_deflate_cont.hip's, the decoder's zgpu_inflate*.hip's.
// No torch, no C++ types cross the boundary; no kernel lives here.
#include "zgpu_engine.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace zgpu {

int fail_hip(zgpu_engine *e, hipError_t err, const char *what, const char *file, int line)
{
    if (e) snprintf(e->err, sizeof e->err, "HIP error %d (%s) at %s:%d: %s", (int)err, hipGetErrorString(err), file, line, what);
    if (err == hipErrorOutOfMemory) return ZGPU_MEM_ERROR;
    return ZGPU_ERRNO;
}

int fail(zgpu_engine *e, int code, const char *msg)
{
    if (e) snprintf(e->err, sizeof e->err, "%s", msg);
    return code;
}

static hipEvent_t next_event(zgpu_engine *e)
{
    if (e->ev_used == e->ev_pool.size()) { hipEvent_t ev; hipEventCreate(&ev); e->ev_pool.push_back(ev); }
    return e->ev_pool[e->ev_used++];
}

// stage timing: HIP events recorded on the launch stream around the stage's launches (StageTimer in zgpu_engine.h, and the launchers of the kernel files)
void prof_span_begin(zgpu_engine *e, hipStream_t st, hipEvent_t *a)
{
    if (e && e->prof) { *a = next_event(e); hipEventRecord(*a, st); }
}
void prof_span_end(zgpu_engine *e, hipStream_t st, int stage, hipEvent_t a)
{
    if (e && e->prof) { hipEvent_t b = next_event(e); hipEventRecord(b, st); e->spans.push_back({stage, a, b}); }
}

void collect_spans(zgpu_engine *e)
{
    for (auto &s : e->spans) { float ms = 0; if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { e->ms[s.stage] += ms; e->launches[s.stage]++; } }
    e->spans.clear(); e->ev_used = 0;
}

uint32_t env_u32(const char *name, uint32_t dflt)
{
    const char *v = getenv(name);
    if (!v || !*v) return dflt;
    long x = strtol(v, nullptr, 10);
    return x > 0 ? (uint32_t)x : dflt;
}

int ensure_stage(zgpu_engine *e, uint64_t in_bytes, uint64_t out_bytes)
{
    int rc;
    if (in_bytes > e->stage_in.cap && (rc = e->stage_in.reserve(e, in_bytes + (in_bytes >> 3) + 4096))) return rc;
    if (out_bytes > e->stage_out.cap && (rc = e->stage_out.reserve(e, out_bytes + (out_bytes >> 3) + 4096))) return rc;
    return ZGPU_OK;
}

// Adler-32 / CRC-32 over 64 KiB pieces (the kernels of the compress side): zero the pieces' records, launch_adler / launch_crc, launch_scan joins them in the run state
int checksum_pass(zgpu_engine *e, const uint8_t *d_bytes, uint64_t nbytes, uint32_t mask, uint32_t batch_cap, DevBuf<ChunkMeta> &meta, hipStream_t st, uint32_t *adler, uint32_t *crc)
{
    const uint64_t npieces = nbytes ? (nbytes + kChunkMax - 1) / kChunkMax : 1;
    const uint32_t batch = (uint32_t)(npieces < batch_cap ? npieces : batch_cap);
    // (the engine's grow-only scratch: checksum-only users call this per buffer)
    if (meta.reserve(e, batch) || e->inf_offs.reserve(e, npieces + 1)) return ZGPU_MEM_ERROR;
    RunState rs{}; rs.adler_a = 1;
    ZGPU_HIP_CHECK(hipMemcpyAsync(e->run, &rs, sizeof rs, hipMemcpyHostToDevice, st));
    for (uint64_t c0 = 0; c0 < npieces; c0 += batch) {
        const uint32_t nb = (uint32_t)(npieces - c0 < batch ? npieces - c0 : batch);
        ZGPU_HIP_CHECK(hipMemsetAsync(meta, 0, (size_t)nb * sizeof(ChunkMeta), st));
        ChunkGeom g{}; g.in = d_bytes; g.in_bytes = nbytes; g.chunk_size = kChunkMax; g.chunk0 = c0; g.nchunks = nb; g.final_chunk = ~0ull;
        if (mask & 1u) launch_adler(g, meta, st); // (not computed: the pieces read a = 0, b = 0; the result is not reported)
        if (mask & 2u) launch_crc(g, meta, st);
        launch_scan(meta, nb, c0, e->inf_offs, e->run, ~0ull, st, (mask & 2u) != 0);
    }
    ZGPU_HIP_CHECK(hipMemcpyAsync(&rs, e->run, sizeof rs, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    *adler = (mask & 1u) ? rs.adler_a | (rs.adler_b << 16) : 1u;
    *crc = (mask & 2u) ? rs.crc : 0u;
    return ZGPU_OK;
}

hipEvent_t engine_copy_event(zgpu_engine *e, size_t i)
{
    while (e->copy_ev.size() <= i) { hipEvent_t ev; if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return nullptr; e->copy_ev.push_back(ev); }
    return e->copy_ev[i];
}

} // namespace zgpu

zgpu_engine::~zgpu_engine()
{
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    for (auto ev : ev_pool) hipEventDestroy(ev);
    for (auto ev : copy_ev) hipEventDestroy(ev);
    for (auto ev : done_ev) hipEventDestroy(ev);
    if (ct_stream) hipStreamDestroy(ct_stream);
    for (int i = 0; i < 2; i++) { if (ct_ev_a[i]) hipEventDestroy(ct_ev_a[i]); if (ct_ev_b[i]) hipEventDestroy(ct_ev_b[i]); }
    if (d2h_stream) hipStreamDestroy(d2h_stream);
    if (pin_tot) hipHostFree(pin_tot);
    if (copy_stream) hipStreamDestroy(copy_stream);
    if (stream) hipStreamDestroy(stream);
    // (the device buffers free themselves, behind this, with the engine's device still set)
}

using namespace zgpu;

extern "C" {
#pragma GCC visibility push(default)

int zgpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *zgpu_version(void) { return "zamd-gpu 0.1 (gfx950; zlib 1.2.3 bit-exact, 64 KiB independent chunks)"; }

int zgpu_engine_create(int device, zgpu_engine **out)
{
    if (!out) return ZGPU_STREAM_ERROR;
    *out = nullptr;
    int n = zgpu_device_count();
    if (device < 0 || device >= n) return ZGPU_ERRNO;
    zgpu_engine *e = new zgpu_engine();
    e->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        e->run.reserve(e, 1) != ZGPU_OK) {
        delete e;
        return ZGPU_ERRNO;
    }
    *out = e;
    return ZGPU_OK;
}

void zgpu_engine_destroy(zgpu_engine *e)
{
    if (e) delete e;
}

const char *zgpu_engine_error(const zgpu_engine *e) { return e ? e->err : "no engine"; }
uint64_t zgpu_debug_handed_on(const zgpu_engine *e) { return e ? e->handed_on : 0; } // chunks the lane-per-chunk loop gave to the wave-per-chunk kernel so far (tests, bench)
int zgpu_debug_sort_fallback(const zgpu_engine *e) { return e ? e->exact_sort : 0; } // non-zero: the fast sort's self-check failed once and the engine sorts with sort_kernel since (tests)

int zgpu_adler32_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, uint32_t *adler_out, void *hip_stream)
{
    if (!e || !adler_out || (!d_in && in_bytes)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    int rc = ensure_deflate_ws(e, 1, false, 1);
    if (rc) return rc;
    uint32_t crc;
    return checksum_pass(e, static_cast<const uint8_t *>(d_in), in_bytes, 1u, 65536, e->inf_meta, st, adler_out, &crc);
}

int zgpu_crc32_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, uint32_t *crc_out, void *hip_stream)
{
    if (!e || !crc_out || (!d_in && in_bytes)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    int rc = ensure_deflate_ws(e, 1, false, 1);
    if (rc) return rc;
    uint32_t adler;
    return checksum_pass(e, static_cast<const uint8_t *>(d_in), in_bytes, 2u, 65536, e->inf_meta, st, &adler, crc_out);
}

void zgpu_profile_enable(zgpu_engine *e, int on) { if (e) e->prof = on != 0; }
void zgpu_profile_reset(zgpu_engine *e) { if (e) { memset(e->ms, 0, sizeof e->ms); memset(e->launches, 0, sizeof e->launches); } }
int zgpu_profile_get(zgpu_engine *e, int stage, double *ms, uint64_t *launches)
{
    if (!e || stage < 0 || stage >= ZGPU_STAGE_COUNT) return ZGPU_STREAM_ERROR;
    if (ms) *ms = e->ms[stage];
    if (launches) *launches = e->launches[stage];
    return ZGPU_OK;
}
const char *zgpu_stage_name(int stage)
{
    static const char *names[ZGPU_STAGE_COUNT] = {"chain", "match", "parse", "lz_serial", "huffman", "stitch", "inflate"};
    return stage >= 0 && stage < ZGPU_STAGE_COUNT ? names[stage] : "?";
}

uint64_t zgpu_deflate_fast_count(zgpu_engine *e, int which)
{
    if (!e || which < 0 || which >= ZGPU_FAST_COUNT_N) return 0;
    return which == ZGPU_FAST_ROUNDS ? e->cf_rounds : which == ZGPU_FAST_TILE_PARSES ? e->cf_tile_parses : e->cf_stat[which - ZGPU_FAST_SAME_ENTRY];
}

int zgpu_corpus_fill_device(zgpu_engine *e, uint32_t kind, uint64_t seed, uint64_t first_chunk, uint64_t nchunks, void *d_out, void *hip_stream)
{
    if (!e || !d_out) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    launch_corpus(kind, seed, first_chunk, nchunks, static_cast<uint8_t *>(d_out), st);
    ZGPU_HIP_CHECK(hipGetLastError());
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    return ZGPU_OK;
}

#pragma GCC visibility pop
} // extern "C"
