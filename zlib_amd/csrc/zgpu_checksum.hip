// zgpu_checksum.hip -- batch checksums (zgpu_checksum_batch_*): Adler-32 and CRC-32 of many independent items of one buffer in one call.
//
// Item k = in[off[k], off[k+1]), any size below 4 GiB, any alignment.  Three launches and one round trip to the host, no workgroup waits on another:
//   plan   one workgroup: checks the offset table (backwards, out of the buffer, 4 GiB or more: the call fails before anything is written) and
//          scans the number of 64 KiB pieces of the LONG items (more than kShortMax bytes); short items have no pieces
//   short  one WAVE per short item, kGroupItems items per 256-lane workgroup behind one CRC table in LDS: a 200-byte item costs a quarter of a
//          sixteenth of a table build, not a whole one.  The record is written from here
//   piece  one workgroup per piece of a long item (which item: a binary search in the scanned piece counts), the arithmetic of adler_kernel and
//          crc_kernel (zgpu_stitch.hip) with word loads from any alignment; a partial (a, b, crc) per piece
//   join   one lane per long item joins its partials in order (adler_join / crc_join, zgpu_common.h) and writes the record
// The CRC table is table[k][b], four tables of 256 words (slicing by four, crc32.c:268-290): a lookup is one ds_read_b32 whose bank is b mod 32
// whichever table it goes to, so lanes conflict only when their bytes differ and agree mod 32 (equal bytes broadcast) -- data decides, no layout
// of a 256-entry table avoids it, and 4 KiB a workgroup leaves the occupancy alone.  Every loop is bounded by the item's length.
#include "zgpu_common.h"
#include "zgpu_engine.h"
#include "../../include/zamd_gpu.h"

namespace zgpu {

constexpr uint32_t kShortMax = 4096;  // items of at most this many bytes are served by one wave
constexpr uint32_t kGroupItems = 16;  // items per workgroup of check_short_kernel: four per wave
struct PiecePart { uint32_t a, b, crc; };

// (one workgroup whose lanes each walk a run of n / 1024 offsets, and a round trip to the host behind it: sized for archives -- thousands of items;
// not measured for n in the millions)
// one workgroup: piece0[k] = pieces of the long items in front of item k, piece0[n] = all pieces; flag[0] |= 1 for a bad table
__global__ void __launch_bounds__(1024) check_plan_kernel(const uint64_t *__restrict__ off, uint64_t n, uint64_t in_bytes, uint64_t *piece0, uint32_t *flag)
{
    __shared__ unsigned long long part[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n + 1023) / 1024, a = tid * per < n ? tid * per : n, z = (tid + 1) * per < n ? (tid + 1) * per : n;
    auto pieces_of = [&](uint64_t i, bool &bad) -> uint64_t {
        const uint64_t lo = off[i], hi = off[i + 1];
        bad = hi < lo || hi > in_bytes || hi - lo >= (1ull << 32);
        const uint64_t len = hi - lo;
        return (bad || len <= kShortMax) ? 0ull : (len + kChunkMax - 1) / kChunkMax;
    };
    unsigned long long sum = 0;
    bool any_bad = false;
    for (uint64_t i = a; i < z; i++) { bool bad; sum += pieces_of(i, bad); any_bad |= bad; }
    if (any_bad) atomicOr(flag, 1u);
    part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    unsigned long long o = part[tid] - sum;
    for (uint64_t i = a; i < z; i++) { bool bad; piece0[i] = o; o += pieces_of(i, bad); }
    if (tid == 1023) piece0[n] = part[1023];
}

// table[k][b]: the CRC register after byte b and k more zero bytes; all 256 lanes of the workgroup
__device__ inline void crc_table_build(uint32_t (*table)[256], uint32_t tid)
{
    uint32_t r = tid;
#pragma unroll
    for (int k = 0; k < 8; k++) r = (r & 1u) ? (r >> 1) ^ kCrcPoly : r >> 1;
    table[0][tid] = r;
    __syncthreads();
#pragma unroll
    for (int k = 1; k < 4; k++) {
        const uint32_t q = table[k - 1][tid];
        table[k][tid] = (q >> 8) ^ table[0][q & 255u];
        __syncthreads();
    }
}

// the finished CRC-32 of p[0, n) (0 for n == 0): bytes up to a word boundary, words four bytes a step, the bytes behind
__device__ inline uint32_t crc_span(const uint32_t (*table)[256], const uint8_t *p, uint32_t n)
{
    uint32_t crc = 0xffffffffu;
    while (n && (reinterpret_cast<uintptr_t>(p) & 3)) { crc = table[0][(crc ^ *p++) & 255u] ^ (crc >> 8); n--; }
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    for (; n >= 4; n -= 4) {
        const uint32_t x = crc ^ *w++;
        crc = table[3][x & 255u] ^ table[2][(x >> 8) & 255u] ^ table[1][(x >> 16) & 255u] ^ table[0][x >> 24];
    }
    p = reinterpret_cast<const uint8_t *>(w);
    for (; n; n--) crc = table[0][(crc ^ *p++) & 255u] ^ (crc >> 8);
    return crc ^ 0xffffffffu;
}

// lane t of `lanes` takes a slice of L = ceil(n / lanes) bytes, the slices aligned to the END of the span (crc_kernel has the reason): [lo, hi)
__device__ inline void end_aligned_slice(uint32_t n, uint32_t lanes, uint32_t t, uint32_t &L, uint32_t &lo, uint32_t &hi)
{
    L = (n + lanes - 1) / lanes;
    const int64_t h = (int64_t)n - (int64_t)(lanes - 1 - t) * L, l = h - L;
    hi = h > 0 ? (uint32_t)h : 0u; lo = l > 0 ? (uint32_t)l : 0u;
}

// Sums of a span of n bytes whose byte i counts (n - i) times in s2: A = 1 + s1, B = n + s2 (mod 65521).  64-bit sums: a full piece of 0xFF
// bytes brings s2 to 255 * 65536 * 65537 / 2 = 5.5e11.  `stride` lanes, this one is `t`; 16-byte loads from the first aligned address on
__device__ inline void adler_sums(const uint8_t *src, uint32_t n, uint32_t t, uint32_t stride, uint64_t &s1, uint64_t &s2)
{
    s1 = 0; s2 = 0;
    uint32_t head = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15);
    if (head > n) head = n;
    for (uint32_t i = t; i < head; i += stride) { const uint32_t b = src[i]; s1 += b; s2 += (uint64_t)(n - i) * b; }
    const uint4 *v = reinterpret_cast<const uint4 *>(src + head);
    const uint32_t nvec = (n - head) >> 4;
    for (uint32_t j = t; j < nvec; j += stride) {
        const uint4 q = v[j];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w}, o = head + (j << 4);
        uint32_t t1 = 0, t2 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int m = 0; m < 4; m++) { const uint32_t b = (w[k] >> (8 * m)) & 255u; t1 += b; t2 += b * (uint32_t)(k * 4 + m); }
        }
        s1 += t1; s2 += (uint64_t)(n - o) * t1 - t2; // (n - o >= 16 > any weight in t2)
    }
    for (uint32_t i = head + (nvec << 4) + t; i < n; i += stride) { const uint32_t b = src[i]; s1 += b; s2 += (uint64_t)(n - i) * b; }
}

// STATE (the stream-ordered batch compress, checksum_batch_enqueue below): state[k] != 0 marks an item the table check has failed -- it is not read
template <bool STATE>
__global__ void __launch_bounds__(256) check_short_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ off, const uint64_t *__restrict__ piece0, uint64_t n,
                                                          uint32_t checks, zgpu_check_item *items, const uint32_t *__restrict__ state)
{
    __shared__ uint32_t table[4][256];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (checks & ZGPU_CHECK_CRC32) crc_table_build(table, tid); // (checks is the launch's: every lane takes the same way)
    for (uint32_t j = 0; j < kGroupItems / 4; j++) {
        const uint64_t k = (uint64_t)blockIdx.x * kGroupItems + j * 4 + wave; // (the wave's own: no barrier below)
        if (k >= n) break;
        if (piece0[k + 1] != piece0[k]) continue; // a long item: the piece kernels'
        if constexpr (STATE) { if (state[k] != 0) continue; }
        const uint64_t lo = off[k];
        const uint32_t len = (uint32_t)(off[k + 1] - lo);
        const uint8_t *src = in + lo;
        uint32_t a = 1, b = 0, crc = 0;
        if ((checks & ZGPU_CHECK_ADLER32) && len) {
            uint64_t s1, s2;
            adler_sums(src, len, lane, 64, s1, s2);
            for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o); s2 += __shfl_down(s2, o); }
            a = (uint32_t)((1 + s1) % kAdlerBase); b = (uint32_t)((len + s2) % kAdlerBase);
        }
        if ((checks & ZGPU_CHECK_CRC32) && len) {
            uint32_t L, slo, shi;
            end_aligned_slice(len, 64, lane, L, slo, shi);
            crc = crc_span(table, src + slo, shi - slo);
            uint32_t op = crc_xpow8n(L); // append L bytes
            for (uint32_t s = 1; s < 64; s <<= 1) {
                const uint32_t right = __shfl_down(crc, s); // the right operand covers exactly s slices: s * L bytes
                if ((lane & (2 * s - 1)) == 0) crc = crc_join(crc, right, op);
                op = crc_mulmod(op, op);
            }
        }
        if (lane == 0) { zgpu_check_item r; r.adler32 = a | (b << 16); r.crc32 = crc; items[k] = r; }
    }
}

// workgroup w: piece p0 + w of the call.  BOUND: launched at an upper bound of the pieces, the number itself is piece0[n]
template <bool BOUND>
__global__ void __launch_bounds__(256) check_piece_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ off, const uint64_t *__restrict__ piece0, uint64_t n,
                                                          uint64_t p0, uint32_t checks, PiecePart *part)
{
    __shared__ uint32_t table[4][256];
    __shared__ uint32_t join[256];
    __shared__ uint64_t red1[4], red2[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t p = p0 + blockIdx.x;
    if constexpr (BOUND) { if (p >= piece0[n]) return; } // (uniform, in front of every barrier)
    uint64_t k = 0, hi_k = n; // the last item whose first piece is at most p (items without pieces share their neighbour's number and lose)
    while (hi_k - k > 1) { const uint64_t mid = k + (hi_k - k) / 2; if (piece0[mid] <= p) k = mid; else hi_k = mid; }
    const uint64_t lo = off[k], len = off[k + 1] - lo, at = (p - piece0[k]) * kChunkMax;
    const uint32_t pn = (uint32_t)(len - at < kChunkMax ? len - at : kChunkMax);
    const uint8_t *src = in + lo + at;
    PiecePart r{1, 0, 0};
    if (checks & ZGPU_CHECK_ADLER32) {
        uint64_t s1, s2;
        adler_sums(src, pn, tid, 256, s1, s2);
        for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o); s2 += __shfl_down(s2, o); }
        if ((tid & 63) == 0) { red1[tid >> 6] = s1; red2[tid >> 6] = s2; }
        __syncthreads();
        r.a = (uint32_t)((1 + red1[0] + red1[1] + red1[2] + red1[3]) % kAdlerBase);
        r.b = (uint32_t)((pn + red2[0] % kAdlerBase + red2[1] % kAdlerBase + red2[2] % kAdlerBase + red2[3] % kAdlerBase) % kAdlerBase);
    }
    if (checks & ZGPU_CHECK_CRC32) {
        crc_table_build(table, tid);
        uint32_t L, slo, shi;
        end_aligned_slice(pn, 256, tid, L, slo, shi);
        join[tid] = crc_span(table, src + slo, shi - slo);
        uint32_t op = crc_xpow8n(L);
        __syncthreads();
        for (uint32_t s = 1; s < 256; s <<= 1) {
            uint32_t v = 0;
            const bool mine = (tid & (2 * s - 1)) == 0;
            if (mine) v = crc_join(join[tid], join[tid + s], op);
            __syncthreads();
            if (mine) join[tid] = v;
            op = crc_mulmod(op, op);
            __syncthreads();
        }
        r.crc = join[0];
    }
    if (tid == 0) part[p] = r;
}

// one lane per item: a long item's partials in order
__global__ void __launch_bounds__(256) check_join_kernel(const uint64_t *__restrict__ off, const uint64_t *__restrict__ piece0, uint64_t n, const PiecePart *__restrict__ part,
                                                         uint32_t checks, zgpu_check_item *items)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t first = piece0[k], np = piece0[k + 1] - first;
    if (np == 0) return; // a short item: written by check_short_kernel
    const uint64_t len = off[k + 1] - off[k];
    uint32_t a = 1, b = 0, crc = 0;
    const uint32_t op_full = (checks & ZGPU_CHECK_CRC32) && np > 1 ? crc_xpow8n(kChunkMax) : 0u;
    for (uint64_t i = 0; i < np; i++) {
        const PiecePart q = part[first + i];
        const uint32_t pl = i + 1 < np ? kChunkMax : (uint32_t)(len - i * kChunkMax);
        if (checks & ZGPU_CHECK_ADLER32) adler_join(a, b, q.a, q.b, pl);
        if (checks & ZGPU_CHECK_CRC32) crc = crc_join(crc, q.crc, pl == kChunkMax ? op_full : crc_xpow8n(pl));
    }
    zgpu_check_item r; r.adler32 = a | (b << 16); r.crc32 = crc;
    items[k] = r;
}

int checksum_batch_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t n, uint32_t checks, zgpu_check_item *d_items, hipStream_t st)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if ((checks & ~3u) || n >= (1ull << 32) || (n && (!d_off || !d_items || (in_bytes && !d_in)))) return fail(e, ZGPU_STREAM_ERROR, "bad checksum batch arguments");
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    int rc;
    if ((rc = e->ck_piece0.reserve(e, n + 1)) || (rc = e->ck_flag.reserve(e, 1))) return rc;
    ZGPU_HIP_CHECK(hipMemsetAsync(e->ck_flag, 0, 4, st));
    hipLaunchKernelGGL(check_plan_kernel, dim3(1), dim3(1024), 0, st, d_off, n, in_bytes, e->ck_piece0.p, e->ck_flag.p);
    ZGPU_HIP_CHECK(hipGetLastError());
    uint32_t bad = 0; uint64_t npieces = 0;
    ZGPU_HIP_CHECK(hipMemcpyAsync(&bad, e->ck_flag, 4, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipMemcpyAsync(&npieces, e->ck_piece0 + n, 8, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (bad) return fail(e, ZGPU_STREAM_ERROR, "checksum batch offsets out of range");
    hipLaunchKernelGGL(check_short_kernel<false>, dim3((uint32_t)((n + kGroupItems - 1) / kGroupItems)), dim3(256), 0, st, d_in, d_off, e->ck_piece0.p, n, checks, d_items, nullptr);
    if (npieces) {
        if ((rc = e->ck_part.reserve(e, npieces * (sizeof(PiecePart) / sizeof(uint32_t))))) return rc;
        PiecePart *part = reinterpret_cast<PiecePart *>(e->ck_part.p);
        const uint64_t slab = 1ull << 24; // workgroups a launch
        for (uint64_t p0 = 0; p0 < npieces; p0 += slab)
            hipLaunchKernelGGL(check_piece_kernel<false>, dim3((uint32_t)(npieces - p0 < slab ? npieces - p0 : slab)), dim3(256), 0, st, d_in, d_off, e->ck_piece0.p, n, p0, checks, part);
        hipLaunchKernelGGL(check_join_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_off, e->ck_piece0.p, n, part, checks, d_items);
    }
    ZGPU_HIP_CHECK(hipGetLastError());
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    return ZGPU_OK;
}

// The same without the round trip, for a call that may not wait (zgpu_deflate_streams_enqueue.hip): the plan is the caller's -- state[k] (0: served) and
// piece0[0..n] over the served long items, made on the device -- and the piece kernel is launched at the host's upper bound of the pieces, npieces_max;
// part: room for that many partials.  Launches only
void checksum_batch_enqueue(const uint8_t *d_in, const uint64_t *d_off, const uint32_t *state, const uint64_t *piece0, uint64_t n, uint64_t npieces_max, uint32_t checks, void *part,
                            zgpu_check_item *d_items, hipStream_t st)
{
    hipLaunchKernelGGL(check_short_kernel<true>, dim3((uint32_t)((n + kGroupItems - 1) / kGroupItems)), dim3(256), 0, st, d_in, d_off, piece0, n, checks, d_items, state);
    const uint64_t slab = 1ull << 24;
    for (uint64_t p0 = 0; p0 < npieces_max; p0 += slab)
        hipLaunchKernelGGL(check_piece_kernel<true>, dim3((uint32_t)(npieces_max - p0 < slab ? npieces_max - p0 : slab)), dim3(256), 0, st, d_in, d_off, piece0, n, p0, checks,
                           static_cast<PiecePart *>(part));
    hipLaunchKernelGGL(check_join_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_off, piece0, n, static_cast<const PiecePart *>(part), checks, d_items);
}

} // namespace zgpu

using namespace zgpu;

extern "C" {
#pragma GCC visibility push(default)

int zgpu_checksum_batch_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_offsets, uint64_t n, uint32_t checks, zgpu_check_item *d_items,
                               void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    return checksum_batch_run(e, static_cast<const uint8_t *>(d_in), in_bytes, d_offsets, n, checks, d_items, st);
}

// host arrays: the bytes, the table and the records staged in the engine's input buffer; the records come home only when the call succeeded
int zgpu_checksum_batch_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *offsets, uint64_t n, uint32_t checks, zgpu_check_item *items)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if ((checks & ~3u) || n >= (1ull << 32) || (n && (!offsets || !items || (in_bytes && !in)))) return fail(e, ZGPU_STREAM_ERROR, "bad checksum batch arguments");
    if (n == 0) return ZGPU_OK;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    const uint64_t o_tab = (in_bytes + 255) & ~255ull, tab_bytes = (n + 1) * sizeof(uint64_t), o_items = o_tab + ((tab_bytes + 255) & ~255ull);
    int rc = ensure_stage(e, o_items + n * sizeof(zgpu_check_item), 0);
    if (rc) return rc;
    uint8_t *sin = e->stage_in;
    hipStream_t st = e->stream;
    if (in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(sin, in, in_bytes, hipMemcpyHostToDevice, st));
    ZGPU_HIP_CHECK(hipMemcpyAsync(sin + o_tab, offsets, tab_bytes, hipMemcpyHostToDevice, st));
    zgpu_check_item *d_items = reinterpret_cast<zgpu_check_item *>(sin + o_items);
    if ((rc = checksum_batch_run(e, sin, in_bytes, reinterpret_cast<const uint64_t *>(sin + o_tab), n, checks, d_items, st))) return rc;
    ZGPU_HIP_CHECK(hipMemcpyAsync(items, d_items, n * sizeof(zgpu_check_item), hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    return ZGPU_OK;
}

#pragma GCC visibility pop
}
