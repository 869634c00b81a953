// zgpu_bgzf.hip -- BGZF (blocked gzip: RFC 1952 + SAM specification 4.1): the block index of a file found on the device, and the decode of all its
// blocks as one batch.
//
// A block says how long it is (BSIZE in the 'B' 'C' extra subfield of its gzip header), so the blocks of a file are a chain of headers from byte 0 to
// the file's end.  Following that chain is one dependent load per block; here it is found in parallel instead:
//   mark     one lane per byte position: is this a BGZF header (1f 8b 08, FEXTRA, a 'B' 'C' subfield)?  A candidate knows where the block behind it
//            would start (next = pos + BSIZE + 1) and its ISIZE.  Candidates are counted per 4096 positions first, then written in position order.
//   link     next becomes the index of the candidate at that position (binary search), END when it is the file's length, BAD otherwise.
//   reach    which candidates does the chain from byte 0 visit?  Pointer doubling: round k marks jump_k[c] for every reached c and squares the jump
//            table, so after round k everything within 2^k - 1 steps of candidate 0 is marked.  ceil(log2(ncand)) + 1 rounds reach the end of any
//            chain; the host fixes that number, no workgroup waits for another.
//   order    chain positions ascend, so a block's number is the prefix sum of `reach` in position order and its output offset the prefix sum of the
//            reached candidates' ISIZE.
// A signature inside a stored block's payload is a candidate too; it may chain to the file's end or even join the true chain.  It is a block only
// if the chain from byte 0 visits it -- "chains to the end" says nothing.
#include "zgpu_engine.h"
#include <cstring>

namespace zgpu {

constexpr uint32_t kMarkSpan = 4096;          // byte positions per workgroup of the mark kernels (256 lanes, 16 positions each)
constexpr uint64_t kNoNext = ~0ull;           // a candidate whose block is not valid (leaves the buffer, shorter than its frame, ISIZE > 65536)
constexpr uint32_t kBgzfBodyMin = 2;          // no deflate stream is shorter (one empty static block): with the smallest header a block holds 28 bytes, so a file has at most in_bytes / 28
constexpr uint32_t kBgzfIsizeMax = 65536;
struct BgzfResult { uint64_t nblocks, out_bytes; uint32_t valid, eof; };

// Is there a BGZF header at `pos`?  Every read is inside [0, in_bytes).  next: where the block ends (kNoNext: the header is there, the block is not valid)
__device__ inline bool bgzf_candidate(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t pos, uint64_t &next, uint32_t &isize)
{
    if (in_bytes - pos < 12) return false; // (pos < in_bytes)
    const uint8_t *p = in + pos;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return false;
    const uint32_t xlen = p[10] | (uint32_t)p[11] << 8;
    if (in_bytes - pos - 12 < xlen) return false;
    uint32_t q = 12, bsize = 0;
    const uint32_t xend = 12 + xlen;
    bool found = false;
    while (q + 4 <= xend) { // bounded by XLEN; every step advances at least 4 bytes
        const uint32_t slen = p[q + 2] | (uint32_t)p[q + 3] << 8;
        if (p[q] == 66 && p[q + 1] == 67 && slen == 2) {
            if (q + 6 <= xend) { bsize = p[q + 4] | (uint32_t)p[q + 5] << 8; found = true; }
            break;
        }
        q += 4 + slen;
    }
    if (!found) return false;
    const uint64_t len = (uint64_t)bsize + 1;
    next = kNoNext; isize = 0;
    if (len >= (uint64_t)xend + kBgzfBodyMin + 8 && len <= in_bytes - pos) { // the header, a deflate body, CRC-32 and ISIZE
        const uint8_t *t = p + len - 4;
        isize = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        if (isize <= kBgzfIsizeMax) next = pos + len;
    }
    return true;
}

// pass 1: candidates per kMarkSpan positions
__global__ void __launch_bounds__(256) bgzf_count_kernel(const uint8_t *__restrict__ in, uint64_t in_bytes, uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t n;
    if (threadIdx.x == 0) n = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kMarkSpan;
    uint32_t mine = 0;
    for (uint32_t j = 0; j < kMarkSpan; j += 256) {
        const uint64_t pos = base + j + threadIdx.x;
        uint64_t next; uint32_t isize;
        if (pos < in_bytes && bgzf_candidate(in, in_bytes, pos, next, isize)) mine++;
    }
    if (mine) atomicAdd(&n, mine);
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = n;
}

// one workgroup: base = exclusive scan of cnt[0, n), base[n] = the total
__global__ void __launch_bounds__(1024) bgzf_base_scan_kernel(const uint32_t *__restrict__ cnt, uint64_t n, uint64_t *__restrict__ base)
{
    __shared__ unsigned long long part[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n + 1023) / 1024, a = tid * per < n ? tid * per : n, z = (tid + 1) * per < n ? (tid + 1) * per : n;
    unsigned long long sum = 0;
    for (uint64_t i = a; i < z; i++) sum += cnt[i];
    part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    unsigned long long o = part[tid] - sum;
    for (uint64_t i = a; i < z; i++) { base[i] = o; o += cnt[i]; }
    if (tid == 1023) base[n] = part[1023];
}

// pass 2: the same candidates, written in position order.  The workgroup's finds go to a list in LDS in any order (there are at most kMarkSpan / 3:
// two candidates are three bytes apart at least); each is then placed by its rank among them.
__global__ void __launch_bounds__(256) bgzf_fill_kernel(const uint8_t *__restrict__ in, uint64_t in_bytes, const uint64_t *__restrict__ base, uint64_t ncand,
                                                        uint64_t *__restrict__ cpos, uint64_t *__restrict__ cnext, uint32_t *__restrict__ cisize)
{
    __shared__ uint32_t n;
    __shared__ uint16_t at[kMarkSpan / 2];
    if (threadIdx.x == 0) n = 0;
    __syncthreads();
    const uint64_t b0 = (uint64_t)blockIdx.x * kMarkSpan;
    for (uint32_t j = 0; j < kMarkSpan; j += 256) {
        const uint64_t pos = b0 + j + threadIdx.x;
        uint64_t next; uint32_t isize;
        if (pos < in_bytes && bgzf_candidate(in, in_bytes, pos, next, isize)) {
            const uint32_t i = atomicAdd(&n, 1u);
            if (i < kMarkSpan / 2) at[i] = (uint16_t)(j + threadIdx.x);
        }
    }
    __syncthreads();
    const uint32_t m = n < kMarkSpan / 2 ? n : kMarkSpan / 2;
    for (uint32_t i = threadIdx.x; i < m; i += 256) {
        const uint32_t off = at[i];
        uint32_t rank = 0;
        for (uint32_t k = 0; k < m; k++) rank += at[k] < off;
        const uint64_t c = base[blockIdx.x] + rank;
        if (c >= ncand) continue; // (the count pass saw the same bytes: cannot happen)
        uint64_t next; uint32_t isize;
        bgzf_candidate(in, in_bytes, b0 + off, next, isize);
        cpos[c] = b0 + off; cnext[c] = next; cisize[c] = isize;
    }
}

// link: jump[c] = the candidate at next (END = ncand when next is the file's length, BAD = ncand + 1 when there is none); both ends are their own
// successors.  reach starts as "candidate 0 sits at byte 0".
__global__ void __launch_bounds__(256) bgzf_link_kernel(const uint64_t *__restrict__ cpos, const uint64_t *__restrict__ cnext, uint32_t ncand, uint64_t in_bytes,
                                                        uint32_t *__restrict__ jump, uint32_t *__restrict__ reach)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncand + 2) return;
    if (c >= ncand) { jump[c] = c; reach[c] = 0; return; }
    const uint64_t next = cnext[c];
    uint32_t j = ncand + 1;
    if (next == in_bytes) j = ncand;
    else if (next != kNoNext) {
        uint32_t lo = c + 1, hi = ncand; // (positions ascend and next > pos)
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (cpos[mid] < next) lo = mid + 1; else hi = mid; }
        if (lo < ncand && cpos[lo] == next) j = lo;
    }
    jump[c] = j;
    reach[c] = (c == 0 && cpos[0] == 0) ? 1u : 0u;
}

// one round of pointer doubling.  Marks are read and written by many lanes of one launch: relaxed atomics, only the value 1 is ever stored, and the
// round bound rests on the marks of earlier launches alone.  A lane that sees a mark set in this same round marks a candidate further along the
// same chain: still one the chain from 0 visits.
__global__ void __launch_bounds__(256) bgzf_reach_kernel(const uint32_t *__restrict__ jump, uint32_t *__restrict__ jump_next, uint32_t *reach, uint32_t n)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const uint32_t j = jump[c];
    if (__hip_atomic_load(&reach[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_store(&reach[j], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    jump_next[c] = jump[j];
}

// one workgroup: block numbers and output offsets = prefix sums over the reached candidates, in position order; the verdict
__global__ void __launch_bounds__(1024) bgzf_order_kernel(const uint8_t *__restrict__ in, uint64_t in_bytes, const uint64_t *__restrict__ cpos, const uint64_t *__restrict__ cnext,
                                                          const uint32_t *__restrict__ cisize, const uint32_t *__restrict__ reach, uint32_t ncand,
                                                          uint64_t *__restrict__ in_off, uint64_t *__restrict__ out_off, BgzfResult *res)
{
    __shared__ unsigned long long pn[1024], pb[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ncand + 1023) / 1024;
    const uint32_t a = (uint64_t)tid * per < ncand ? tid * per : ncand, z = (uint64_t)(tid + 1) * per < ncand ? (tid + 1) * per : ncand;
    unsigned long long sn = 0, sb = 0;
    for (uint32_t i = a; i < z; i++) if (reach[i]) { sn++; sb += cisize[i]; }
    pn[tid] = sn; pb[tid] = sb;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long an = tid >= d ? pn[tid - d] : 0, ab = tid >= d ? pb[tid - d] : 0;
        __syncthreads();
        pn[tid] += an; pb[tid] += ab;
        __syncthreads();
    }
    unsigned long long on = pn[tid] - sn, ob = pb[tid] - sb;
    for (uint32_t i = a; i < z; i++) {
        if (!reach[i]) continue;
        in_off[on] = cpos[i]; out_off[on] = ob;
        if (cnext[i] == in_bytes) { // the file's last block: is it the end block bgzip writes?
            const uint8_t eofb[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            bool same = in_bytes - cpos[i] == 28;
            for (uint32_t k = 0; same && k < 28; k++) same = in[cpos[i] + k] == eofb[k];
            res->eof = same ? 1u : 0u;
        }
        on++; ob += cisize[i];
    }
    if (tid == 1023) {
        in_off[pn[1023]] = in_bytes; out_off[pn[1023]] = pb[1023];
        res->nblocks = pn[1023]; res->out_bytes = pb[1023];
        res->valid = (reach[ncand] && !reach[ncand + 1]) ? 1u : 0u; // the chain from 0 ends exactly at the file's length
    }
}

// after the batch decode: a block that would decode to more than its ISIZE (the batch's "room too small") has a wrong ISIZE, and a block's deflate
// data must end where its trailer begins.  first[0] = the first block that failed (start value: ~0)
// states (the integrity test, which knows no room): a block whose deflate data decoded, to more than the ISIZE the index read (out_off), gets the
// record the decode gives it -- there the trailer is never looked at
__global__ void __launch_bounds__(256) bgzf_verdict_kernel(zgpu_inflate_item *items, const uint64_t *__restrict__ in_off, uint64_t n, unsigned long long *first,
                                                           const BatchItemState *__restrict__ states, const uint64_t *__restrict__ out_off)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    zgpu_inflate_item it = items[k];
    if (states && states[k].code == ZGPU_OK && states[k].out_bytes > out_off[k + 1] - out_off[k]) {
        it = zgpu_inflate_item{}; it.code = ZGPU_DATA_ERROR; it.msg = kMsgLengthCheck; it.adler32 = 1; items[k] = it;
    } else
    if (it.code == ZGPU_BUF_ERROR) { it.code = ZGPU_DATA_ERROR; it.msg = kMsgLengthCheck; it.out_bytes = 0; items[k] = it; }
    else if (it.code == ZGPU_OK && it.in_used != in_off[k + 1] - in_off[k]) { it.code = ZGPU_DATA_ERROR; it.msg = kMsgTrailing; it.out_bytes = 0; it.in_used = 0; items[k] = it; }
    if (it.code != ZGPU_OK) atomicMin(first, (unsigned long long)k);
}

// The index of d_in[0, in_bytes) in the engine's own tables (e->bz_in_off, e->bz_out_off: *nblocks + 1 entries each).
static int bgzf_index_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, uint64_t *nblocks, uint64_t *out_bytes, uint32_t *eof, hipStream_t st)
{
    *nblocks = 0; *out_bytes = 0; *eof = 0;
    int rc;
    if (in_bytes == 0) { // no blocks: both tables are the one entry 0
        if ((rc = e->bz_in_off.reserve(e, 1)) || (rc = e->bz_out_off.reserve(e, 1))) return rc;
        ZGPU_HIP_CHECK(hipMemsetAsync(e->bz_in_off, 0, 8, st));
        ZGPU_HIP_CHECK(hipMemsetAsync(e->bz_out_off, 0, 8, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        return ZGPU_OK;
    }
    const uint64_t nspan = (in_bytes + kMarkSpan - 1) / kMarkSpan;
    if (nspan >= (1ull << 31)) return fail(e, ZGPU_STREAM_ERROR, "BGZF index: the buffer is too large");
    if ((rc = e->bz_cnt.reserve(e, nspan)) || (rc = e->bz_base.reserve(e, nspan + 1)) || (rc = e->bz_res.reserve(e, sizeof(BgzfResult) / 4))) return rc;
    hipLaunchKernelGGL(bgzf_count_kernel, dim3((uint32_t)nspan), dim3(256), 0, st, d_in, in_bytes, e->bz_cnt.p);
    hipLaunchKernelGGL(bgzf_base_scan_kernel, dim3(1), dim3(1024), 0, st, e->bz_cnt.p, nspan, e->bz_base.p);
    ZGPU_HIP_CHECK(hipGetLastError());
    uint64_t ncand = 0;
    ZGPU_HIP_CHECK(hipMemcpyAsync(&ncand, e->bz_base + nspan, 8, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (ncand == 0) return fail(e, ZGPU_DATA_ERROR, "invalid BGZF block chain");
    if (ncand >= (1ull << 31)) return fail(e, ZGPU_STREAM_ERROR, "BGZF index: too many candidate headers");
    const uint32_t nc = (uint32_t)ncand;
    if ((rc = e->bz_pos.reserve(e, ncand)) || (rc = e->bz_next.reserve(e, ncand)) || (rc = e->bz_isize.reserve(e, ncand)) || (rc = e->bz_jump_a.reserve(e, ncand + 2)) ||
        (rc = e->bz_jump_b.reserve(e, ncand + 2)) || (rc = e->bz_reach.reserve(e, ncand + 2)) || (rc = e->bz_in_off.reserve(e, ncand + 1)) || (rc = e->bz_out_off.reserve(e, ncand + 1)))
        return rc;
    hipLaunchKernelGGL(bgzf_fill_kernel, dim3((uint32_t)nspan), dim3(256), 0, st, d_in, in_bytes, e->bz_base.p, ncand, e->bz_pos.p, e->bz_next.p, e->bz_isize.p);
    const uint32_t ngrid = (nc + 2 + 255) / 256;
    hipLaunchKernelGGL(bgzf_link_kernel, dim3(ngrid), dim3(256), 0, st, e->bz_pos.p, e->bz_next.p, nc, in_bytes, e->bz_jump_a.p, e->bz_reach.p);
    uint32_t rounds = 1; // ceil(log2(ncand)) + 1: after them every candidate within 2 * ncand - 1 steps of candidate 0 is marked, and no chain is longer than ncand
    while ((1ull << (rounds - 1)) < ncand) rounds++;
    uint32_t *ja = e->bz_jump_a, *jb = e->bz_jump_b;
    for (uint32_t k = 0; k < rounds; k++) {
        hipLaunchKernelGGL(bgzf_reach_kernel, dim3(ngrid), dim3(256), 0, st, ja, jb, e->bz_reach.p, nc + 2);
        uint32_t *t = ja; ja = jb; jb = t;
    }
    BgzfResult *d_res = reinterpret_cast<BgzfResult *>(e->bz_res.p);
    ZGPU_HIP_CHECK(hipMemsetAsync(d_res, 0, sizeof(BgzfResult), st));
    hipLaunchKernelGGL(bgzf_order_kernel, dim3(1), dim3(1024), 0, st, d_in, in_bytes, e->bz_pos.p, e->bz_next.p, e->bz_isize.p, e->bz_reach.p, nc, e->bz_in_off.p, e->bz_out_off.p, d_res);
    ZGPU_HIP_CHECK(hipGetLastError());
    BgzfResult r{};
    ZGPU_HIP_CHECK(hipMemcpyAsync(&r, d_res, sizeof r, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (!r.valid) return fail(e, ZGPU_DATA_ERROR, "invalid BGZF block chain");
    *nblocks = r.nblocks; *out_bytes = r.out_bytes; *eof = r.eof;
    return ZGPU_OK;
}

static void bad_chain(zgpu_inflate_result *res)
{
    res->first_bad_chunk = -1; res->error_code = ZGPU_DATA_ERROR; res->error_msg = kMsgBgzfChain;
}

// index, then every block as one gzip item of the batch decoder.  d_out == nullptr: into e->stage_out, grown to what the index says.
// d_items: optional (device); *items_out: where the records are.  A block that failed: ZGPU_DATA_ERROR, every other block's bytes are in place.
// verify: the blocks go through the integrity test instead -- no destination at all, d_out and out_cap are not looked at
static int bgzf_inflate_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, uint8_t *d_out, uint64_t out_cap, zgpu_inflate_item *d_items, zgpu_inflate_result *res,
                            uint64_t *nblocks_out, zgpu_inflate_item **items_out, hipStream_t st, bool verify = false)
{
    uint64_t n = 0, total = 0;
    uint32_t eof = 0;
    *nblocks_out = 0;
    int rc = bgzf_index_run(e, d_in, in_bytes, &n, &total, &eof, st);
    if (rc == ZGPU_DATA_ERROR) bad_chain(res);
    if (rc) return rc;
    res->out_bytes = total;
    if (!verify && total > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    if (n == 0) return ZGPU_OK;
    if (!verify && !d_out) { if ((rc = ensure_stage(e, 0, total + 64))) return rc; d_out = e->stage_out; }
    if (!d_items) { if ((rc = e->bz_items.reserve(e, n))) return rc; d_items = e->bz_items; }
    uint64_t nfailed = 0;
    const BatchItemState *states = nullptr;
    if (verify) rc = inflate_batch_verify_run(e, d_in, in_bytes, e->bz_in_off, n, ZGPU_WRAP_GZIP, 0, d_items, &nfailed, &states, st);
    else rc = inflate_batch_run(e, d_in, in_bytes, e->bz_in_off, n, ZGPU_WRAP_GZIP, 0, d_out, total, e->bz_out_off, d_items, &nfailed, st);
    if (rc) return rc;
    *nblocks_out = n; *items_out = d_items;
    unsigned long long *first = reinterpret_cast<unsigned long long *>(e->bz_res.p); // (the index's record has been read)
    unsigned long long h_first = ~0ull;
    ZGPU_HIP_CHECK(hipMemsetAsync(first, 0xff, 8, st));
    hipLaunchKernelGGL(bgzf_verdict_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_items, e->bz_in_off.p, n, first, states, e->bz_out_off.p);
    ZGPU_HIP_CHECK(hipGetLastError());
    ZGPU_HIP_CHECK(hipMemcpyAsync(&h_first, first, 8, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (h_first != ~0ull) {
        zgpu_inflate_item it{};
        ZGPU_HIP_CHECK(hipMemcpyAsync(&it, d_items + h_first, sizeof it, hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        res->first_bad_chunk = (int32_t)h_first; res->error_code = it.code; res->error_msg = it.msg;
        return fail(e, ZGPU_DATA_ERROR, zgpu_inflate_message(it.msg));
    }
    return ZGPU_OK;
}

static void inflate_result_init(zgpu_inflate_result *res)
{
    memset(res, 0, sizeof *res);
    res->adler32 = 1; res->first_bad_chunk = -1;
}

} // namespace zgpu

using namespace zgpu;

extern "C" {
#pragma GCC visibility push(default)

int zgpu_bgzf_index_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, uint64_t *d_in_offsets, uint64_t *d_out_offsets, uint64_t cap_blocks,
                           uint64_t *nblocks, uint64_t *out_bytes, uint32_t *ends_with_eof_block, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!nblocks || !d_in_offsets || !d_out_offsets || (!d_in && in_bytes)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    uint64_t n = 0, total = 0;
    uint32_t eof = 0;
    const int rc = bgzf_index_run(e, static_cast<const uint8_t *>(d_in), in_bytes, &n, &total, &eof, st);
    if (rc) return rc;
    *nblocks = n;
    if (out_bytes) *out_bytes = total;
    if (ends_with_eof_block) *ends_with_eof_block = eof;
    if (n > cap_blocks) return fail(e, ZGPU_BUF_ERROR, "BGZF index: more blocks than the tables hold");
    ZGPU_HIP_CHECK(hipMemcpyAsync(d_in_offsets, e->bz_in_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    ZGPU_HIP_CHECK(hipMemcpyAsync(d_out_offsets, e->bz_out_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    return ZGPU_OK;
}

int zgpu_bgzf_inflate_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t out_cap, zgpu_inflate_item *d_items,
                             zgpu_inflate_result *res, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!res || (!d_in && in_bytes) || (!d_out && out_cap)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    inflate_result_init(res);
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    uint64_t n = 0;
    zgpu_inflate_item *where = nullptr;
    return bgzf_inflate_run(e, static_cast<const uint8_t *>(d_in), in_bytes, static_cast<uint8_t *>(d_out), out_cap, d_items, res, &n, &where, st);
}

// the file goes up once; the index and the decode both read it there.  A block that failed leaves its part of `out` unspecified.
int zgpu_bgzf_inflate_host(zgpu_engine *e, const void *in, uint64_t in_bytes, void *out, uint64_t out_cap, zgpu_inflate_item *items, zgpu_inflate_result *res)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!res || (!in && in_bytes) || (!out && out_cap)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    inflate_result_init(res);
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    int rc = ensure_stage(e, in_bytes + 64, 0);
    if (rc) return rc;
    if (in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, in, in_bytes, hipMemcpyHostToDevice, st));
    uint64_t n = 0;
    zgpu_inflate_item *d_items = nullptr;
    rc = bgzf_inflate_run(e, e->stage_in, in_bytes, nullptr, out_cap, nullptr, res, &n, &d_items, st);
    if ((rc == ZGPU_OK || rc == ZGPU_DATA_ERROR) && n) { // (n: the decode ran)
        if (res->out_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost, st));
        if (items) ZGPU_HIP_CHECK(hipMemcpyAsync(items, d_items, n * sizeof(zgpu_inflate_item), hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    }
    return rc;
}

int zgpu_bgzf_verify_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, zgpu_inflate_item *d_items, zgpu_inflate_result *res, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!res || (!d_in && in_bytes)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    inflate_result_init(res);
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    uint64_t n = 0;
    zgpu_inflate_item *where = nullptr;
    return bgzf_inflate_run(e, static_cast<const uint8_t *>(d_in), in_bytes, nullptr, 0, d_items, res, &n, &where, st, true);
}

int zgpu_bgzf_verify_host(zgpu_engine *e, const void *in, uint64_t in_bytes, zgpu_inflate_item *items, zgpu_inflate_result *res)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!res || (!in && in_bytes)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    inflate_result_init(res);
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    int rc = ensure_stage(e, in_bytes + 64, 0);
    if (rc) return rc;
    if (in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, in, in_bytes, hipMemcpyHostToDevice, st));
    uint64_t n = 0;
    zgpu_inflate_item *d_items = nullptr;
    rc = bgzf_inflate_run(e, e->stage_in, in_bytes, nullptr, 0, nullptr, res, &n, &d_items, st, true);
    if ((rc == ZGPU_OK || rc == ZGPU_DATA_ERROR) && n && items) { // (n: the test ran)
        ZGPU_HIP_CHECK(hipMemcpyAsync(items, d_items, n * sizeof(zgpu_inflate_item), hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    }
    return rc;
}

#pragma GCC visibility pop
}
