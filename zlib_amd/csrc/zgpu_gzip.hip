// zgpu_gzip.hip -- multi-member gzip (RFC 1952 2.2: `cat a.gz b.gz`, appended logs, .warc.gz): every member of a file in one batch of the decoder.
//
// A member does not say how long it is, so its end is known only once it has been decoded.  The finder of zgpu_bgzf.hip with one difference: `next`
// comes from the decoder, not from a header field.
//   mark     one lane per byte position: 1f 8b 08 and a flag byte without reserved bits is a candidate.  Counted per 4096 positions, then written in
//            position order.
//   decode   every candidate is an item of the batch decoder.  Its input runs to the end of the file (or of the decoder's 512 MiB window): it is NOT
//            cut at the next candidate, which may be a false one.  Its output range is a guess -- the word in front of the next candidate, the ISIZE
//            of a true member that a true candidate follows -- and the exclusive scan of the guesses is the trial layout.  An item whose range is
//            too small still reports how many input bytes it used and how many bytes it decodes to.
//   link     a candidate that decoded (ZGPU_OK or ZGPU_BUF_ERROR) links to the candidate at the position behind its trailer (binary search); END when
//            that is the file's length or no candidate (bytes behind the last member that begin no member are ignored).
//   reach    pointer doubling from candidate 0, ceil(log2(ncand)) + 1 rounds fixed by the host.  A signature inside a stored block is a member only
//            if the chain from byte 0 visits it, however well it decodes.
//   order    prefix sums over the reached candidates in position order: member numbers and the final output offsets.
//   place    every member decoded and the trial offsets are the final ones (always so when there is no false candidate): done.  Otherwise the members
//            alone are decoded once more, with their exact ranges.  Never a third time, never a round trip per member.
//
// Cost.  The candidate count is read back once, after the count kernel; the workspace is proportional to it (about 100 bytes a candidate, in buffers
// the engine owns), and a hostile file of nothing but signatures whose tables cannot be held returns ZGPU_MEM_ERROR.  A false candidate costs one
// wasted decode, bounded by its 512 MiB input window.
#include "zgpu_engine.h"
#include <atomic>
#include <cstring>

namespace zgpu {

constexpr uint32_t kGzSpan = 4096;               // byte positions per workgroup of the mark kernels (256 lanes, 16 positions each)
constexpr uint64_t kGzNoNext = ~0ull;            // a candidate that is no member, or a member that failed: nothing follows it
constexpr uint64_t kGzWindow = (1ull << 29) - 1; // input bytes an item of the batch decoder may span
constexpr uint32_t kGzMemberMin = 20;            // 10 bytes of header, 2 of deflate data, 8 of trailer
struct GzipResult { uint64_t nreach, ngood, out_bytes, in_used; uint32_t in_place, pad; };

static std::atomic<uint64_t> g_one_pass{0}, g_two_pass{0};

// Is there a member header at `pos`?  Every read is inside [0, in_bytes): a signature in the file's last 3 bytes is none, one in the last 19 is a
// candidate whose header fails.
__device__ inline bool gzip_candidate(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t pos)
{
    if (pos >= in_bytes || in_bytes - pos < 4) return false;
    const uint8_t *p = in + pos;
    return p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && (p[3] & 0xe0) == 0;
}

// pass 1: candidates per kGzSpan positions
__global__ void __launch_bounds__(256) gzip_count_kernel(const uint8_t *__restrict__ in, uint64_t in_bytes, uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t n;
    if (threadIdx.x == 0) n = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kGzSpan;
    uint32_t mine = 0;
    for (uint32_t j = 0; j < kGzSpan; j += 256)
        if (gzip_candidate(in, in_bytes, base + j + threadIdx.x)) mine++;
    if (mine) atomicAdd(&n, mine);
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = n;
}

// one workgroup: base = exclusive scan of cnt[0, n), base[n] = the total
__global__ void __launch_bounds__(1024) gzip_base_scan_kernel(const uint32_t *__restrict__ cnt, uint64_t n, uint64_t *__restrict__ base)
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

// pass 2: the same candidates, written in position order (two candidates are three bytes apart at least: a workgroup finds at most kGzSpan / 3).
// cpos[ncand] = in_bytes closes the table.
__global__ void __launch_bounds__(256) gzip_fill_kernel(const uint8_t *__restrict__ in, uint64_t in_bytes, const uint64_t *__restrict__ base, uint64_t ncand,
                                                        uint64_t *__restrict__ cpos)
{
    __shared__ uint32_t n;
    __shared__ uint16_t at[kGzSpan / 2];
    if (threadIdx.x == 0) n = 0;
    __syncthreads();
    const uint64_t b0 = (uint64_t)blockIdx.x * kGzSpan;
    for (uint32_t j = 0; j < kGzSpan; j += 256) {
        if (gzip_candidate(in, in_bytes, b0 + j + threadIdx.x)) {
            const uint32_t i = atomicAdd(&n, 1u);
            if (i < kGzSpan / 2) at[i] = (uint16_t)(j + threadIdx.x);
        }
    }
    __syncthreads();
    const uint32_t m = n < kGzSpan / 2 ? n : kGzSpan / 2;
    for (uint32_t i = threadIdx.x; i < m; i += 256) {
        const uint32_t off = at[i];
        uint32_t rank = 0;
        for (uint32_t k = 0; k < m; k++) rank += at[k] < off;
        const uint64_t c = base[blockIdx.x] + rank;
        if (c >= ncand) continue; // (the count pass saw the same bytes: cannot happen)
        cpos[c] = b0 + off;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) cpos[ncand] = in_bytes;
}

// per candidate: where its input ends, and the guess of what it decodes to -- the little-endian word in front of the next candidate (the file's end
// behind the last).  0 when the gap holds no member, or the word is more than deflate data of that length can expand to (1032 : 1).
__global__ void __launch_bounds__(256) gzip_guess_kernel(const uint8_t *__restrict__ in, uint64_t in_bytes, const uint64_t *__restrict__ cpos, uint32_t ncand,
                                                         uint64_t *__restrict__ in_end, uint32_t *__restrict__ guess)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncand) return;
    const uint64_t pos = cpos[c], nxt = cpos[c + 1]; // (cpos holds ncand + 1 entries)
    in_end[c] = in_bytes - pos < kGzWindow ? in_bytes : pos + kGzWindow;
    uint32_t g = 0;
    if (nxt > pos && nxt <= in_bytes && nxt - pos >= kGzMemberMin) {
        const uint8_t *t = in + nxt - 4; // (nxt >= 20)
        g = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        if ((uint64_t)g > 1032ull * (nxt - pos) + 64) g = 0;
    }
    guess[c] = g;
}

// one workgroup: trial[0..n] = exclusive scan of the guesses; when they sum to more than out_cap every range is made empty instead (the decode is
// then a sizing pass: every item reports ZGPU_BUF_ERROR with its true sizes)
__global__ void __launch_bounds__(1024) gzip_trial_kernel(const uint32_t *__restrict__ guess, uint32_t n, uint64_t out_cap, uint64_t *__restrict__ trial)
{
    __shared__ unsigned long long part[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n + 1023) / 1024;
    const uint32_t a = (uint64_t)tid * per < n ? tid * per : n, z = (uint64_t)(tid + 1) * per < n ? (tid + 1) * per : n;
    unsigned long long sum = 0;
    for (uint32_t i = a; i < z; i++) sum += guess[i];
    part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const bool fits = part[1023] <= out_cap;
    unsigned long long o = part[tid] - sum;
    for (uint32_t i = a; i < z; i++) { trial[i] = fits ? o : 0; o += guess[i]; }
    if (tid == 1023) trial[n] = fits ? part[1023] : 0;
}

// link: jump[c] = the candidate at the position behind c's trailer, END = ncand when that is the file's length, no candidate, or c did not decode; END
// is its own successor.  cnext[c]: that position (kGzNoNext: c did not decode).  An item whose range was too small has not had its trailer looked
// at: its eight bytes must at least be there, or it is a member cut short.  reach starts as "candidate 0".
__global__ void __launch_bounds__(256) gzip_link_kernel(const BatchItemState *__restrict__ states, zgpu_inflate_item *items, const uint64_t *__restrict__ cpos, uint32_t ncand,
                                                        uint64_t in_bytes, uint64_t *__restrict__ cnext, uint32_t *__restrict__ jump, uint32_t *__restrict__ reach)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c > ncand) return;
    if (c == ncand) { jump[c] = c; reach[c] = 0; return; }
    zgpu_inflate_item it = items[c];
    const BatchItemState s = states[c];
    uint64_t next = kGzNoNext;
    if (it.code == ZGPU_OK) next = cpos[c] + it.in_used;
    else if (it.code == ZGPU_BUF_ERROR) {
        const uint64_t end = s.body_lo + s.used + 8;
        if (end <= s.in_hi) { next = end; it.out_bytes = s.out_bytes; it.in_used = end - s.in_lo; }
        else { it.code = ZGPU_DATA_ERROR; it.msg = kMsgTruncated; it.out_bytes = 0; it.in_used = 0; }
        items[c] = it;
    }
    if (next != kGzNoNext && (next <= cpos[c] || next > in_bytes)) next = kGzNoNext; // (a member ends behind its start, inside the file: cannot happen)
    uint32_t j = ncand;
    if (next != kGzNoNext && next < in_bytes) {
        uint32_t lo = c + 1, hi = ncand; // (positions ascend and next > pos)
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (cpos[mid] < next) lo = mid + 1; else hi = mid; }
        if (lo < ncand && cpos[lo] == next) j = lo;
    }
    cnext[c] = next;
    jump[c] = j;
    reach[c] = c == 0 ? 1u : 0u;
}

// one round of pointer doubling (zgpu_bgzf.hip, bgzf_reach_kernel): relaxed atomics, only the value 1 is ever stored, and the round bound rests on the
// marks of earlier launches alone
__global__ void __launch_bounds__(256) gzip_reach_kernel(const uint32_t *__restrict__ jump, uint32_t *__restrict__ jump_next, uint32_t *reach, uint32_t n)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const uint32_t j = jump[c];
    if (j >= n) return; // (link writes only indices up to END = n - 1)
    if (__hip_atomic_load(&reach[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_store(&reach[j], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    jump_next[c] = jump[j];
}

// one workgroup: member numbers and output offsets = prefix sums over the reached candidates, in position order.  A reached candidate that did not
// decode is the chain's last: it is the failed member, the ones in front of it are the good ones.  mitems[m] = the record of member m;
// in_off[ngood] = where the good members end (the failed member's start, or the end of the last member); out_off[ngood] = their bytes.
// in_place: every good member decoded into the place the final layout gives it.
__global__ void __launch_bounds__(1024) gzip_order_kernel(const uint64_t *__restrict__ cpos, const uint64_t *__restrict__ cnext, const zgpu_inflate_item *__restrict__ items,
                                                          const uint64_t *__restrict__ trial, const uint32_t *__restrict__ reach, uint32_t ncand,
                                                          uint64_t *__restrict__ in_off, uint64_t *__restrict__ out_off, zgpu_inflate_item *__restrict__ mitems, GzipResult *res)
{
    __shared__ unsigned long long pn[1024], pb[1024];
    __shared__ uint32_t moved;
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ncand + 1023) / 1024;
    const uint32_t a = (uint64_t)tid * per < ncand ? tid * per : ncand, z = (uint64_t)(tid + 1) * per < ncand ? (tid + 1) * per : ncand;
    if (tid == 0) moved = 0;
    unsigned long long sn = 0, sb = 0;
    for (uint32_t i = a; i < z; i++) if (reach[i]) { sn++; if (cnext[i] != kGzNoNext) sb += items[i].out_bytes; }
    pn[tid] = sn; pb[tid] = sb;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long an = tid >= d ? pn[tid - d] : 0, ab = tid >= d ? pb[tid - d] : 0;
        __syncthreads();
        pn[tid] += an; pb[tid] += ab;
        __syncthreads();
    }
    const unsigned long long nreach = pn[1023], total = pb[1023];
    unsigned long long on = pn[tid] - sn, ob = pb[tid] - sb;
    for (uint32_t i = a; i < z; i++) {
        if (!reach[i]) continue;
        const zgpu_inflate_item it = items[i];
        const bool good = cnext[i] != kGzNoNext;
        in_off[on] = cpos[i]; out_off[on] = ob; mitems[on] = it;
        if (good && (it.code != ZGPU_OK || trial[i] != ob)) atomicOr(&moved, 1u);
        if (on + 1 == nreach) { // the chain's last
            res->ngood = good ? nreach : nreach - 1;
            res->in_used = good ? cnext[i] : cpos[i];
            if (good) { in_off[nreach] = cnext[i]; out_off[nreach] = total; }
        }
        on++; if (good) ob += it.out_bytes;
    }
    __syncthreads();
    if (tid == 1023) { res->nreach = nreach; res->out_bytes = total; res->in_place = moved ? 0u : 1u; }
}

// after the second decode: first[0] = the first member that failed (start value: ~0)
__global__ void __launch_bounds__(256) gzip_verdict_kernel(const zgpu_inflate_item *__restrict__ items, uint64_t n, unsigned long long *first)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    if (items[k].code != ZGPU_OK) atomicMin(first, (unsigned long long)k);
}

static int header_error(zgpu_engine *e, zgpu_inflate_result *res)
{
    res->first_bad_chunk = 0; res->error_code = ZGPU_DATA_ERROR; res->error_msg = kMsgHeaderCheck; res->out_bytes = 0; res->in_used = 0;
    return fail(e, ZGPU_DATA_ERROR, zgpu_inflate_message(kMsgHeaderCheck));
}

// The members of d_in[0, in_bytes) decoded to d_out[0, out_cap).  Leaves the tables in the engine's buffers: e->bz_in_off / e->bz_out_off (*nm + 1
// entries) and e->bz_items (*nm records, and the failed member's behind them when the code is ZGPU_DATA_ERROR and *have_bad).
static int gzip_inflate_run(zgpu_engine *e, const uint8_t *d_in, uint64_t in_bytes, uint8_t *d_out, uint64_t out_cap, uint64_t *nm, bool *have_bad, zgpu_inflate_result *res,
                            hipStream_t st)
{
    *nm = 0; *have_bad = false;
    int rc;
    const uint64_t most = in_bytes < (1ull << 50) ? 1032 * in_bytes + 64 : ~0ull; // no file decodes to more: room beyond it is never used
    if (out_cap > most) out_cap = most;
    if ((rc = e->bz_in_off.reserve(e, 1)) || (rc = e->bz_out_off.reserve(e, 1))) return rc;
    if (in_bytes == 0) { // a file of no members: both tables are the one entry 0
        ZGPU_HIP_CHECK(hipMemsetAsync(e->bz_in_off, 0, 8, st));
        ZGPU_HIP_CHECK(hipMemsetAsync(e->bz_out_off, 0, 8, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        return ZGPU_OK;
    }
    const uint64_t nspan = (in_bytes + kGzSpan - 1) / kGzSpan;
    if (nspan >= (1ull << 31)) return fail(e, ZGPU_STREAM_ERROR, "gzip members: the buffer is too large");
    if ((rc = e->bz_cnt.reserve(e, nspan)) || (rc = e->bz_base.reserve(e, nspan + 1)) || (rc = e->bz_res.reserve(e, (sizeof(GzipResult) + 3) / 4))) return rc;
    // ---- mark ----
    hipLaunchKernelGGL(gzip_count_kernel, dim3((uint32_t)nspan), dim3(256), 0, st, d_in, in_bytes, e->bz_cnt.p);
    hipLaunchKernelGGL(gzip_base_scan_kernel, dim3(1), dim3(1024), 0, st, e->bz_cnt.p, nspan, e->bz_base.p);
    ZGPU_HIP_CHECK(hipGetLastError());
    uint64_t ncand = 0;
    uint8_t head[4] = {0, 0, 0, 0};
    ZGPU_HIP_CHECK(hipMemcpyAsync(&ncand, e->bz_base + nspan, 8, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipMemcpyAsync(head, d_in, in_bytes < 4 ? in_bytes : 4, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (in_bytes < 4 || head[0] != 0x1f || head[1] != 0x8b || head[2] != 8 || (head[3] & 0xe0) || ncand == 0) return header_error(e, res);
    if (ncand >= (1ull << 31)) return fail(e, ZGPU_MEM_ERROR, "gzip members: too many candidate headers");
    const uint32_t nc = (uint32_t)ncand;
    if ((rc = e->bz_pos.reserve(e, ncand + 1)) || (rc = e->gz_in_end.reserve(e, ncand)) || (rc = e->gz_guess.reserve(e, ncand)) || (rc = e->gz_trial.reserve(e, ncand + 1)) ||
        (rc = e->gz_next.reserve(e, ncand)) || (rc = e->gz_items.reserve(e, ncand)) || (rc = e->bz_items.reserve(e, ncand)) || (rc = e->bz_jump_a.reserve(e, ncand + 1)) ||
        (rc = e->bz_jump_b.reserve(e, ncand + 1)) || (rc = e->bz_reach.reserve(e, ncand + 1)) || (rc = e->bz_in_off.reserve(e, ncand + 1)) || (rc = e->bz_out_off.reserve(e, ncand + 1)))
        return rc;
    hipLaunchKernelGGL(gzip_fill_kernel, dim3((uint32_t)nspan), dim3(256), 0, st, d_in, in_bytes, e->bz_base.p, ncand, e->bz_pos.p);
    // ---- decode every candidate ----
    const uint32_t cgrid = (nc + 255) / 256, ngrid = (nc + 1 + 255) / 256;
    hipLaunchKernelGGL(gzip_guess_kernel, dim3(cgrid), dim3(256), 0, st, d_in, in_bytes, e->bz_pos.p, nc, e->gz_in_end.p, e->gz_guess.p);
    hipLaunchKernelGGL(gzip_trial_kernel, dim3(1), dim3(1024), 0, st, e->gz_guess.p, nc, out_cap, e->gz_trial.p);
    ZGPU_HIP_CHECK(hipGetLastError());
    const BatchItemState *states = nullptr;
    uint64_t nfailed = 0;
    if ((rc = inflate_batch_run_ranges(e, d_in, in_bytes, e->bz_pos, e->gz_in_end, ncand, ZGPU_WRAP_GZIP, 0, d_out, out_cap, e->gz_trial, e->gz_trial + 1, e->gz_items, &nfailed,
                                       &states, st, /* no_pieces: the candidates overlap in the input */ true)))
        return rc;
    // ---- link, reach, order ----
    hipLaunchKernelGGL(gzip_link_kernel, dim3(ngrid), dim3(256), 0, st, states, e->gz_items.p, e->bz_pos.p, nc, in_bytes, e->gz_next.p, e->bz_jump_a.p, e->bz_reach.p);
    uint32_t rounds = 1; // ceil(log2(ncand)) + 1: no chain is longer than ncand
    while ((1ull << (rounds - 1)) < ncand) rounds++;
    uint32_t *ja = e->bz_jump_a, *jb = e->bz_jump_b;
    for (uint32_t k = 0; k < rounds; k++) {
        hipLaunchKernelGGL(gzip_reach_kernel, dim3(ngrid), dim3(256), 0, st, ja, jb, e->bz_reach.p, nc + 1);
        uint32_t *t = ja; ja = jb; jb = t;
    }
    GzipResult *d_res = reinterpret_cast<GzipResult *>(e->bz_res.p);
    ZGPU_HIP_CHECK(hipMemsetAsync(d_res, 0, sizeof(GzipResult), st));
    hipLaunchKernelGGL(gzip_order_kernel, dim3(1), dim3(1024), 0, st, e->bz_pos.p, e->gz_next.p, e->gz_items.p, e->gz_trial.p, e->bz_reach.p, nc, e->bz_in_off.p, e->bz_out_off.p,
                       e->bz_items.p, d_res);
    ZGPU_HIP_CHECK(hipGetLastError());
    GzipResult r{};
    ZGPU_HIP_CHECK(hipMemcpyAsync(&r, d_res, sizeof r, hipMemcpyDeviceToHost, st));
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (r.nreach == 0 || r.nreach > ncand || r.ngood > r.nreach) return fail(e, ZGPU_ERRNO, "gzip members: the finder lost its chain");
    // ---- place ----
    res->out_bytes = r.out_bytes; res->in_used = r.in_used;
    if (r.out_bytes > out_cap) return fail(e, ZGPU_BUF_ERROR, "output capacity too small");
    uint64_t ngood = r.ngood;
    bool bad = r.ngood < r.nreach; // the chain's last member failed: its record is e->bz_items[ngood]
    if (r.in_place) g_one_pass++;
    else {
        g_two_pass++;
        if (ngood) {
            if ((rc = inflate_batch_run(e, d_in, in_bytes, e->bz_in_off, ngood, ZGPU_WRAP_GZIP, 0, d_out, out_cap, e->bz_out_off, e->bz_items, &nfailed, st))) return rc;
            if (nfailed) { // (a member whose range was too small the first time has had its CRC-32 and ISIZE checked only now)
                unsigned long long *first = reinterpret_cast<unsigned long long *>(e->bz_res.p), h_first = ~0ull;
                ZGPU_HIP_CHECK(hipMemsetAsync(first, 0xff, 8, st));
                hipLaunchKernelGGL(gzip_verdict_kernel, dim3((uint32_t)((ngood + 255) / 256)), dim3(256), 0, st, e->bz_items.p, ngood, first);
                ZGPU_HIP_CHECK(hipGetLastError());
                ZGPU_HIP_CHECK(hipMemcpyAsync(&h_first, first, 8, hipMemcpyDeviceToHost, st));
                ZGPU_HIP_CHECK(hipStreamSynchronize(st));
                if (h_first < ngood) { ngood = h_first; bad = true; }
            }
        }
    }
    *nm = ngood; *have_bad = bad;
    if (bad) {
        zgpu_inflate_item it{};
        uint64_t at[2] = {0, 0};
        ZGPU_HIP_CHECK(hipMemcpyAsync(&it, e->bz_items + ngood, sizeof it, hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipMemcpyAsync(&at[0], e->bz_in_off + ngood, 8, hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipMemcpyAsync(&at[1], e->bz_out_off + ngood, 8, hipMemcpyDeviceToHost, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
        res->first_bad_chunk = (int32_t)ngood; res->error_code = it.code; res->error_msg = it.msg;
        res->in_used = at[0]; res->out_bytes = at[1];
        return fail(e, ZGPU_DATA_ERROR, zgpu_inflate_message(it.msg));
    }
    return ZGPU_OK;
}

static void gzip_result_init(zgpu_inflate_result *res)
{
    memset(res, 0, sizeof *res);
    res->adler32 = 1; res->first_bad_chunk = -1;
}

} // namespace zgpu

using namespace zgpu;

extern "C" {
#pragma GCC visibility push(default)

uint64_t zgpu_gzip_members_count(int which) { return which == 0 ? g_one_pass.load() : which == 1 ? g_two_pass.load() : 0; }

int zgpu_gzip_inflate_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t out_cap, uint64_t *d_in_offsets, uint64_t *d_out_offsets,
                             zgpu_inflate_item *d_items, uint64_t cap_members, uint64_t *nmembers, zgpu_inflate_result *res, void *hip_stream)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!res || !nmembers || (!d_in && in_bytes) || (!d_out && out_cap)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    gzip_result_init(res);
    *nmembers = 0;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    uint64_t nm = 0;
    bool bad = false;
    const int rc = gzip_inflate_run(e, static_cast<const uint8_t *>(d_in), in_bytes, static_cast<uint8_t *>(d_out), out_cap, &nm, &bad, res, st);
    *nmembers = nm;
    if (rc != ZGPU_OK && !(rc == ZGPU_DATA_ERROR && bad)) return rc; // (a failed member: the ones in front of it are delivered)
    if (d_in_offsets || d_out_offsets || d_items) {
        if (nm > cap_members) return rc ? rc : fail(e, ZGPU_BUF_ERROR, "gzip members: more members than the tables hold");
        const uint64_t nrec = nm + (bad && nm < cap_members ? 1 : 0);
        if (d_in_offsets) ZGPU_HIP_CHECK(hipMemcpyAsync(d_in_offsets, e->bz_in_off, (nm + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        if (d_out_offsets) ZGPU_HIP_CHECK(hipMemcpyAsync(d_out_offsets, e->bz_out_off, (nm + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        if (d_items && nrec) ZGPU_HIP_CHECK(hipMemcpyAsync(d_items, e->bz_items, nrec * sizeof(zgpu_inflate_item), hipMemcpyDeviceToDevice, st));
        ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    }
    return rc;
}

// the file goes up once; the finder and both decodes read it there.  No file decodes to more than 1032 times its length: the device's room is the
// smaller of that and out_cap.
int zgpu_gzip_inflate_host(zgpu_engine *e, const void *in, uint64_t in_bytes, void *out, uint64_t out_cap, uint64_t *in_offsets, uint64_t *out_offsets, zgpu_inflate_item *items,
                           uint64_t cap_members, uint64_t *nmembers, zgpu_inflate_result *res)
{
    if (!e) return ZGPU_STREAM_ERROR;
    if (!res || !nmembers || (!in && in_bytes) || (!out && out_cap)) return fail(e, ZGPU_STREAM_ERROR, "null argument");
    gzip_result_init(res);
    *nmembers = 0;
    ZGPU_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const uint64_t most = in_bytes < (1ull << 50) ? 1032 * in_bytes + 64 : ~0ull, room = out_cap < most ? out_cap : most; // (what gzip_inflate_run uses of it)
    int rc = ensure_stage(e, in_bytes + 64, room + 64);
    if (rc) return rc;
    if (in_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(e->stage_in, in, in_bytes, hipMemcpyHostToDevice, st));
    uint64_t nm = 0;
    bool bad = false;
    rc = gzip_inflate_run(e, e->stage_in, in_bytes, e->stage_out, room, &nm, &bad, res, st);
    *nmembers = nm;
    if (rc != ZGPU_OK && !(rc == ZGPU_DATA_ERROR && bad)) return rc; // (a failed member: the ones in front of it are delivered)
    if (res->out_bytes) ZGPU_HIP_CHECK(hipMemcpyAsync(out, e->stage_out, res->out_bytes, hipMemcpyDeviceToHost, st));
    const bool tables = in_offsets || out_offsets || items;
    if (tables && nm <= cap_members) {
        const uint64_t nrec = nm + (bad && nm < cap_members ? 1 : 0);
        if (in_offsets) ZGPU_HIP_CHECK(hipMemcpyAsync(in_offsets, e->bz_in_off, (nm + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (out_offsets) ZGPU_HIP_CHECK(hipMemcpyAsync(out_offsets, e->bz_out_off, (nm + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (items && nrec) ZGPU_HIP_CHECK(hipMemcpyAsync(items, e->bz_items, nrec * sizeof(zgpu_inflate_item), hipMemcpyDeviceToHost, st));
    }
    ZGPU_HIP_CHECK(hipStreamSynchronize(st));
    if (tables && nm > cap_members && rc == ZGPU_OK) return fail(e, ZGPU_BUF_ERROR, "gzip members: more members than the tables hold");
    return rc;
}

#pragma GCC visibility pop
}
