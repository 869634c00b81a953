// zgpu_streams.hip -- the small kernels of the batch compress of many independent streams, for both of its calls (zgpu_deflate_streams.hip is the
// blocking call's host side, zgpu_deflate_streams_enqueue.hip the stream-ordered call's, zgpu_deflate_streams_plan.h the plan): where every stream starts
// (its state, its header), what closes it (trailer, record), the entries of the streams' first tiles, and the packing of the finished streams for the
// host entry.  The tiles themselves are sorted, walked and parsed by the ROWS instantiations of sort4_kernel, walk_kernel and parse2_kernel; the blocks'
// scans are the batched kernels of zgpu_cont.hip, and the blocks of all streams of a batch are coded by one launch of huffman_kernel<true, true>.
#include "zgpu_common.h"
#include "zgpu_engine.h"
#include "zgpu_deflate_streams_plan.h"

namespace zgpu {

// what every stream of a call starts with, and the whole stream of an empty item (header, the one empty static block 03 00, trailer): words, zero-filled
struct StreamsHead {
    uint32_t head[3]; uint32_t head_words;   // the header, zero-filled to a whole word behind which the first block's bits are ORed in
    uint32_t empty[5]; uint32_t empty_bytes; // an empty item's stream
    uint32_t head_bits, flags;
};

// item k's state and header.  A room that cannot hold the smallest stream: overflow from the start, nothing written
__device__ __forceinline__ void streams_head_item(uint64_t k, const uint64_t *__restrict__ in_off, const uint64_t *__restrict__ oo, const StreamsHead &h, ContState *__restrict__ st,
                                                  uint8_t *__restrict__ out)
{
    const uint64_t L = in_off[k + 1] - in_off[k], room = oo[k + 1] - oo[k];
    ContState s{};
    s.out_bits = h.head_bits; s.data_type = 2; s.last_eob = 8; s.first_block = 1;
    uint32_t *w = reinterpret_cast<uint32_t *>(out + oo[k]);
    if (L == 0) {
        if (room >= ((h.empty_bytes + 3) & ~3u)) { for (uint32_t i = 0; i < (h.empty_bytes + 3) / 4; i++) w[i] = h.empty[i]; s.out_bits = 8ull * h.empty_bytes; }
        else s.overflow = 1;
    } else if (streams_room_cap(room, h.flags) == 0) s.overflow = 1;
    else for (uint32_t i = 0; i < h.head_words; i++) w[i] = h.head[i];
    st[k] = s;
}
// state: the stream-ordered call's table check (nullptr: the blocking call, whose host has checked the tables) -- an item it has failed (state[k] != 0)
// gets a state that says nothing and writes nothing.  totals: the blocking call's counters, cleared here (nullptr: the stream-ordered call clears its
// own in senq_clear_kernel, the launch in front)
__global__ void __launch_bounds__(256) streams_head_kernel(const uint64_t *__restrict__ in_off, const uint64_t *__restrict__ oo, const uint32_t *__restrict__ state, uint64_t n,
                                                           StreamsHead h, ContState *__restrict__ st, uint8_t *__restrict__ out, uint16_t *__restrict__ entry0,
                                                           unsigned long long *__restrict__ totals)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k == 0) { *entry0 = 0; if (totals) { totals[0] = 0; totals[1] = 0; totals[2] = 0; } }
    if (k >= n) return;
    if (state && state[k] != kSenqServed) { ContState s{}; s.data_type = 2; st[k] = s; return; }
    streams_head_item(k, in_off, oo, h, st, out);
}

// a stream's first tile is entered at 0: the chain over the launch's tiles has left the exit of the tile in front there
__global__ void __launch_bounds__(256) streams_entry_kernel(const TileRow *__restrict__ rows, uint32_t ntiles, uint16_t *__restrict__ entry)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t < ntiles && rows[t].nent == 1) entry[t] = 0;
}

// item k's trailer and record; totals: [0] bytes of all streams, [1] tokens, [2] records that are not ZGPU_OK
__device__ __forceinline__ void streams_finish_item(uint64_t k, const uint64_t *__restrict__ in_off, const uint64_t *__restrict__ oo, const StreamsHead &h, const ContState *__restrict__ st,
                                                    const zgpu_check_item *__restrict__ chk, uint32_t want_crc, uint8_t *__restrict__ out,
                                                    zgpu_deflate_batch_item *__restrict__ items, unsigned long long *__restrict__ totals)
{
    const uint64_t L = in_off[k + 1] - in_off[k];
    const ContState s = st[k];
    zgpu_deflate_batch_item it{};
    it.out_lo = oo[k]; it.in_bytes = (uint32_t)L; it.adler32 = chk[k].adler32; it.crc32 = want_crc ? chk[k].crc32 : 0u; it.data_type = s.data_type;
    if (s.overflow) { it.code = ZGPU_BUF_ERROR; it.out_bytes = 0; atomicAdd(&totals[2], 1ull); }
    else {
        uint64_t nbytes = (s.out_bits + 7) >> 3; // (bi_windup; an empty item's stream is whole already)
        if (L) {
            uint8_t *t = out + oo[k] + nbytes;
            const uint32_t ad = it.adler32, crc = chk[k].crc32, isz = (uint32_t)L;
            if (h.flags & ZGPU_F_ZLIB_WRAP) { t[0] = (uint8_t)(ad >> 24); t[1] = (uint8_t)(ad >> 16); t[2] = (uint8_t)(ad >> 8); t[3] = (uint8_t)ad; nbytes += 4; }
            else if (h.flags & ZGPU_F_GZIP_WRAP) {
                for (uint32_t i = 0; i < 4; i++) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)(isz >> (8 * i)); }
                nbytes += 8;
            }
        }
        it.code = ZGPU_OK; it.out_bytes = nbytes;
        atomicAdd(&totals[0], (unsigned long long)nbytes);
    }
    atomicAdd(&totals[1], (unsigned long long)s.ntokens);
    items[k] = it;
}
// state as for streams_head_kernel: a failed item's record is the failed record of the other enqueue calls -- it has read nothing and written nothing
__global__ void __launch_bounds__(256) streams_finish_kernel(const uint64_t *__restrict__ in_off, const uint64_t *__restrict__ oo, const uint32_t *__restrict__ state, uint64_t n,
                                                             StreamsHead h, const ContState *__restrict__ st, const zgpu_check_item *__restrict__ chk, uint32_t want_crc,
                                                             uint8_t *__restrict__ out, zgpu_deflate_batch_item *__restrict__ items, unsigned long long *__restrict__ totals)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    if (state && state[k] != kSenqServed) {
        zgpu_deflate_batch_item r{};
        r.code = ZGPU_STREAM_ERROR; r.data_type = 2; r.adler32 = 1;
        items[k] = r;
        atomicAdd(&totals[kScntFailed], 1ull);
        return;
    }
    streams_finish_item(k, in_off, oo, h, st, chk, want_crc, out, items, totals);
}

// the host entry's packing: the streams out of their rooms, back to back.  A workgroup fills 4096 bytes of the packed output, a lane 16 of them
constexpr uint32_t kPackSpan = 4096;
__global__ void __launch_bounds__(256) streams_pack_kernel(const uint8_t *__restrict__ rooms, const uint64_t *__restrict__ oo, const uint64_t *__restrict__ po, uint64_t n,
                                                           uint8_t *__restrict__ packed)
{
    __shared__ uint64_t k_first;
    const uint64_t total = po[n], d0 = (uint64_t)blockIdx.x * kPackSpan;
    if (threadIdx.x == 0) {
        uint64_t lo = 0, hi = n; // the last k with po[k] <= d0 (d0 < total = po[n])
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (po[mid] <= d0) lo = mid; else hi = mid; }
        k_first = lo;
    }
    __syncthreads();
    uint64_t k = k_first;
    const uint64_t d = d0 + threadIdx.x * 16;
    if (d >= total) return;
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < 16 && d + i < total; i++) {
        while (d + i >= po[k + 1]) k++; // (items that produced nothing are passed over)
        w[i >> 2] |= (uint32_t)rooms[oo[k] + (d + i - po[k])] << (8 * (i & 3));
    }
    if (d + 16 <= total) *reinterpret_cast<uint4 *>(packed + d) = make_uint4(w[0], w[1], w[2], w[3]);
    else for (uint32_t i = 0; d + i < total; i++) packed[d + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

static StreamsHead make_head(const FrameHead &fh, uint32_t flags)
{
    StreamsHead h{};
    uint8_t b[12] = {0}, eb[20] = {0};
    for (uint32_t i = 0; i < fh.n; i++) { b[i] = fh.b[i]; eb[i] = fh.b[i]; }
    h.head_words = ((fh.n + 4u) & ~3u) / 4; h.head_bits = 8u * fh.n; h.flags = flags;
    uint32_t m = fh.n;
    eb[m++] = 3; eb[m++] = 0; // the final, empty static block (trees.c:883-897 with no token)
    if (flags & ZGPU_F_ZLIB_WRAP) { eb[m + 3] = 1; m += 4; } // Adler-32 of nothing, big-endian
    else if (flags & ZGPU_F_GZIP_WRAP) m += 8;               // CRC-32 and ISIZE of nothing
    h.empty_bytes = m;
    for (uint32_t i = 0; i < 12; i++) h.head[i >> 2] |= (uint32_t)b[i] << (8 * (i & 3));
    for (uint32_t i = 0; i < 20; i++) h.empty[i >> 2] |= (uint32_t)eb[i] << (8 * (i & 3));
    return h;
}

void launch_streams_head(const uint64_t *in_off, const uint64_t *oo, const uint32_t *state, uint64_t n, const FrameHead &fh, uint32_t flags, ContState *st, uint8_t *out, uint16_t *entry0,
                         unsigned long long *totals, hipStream_t s)
{
    hipLaunchKernelGGL(streams_head_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, in_off, oo, state, n, make_head(fh, flags), st, out, entry0, totals);
}
void launch_streams_entry(const TileRow *rows, uint32_t ntiles, uint16_t *entry, hipStream_t s)
{
    hipLaunchKernelGGL(streams_entry_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, s, rows, ntiles, entry);
}
void launch_streams_finish(const uint64_t *in_off, const uint64_t *oo, const uint32_t *state, uint64_t n, const FrameHead &fh, uint32_t flags, const ContState *st,
                           const zgpu_check_item *chk, bool want_crc, uint8_t *out, zgpu_deflate_batch_item *items, unsigned long long *totals, hipStream_t s)
{
    hipLaunchKernelGGL(streams_finish_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, in_off, oo, state, n, make_head(fh, flags), st, chk, want_crc ? 1u : 0u, out, items,
                       totals);
}
void launch_streams_pack(const uint8_t *rooms, const uint64_t *oo, const uint64_t *po, uint64_t n, uint64_t total, uint8_t *packed, hipStream_t s)
{
    if (total) hipLaunchKernelGGL(streams_pack_kernel, dim3((uint32_t)((total + kPackSpan - 1) / kPackSpan)), dim3(256), 0, s, rooms, oo, po, n, packed);
}

} // namespace zgpu
