/* zamd_gpu.h -- C ABI of the MI355X-native DEFLATE engine (libzamd_gpu.so).
 *
 * This is the thin HIP shim SURVEY.md section 8(b) asks for: plain pointers, sizes and int status codes,
 * no C++ or torch types.  It sits *below* the unchanged zlib API: the zlib-compatible host library
 * (include/zamd_zlib.h, libzamd_z.so) implements deflate()/inflate()/compress2()/uncompress() on top
 * of the *_host entry points below, at the place where the reference dispatches to its per-level
 * compress function and to inflate_fast:
 *
 *   zgpu_deflate_*   replaces  configuration_table[level].func(s, flush)   /root/reference/qcsrc/deflate.c:790
 *                    i.e. deflate_fast / deflate_slow + longest_match      qcsrc/deflate.c:1027-1168,1448-1674
 *                    and _tr_flush_block / compress_block                  qcsrc/trees.c:921-1016,1072-1118
 *                    and the adler32 update inside read_buf                qcsrc/deflate.c:968-970
 *   zgpu_inflate_*   replaces  the TYPE..LEN..CHECK states of inflate()    qcsrc/inflate.c:773-1098
 *                    with inflate_table and inflate_fast                   qcsrc/inftrees.c:32, qcsrc/inffast.c:67
 *
 * Unit of work: a "chunk" = up to 65536 input bytes compressed as an independent raw-deflate segment,
 * exactly what the reference emits for a fresh stream deflateInit2(level, 8, -15, 8, 0) fed the chunk
 * and finished with Z_FULL_FLUSH (or Z_FINISH for the last chunk of a stream) -- "mode B" of
 * SURVEY.md section 8(c).  Output is bit-exact with that.
 *
 * Status codes are zlib's (h/zlib.h:170-178) so the host library can return them unchanged.
 */
#ifndef ZAMD_GPU_H
#define ZAMD_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZGPU_OK 0
#define ZGPU_ERRNO (-1)        /* HIP runtime failure; text in zgpu_engine_error() */
#define ZGPU_STREAM_ERROR (-2) /* bad parameters */
#define ZGPU_DATA_ERROR (-3)   /* malformed deflate data (inflate) */
#define ZGPU_MEM_ERROR (-4)    /* device allocation failed */
#define ZGPU_BUF_ERROR (-5)    /* output capacity too small */

#define ZGPU_CHUNK_MAX 65536u

/* flags for zgpu_deflate_params.flags */
#define ZGPU_F_FINAL 1u     /* the last chunk of this call ends the stream (BFINAL + byte align) */
#define ZGPU_F_ZLIB_WRAP 2u /* prepend the 2-byte zlib header, append the big-endian Adler-32 (needs FINAL) */
#define ZGPU_F_POS0 4u      /* chunks other than the first are "position-0 matchable" (mode A) */
#define ZGPU_F_POS0_ALL 8u  /* every chunk, including the first, is position-0 matchable */
#define ZGPU_F_GZIP_WRAP 16u /* gzip member: the 10-byte header deflate() writes without a gz_header (qcsrc/deflate.c:578-596),
                               the body, CRC-32 and length little-endian (deflate.c:833-843); needs FINAL */
#define ZGPU_F_CRC32 32u     /* also compute the CRC-32 of the input (result.crc32) without writing a wrapper */

#define ZGPU_F_CONTINUOUS 64u /* zgpu_deflate_device / zgpu_deflate_host: the input as ONE continuous stream, byte for byte what the reference's un-flushed
                                deflate() -- plain compress2(), qcsrc/compress.c:22-58 -- emits: the 32 KiB window slides through the whole input
                                (qcsrc/deflate.c:1266-1358), matches cross every 64 KiB boundary, blocks are cut every 16383 tokens counted from the
                                stream's start (h/deflate.h:313).  Needs FINAL; chunk_size, POS0*, prime do not apply; no chunk table. */

#define ZGPU_F_BGZF_WRAP 128u /* zgpu_deflate_segments_device / _host only: every segment becomes one BGZF block (SAM specification 4.1) -- the 18-byte gzip header
                                bgzip writes (FEXTRA with the one subfield 'B' 'C', whose value BSIZE is the block's total length - 1), the raw body, CRC-32 and
                                ISIZE.  Needs FINAL, no other wrapper flag, segments of at most 65280 bytes (then BSIZE always fits its 16 bits) and the default
                                geometry (zgpu_deflate_set_geometry 15 / 8); anything else is ZGPU_STREAM_ERROR.  out_offsets marks where each block begins. */

/* LZ77 match-finder implementation selector (debug / A-B measurements) */
#define ZGPU_LZ_AUTO 0
#define ZGPU_LZ_SERIAL 1   /* one lane per chunk, tables in HBM: any level 1..9 */
#define ZGPU_LZ_PARALLEL 2 /* static-chain search over all positions (link ring in LDS) + scan parse: levels 4..9 */
#define ZGPU_LZ_SORTED 3   /* the same search over counting-sorted hash buckets: levels 4..9 */
#define ZGPU_LZ_WALK 4     /* parse-driven search over the same buckets (only the positions deflate_slow searches): levels 4..9, the default */
#define ZGPU_LZ_FAST 5     /* levels 1-3: deflate_fast over the sorted buckets, one lane per chunk, a flag byte per position for "in the chains" */
#define ZGPU_LZ_FASTWIN 6  /* levels 1-3: deflate_fast, one wave per chunk, 64 positions a step, window + chain bits in LDS: the default there */

typedef struct zgpu_engine zgpu_engine;

typedef struct {
    int32_t level;       /* 1..9 */
    uint32_t chunk_size; /* 1..65536; 0 selects 65536 */
    uint32_t flags;      /* ZGPU_F_* */
    int32_t lz_impl;     /* ZGPU_LZ_* */
    int32_t strategy;    /* 0 Z_DEFAULT_STRATEGY, 1 Z_FILTERED, 2 Z_HUFFMAN_ONLY, 3 Z_RLE, 4 Z_FIXED (qcsrc/deflate.c:1485-1497,
                            1594-1611; trees.c:986).  Not served by ZGPU_LZ_PARALLEL. */
    uint32_t prime;      /* deflatePrime (qcsrc/deflate.c:404-413): (nbits << 16) | value, nbits 0..16.  The first chunk of the call starts behind these
                            bits (its blocks are shifted, the padding of its stored blocks and of its end moves with them).  Not with a
                            wrapper flag.  0: none. */
} zgpu_deflate_params;

typedef struct {
    uint64_t out_bytes;  /* bytes written to the output buffer */
    uint64_t nchunks;
    uint32_t adler32;    /* Adler-32 of the whole input (1 for empty input) */
    uint32_t data_type;  /* Z_BINARY 0 / Z_TEXT 1 / Z_UNKNOWN 2, as strm->data_type after the first block */
    uint64_t ntokens;    /* literal/match tokens over all chunks (diagnostic) */
    uint32_t crc32;      /* CRC-32 of the whole input when ZGPU_F_GZIP_WRAP or ZGPU_F_CRC32 was given, else 0 */
    uint32_t reserved;
} zgpu_deflate_result;

typedef struct {
    uint64_t out_bytes;   /* bytes produced */
    uint32_t adler32;     /* Adler-32 of the produced bytes */
    int32_t first_bad_chunk; /* -1, or the first chunk that failed */
    int32_t error_code;   /* ZGPU_OK or the failure of first_bad_chunk */
    uint32_t error_msg;   /* index into zgpu_inflate_message() */
    uint32_t crc32;       /* CRC-32 of the produced bytes */
    uint32_t in_used_bits; /* with `incomplete`: bits of the byte at in + in_used that are consumed as well (0..7): the stream goes on at that bit
                              (zgpu_inflate_stream_host3's start_bit) */
    /* zgpu_inflate_stream_host2 / 3 with ZGPU_INF_STREAM (otherwise in_used = in_bytes, the flags 0): */
    uint64_t in_used;     /* input bytes consumed: up to the end of the final block, or of the last segment / piece that decoded */
    uint32_t stream_end;  /* the final block was reached */
    uint32_t incomplete;  /* the input stops inside a block: out_bytes / in_used cover the segments in front of it (possibly none) */
} zgpu_inflate_result;

/* ---- multi-GPU: the per-rank raw bodies gathered into ONE RFC 1950 stream on rank 0 over RCCL / xGMI (zlib_amd/csrc/zgpu_comm.hip) ----
 * One process per GPU; rank r compresses its contiguous chunk range with zgpu_deflate_device (flags = ZGPU_F_FINAL on the last rank only, no
 * wrapper) and the only exchange is this gather.  The reference has no distributed path.  RCCL is dlopen()ed by the first call here.
 *   rank 0: zgpu_comm_unique_id(id); the 128 bytes reach the other ranks by any channel; every rank: zgpu_comm_create(device, world, rank, id, &c);
 *   per stream, every rank: zgpu_deflate_gather_sizes (an all-gather of three u64 per rank: rank 0 learns the exact size of the stream),
 *   then zgpu_deflate_gather (one send per peer; on rank 0 one receive per peer at its offset, all in one group).  Both calls return when the
 *   stream has drained on the calling rank: d_body may be reused then.  The gathered stream's header is the default strategy's (FLEVEL from the level). */
typedef struct zgpu_comm zgpu_comm;
#define ZGPU_COMM_ID_BYTES 128
int zgpu_comm_unique_id(void *id128);
int zgpu_comm_create(int device, int world, int rank, const void *id128, zgpu_comm **out);
void zgpu_comm_destroy(zgpu_comm *c);
const char *zgpu_comm_error(void); /* the calling thread's last failure */
/* table: world x {body bytes, Adler-32, input bytes}; offsets[r] = where rank r's body starts in the stream (offsets[0] = 2),
 * offsets[world] = where the 4-byte trailer goes, *total = the stream's length */
void zgpu_gather_layout(int world, const uint64_t *table, uint64_t *offsets, uint64_t *total);
int zgpu_deflate_gather_sizes(zgpu_comm *c, uint64_t body_bytes, uint32_t adler32, uint64_t in_bytes, uint64_t *table, uint64_t *total, void *hip_stream);
int zgpu_deflate_gather(zgpu_comm *c, const void *d_body, const uint64_t *table, int level, void *d_out, uint64_t out_cap, uint32_t *adler_out,
                        void *hip_stream);

/* ---- engine lifetime ---- */
int zgpu_device_count(void);
int zgpu_engine_create(int device, zgpu_engine **out);
void zgpu_engine_destroy(zgpu_engine *e);
const char *zgpu_engine_error(const zgpu_engine *e);
const char *zgpu_version(void);
uint64_t zgpu_debug_handed_on(const zgpu_engine *e); /* diagnostic: chunks of level 1-3 calls that went from the lane-per-chunk loop to the wave-per-chunk kernel */
int zgpu_debug_sort_fallback(const zgpu_engine *e);  /* diagnostic: non-zero once the fast sort's self-check has failed on this engine and its calls use the ballot-ranked sort */

/* deflateInit2's geometry (qcsrc/deflate.c:222-297) for the calls that follow: windowBits 9..15 (the window is 2^windowBits bytes, matches reach
 * 2^windowBits - 262 back, the window slides every 2^windowBits bytes) and memLevel 1..9 (hash of memLevel + 7 bits, a block is cut after
 * 2^(memLevel+6) - 1 tokens).  15 / 8 is the default and what every kernel is built for; any other geometry is served by the lane-per-chunk loop
 * (ZGPU_LZ_SERIAL) and the same block-construction kernel, bit-exact with the reference's chunk function under that deflateInit2.  Output
 * capacity: zgpu_deflate_bound_geometry. */
int zgpu_deflate_set_geometry(zgpu_engine *e, int window_bits, int mem_level);
uint64_t zgpu_deflate_bound_geometry(uint64_t in_bytes, uint32_t chunk_size, int window_bits, int mem_level);

/* deflateTune (qcsrc/deflate.c:453-470): while `on`, the deflate calls of this engine use these four parameters of the match
 * search instead of the level's row of configuration_table (deflate.c:137-149); the level keeps its compress function
 * (deflate_fast for 1..3, deflate_slow for 4..9). */
int zgpu_deflate_set_tuning(zgpu_engine *e, int on, uint32_t good_length, uint32_t max_lazy, uint32_t nice_length, uint32_t max_chain);

/* worst-case output bytes for in_bytes of input cut into chunk_size pieces (framing included) */
uint64_t zgpu_deflate_bound(uint64_t in_bytes, uint32_t chunk_size);

/* ---- deflate ---- */
/* Device-resident: d_in/d_out are device pointers on the engine's device; d_chunk_offsets (optional)
 * receives nchunks+1 byte offsets of each chunk's segment inside d_out.  hip_stream may be NULL
 * (engine's own stream).  Blocks until the result is known. */
int zgpu_deflate_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const zgpu_deflate_params *p,
                        void *d_out, uint64_t out_cap, uint64_t *d_chunk_offsets, zgpu_deflate_result *res,
                        void *hip_stream);
/* Host buffers: stages through device memory (H2D, kernels, D2H). chunk_offsets (optional, host)
 * receives nchunks+1 offsets. */
int zgpu_deflate_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const zgpu_deflate_params *p, void *out,
                      uint64_t out_cap, uint64_t *chunk_offsets, zgpu_deflate_result *res);

/* ---- ONE continuous stream, feed by feed (zlib_amd/csrc/zgpu_cont.hip the kernels, zgpu_deflate_cont.hip the host side): what deflate() of the zlib API is built on ----
 * The stream's state between feeds lives with the CALLER (zgpu_cont_state + the tokens of the block that is still filling); the engine keeps nothing.
 * All positions are positions in the stream (a preset dictionary's bytes count: the first one is position 0).
 *   hist, in   buf = hist followed by in (two host buffers, so that a caller's large input need not be copied behind the little history the stream keeps):
 *              the bytes the parse can still reach followed by the bytes it has not parsed.  buf[0] is stream position cs->abs0, which must be at most
 *              cs->entry - 32512 (or 0) -- and at most cs->block_start when that lies within 65536 + 512 of cs->entry (a block that may still be stored
 *              is copied from there)
 *   check_from offset into buf of the first byte whose checksum is wanted: res->adler32 / crc32 cover buf[check_from ..) alone (hist_bytes + in_bytes: nothing)
 *   mode       ZGPU_CONT_MORE: more input follows; the parse stops 512 bytes (or a little less) in front of the end of buf and cs->entry says where --
 *              the caller keeps the bytes from cs->entry - 32512 on for the next feed.  ZGPU_CONT_FLUSH: the segment ends here as at Z_SYNC_FLUSH /
 *              Z_PARTIAL_FLUSH / Z_FULL_FLUSH (lookahead runs out at the end of buf, the block that is filling is closed; the marker behind it is the
 *              caller's to write -- it knows cs->bit_count / bit_value and cs->last_eob).  ZGPU_CONT_FINISH: the same with the final bit, padded to a byte.
 *   hist_bits  levels 1-3 (deflate_fast leaves the strings inside a long match out of its hash chains, qcsrc/deflate.c:1510-1534, so WHICH positions of the
 *              history are in the chains is part of the stream's state): ZGPU_CONT_HIST_WORDS words, bit j = the position max(cs->entry - 32512, the
 *              stream position of buf's first byte if that is later) + j is in the chains; in and out; all zero for a fresh stream, ones for a preset
 *              dictionary's positions but its last two.  Levels 4-9 do not look at it (may be NULL).
 *   excl       (levels 4-9) stream positions inside buf's history that are NOT in the hash chains: the two in front of every earlier flush point (zlib 1.2.3 never
 *              inserts them, qcsrc/deflate.c:1576 with lookahead < MIN_MATCH)
 *   out        whole bytes of the stream from the byte the last feed left unfinished (cs->bit_count bits of it are in cs->bit_value); res->out_bytes */
#define ZGPU_CONT_MORE 0
#define ZGPU_CONT_FLUSH 1
#define ZGPU_CONT_FINISH 2
#define ZGPU_CONT_CARRY_TOKENS 16384
typedef struct {
    uint64_t abs0;        /* in: stream position of buf[0] */
    uint64_t entry;       /* in/out: stream position the parse stands at with nothing in hand (deflate_slow between two matches) */
    uint64_t block_start; /* in/out: stream position of the first byte of the block that is filling */
    uint32_t carry_ntok;  /* in/out: tokens of that block so far (in carry_tok) */
    uint32_t bit_count, bit_value; /* in/out: bits of the stream's next byte that are decided already (0..7 of them) */
    uint32_t data_type;   /* in/out: 2 (Z_UNKNOWN) until the first block has decided */
    uint32_t first_block; /* in/out: 1 until the stream's first block is out */
    uint32_t last_eob;    /* in/out: last_eob_len (qcsrc/trees.c:1117) -- what _tr_align looks at; 8 for a fresh stream */
} zgpu_cont_state;
uint64_t zgpu_deflate_cont_bound(uint64_t buf_bytes); /* output capacity that is enough for one feed */
#define ZGPU_CONT_HIST_WORDS 1032
/* deflate_fast behind deflate_slow (deflateParams 4..9 -> 1..3): longest_match seeds its best length with prev_length (qcsrc/deflate.c:1035), which deflate_fast never
 * sets and deflate_slow leaves at 0 when its last token was a match (:1630-1636).  zgpu_deflate_cont_last_match: 1 / 0 when the engine's last level 4..9 ZGPU_CONT_FLUSH feed
 * ended on a match / a literal, -1 when it made no token (nothing changes).  While prev0 is set, level 1..3 feeds search as the reference does with prev_length 0: the
 * first candidate taken must also have the byte in front of it equal to the byte in front of the string; byte_before is the stream's byte in front of the feed's
 * buffer (-1: none; it can be a candidate's neighbour only behind Z_FULL_FLUSH).  The caller resets both (0, -1) after its feed, like the tuning. */
int zgpu_deflate_cont_set_stale(zgpu_engine *e, int prev0, int byte_before);
int zgpu_deflate_cont_last_match(zgpu_engine *e);
int zgpu_deflate_cont_host(zgpu_engine *e, const void *hist, uint64_t hist_bytes, const void *in, uint64_t in_bytes, uint64_t check_from, const zgpu_deflate_params *p,
                           int mode, zgpu_cont_state *cs, uint32_t *carry_tok, uint32_t *hist_bits, const uint64_t *excl, uint32_t nexcl, void *out, uint64_t out_cap,
                           zgpu_deflate_result *res);

/* Batch of independent small buffers: segment k = in[seg_offsets[k] .. seg_offsets[k+1]), each at most
 * 65536 bytes, becomes one chunk.  With ZGPU_F_FINAL every segment is a complete raw-deflate stream of its
 * own (Z_FINISH); without it every segment ends with the full-flush marker.  ZGPU_F_POS0_ALL applies to all
 * segments.  With ZGPU_F_FINAL, ZGPU_F_ZLIB_WRAP or ZGPU_F_GZIP_WRAP makes every segment one complete zlib stream (what
 * compress2() of the segment emits) or one gzip member (the header deflate() writes, qcsrc/deflate.c:578-596, and its own
 * CRC-32 / ISIZE); out_offsets then marks where each stream begins.  out_offsets (optional) receives nseg+1 output offsets. */
int zgpu_deflate_segments_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_seg_offsets,
                                 uint64_t nseg, const zgpu_deflate_params *p, void *d_out, uint64_t out_cap,
                                 uint64_t *d_out_offsets, zgpu_deflate_result *res, void *hip_stream);
int zgpu_deflate_segments_host(zgpu_engine *e, const void *in, const uint64_t *seg_offsets, uint64_t nseg,
                               const zgpu_deflate_params *p, void *out, uint64_t out_cap, uint64_t *out_offsets,
                               zgpu_deflate_result *res);

/* The same calls with one record per segment (d_items / items: nseg records, device memory for the device entry; NULL: none, which is what the
 * two entries above are).  The output bytes do not change.  Record k:
 *   out_lo, out_bytes  where segment k's stream lies in the output, its wrapper included (out_offsets[k] and the distance to the next)
 *   in_bytes           the segment's length
 *   data_type          Z_BINARY 0 / Z_TEXT 1 as strm->data_type after the segment's first block; an empty segment: Z_UNKNOWN 2
 *   adler32            of the segment's input (1 for an empty one)
 *   crc32              of the segment's input when ZGPU_F_GZIP_WRAP, ZGPU_F_BGZF_WRAP or ZGPU_F_CRC32 was given, else 0
 * A call that runs in several batches writes the records batch by batch; they are complete when the call returns ZGPU_OK. */
typedef struct {
    uint64_t out_lo, out_bytes;
    uint32_t in_bytes, data_type, adler32, crc32;
} zgpu_deflate_item;
int zgpu_deflate_segments_items_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_seg_offsets,
                                       uint64_t nseg, const zgpu_deflate_params *p, void *d_out, uint64_t out_cap,
                                       uint64_t *d_out_offsets, zgpu_deflate_result *res, zgpu_deflate_item *d_items, void *hip_stream);
int zgpu_deflate_segments_items_host(zgpu_engine *e, const void *in, const uint64_t *seg_offsets, uint64_t nseg,
                                     const zgpu_deflate_params *p, void *out, uint64_t out_cap, uint64_t *out_offsets,
                                     zgpu_deflate_result *res, zgpu_deflate_item *items);

/* Output capacity that is enough for zgpu_deflate_segments_* of nseg segments holding in_bytes in all (flags: the wrapper asked for; 26 bytes a segment for ZGPU_F_BGZF_WRAP), on an
 * engine with the default geometry (windowBits 15, memLevel 8; zgpu_deflate_set_geometry); the host entry sizes its own staging in any case. */
uint64_t zgpu_deflate_segments_bound(uint64_t nseg, uint64_t in_bytes, uint32_t flags);

/* ---- stream-ordered batch deflate: the segment calls above, enqueued ----
 * For a caller whose data lives on the GPU.  Item k = d_in[d_in_offsets[k] .. d_in_offsets[k+1]), at most 65536 bytes (65280 with ZGPU_F_BGZF_WRAP), becomes
 * the stream zgpu_deflate_segments_items_device makes of that segment with the same p: raw deflate, or with ZGPU_F_ZLIB_WRAP / ZGPU_F_GZIP_WRAP /
 * ZGPU_F_BGZF_WRAP a zlib stream, a gzip member, a BGZF block (BSIZE filled in; the 28-byte end block is the caller's to append); ZGPU_F_CRC32 as usual.
 * A call puts kernel launches on hip_stream (null: the engine's stream) as ONE chain and returns; it does not synchronize, allocate,
 * copy to or from host memory, record an event, use a second stream or time anything, and it uses no device memory of the engine's: its scratch is d_ws,
 * device memory of the caller's, 256-byte aligned, of at least zgpu_deflate_batch_workspace_bytes(n, batch_items) bytes (a function of n and of
 * min(n, batch_items) alone -- never of the bytes, the level or the wrapper; it needs no engine and no GPU; about 1.39 MiB per item of a round, the staging
 * buffer the round's items are gathered into included).  The engine supplies the device, the error text, zgpu_deflate_set_tuning's row and the choice of the sort, nothing else:
 * two calls with different workspaces may be in flight on different streams of one engine, a call can wait in a stream behind the kernel that makes its
 * input, and it can be captured into a graph (not the first call of a process: that one loads the code).  d_in, the tables, d_out, d_items, d_summary
 * and d_ws are read and written in stream order: they must be valid when the work runs, and stay untouched by other streams until it is done.
 * batch_items: items per round of launches, 0 = min(n, 4096).  Rounds follow one another in stream order in the same workspace; the packed entry's
 * running total is carried from round to round on the device.
 * Served: ZGPU_F_FINAL (required), levels 1..9 with ZGPU_LZ_AUTO -- levels 4-9 the parse-driven search (ZGPU_LZ_WALK), levels 1-3 the wave-per-chunk
 * kernel (ZGPU_LZ_FASTWIN) -- Z_DEFAULT_STRATEGY, Z_FILTERED, Z_FIXED, the engine's zgpu_deflate_set_tuning as in the blocking call.
 * Refused at once with ZGPU_STREAM_ERROR and nothing enqueued: what the chain cannot serve without a decision of the host's or the lane-per-chunk loop's
 * tables -- Z_HUFFMAN_ONLY, Z_RLE, a deflateTune row the record searches or the levels 1-3 kernels refuse, a geometry other than windowBits 15 /
 * memLevel 8, prime, ZGPU_F_POS0 / _POS0_ALL / _CONTINUOUS, any lz_impl but ZGPU_LZ_AUTO, two wrappers -- and every argument the host can judge: a null
 * pointer that is needed, n >= 2^32, ws_bytes too small, d_ws not 256-byte aligned.  n == 0 enqueues at most the launch that clears the summary.
 * d_items[k] (device memory, n records): code = ZGPU_OK with out_lo / out_bytes / in_bytes / data_type / adler32 / crc32 exactly as zgpu_deflate_item has
 * them for that segment.  The host never sees the tables, so a bad entry fails its item, not the call: offsets that run backwards or leave in_bytes
 * (counted in nbad_offsets) or lie further apart than an item may be long (ntoo_long) give code = ZGPU_STREAM_ERROR, out_bytes = in_bytes = 0,
 * adler32 = 1, crc32 = 0, data_type = 2; such an item reads nothing, writes nothing and occupies no output, and every other item is served as if it
 * were not there.
 * zgpu_deflate_batch_enqueue: d_out_offsets (n + 1 entries, read) gives item k the room d_out[oo[k] .. oo[k+1]).  A stream that does not fit: ZGPU_BUF_ERROR
 * with out_bytes = the size needed, its room untouched.  A range that runs backwards or leaves out_cap: ZGPU_STREAM_ERROR, counted in nbad_offsets.
 * zgpu_deflate_batch_packed_enqueue: the streams lie back to back in item order, as the blocking call lays them; d_out_offsets (n + 1 entries, written)
 * and total = d_out_offsets[n] are always written.  total > out_cap: overflow = 1, the items that lie wholly inside out_cap are written and ZGPU_OK, the
 * others ZGPU_BUF_ERROR with their sizes.
 * No byte outside d_out[0, out_cap), d_items, d_summary (optional) and d_ws is ever written.  nfailed = records that are not ZGPU_OK.
 * The sort's self-check: the chain sorts with the fast position sort unless the engine is set to the exact one.  Its fault word lies in d_ws, is cleared at
 * the head of the chain and read by the call's last launch: raised, sort_fault = 1, every record has code = ZGPU_ERRNO, nfailed = n, and the bytes in d_out
 * are unspecified (but inside d_out).  The blocking calls redo themselves with the exact sort then; an enqueued call has returned long before, so the
 * CALLER does it: zgpu_engine_set_exact_sort(e, 1) -- the setting the blocking fallback makes, reported by zgpu_debug_sort_fallback -- and enqueue again.
 * Rates (profiles/r09_deflate_enqueue_table.txt, level 6, device-resident), enqueue over blocking: 0.84 for 200 batches of 64 items of 4 KiB on one stream,
 * 1.005 for one batch of 4,096 items of 64 KiB, 1.14 for one batch of 16,384 items of 4 KiB in the default rounds of 4,096 (1.003 in one round). */
typedef struct {
    int32_t code;
    uint32_t data_type;
    uint64_t out_lo, out_bytes;
    uint32_t in_bytes, adler32, crc32, reserved;
} zgpu_deflate_batch_item;
typedef struct {
    uint64_t nfailed, nbad_offsets, ntoo_long, total;
    uint32_t overflow, sort_fault;
} zgpu_deflate_batch_summary;
uint64_t zgpu_deflate_batch_workspace_bytes(uint64_t n, uint32_t batch_items); /* 0: n >= 2^32 */
int zgpu_deflate_batch_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, const zgpu_deflate_params *p,
                               void *d_out, uint64_t out_cap, const uint64_t *d_out_offsets, zgpu_deflate_batch_item *d_items,
                               zgpu_deflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes, uint32_t batch_items, void *hip_stream);
int zgpu_deflate_batch_packed_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, const zgpu_deflate_params *p,
                                      void *d_out, uint64_t out_cap, uint64_t *d_out_offsets, zgpu_deflate_batch_item *d_items,
                                      zgpu_deflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes, uint32_t batch_items, void *hip_stream);
int zgpu_engine_set_exact_sort(zgpu_engine *e, int on); /* on != 0: the engine's calls use the ballot-ranked sort, which needs no self-check; 0: the fast sort again */

/* ---- batch deflate of items of ANY length: many continuous streams in one call (zlib_amd/csrc/zgpu_deflate_streams.hip) ----
 * The segment and enqueue calls above stop at 65,536 bytes an item, because an item is one chunk there.  Here item k = in[in_offsets[k] .. in_offsets[k+1]), of any
 * length from 0 to below 2^32, becomes exactly the bytes the reference's one-call stream gives for that item alone: compress2(level) with ZGPU_F_ZLIB_WRAP,
 * deflateInit2(level, Z_DEFLATED, 31 or -15, 8, strategy) + deflate(Z_FINISH) with ZGPU_F_GZIP_WRAP or no wrapper -- what zgpu_deflate_device with
 * ZGPU_F_CONTINUOUS gives one input.  Every stream is cut into tiles as a continuous stream is (zgpu_cont.hip), and the tiles of ALL items share the launches
 * of the sort, the walkers, the chain of entries and the token parse, and so do the blocks of all streams of a batch in block construction: one launch each
 * per batch of tiles, whatever the number of streams.  The scans around block construction (tokens -> blocks, bit positions, the bits into the room, the carry)
 * are the continuous stream's own kernels, launched stream by stream of the batch, with no wait for the host in between.  Batches of tiles are
 * sized by the device's memory or ZGPU_CONT_BATCH_TILES (read per call) over the tiles of all items laid end to end; they end wherever they end, also inside a stream.
 *   zgpu_deflate_streams_bound   a room that always suffices for an item of item_bytes: zgpu_deflate_cont_bound plus the wrapper named in flags, rounded up to 4
 *   zgpu_deflate_streams_layout  out_offsets[0..n] and *total (optional) from the sizes alone, rooms of zgpu_deflate_streams_bound each; host arithmetic, needs no
 *                                engine and no GPU; ZGPU_STREAM_ERROR for a null table or one that runs backwards
 *   zgpu_deflate_streams_device  the caller gives item k the room d_out[oo[k] .. oo[k+1]); every oo[k] is a multiple of 4 and d_out is 4-byte aligned (the
 *                                stitch kernels work in 32-bit words and OR bits into place; the call clears what it must).  Bytes of a room behind its stream
 *                                are unspecified; no byte outside the rooms is written.  d_in_offsets, d_out_offsets and d_items (n records, required) are device
 *                                memory.  The call blocks until the result is known and reads its tables on the host.
 *   zgpu_deflate_streams_host    lays the rooms out itself, packs the streams back to back on the device and copies them home once: out_offsets[0..n] as
 *                                zgpu_deflate_segments_host writes them, items[k].out_lo = out_offsets[k].  in_offsets[0] is 0.  All streams together larger than
 *                                out_cap: ZGPU_BUF_ERROR.
 * Record k (zgpu_deflate_batch_item): code, out_lo, out_bytes (wrapper included), in_bytes, data_type, adler32, crc32 as the enqueue calls write them.  A stream
 * that does not fit its room fails its item alone: code = ZGPU_BUF_ERROR, out_bytes = 0, nothing written outside its room; every other item is served as
 * if it were not there, and the call returns ZGPU_OK.  res: out_bytes, ntokens and nchunks (= tiles) summed over the items, adler32 / crc32 / data_type of the
 * last item, reserved = the number of records that are not ZGPU_OK.
 * A table entry that runs backwards, leaves in_bytes / out_cap or (out_offsets) is no multiple of 4 fails the call with ZGPU_STREAM_ERROR before anything is launched.
 * Served: ZGPU_F_FINAL (required), levels 4..9, all five strategies, at most one of ZGPU_F_ZLIB_WRAP / ZGPU_F_GZIP_WRAP, ZGPU_F_CRC32, zgpu_deflate_set_tuning as the
 * continuous stream honours it.  Refused at once with ZGPU_STREAM_ERROR, the output untouched: levels 0..3 (the levels 1-3 tile path is a host-driven loop of
 * rounds; those levels stay with one stream per call), a geometry other than windowBits 15 / memLevel 8, prime, ZGPU_F_POS0 / _POS0_ALL / _BGZF_WRAP /
 * _CONTINUOUS, any lz_impl but ZGPU_LZ_AUTO, two wrappers, n >= 2^32.  The sort's self-check stays: a raised fault word makes the call redo itself with the exact sort.
 * Rates (profiles/r10_streams_table.txt, level 6, zlib wrapper, device-resident), the one-by-one loop of continuous streams over this call: 7.1 for 256 items of
 * 1 MiB (334 ms against 47), 11.7 for 4,096 items of 96 KiB (5.2 s against 0.45 s), 1.3 for 16 items of 64 MiB (80 ms against 60). */
uint64_t zgpu_deflate_streams_bound(uint64_t item_bytes, uint32_t flags);
int zgpu_deflate_streams_layout(const uint64_t *in_offsets, uint64_t n, uint32_t flags, uint64_t *out_offsets, uint64_t *total);
int zgpu_deflate_streams_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, const zgpu_deflate_params *p,
                                void *d_out, uint64_t out_cap, const uint64_t *d_out_offsets, zgpu_deflate_batch_item *d_items, zgpu_deflate_result *res,
                                void *hip_stream);
int zgpu_deflate_streams_host(zgpu_engine *e, const void *in, const uint64_t *in_offsets, uint64_t n, const zgpu_deflate_params *p, void *out, uint64_t out_cap,
                              uint64_t *out_offsets, zgpu_deflate_batch_item *items, zgpu_deflate_result *res);

/* ---- the same, stream-ordered: items of ANY length compressed on the caller's stream (zlib_amd/csrc/zgpu_deflate_streams_enqueue.hip) ----
 * zgpu_deflate_streams_enqueue makes exactly what zgpu_deflate_streams_device makes -- item k = d_in[io[k] .. io[k+1]), 0 to below 2^32 bytes, becomes the
 * same bytes in its room d_out[oo[k] .. oo[k+1]), with the same record -- as ONE chain of kernel launches on hip_stream (null: the engine's), and returns.
 * The contract is that of zgpu_deflate_batch_enqueue above, word for word: the call does not synchronize, allocate, copy to or from host memory, record an
 * event, use a second stream or time anything, and uses no device memory of the engine's.  The scratch is d_ws: 256-byte aligned, at least
 * zgpu_deflate_streams_workspace_bytes(n, in_bytes, batch_tiles) bytes, a function of those three numbers alone (never of the level or the wrapper) that
 * needs no engine and no GPU.  Two calls with different workspaces may be in flight on two streams of one engine; a call can wait behind the kernel that
 * makes its input; it can be captured into a graph, though not as the first call of a process (code objects load, and two kernels' attributes are set, on
 * first use).  Served and refused parameters are zgpu_deflate_streams_device's: levels 4..9, all five strategies, one wrapper at most, ZGPU_F_CRC32,
 * zgpu_deflate_set_tuning, ZGPU_F_FINAL required; ZGPU_STREAM_ERROR with nothing enqueued for the rest, and for what the host can judge of the arguments:
 * a null pointer that is needed, n >= 2^32, d_out not 4-byte aligned, d_ws not 256-byte aligned, ws_bytes too small.  n == 0 enqueues at most the launch
 * that clears the summary.
 * The plan is made on the device.  The host knows neither the items' sizes nor the number of tiles; it lays the tile list out for
 * ntiles_max = in_bytes / 32512 + n tiles (a stream of L bytes has at most L / 32512 + 1) and enqueues ceil(ntiles_max / batch_tiles) rounds of launches;
 * rows behind the real tiles are padding, for which every kernel leaves at its top.  batch_tiles = tiles per round: 0 selects 2,048, more than 32,768 is
 * 32,768, and a round is never larger than ntiles_max.  A tile of a round costs 2,110,800 bytes of workspace (the sorted buckets 1,058,832, tokens
 * 262,144, the streams' compact tokens 327,680, seven block slots 460,544, the rest 1,600); besides that the call needs 92 bytes an item and 46 per tile
 * of ntiles_max.  The seven scans around block construction run as seven launches per round over all streams of the round.
 * The host never sees the tables, so a bad entry fails its item, not the call: ZGPU_STREAM_ERROR, out_bytes = in_bytes = 0, adler32 = 1, crc32 = 0,
 * data_type = 2 for an item whose input range runs backwards or leaves in_bytes, whose room runs backwards, leaves out_cap or does not start at a
 * multiple of 4 (all counted in nbad_offsets), or that is 4 GiB or longer (ntoo_long).  Such an item has no tiles, reads nothing and writes nothing, and
 * every other item is served as if it were not there.  Input ranges may overlap; when they ask for more than ntiles_max tiles, the items whose last
 * tile -- counted over all items with good entries in table order -- lies behind ntiles_max fail as bad entries.  A room too small is ZGPU_BUF_ERROR
 * with out_bytes = 0, as in the blocking call.
 * Summary (optional): nfailed = records that are not ZGPU_OK, nbad_offsets, ntoo_long, total = the sum of out_bytes, overflow = 0, sort_fault as for
 * zgpu_deflate_batch_enqueue: the fault word lies in d_ws, is cleared at the head and read by the last launch; raised, every record has code =
 * ZGPU_ERRNO and the caller answers with zgpu_engine_set_exact_sort and enqueues again.
 * Rooms without the host knowing the sizes: zgpu_deflate_streams_rooms_bound(n, in_bytes, flags) is a closed form that is at least
 * zgpu_deflate_streams_layout's total for every table of n items that runs forward and ends inside in_bytes (equal for one item of in_bytes), and
 * zgpu_deflate_streams_layout_enqueue writes d_out_offsets[0..n] on the device: rooms of zgpu_deflate_streams_bound each -- for a good table exactly what
 * zgpu_deflate_streams_layout gives -- and a room of 0 for an entry that runs backwards or leaves in_bytes.
 * Not served here: levels 0..3, a packed-output entry, preset dictionaries. */
uint64_t zgpu_deflate_streams_workspace_bytes(uint64_t n, uint64_t in_bytes, uint32_t batch_tiles); /* 0: n >= 2^32 */
uint64_t zgpu_deflate_streams_rooms_bound(uint64_t n, uint64_t in_bytes, uint32_t flags);
int zgpu_deflate_streams_layout_enqueue(zgpu_engine *e, const uint64_t *d_in_offsets, uint64_t n, uint64_t in_bytes, uint32_t flags, uint64_t *d_out_offsets,
                                        void *hip_stream);
int zgpu_deflate_streams_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, const zgpu_deflate_params *p,
                                 void *d_out, uint64_t out_cap, const uint64_t *d_out_offsets, zgpu_deflate_batch_item *d_items,
                                 zgpu_deflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes, uint32_t batch_tiles, void *hip_stream);

/* ---- BGZF: blocked gzip, the container of bgzip, BAM, tabix and .vcf.gz (RFC 1952 + SAM specification 4.1) ----
 * A file is gzip members laid end to end, each at most 64 KiB long and decoding to at most 64 KiB, each carrying its own total length in its header
 * (BSIZE in the 'B' 'C' extra subfield), closed by a fixed 28-byte empty block.
 * Encode: the input is cut every block_size bytes (0 selects 65280, which is also the most), every piece becomes one block whose body is what
 * deflateInit2(level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) + deflate(Z_FINISH) of the piece emits (the segments path with ZGPU_F_BGZF_WRAP), and the
 * end block is appended; empty input gives the end block alone.  level 1..9 (the segment engine has no level 0: stored blocks are not written here),
 * strategy as in zgpu_deflate_params.  out_offsets (optional; nblocks + 2 entries, device memory for the device entry): where every block begins, where
 * the end block begins, the file's length.  res->nchunks = nblocks (the end block not counted), res->crc32 / adler32 cover the whole input.
 * Out of scope: level 0, preset dictionaries, htslib's .gzi file I/O (the two arrays of
 * zgpu_bgzf_index_device hold its content; writing the file of 8-byte pairs is a caller's loop), BAM / VCF record awareness.  General multi-member
 * gzip, whose members carry no size, is zgpu_gzip_inflate_* below. */
uint64_t zgpu_bgzf_bound(uint64_t in_bytes, uint32_t block_size); /* output capacity that is enough */
int zgpu_bgzf_deflate_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, int level, int strategy, uint32_t block_size, void *d_out, uint64_t out_cap,
                             uint64_t *d_out_offsets, zgpu_deflate_result *res, void *hip_stream);
int zgpu_bgzf_deflate_host(zgpu_engine *e, const void *in, uint64_t in_bytes, int level, int strategy, uint32_t block_size, void *out, uint64_t out_cap,
                           uint64_t *out_offsets, zgpu_deflate_result *res);
/* One chunk with a preset dictionary (deflateSetDictionary, qcsrc/deflate.c:315-354).  `window` holds the dictionary bytes the
 * reference copies into its window -- the last min(length, 32506) bytes of the dictionary, at least 3 -- followed by the data;
 * window_bytes <= 65536.  Output: the raw deflate stream of the data alone, exactly what the reference's fresh stream emits
 * after deflateSetDictionary when it is finished (ZGPU_F_FINAL) or full-flushed; ZGPU_F_CRC32 as usual.  result.adler32 /
 * crc32 / data_type describe the data alone.  (One lane works on one chunk here: meant for the first chunk of a stream.) */
int zgpu_deflate_dict_chunk_host(zgpu_engine *e, const void *window, uint32_t window_bytes, uint32_t dict_bytes,
                                 const zgpu_deflate_params *p, void *out, uint64_t out_cap, zgpu_deflate_result *res);

/* ---- inflate ---- */
/* Segment k = d_in[offsets[k] .. offsets[k+1]) is a raw-deflate segment that decodes to at most
 * chunk_size bytes, written at d_out + k*chunk_size (every segment but the last must decode to exactly
 * chunk_size bytes).  chunk_size == 0 selects "compact" mode: segments of any size up to 65536 bytes are
 * decoded and their outputs concatenated (streams that were flushed in the middle of a chunk).  The last
 * segment must end with a final block; the others end with a stored empty block (flush marker).
 * chunk_size == ZGPU_WHOLE_STREAM with nchunks == 1: the one segment is a complete raw-deflate stream of any size
 * (< 512 MiB compressed, < 4 GiB decoded) that was not produced in chunks; one workgroup decodes it from end to end
 * (inflate.c:773-1076 + inffast.c:67-302 as they run for any stream).  When out_cap is too small the call returns
 * ZGPU_BUF_ERROR with res->out_bytes = the size the stream decodes to. */
#define ZGPU_WHOLE_STREAM 0xFFFFFFFFu
int zgpu_inflate_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_chunk_offsets,
                        uint64_t nchunks, uint32_t chunk_size, void *d_out, uint64_t out_cap,
                        zgpu_inflate_result *res, void *hip_stream);
int zgpu_inflate_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *chunk_offsets,
                      uint64_t nchunks, uint32_t chunk_size, void *out, uint64_t out_cap, zgpu_inflate_result *res);
/* Find the chunk boundaries of a mode-B stream that carries no side table: scans for the
 * 00 00 FF FF flush markers on the device and validates the split by decoding.
 * offsets (host, capacity max_chunks+1) receives the boundaries relative to in (raw body, no zlib
 * header).  Returns ZGPU_OK and *nchunks, or ZGPU_DATA_ERROR when no consistent split exists. */
int zgpu_inflate_find_chunks_host(zgpu_engine *e, const void *in, uint64_t in_bytes, uint32_t chunk_size,
                                  uint64_t *offsets, uint64_t max_chunks, uint64_t *nchunks);
/* The same search, delivering the decoded bytes: raw deflate body in (no zlib header / trailer), bytes out.  A body
 * that does not split into independent segments (any other producer's stream) is decoded in pieces found by search (see
 * zgpu_inflate_spec_count below) or, failing that, as ZGPU_WHOLE_STREAM. */
int zgpu_inflate_stream_host(zgpu_engine *e, const void *in, uint64_t in_bytes, void *out, uint64_t out_cap,
                             zgpu_inflate_result *res);
/* The same for the REST OF A STREAM (flags = ZGPU_INF_STREAM): `in` starts at a block boundary and may reach beyond the end of the
 * deflate data -- trailers, further members, anything.  The stream ends with its final block (res->stream_end, res->in_used =
 * offset of the first byte behind it); input that stops inside a block is not an error: the call delivers the full-flush
 * segments in front of the incomplete one (res->incomplete, res->in_used, res->out_bytes; all three can be 0) and is repeated from
 * in + in_used when more has arrived.  This is what inflate() of the zlib API needs (qcsrc/inflate.c:1114: DONE leaves the rest of
 * the input with the caller).  flags = 0 is zgpu_inflate_stream_host. */
#define ZGPU_INF_STREAM 1u
int zgpu_inflate_stream_host2(zgpu_engine *e, const void *in, uint64_t in_bytes, uint32_t flags, void *out, uint64_t out_cap,
                              zgpu_inflate_result *res);
/* The same for a stream that is taken up again INSIDE a byte: a stream of another producer that carries no flush markers is delivered piece by
 * piece as it arrives (qcsrc/inflate.c:323-371: the reference's inflate() hands output on with 32 KiB of window kept; here the caller keeps the
 * last 32 KiB it received and gives them to zgpu_inflate_set_dictionary before the next call).  A call whose input stops inside a block returns
 * the whole pieces in front of it (res->incomplete, res->out_bytes) and where they end: byte res->in_used, bit res->in_used_bits -- the next call
 * passes in + in_used and start_bit = in_used_bits.  start_bit 0 is zgpu_inflate_stream_host2. */
int zgpu_inflate_stream_host3(zgpu_engine *e, const void *in, uint64_t in_bytes, uint32_t start_bit, uint32_t flags, void *out, uint64_t out_cap,
                              zgpu_inflate_result *res);
/* A body that does not split at flush markers and holds at least 128 KiB (ZGPU_SPEC_MIN_BYTES) is decoded in pieces all the same: block starts
 * are searched behind every 1/4096 of the input (at least 32 KiB apart), every piece is decoded with the 32 KiB in front of it unknown,
 * the chain of pieces is checked and the unknowns filled in afterwards (zgpu_inflate_stream.hip, spec_*).  A stream whose pieces do
 * not chain -- damaged, cut short, or one false block start -- goes through the one-workgroup decoder and gets its verdict.
 * Diagnostics: how many streams this process decoded in pieces / sent to the one-workgroup decoder. */
/* Test hook: the next launch of the fast position sort reports that its self-check failed (the LDS did not serve an atomic's lanes in
 * lane order), so that the engine's fallback -- redo the call with the ballot-ranked sort, and keep to it -- can be exercised. */
void zgpu_debug_inject_sort_fault(void);
uint64_t zgpu_inflate_spec_count(int which); /* 0: decoded in pieces, 1: one-workgroup decodes (both: zgpu_inflate_stream_host*);
                                              * 2: long items of blocking batch decodes decoded in pieces, 3: long items of them that fell back
                                              * to the one-workgroup decoder (zgpu_inflate_batch_*, see there); 4: long items of sizing passes
                                              * sized in pieces, 5: long items of them that fell back to the one-wave sizing kernel
                                              * (zgpu_inflate_batch_sizes_*, the sizing half of zgpu_inflate_batch_packed_*); 6: long items of
                                              * blocking integrity tests verified in pieces, 7: long items of them that fell back to the
                                              * one-workgroup verifier (zgpu_inflate_batch_verify_host / _device) */
const char *zgpu_inflate_message(uint32_t index);
/* Preset dictionary of the inflate calls that follow (inflateSetDictionary, qcsrc/inflate.c:1200-1236): the first segment of a
 * call may reach back into its last min(len, 32768) bytes.  Stays set until replaced; len 0 clears it. */
int zgpu_inflate_set_dictionary(zgpu_engine *e, const void *dict, uint32_t len);
/* Which checks of the decoded bytes the inflate calls that follow compute into zgpu_inflate_result: ZGPU_CHECK_ADLER32 (what a zlib
 * stream's trailer holds, qcsrc/inflate.c:1083-1094), ZGPU_CHECK_CRC32 (a gzip member's), both (the default) or none (raw deflate:
 * inflate() keeps no check there, inflate.c:862-866).  A check that is not computed reads adler32 = 1 / crc32 = 0.  Each one is a pass
 * over the output (0.7 and 2.5 ms per 4 GiB).  Stays set until replaced. */
#define ZGPU_CHECK_ADLER32 1u
#define ZGPU_CHECK_CRC32 2u
int zgpu_inflate_set_checks(zgpu_engine *e, uint32_t mask);

/* ---- batch inflate: many independent streams in one call ----
 * Item k is the stream d_in[d_in_offsets[k] .. d_in_offsets[k+1]), decoded to d_out[d_out_offsets[k] .. d_out_offsets[k+1]); every item is a
 * stream of its own and gets its own record in d_items[k].  wrap says what the items carry, as inflateInit2's windowBits does
 * (qcsrc/inflate.c:589-760): ZGPU_WRAP_RAW -15, ZGPU_WRAP_ZLIB 15, ZGPU_WRAP_GZIP 31, ZGPU_WRAP_AUTO 47 (zlib or gzip by the magic).  An item must
 * reach its final block; what follows its trailer (or, raw, its final block) is left alone.  Limits per item: < 512 MiB compressed, < 4 GiB
 * decoded (an item past them gets ZGPU_DATA_ERROR with "segment table out of range" / "segment decodes to more than chunk_size bytes").  No preset dictionary (zgpu_inflate_set_dictionary does not apply); multi-member gzip items decode their first member (a whole multi-member file: zgpu_gzip_inflate_* below).
 * Record of item k:
 *   code       ZGPU_OK, ZGPU_DATA_ERROR, ZGPU_BUF_ERROR (out_bytes = the size that would have been needed) or 2 (Z_NEED_DICT: FDICT set)
 *   msg        index for zgpu_inflate_message() (the reference's text for a header or trailer failure)
 *   out_bytes  decoded size
 *   in_used    input bytes up to the end of the trailer (raw: of the final block)
 *   adler32 / crc32  of the decoded bytes: checks takes ZGPU_CHECK_* bits; the check the wrapper needs is always computed (AUTO: both); a check
 *              that is not computed reads adler32 = 1 / crc32 = 0.
 * The call fails only for bad arguments (offsets that run backwards or leave their buffer), allocation or HIP errors; *nfailed (optional)
 * receives the number of items whose code is not ZGPU_OK.  The device entry blocks until the records are in d_items.
 * Long items: an item whose deflate data (the item behind its header) has ZGPU_BATCH_PIECES_MIN_BYTES bytes or more -- an environment variable read at
 * every call, 131072 unless set, 0: no item -- is not decoded by one workgroup from end to end but in pieces that start at block boundaries found by
 * search, the pieces of all long items of the call in shared launches (zlib_amd/csrc/zgpu_inflate_batch_pieces.hip).  Records and bytes are those of the
 * one-workgroup decoder: a long item whose pieces do not chain cleanly into its room (damage, truncation, a room too small) is decoded again by it,
 * once.  ZGPU_BATCH_PIECES_ROUND_BYTES (default 512 MiB) caps the output room one round of the piece path serves; scratch the engine cannot reserve
 * sends a round's items to the one-workgroup decoder and is no error.  This covers the blocking decode (these two calls, the decode half of
 * zgpu_inflate_batch_packed_*, zgpu_bgzf_*, the final decode of zgpu_gzip_inflate_*) and, in a form of its own, the blocking sizing pass (see
 * zgpu_inflate_batch_sizes_* below) and the blocking integrity test (zgpu_inflate_batch_verify_* further down): the *_enqueue calls give every item to
 * one workgroup as before.
 * zgpu_inflate_spec_count(2) / (3) count the long items decoded in pieces / fallen back -- the decode only, also inside a packed call. */
#define ZGPU_WRAP_RAW 0
#define ZGPU_WRAP_ZLIB 1
#define ZGPU_WRAP_GZIP 2
#define ZGPU_WRAP_AUTO 3
typedef struct {
    int32_t code;
    uint32_t msg;
    uint64_t out_bytes;
    uint64_t in_used;
    uint32_t adler32, crc32;
} zgpu_inflate_item;
int zgpu_inflate_batch_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap,
                              uint32_t checks, void *d_out, uint64_t out_cap, const uint64_t *d_out_offsets, zgpu_inflate_item *d_items,
                              uint64_t *nfailed, void *hip_stream);
/* The same with host arrays.  Only the decoded bytes of the items that succeed are written to out. */
int zgpu_inflate_batch_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *in_offsets, uint64_t n, int wrap,
                            uint32_t checks, void *out, uint64_t out_cap, const uint64_t *out_offsets, zgpu_inflate_item *items,
                            uint64_t *nfailed);

/* ---- batch inflate without known sizes: the sizing pass and the packed decode ----
 * A zlib or raw-deflate stream carries no decoded size, and a gzip ISIZE is a claim modulo 2^32.  The sizing pass reads every item the way the batch
 * decoder reads it -- the same wrapper rules, the same deflate decoder -- and counts the bytes its symbols stand for instead of producing them: no
 * destination is needed, none is touched.  Record k: code ZGPU_OK, ZGPU_DATA_ERROR or 2 (FDICT); msg the index zgpu_inflate_batch_* gives the same
 * item; out_bytes the decoded size; in_used the end of the final block plus the wrapper's trailer length (an item that ends inside its trailer is
 * "segment ends inside a block", as in the decoder); adler32 = 1, crc32 = 0.  A failed item has out_bytes = in_used = 0.
 * What it cannot say: it computes no Adler-32 or CRC-32 and compares no ISIZE -- its verdict is the decoder's minus the trailer checks.  An item
 * whose check value or length field is wrong is ZGPU_OK here and ZGPU_DATA_ERROR ("incorrect data check" / "incorrect length check") in a decode.
 * Arguments, limits (< 512 MiB compressed, < 4 GiB decoded per item, no preset dictionary), ZGPU_STREAM_ERROR for offsets that run backwards or
 * leave the buffer and *nfailed are zgpu_inflate_batch_*'s.  One read-back, at the end; the device entry blocks until the records are in d_items.
 * Long items are sized in pieces too (these two calls and the sizing half of zgpu_inflate_batch_packed_*; not zgpu_inflate_batch_sizes_enqueue): a
 * piece that starts at a block boundary is counted by one wave with no knowledge of what lies in front of it, and a chain over the item's pieces
 * settles what a piece cannot -- that each ended where the next starts, the total, and that no match of a later piece reaches in front of the item's
 * first byte.  An item that does not come out clean is sized again by the one-wave kernel, once: every record is the one-wave kernel's.  The threshold
 * is ZGPU_BATCH_PIECES_SIZES_MIN_BYTES, read at every call; not set, it follows ZGPU_BATCH_PIECES_MIN_BYTES (131072; 0: no item is long).
 * ZGPU_BATCH_PIECES_SIZES_ROUND_SLOTS caps the piece slots of one round (not set: no cap; the tests' switch); ZGPU_BATCH_PIECES_ROUND_BYTES has no
 * meaning here, sizing has no rooms.  A call without long items pays 104 bytes more of the read-back it makes anyway, nothing else; one with long
 * items a second read-back.  zgpu_inflate_spec_count(4) / (5) count the long items sized in pieces / fallen back. */
int zgpu_inflate_batch_sizes_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap,
                                    zgpu_inflate_item *d_items, uint64_t *nfailed, void *hip_stream);
int zgpu_inflate_batch_sizes_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *in_offsets, uint64_t n, int wrap,
                                  zgpu_inflate_item *items, uint64_t *nfailed);
/* The packed decode: the sizing pass, the layout made on the device, then zgpu_inflate_batch_* into that layout.  d_out_offsets (out, n + 1 entries):
 * item k starts at the sizes in front of it, every start rounded up to `align` (a power of two from 1 to 256, else ZGPU_STREAM_ERROR);
 * d_out_offsets[n] = *total = the end of the last item.  An item whose sizing failed has an empty range and keeps the sizing pass's record; the
 * records of the others are the decoder's (adler32 / crc32 as `checks` asks, trailer mismatches reported as in zgpu_inflate_batch_*).
 * *total > out_cap: ZGPU_BUF_ERROR -- *total and d_out_offsets are written, d_items holds the sizing records, nothing is decoded; allocate and call
 * zgpu_inflate_batch_* with that table.  n == 0: ZGPU_OK, *total = 0.  The host entry writes only the bytes of the items that succeed. */
int zgpu_inflate_batch_packed_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap,
                                     uint32_t checks, uint32_t align, void *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                                     zgpu_inflate_item *d_items, uint64_t *total, uint64_t *nfailed, void *hip_stream);
int zgpu_inflate_batch_packed_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *in_offsets, uint64_t n, int wrap,
                                   uint32_t checks, uint32_t align, void *out, uint64_t out_cap, uint64_t *out_offsets, zgpu_inflate_item *items,
                                   uint64_t *total, uint64_t *nfailed);

/* ---- batch integrity test: are these streams intact?  No destination ----
 * Every item is decoded in full -- the same wrapper rules, the same deflate decoder, every match copied -- inside a 32 KiB ring in the workgroup's
 * LDS, and where the decoder would flush a half of the ring to memory the bytes go into the item's running Adler-32 / CRC-32 instead.  The trailer is
 * then compared as zgpu_inflate_batch_* compares it.  No decoded byte is written to device memory or read from it: the call needs the input, 144 bytes
 * of scratch per item and -- where items are long, see below -- a piece scratch bounded by a slot cap, whatever the items decode to (gzip -t, unzip -t, bgzip -t, a scrubber, a pack-file fsck).
 * Record k equals, field for field, the record zgpu_inflate_batch_* gives the same item with the same `checks` and an output range of exactly the
 * right size: code (ZGPU_OK, ZGPU_DATA_ERROR or 2 for FDICT; ZGPU_BUF_ERROR cannot occur), msg ("incorrect data check", "incorrect length check", a
 * trailer that does not fit as "segment ends inside a block", every decoder message), out_bytes, in_used, adler32 and crc32 (the check the wrapper
 * needs is always computed, AUTO: both; the others as `checks` asks; one that is not computed reads 1 / 0).  A failed item has out_bytes = in_used = 0.
 * What it does not promise: speed over a decode -- it does all the decoder's work but the stores; its claim is memory.  Arguments, limits (< 512 MiB
 * compressed, < 4 GiB decoded per item, no preset dictionary, a multi-member gzip item is its first member), ZGPU_STREAM_ERROR for offsets that run
 * backwards or leave the buffer, *nfailed and n == 0 are zgpu_inflate_batch_sizes_*'s.  One read-back, at the end; the device entry blocks until the
 * records are in d_items.
 * Long items are checked in pieces (these two calls and what stands on them: zamd_uncompress_verify_batch, zamd_unzip_test_batch; not
 * zgpu_inflate_batch_verify_enqueue, where no host sees the items' sizes, and not zgpu_bgzf_verify_*, whose blocks are never long).  Check values need
 * every byte, in order, with the real 32 KiB in front of every piece, and the call has no room for a decoded byte: the pieces are decoded twice, both
 * times inside LDS.  A first pass leaves per piece slot its tail -- the last 32 Ki symbols, as the decode in pieces keeps them -- and where it ended; a chain
 * over the item's pieces and the window kernels turn the tails into the real 32 KiB behind every piece; a second pass decodes every piece again behind
 * the window of the piece in front, folds its bytes as the one-workgroup verifier does, and finds a distance that reaches in front of the item exactly.
 * The pieces' Adler-32 / CRC-32 are joined in order into the item's, and the trailer is compared by the code that compares every trailer: a long item
 * with a wrong Adler-32, CRC-32 or ISIZE stays in pieces.  An item that does not come out clean (damage, a cut item, a false start, a reach in front of
 * the item, more than 4 GiB) is verified again by one workgroup, once: every record is the one-workgroup verifier's.  Memory: a slot costs its tail
 * (64 KiB), its window (32 KiB) and under 128 bytes of records, and rounds are cut under ZGPU_BATCH_PIECES_VERIFY_ROUND_SLOTS slots (default 1024: one
 * residency of the second pass, about 96 MiB of scratch) -- an item with more slots makes a round of its own --, so the scratch depends neither on what
 * the items decode to nor on their number.  The threshold is ZGPU_BATCH_PIECES_VERIFY_MIN_BYTES, read at every call; not set, it follows
 * ZGPU_BATCH_PIECES_MIN_BYTES where that is set; neither set, it is 20000000 -- measured (profiles/r14_batch_verify_long_table.txt): two passes over every
 * piece lose to one workgroup per item on 256 items of 1 MiB and win 2.59 times on 16 items of 64 MiB, whose bodies are that long; 0: every item to one
 * workgroup.  An input that is not 16-byte aligned or shorter than the threshold never enters
 * the path; scratch the engine cannot reserve sends a round's items to the one-workgroup verifier and is no error.  A call without long items pays 104
 * bytes more of the read-back it makes anyway, nothing else; one with long items a second read-back.  zgpu_inflate_spec_count(6) / (7) count the long
 * items verified in pieces / fallen back; the decode's and the sizing pass's counters do not move in a verify call. */
int zgpu_inflate_batch_verify_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap,
                                     uint32_t checks, zgpu_inflate_item *d_items, uint64_t *nfailed, void *hip_stream);
int zgpu_inflate_batch_verify_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *in_offsets, uint64_t n, int wrap,
                                   uint32_t checks, zgpu_inflate_item *items, uint64_t *nfailed);

/* ---- stream-ordered batch inflate: the four jobs above, enqueued ----
 * For a caller whose data lives on the GPU.  A call puts hipMemsetAsync and kernel launches on hip_stream (null: the engine's stream) as ONE chain and
 * returns; it does not synchronize, allocate, copy to or from host memory, record an event, use a second stream or time anything, and it uses no device
 * memory of the engine's: its scratch is d_ws, device memory of the caller's, 256-byte aligned, of at least
 * zgpu_inflate_batch_workspace_bytes(job, n) bytes (a function of n alone -- never of out_cap or of what the items decode to; it needs no engine and no
 * GPU).  The engine supplies the device and the error text, nothing else: two calls with different workspaces may be in flight on different streams of
 * one engine, a call can wait in a stream behind the copy that brings its input, and it can be captured into a graph (not the first call of a
 * process: that one loads the code).  d_in, the offset tables, d_out, d_items, d_summary and d_ws are read and written in stream order: they must be
 * valid when the work runs, and stay untouched by other streams until it is done; the results are there when the stream has reached that point.
 * Arguments the host can judge -- a null pointer that is needed, wrap, checks or align out of range, n >= 2^32, ws_bytes too small, d_ws not 256-byte
 * aligned -- return ZGPU_STREAM_ERROR at once with nothing enqueued.  n == 0 enqueues at most the summary's memset.
 * d_items[k] is, field for field, the record the blocking entry point of the same job gives item k with the same arguments.  What differs: offsets that
 * run backwards or leave their buffer do not fail the call (the host never sees them).  Such an item reads and writes nothing and gets
 * code = ZGPU_STREAM_ERROR, msg = 0, out_bytes = in_used = 0, adler32 = 1, crc32 = 0; it counts in nfailed and in nbad_offsets, and every other item is
 * served as if it were not there.
 * d_summary (optional, device memory): nfailed = items whose code is not ZGPU_OK; nbad_offsets; packed only: total = d_out_offsets[n], and
 * overflow = 1 when total > out_cap -- then, as ZGPU_BUF_ERROR of the blocking call, d_out_offsets and total are written, d_items holds the sizing
 * records and no decoded byte is written (the decode stage's items are emptied on the device; there is no second sizing pass).
 * The decode and the packed decode run the decoder in a mode of its own: every item through the ring of its workgroup (the ring the blocking decode
 * picks), its Adler-32 / CRC-32 folded out of the ring in the flush that stores the bytes, so no pass reads the output again and no count has to
 * reach the host.  Rates (profiles/r08_batch_enqueue_table.txt, level 6, device-resident): 200 batches of 64 items of 4 KiB, 151 us a batch against
 * 207 us through 200 blocking calls; one large batch takes what the blocking call takes (enqueue / blocking 0.95 to 1.01 over both shapes and rings). */
#define ZGPU_BATCH_JOB_DECODE 0
#define ZGPU_BATCH_JOB_SIZES 1
#define ZGPU_BATCH_JOB_VERIFY 2
#define ZGPU_BATCH_JOB_PACKED 3
typedef struct {
    uint64_t nfailed, nbad_offsets, total;
    uint32_t overflow, reserved;
} zgpu_inflate_batch_summary;
uint64_t zgpu_inflate_batch_workspace_bytes(int job, uint64_t n); /* 0: no such job, or n >= 2^32 */
int zgpu_inflate_batch_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap,
                               uint32_t checks, void *d_out, uint64_t out_cap, const uint64_t *d_out_offsets, zgpu_inflate_item *d_items,
                               zgpu_inflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes, void *hip_stream);
int zgpu_inflate_batch_sizes_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap,
                                     zgpu_inflate_item *d_items, zgpu_inflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes,
                                     void *hip_stream);
int zgpu_inflate_batch_verify_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap,
                                      uint32_t checks, zgpu_inflate_item *d_items, zgpu_inflate_batch_summary *d_summary, void *d_ws,
                                      uint64_t ws_bytes, void *hip_stream);
int zgpu_inflate_batch_packed_enqueue(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_in_offsets, uint64_t n, int wrap,
                                      uint32_t checks, uint32_t align, void *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                                      zgpu_inflate_item *d_items, zgpu_inflate_batch_summary *d_summary, void *d_ws, uint64_t ws_bytes,
                                      void *hip_stream);

/* ---- BGZF decode (the encode side and the format: zgpu_bgzf_deflate_* above) ---- */
/* The block index of a BGZF file in device memory, found on the device from the headers alone (zlib_amd/csrc/zgpu_bgzf.hip): d_in_offsets[0..n] =
 * where every block begins, entry n = in_bytes; d_out_offsets[0..n] = the exclusive sum of the blocks' ISIZE (entry n = *out_bytes).  Both arrays
 * (device memory, cap_blocks + 1 entries each) are what a .gzi index holds and are the tables zgpu_inflate_batch_device(..., ZGPU_WRAP_GZIP, ...)
 * takes.  cap_blocks too small: ZGPU_BUF_ERROR with *nblocks = the number of blocks (nothing written).  The file is valid only if its blocks chain
 * from byte 0 to exactly in_bytes: bad magic at a chain position, no 'B' 'C' subfield there, a block that leaves the buffer or is shorter than its own
 * frame (header, two bytes of deflate data, trailer), trailing bytes or an ISIZE above 65536 give ZGPU_DATA_ERROR (zgpu_engine_error(): "invalid BGZF block chain", also in zgpu_inflate_message()).
 * Empty blocks in the middle (concatenated files) are ordinary blocks; a file without the end block is valid, *ends_with_eof_block says which it is.
 * An empty buffer is a valid file of no blocks.  Blocks until the tables are written. */
int zgpu_bgzf_index_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, uint64_t *d_in_offsets, uint64_t *d_out_offsets, uint64_t cap_blocks,
                           uint64_t *nblocks, uint64_t *out_bytes, uint32_t *ends_with_eof_block, void *hip_stream);
/* Decode a whole BGZF file: the index above, then every block as one item of the batch decoder (ZGPU_WRAP_GZIP: CRC-32 and ISIZE of every block are
 * checked on the device).  res->out_bytes = the sum of ISIZE; out_cap too small: ZGPU_BUF_ERROR with res->out_bytes = the size needed, nothing decoded.
 * items (optional; one record per block, the end block included; device memory for the device entry, room for as many blocks as the file can hold --
 * in_bytes / 28 records are always enough: a block is 12 bytes of header, an extra field of 6 at least, a deflate body of 2 at least and 8 of trailer,
 * and what is shorter is no block -- or for the count zgpu_bgzf_index_device gave): each block's own verdict.  A block that decodes to more than its ISIZE
 * is a ZGPU_DATA_ERROR ("incorrect length check") of that block, as is one whose deflate data ends in front of its trailer.  When a block fails the call
 * returns ZGPU_DATA_ERROR with res->first_bad_chunk / error_code / error_msg describing the first such block; every other block's bytes are in place.
 * A file whose blocks do not chain: ZGPU_DATA_ERROR with first_bad_chunk = -1.  res->adler32 / crc32 are not computed (1 / 0).  The host entry uploads
 * the file once and decodes from there. */
int zgpu_bgzf_inflate_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t out_cap, zgpu_inflate_item *d_items,
                             zgpu_inflate_result *res, void *hip_stream);
int zgpu_bgzf_inflate_host(zgpu_engine *e, const void *in, uint64_t in_bytes, void *out, uint64_t out_cap, zgpu_inflate_item *items, zgpu_inflate_result *res);
/* Test a whole BGZF file (bgzip -t): the index above, then every block as one item of zgpu_inflate_batch_verify_*.  There is no `out` and so no
 * ZGPU_BUF_ERROR; everything else -- the return code, res->out_bytes (the sum of ISIZE), first_bad_chunk / error_code / error_msg, the verdict on a
 * file whose blocks do not chain, the optional per-block records -- is what zgpu_bgzf_inflate_* says of the same file. */
int zgpu_bgzf_verify_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, zgpu_inflate_item *d_items, zgpu_inflate_result *res, void *hip_stream);
int zgpu_bgzf_verify_host(zgpu_engine *e, const void *in, uint64_t in_bytes, zgpu_inflate_item *items, zgpu_inflate_result *res);

/* ---- multi-member gzip (RFC 1952 2.2: `cat a.gz b.gz`, logs appended to one .gz, .warc.gz), all members in one batch (zlib_amd/csrc/zgpu_gzip.hip) ----
 * out receives the members' decoded bytes, concatenated in file order.  Member k reads in[in_offsets[k] .. in_offsets[k+1]) and writes
 * out[out_offsets[k] .. out_offsets[k+1]); items[k] is what zgpu_inflate_batch_* gives for it with ZGPU_WRAP_GZIP (the same header rules, CRC-32 and
 * ISIZE checked on the device, the same message indices).  The three arrays are optional (device memory for the device entry); cap_members is their
 * room: cap_members + 1 entries for the two offset tables, cap_members records.  in_bytes / 20 is always enough (10 bytes of header, 2 of deflate
 * data, 8 of trailer).  More members than cap_members: ZGPU_BUF_ERROR with *nmembers set and nothing written to the arrays.
 * A member's end is known only once it is decoded: every position that looks like a member header (1f 8b 08, no reserved flag bit) is decoded as a
 * candidate, and the members are the candidates that the chain from byte 0 visits -- a signature inside a stored block, even a complete valid member
 * held as payload (a .tar.gz of .gz files), is none.  A file without such payload is decoded once; otherwise the members are decoded a second time
 * into their final places (zgpu_gzip_members_count).  A false candidate costs one wasted decode; the workspace is proportional to the number of
 * candidates, and a file of signatures whose tables cannot be held gives ZGPU_MEM_ERROR.
 *   empty input                  ZGPU_OK, a valid file of no members: *nmembers = 0, res->out_bytes = 0
 *   no member header at byte 0   ZGPU_DATA_ERROR, res->first_bad_chunk = 0, res->error_msg = "incorrect header check" (there is no transparent mode here)
 *   a member that fails          (header, damaged data, input cut short, CRC-32, ISIZE) ZGPU_DATA_ERROR: res->first_bad_chunk its index, res->error_msg
 *                                its message, res->out_bytes the total of the members in front of it, whose bytes are in place, res->in_used where the
 *                                failed member begins, *nmembers the good ones (the arrays describe those; items[*nmembers] is the failed member's
 *                                record when cap_members has room for it).  Nothing behind the failed member is delivered: that is where gzread() stops.
 *   bytes behind the last member that begin no member header (padding, zeros)
 *                                ZGPU_OK, ignored as gzread() ignores them; res->in_used = the end of the last member, in_used < in_bytes tells
 *   out_cap too small            ZGPU_BUF_ERROR, res->out_bytes = the size needed; the contents of out are unspecified
 * Limits per member are a batch item's: < 512 MiB compressed, < 4 GiB decoded (a member of 4 GiB or more, whose ISIZE wraps, is refused).  No preset
 * dictionary.  res->adler32 / crc32 are not computed (1 / 0).  The device entry blocks until the result is known; the host entry uploads the file once. */
int zgpu_gzip_inflate_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, void *d_out, uint64_t out_cap, uint64_t *d_in_offsets, uint64_t *d_out_offsets,
                             zgpu_inflate_item *d_items, uint64_t cap_members, uint64_t *nmembers, zgpu_inflate_result *res, void *hip_stream);
int zgpu_gzip_inflate_host(zgpu_engine *e, const void *in, uint64_t in_bytes, void *out, uint64_t out_cap, uint64_t *in_offsets, uint64_t *out_offsets,
                           zgpu_inflate_item *items, uint64_t cap_members, uint64_t *nmembers, zgpu_inflate_result *res);
uint64_t zgpu_gzip_members_count(int which); /* diagnostics: 0 = calls that decoded every member once, 1 = calls that needed the second decode */

/* ---- checksums (qcsrc/adler32.c:57-149) ---- */
int zgpu_adler32_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, uint32_t *adler_out, void *hip_stream);
/* CRC-32 as crc32() computes it (qcsrc/crc32.c:219-266), chunk CRCs joined like crc32_combine (crc32.c:370-423) */
int zgpu_crc32_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, uint32_t *crc_out, void *hip_stream);

/* ---- batch checksums: many independent items of one buffer in one call (zlib_amd/csrc/zgpu_checksum.hip) ----
 * Item k = in[offsets[k] .. offsets[k+1]): n + 1 nondecreasing offsets, the last at most in_bytes; any size below 4 GiB, any alignment.  checks takes
 * ZGPU_CHECK_* bits; record k holds adler32(1, item) and crc32(0, item) as the reference computes them.  A check that is not asked for reads
 * adler32 = 1 / crc32 = 0, and so does an empty item.  Offsets that run backwards or leave the buffer (or an item of 4 GiB or more) are found on the
 * device before anything is written: ZGPU_STREAM_ERROR, the records untouched.  Items of at most 4096 bytes are served one per wave, sixteen to a
 * workgroup and its CRC table; longer ones in pieces of 64 KiB whose partial results a second launch joins in order.  Blocks until the records are
 * written. */
typedef struct {
    uint32_t adler32, crc32;
} zgpu_check_item;
int zgpu_checksum_batch_device(zgpu_engine *e, const void *d_in, uint64_t in_bytes, const uint64_t *d_offsets, uint64_t n, uint32_t checks,
                               zgpu_check_item *d_items, void *hip_stream);
int zgpu_checksum_batch_host(zgpu_engine *e, const void *in, uint64_t in_bytes, const uint64_t *offsets, uint64_t n, uint32_t checks,
                             zgpu_check_item *items);

/* ---- measurement support ---- */
/* Per-stage device time (HIP events on the launch stream), accumulated while profiling is on. */
enum {
    ZGPU_STAGE_CHAIN = 0, /* hash + static chain links */
    ZGPU_STAGE_MATCH,     /* longest-match search */
    ZGPU_STAGE_PARSE,     /* lazy/greedy parse -> tokens */
    ZGPU_STAGE_LZ_SERIAL, /* serial LZ77 (levels 1-3, or forced) */
    ZGPU_STAGE_HUFFMAN,   /* histogram + tree build + bit emit */
    ZGPU_STAGE_STITCH,    /* size scan + concatenation + Adler-32 */
    ZGPU_STAGE_INFLATE,
    ZGPU_STAGE_COUNT
};
void zgpu_profile_enable(zgpu_engine *e, int on);
void zgpu_profile_reset(zgpu_engine *e);
/* total milliseconds and launch count of one stage since the last reset */
int zgpu_profile_get(zgpu_engine *e, int stage, double *ms, uint64_t *launches);
const char *zgpu_stage_name(int stage);

/* Levels 1-3, one continuous stream: what the rounds of the tile parse did since the engine was made (diagnostic).  Rounds and tile
 * parses are always counted on the host.  The other six are the kernel's own counters of the tiles that were parsed AGAIN, summed over the rounds of
 * every call made while the environment variable ZGPU_FAST_STATS is set (read per call; without it they stay 0 and the kernel counts nothing; the phases
 * of a round 0 parse no tile again and add nothing): with it
 * the 32 bytes come back with the read-back each round already makes.  0 for a null engine or an unknown counter. */
enum {
    ZGPU_FAST_ROUNDS = 0,       /* rounds, over all batches */
    ZGPU_FAST_TILE_PARSES,      /* tiles launched, over all rounds */
    ZGPU_FAST_SAME_ENTRY,       /* parsed again and entered where it had entered last time */
    ZGPU_FAST_STOPPED_EARLY,    /* ... and stopped early: its old results stand */
    ZGPU_FAST_DIFFERENT_TOKEN,  /* ... and met a token that differs from last time's */
    ZGPU_FAST_REACH_TO_END,     /* ... with changed history within reach up to the tile's end */
    ZGPU_FAST_WINDOWS_TO_DIFF,  /* 64-position windows in front of the first different token, summed */
    ZGPU_FAST_WINDOWS_OF_DIFF,  /* windows of the tiles that met one, summed */
    ZGPU_FAST_COUNT_N
};
uint64_t zgpu_deflate_fast_count(zgpu_engine *e, int which);

/* Seeded synthetic corpora of SURVEY.md 8(d), generated in HBM (zlib_amd/csrc/corpus.h).
 * kind 0 silesia-mix, 1 log-text; d_out receives nchunks * 65536 bytes. */
int zgpu_corpus_fill_device(zgpu_engine *e, uint32_t kind, uint64_t seed, uint64_t first_chunk, uint64_t nchunks,
                            void *d_out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
