/* zamd_batch.h -- many small independent streams in one call, zlib style (libzamd_z.so).
 *
 * Item k is source[k] (sourceLen[k] bytes) into dest[k] (room destLen[k]); every item is a stream of its own and gets its own verdict in
 * status[k], the code compress2() / uncompress() of this library return for that item alone.  The return value is Z_OK when every item
 * succeeded, else the code of the first item that did not (Z_STREAM_ERROR for bad arguments: then no item was touched).
 */
#ifndef ZAMD_BATCH_H
#define ZAMD_BATCH_H
#include <stddef.h>
#include "zamd_zlib.h"

#ifdef __cplusplus
extern "C" {
#endif

/* windowBits 15: each item becomes what compress2(item, level) gives; 31: a gzip member as deflateInit2(level, Z_DEFLATED, 31, 8,
 * Z_DEFAULT_STRATEGY) + deflate(Z_FINISH) gives it; -15: raw deflate the same way.  status[k]: Z_OK (destLen[k] = the stream's length) or
 * Z_BUF_ERROR when destLen[k] is too small (destLen[k] unchanged).  Items of at most 64 KiB at levels 1-9 are compressed together in one
 * launch of the engine (zgpu_deflate_segments_host).  Larger items at levels 4-9 are compressed together as well, many continuous streams whose
 * tiles share the engine's launches (zgpu_deflate_streams_host; 256 items of 1 MiB at level 6: 54 ms against 364 ms one by one, from host buffers,
 * profiles/r10_streams_table.txt), in calls of at most 1 GiB of input.  Level 0, larger items at levels 1-3 and
 * items of 4 GiB or more are served one by one through compress2() / deflateInit2(), which handle any size.
 * zamd_compress2_batch_count (diagnostic, since the library was loaded): 0 = zgpu_deflate_streams_host calls made, 1 = items served one by one. */
int zamd_compress2_batch(Bytef *const *dest, uLongf *destLen, const Bytef *const *source, const uLong *sourceLen, size_t n, int level,
                         int windowBits, int *status);
unsigned long long zamd_compress2_batch_count(int which);

/* windowBits 15 zlib, 31 gzip, 47 either (by the magic), -15 raw deflate.  status[k] as uncompress() (qcsrc/uncompr.c:50-56) gives it:
 * Z_OK (destLen[k] = the decoded size), Z_BUF_ERROR when destLen[k] is too small, Z_DATA_ERROR for a damaged or truncated stream and for one
 * that needs a preset dictionary.  Items of 512 MiB of input or more are served one by one.  Items of any size below that share the one engine
 * call: one workgroup decodes an item of less than 128 KiB of deflate data, a longer one is decoded in pieces, the pieces of all long items in shared
 * launches (zgpu_inflate_batch_host in zamd_gpu.h; zamd_uncompress_batch_packed's decode and the ZIP batch read likewise).  The sizing pass and the
 * integrity test below take their long items in pieces too, each in a form of its own (the integrity test from 20,000,000 bytes of deflate data): the sizing pass counts the pieces, the integrity test decodes
 * them inside the workgroups' local memory and joins their check values. */
int zamd_uncompress_batch(Bytef *const *dest, uLongf *destLen, const Bytef *const *source, const uLong *sourceLen, size_t n, int windowBits,
                          int *status);

/* When the decoded sizes are not known (a zlib or raw-deflate stream carries none, a gzip ISIZE is a claim modulo 2^32).  windowBits as above.
 *
 * zamd_uncompress_sizes_batch: destLen[k] = the size item k decodes to (0 when it does not); status[k] Z_OK or Z_DATA_ERROR (damaged, truncated,
 * in need of a dictionary).  Nothing is decoded into memory (zgpu_inflate_batch_sizes_host), and so the trailers are not checked: an item whose
 * Adler-32, CRC-32 or ISIZE is wrong is Z_OK here and Z_DATA_ERROR when it is decoded.  Items of 512 MiB of input or more are sized one by one
 * through inflate(), their output discarded (those do have their trailers checked).
 *
 * zamd_uncompress_batch_packed: all items into dest, back to back: item k is dest[destOffsets[k] .. destOffsets[k+1]), destOffsets has n + 1
 * entries.  *destCap in: the room of dest; out: the bytes used, or needed.  status[k] as zamd_uncompress_batch gives it; an item that fails has an
 * empty range.  Z_BUF_ERROR when the room is too small: destOffsets and *destCap are valid (call zamd_uncompress_batch or this again with that
 * much room), status holds the sizing pass's verdicts and nothing is decoded.  One engine call (zgpu_inflate_batch_packed_host) when every item
 * has less than 512 MiB of input; otherwise the large ones are sized and decoded one by one.
 *
 * Both: the return value is the first failing item's code; Z_STREAM_ERROR for bad arguments touches nothing; n == 0 is Z_OK and creates no engine. */
int zamd_uncompress_sizes_batch(uLongf *destLen, const Bytef *const *source, const uLong *sourceLen, size_t n, int windowBits, int *status);
int zamd_uncompress_batch_packed(Bytef *dest, uLongf *destCap, uLong *destOffsets, const Bytef *const *source, const uLong *sourceLen, size_t n,
                                 int windowBits, int *status);

/* The integrity test: are these streams intact?  No destination (gzip -t over many streams, a scrubber, a pack-file fsck).  windowBits as above.
 * status[k] = what zamd_uncompress_batch gives item k with enough room: Z_OK, or Z_DATA_ERROR (damaged, truncated, in need of a dictionary, a wrong
 * Adler-32, CRC-32 or ISIZE -- the trailers ARE checked here).  destLen (optional, may be NULL): destLen[k] = the decoded size, 0 for a failed item.
 * Every item is decoded in full on the device, inside the workgroup's local memory, and its check values are taken there
 * (zgpu_inflate_batch_verify_host): no room for any decoded byte is allocated anywhere.  An item of 20,000,000 bytes of deflate data or more is checked in
 * pieces, the pieces of all long items in shared launches; that costs scratch per piece slot, bounded by a slot cap (about 96 MiB) whatever the items
 * decode to and however many there are.  Items of 512 MiB of input or more go one by one through
 * inflate(), their output discarded.  The return value is the first failing item's code; Z_STREAM_ERROR for bad arguments touches nothing; n == 0
 * is Z_OK and creates no engine. */
int zamd_uncompress_verify_batch(uLongf *destLen, const Bytef *const *source, const uLong *sourceLen, size_t n, int windowBits, int *status);

/* crc32() / adler32() of many buffers, all items in one engine call (zgpu_checksum_batch_host).  crc[k] / adler[k] hold the running value on
 * entry, as the first argument of crc32() / adler32() (0 / 1 for a fresh one), and crc32(crc[k], buf[k], len[k]) / adler32(...) on return: the
 * items' own checksums come from the device, the running values are folded in on the host with crc32_combine / adler32_combine.  Items of any
 * size below 4 GiB.  Z_OK; Z_STREAM_ERROR for bad arguments (a null array with n > 0, a null buffer with a length, an item of 4 GiB or more: nothing
 * is touched); Z_MEM_ERROR when memory or the engine is not to be had.  n == 0 is Z_OK and creates no engine. */
int zamd_crc32_batch(uLong *crc, const Bytef *const *buf, const uLong *len, size_t n);
int zamd_adler32_batch(uLong *adler, const Bytef *const *buf, const uLong *len, size_t n);

#ifdef __cplusplus
}
#endif
#endif
