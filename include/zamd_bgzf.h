/* zamd_bgzf.h -- BGZF, the blocked gzip of bgzip, BAM, tabix and .vcf.gz, zlib style (libzamd_z.so).
 *
 * A BGZF file is gzip members ("blocks") laid end to end, each at most 64 KiB long and decoding to at most 64 KiB, each carrying its own length in
 * its header, closed by a fixed 28-byte empty block (RFC 1952 + SAM specification 4.1).  All blocks of a file are compressed, or decoded, in one
 * call of the engine; a byte range is decoded from the blocks that cover it alone.
 *
 * Return codes: Z_OK, Z_BUF_ERROR (the room is too small, or a range leaves the file), Z_DATA_ERROR (the blocks do not chain from byte 0 to exactly
 * the file's end, or a block is damaged), Z_STREAM_ERROR (bad arguments), Z_MEM_ERROR (no memory, no usable GPU).
 *
 * Out of scope: level 0 (the segment engine writes no stored-only blocks), general multi-member gzip whose members carry no size, preset
 * dictionaries, htslib's .gzi file I/O (zamd_bgzf_index's array holds its content: writing the file of 8-byte pairs is a caller's loop), BAM / VCF
 * record awareness.
 */
#ifndef ZAMD_BGZF_H
#define ZAMD_BGZF_H
#include <stddef.h>
#include "zamd_zlib.h"

#ifdef __cplusplus
extern "C" {
#endif

/* room that is enough for zamd_bgzf_compress of sourceLen bytes */
uLong zamd_bgzf_bound(uLong sourceLen);

/* source cut every 65280 bytes, every piece one block whose body is what deflateInit2(level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) +
 * deflate(Z_FINISH) of the piece emits, and the end block; level 1..9 or Z_DEFAULT_COMPRESSION.  *destLen: in the room, out the file's length. */
int zamd_bgzf_compress(Bytef *dest, uLongf *destLen, const Bytef *source, uLong sourceLen, int level);

/* the whole file; CRC-32 and ISIZE of every block are checked.  *destLen too small: Z_BUF_ERROR with *destLen = the size needed. */
int zamd_bgzf_uncompress(Bytef *dest, uLongf *destLen, const Bytef *source, uLong sourceLen);

/* bgzip -t: the whole file tested, nothing delivered -- every block decoded in the device's local memory, its CRC-32 and ISIZE compared there
 * (zgpu_bgzf_verify_host); no room for the decoded bytes is allocated.  *decodedLen (optional): the decoded size, when the file is good.  Return codes
 * are zamd_bgzf_uncompress's for the same file, without Z_BUF_ERROR; an empty file is Z_OK and creates no engine. */
int zamd_bgzf_test(const Bytef *source, uLong sourceLen, uLongf *decodedLen);

/* The block index, from the headers alone, on the host (no GPU needed): blocks[k] = where block k begins in the file and in the decoded data,
 * k = 0..n-1, and blocks[n] = (sourceLen, the decoded size).  cap: entries `blocks` has room for; when n + 1 > cap the call returns Z_BUF_ERROR with
 * *n set and nothing written (blocks may be NULL then).  *has_eof (optional): the file ends with the 28-byte end block.  Z_DATA_ERROR when the
 * blocks do not chain from byte 0 to exactly sourceLen: bad magic or no 'B' 'C' subfield at a chain position, a block that leaves the buffer or is
 * shorter than its own frame (header, two bytes of deflate data, trailer), trailing bytes, an ISIZE above 65536. */
typedef struct { unsigned long long coffset, uoffset; } zamd_bgzf_block;
int zamd_bgzf_index(const Bytef *source, uLong sourceLen, zamd_bgzf_block *blocks, size_t cap, size_t *n, int *has_eof);

/* dest[0, len) = the decoded bytes [uoffset, uoffset + len): only the blocks that cover the range are decoded, in one call of the engine.
 * blocks, n: what zamd_bgzf_index gave (n + 1 entries).  Z_BUF_ERROR when the range leaves the file. */
int zamd_bgzf_uncompress_range(Bytef *dest, const Bytef *source, uLong sourceLen, const zamd_bgzf_block *blocks, size_t n, unsigned long long uoffset,
                               uLong len);

#ifdef __cplusplus
}
#endif
#endif
