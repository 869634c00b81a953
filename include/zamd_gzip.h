/* zamd_gzip.h -- multi-member gzip files, zlib style (libzamd_z.so): `cat a.gz b.gz`, logs appended to one .gz, .warc.gz.
 *
 * All members of the file are decoded in one call of the engine (zgpu_gzip_inflate_host, include/zamd_gpu.h), where gzread() and inflate() take one
 * call per member.  A member is what the chain of members from byte 0 visits: a gzip signature inside a stored block is payload, even when a
 * complete valid member follows it.  Bytes behind the last member that begin no member header are ignored, as gzread() ignores them; *sourceUsed
 * says where the last member ended.
 *
 * Out of scope: members of 4 GiB or more (ISIZE wraps) or of 512 MiB or more compressed, preset dictionaries, input that does not begin with a gzip
 * member (no transparent mode).
 */
#ifndef ZAMD_GZIP_H
#define ZAMD_GZIP_H
#include "zamd_zlib.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dest[0, *destLen) = the decoded bytes of all members, in file order; CRC-32 and ISIZE of every member are checked.  *destLen: in the room.
 *   Z_OK            *destLen = the decoded size
 *   Z_BUF_ERROR     *destLen = the size needed
 *   Z_DATA_ERROR    a member failed (or the file does not begin with one): *destLen = the bytes of the good members in front of it, which are in
 *                   dest; *sourceUsed = where the failed member begins
 *   Z_MEM_ERROR     no memory, no usable GPU
 *   Z_STREAM_ERROR  dest or destLen NULL with sourceLen != 0, source NULL with sourceLen != 0
 * sourceLen == 0 is a valid file of no members: Z_OK, *destLen = 0, and no engine is created.  *sourceUsed (optional): where the last good member
 * ends; *members (optional): how many good members there are.  The engine is the one of the zamd_*_batch calls (ZAMD_DEVICE). */
int zamd_gunzip(Bytef *dest, uLongf *destLen, const Bytef *source, uLong sourceLen, uLong *sourceUsed, uLong *members);

#ifdef __cplusplus
}
#endif
#endif
