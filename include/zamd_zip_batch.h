/* zamd_zip_batch.h -- PKZIP archives in batches (libzamd_z.so): all members of a call through ONE call of the batch engine.
 *
 * include/zamd_zip.h serves a member at a time, a whole deflate() / inflate() stream each; an archive of thousands of small files -- jar, apk,
 * docx, npz, wheels -- pays that per member.  These two calls take the members together:
 *   writing  members of at most 65536 bytes at levels 1-9 (-1 = 6) are the segments of one zgpu_deflate_segments_items_host call (raw streams, no
 *            wrapper; CRC-32, compressed size and data type come from its per-segment records); at level 0 the bytes are copied and all CRC-32s
 *            come from one zgpu_checksum_batch_host call.  Larger members take zamd_zip_add's own path, one by one, at their turn.
 *   reading  deflated members below 512 MiB compressed are the items of one zgpu_inflate_batch_host call (each framed as the gzip member
 *            zamd_unzip_read frames it as: CRC-32 and size are checked on the device); stored members are read into place and checked with
 *            one zgpu_checksum_batch_host call.  Larger members go through zamd_unzip_read one by one, and so does every member the batch
 *            decoder refuses: its code is zamd_unzip_read's own.
 * Same limits as zamd_zip.h: no zip64, no encryption, no data descriptors, archives in files.  The batch calls use the engine of
 * include/zamd_batch.h (one call at a time, on the device ZAMD_DEVICE names).
 */
#ifndef ZAMD_ZIP_BATCH_H
#define ZAMD_ZIP_BATCH_H
#include <stddef.h>
#include "zamd_zip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* n members at one level.  The archive bytes written are exactly those of n calls of
 *     zamd_zip_add(z, name[k], data[k], len[k], level, dos_date[k], comment ? comment[k] : NULL)
 * in order: file order and offsets are the sequential writer's, whatever order the work was done in.  comment may be NULL (no comments), as may
 * any name[k] ("-") or comment[k].  Every argument check zamd_zip_add makes is made for all members before anything is written -- the limit of
 * 65535 entries counts the archive's entries plus n: ZAMD_ZIP_PARAMERROR, and the file is as it was.  n == 0: ZAMD_ZIP_OK, nothing happens. */
int zamd_zip_add_batch(zamd_zip *z, size_t n, const char *const *name, const void *const *data, const unsigned long *len, int level,
                       const unsigned long *dos_date, const char *const *comment);

/* n members into n buffers: result[k] = what zamd_unzip_read(u, index ? index[k] : (int)k, out[k], cap[k]) returns -- the member's size, or a
 * negative ZAMD_ZIP_* code for that member alone (CRC mismatch or damaged deflate data: ZAMD_ZIP_CRCERROR; a directory whose sizes lie:
 * ZAMD_ZIP_BADZIPFILE, or ZAMD_ZIP_CRCERROR where zamd_unzip_read may say either; cap[k] below the directory's size: ZAMD_ZIP_PARAMERROR).  One bad
 * member never disturbs another member's bytes; indices may repeat.  Returns ZAMD_ZIP_OK when no result is negative, else the first negative
 * one.  u == NULL, or n > 0 with a null out, cap or result: ZAMD_ZIP_PARAMERROR, nothing touched.  n == 0: ZAMD_ZIP_OK. */
int zamd_unzip_read_batch(zamd_unzip *u, const int *index, size_t n, void *const *out, const unsigned long *cap, long *result);

/* unzip -t for n members at once, nothing delivered: zamd_zip_test.h */

#ifdef __cplusplus
}
#endif
#endif
