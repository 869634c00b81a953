/* zamd_zip_test.h -- unzip -t in one call (libzamd_z.so): the members of an archive tested, none delivered.
 *
 * The integrity test of include/zamd_zip_batch.h's reader: the same engine, the same framing, and no room for a decoded byte -- deflated members
 * are decoded inside the device's local memory and their CRC-32 and size compared there (zgpu_inflate_batch_verify_host, include/zamd_gpu.h).
 */
#ifndef ZAMD_ZIP_TEST_H
#define ZAMD_ZIP_TEST_H
#include <stddef.h>
#include "zamd_zip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* unzip -t: n members tested, none delivered.  result[k] = what zamd_unzip_read(u, index ? index[k] : (int)k, room, the directory's size) returns
 * for a room of that size -- the member's size, or its negative ZAMD_ZIP_* code.  Deflated members are framed as zamd_unzip_read_batch (zamd_zip_batch.h) frames them
 * and go through one integrity test (zgpu_inflate_batch_verify_host: decoded in the device's local memory, CRC-32 and size compared there, no room
 * for the decoded bytes anywhere); stored members through one zgpu_checksum_batch_host call.  A member the test refuses, and one of 512 MiB of
 * compressed data or more, is read by zamd_unzip_read into a scratch buffer that is freed again: its code is that call's own.  Returns as
 * zamd_unzip_read_batch.  u == NULL, or n > 0 with a null result: ZAMD_ZIP_PARAMERROR, nothing touched.  n == 0: ZAMD_ZIP_OK. */
int zamd_unzip_test_batch(zamd_unzip *u, const int *index, size_t n, long *result);

#ifdef __cplusplus
}
#endif
#endif
