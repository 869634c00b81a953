/* oracle/abi_client.c -- TEST INFRASTRUCTURE ONLY.  A zlib client of a few lines, compiled by oracle/Makefile against the REFERENCE's
 * h/zlib.h and linked with the product's libzamd_z.so (_ref/client_zamd): the drop-in check of tests/test_abi.py.  Prints the library's
 * version, sizeof(z_stream) as the reference's header lays it out, compressBound(65536) and what deflateInit says. */
#include "zlib.h"
#include <stdio.h>
int main(void) {
    z_stream s; s.zalloc = 0; s.zfree = 0; s.opaque = 0;
    printf("%s %d %lu ", zlibVersion(), (int)sizeof(z_stream), compressBound(65536));
    int rc = deflateInit(&s, 6);
    printf("%d %s\n", rc, rc == Z_OK ? "ok" : (s.msg ? s.msg : zError(rc)));
    if (rc == Z_OK) deflateEnd(&s);
    return 0; }
