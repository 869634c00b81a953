// deflate_batch_plan_model.cpp -- prints the workspace layouts of zlib_amd/csrc/zgpu_deflate_batch_plan.h for tests/test_deflate_batch_plan_cpu.py.  Host only:
// the plan header has no HIP type, this program makes no HIP call and is run as a program, never loaded into Python.
// usage: deflate_batch_plan_model N BATCH_ITEMS [N BATCH_ITEMS ...] -- one line per pair: n= batch= round= total= bytes= then name=off:bytes:align for every region
#include "../../zlib_amd/csrc/zgpu_deflate_batch_plan.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc < 3 || (argc - 1) % 2) { fprintf(stderr, "usage: %s N BATCH_ITEMS [N BATCH_ITEMS ...]\n", argv[0]); return 2; }
    for (int i = 1; i + 1 < argc; i += 2) {
        const uint64_t n = strtoull(argv[i], nullptr, 10);
        const uint32_t batch = (uint32_t)strtoul(argv[i + 1], nullptr, 10);
        const zgpu::DeflateWsPlan p = zgpu::deflate_batch_ws_plan(n, batch);
        printf("n=%" PRIu64 " batch=%u round=%" PRIu64 " total=%" PRIu64 " bytes=%" PRIu64, n, batch, p.round, p.total, zgpu::deflate_batch_ws_bytes(n, batch));
        for (int r = 0; r < zgpu::kDeflateWsRegions; r++) {
            const zgpu::DeflateWsRegion &g = zgpu::deflate_ws_region(p, r);
            printf(" %s=%" PRIu64 ":%" PRIu64 ":%" PRIu64, zgpu::deflate_ws_region_name(r), g.off, g.bytes, g.align);
        }
        printf("\n");
    }
    return 0;
}
