// inflate_batch_plan_model.cpp -- prints the workspace layouts of zlib_amd/csrc/zgpu_inflate_batch_plan.h for tests/test_inflate_batch_plan_cpu.py.  Host only:
// the plan header has no HIP type, this program makes no HIP call and is run as a program, never loaded into Python.
// usage: inflate_batch_plan_model JOB N [JOB N ...] -- one line per pair: job= n= total= then name=off:bytes:align for every region
#include "../../zlib_amd/csrc/zgpu_inflate_batch_plan.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc < 3 || (argc - 1) % 2) { fprintf(stderr, "usage: %s JOB N [JOB N ...]\n", argv[0]); return 2; }
    for (int i = 1; i + 1 < argc; i += 2) {
        const int job = atoi(argv[i]);
        const uint64_t n = strtoull(argv[i + 1], nullptr, 10);
        const zgpu::BatchWsPlan p = zgpu::inflate_batch_ws_plan(job, n);
        printf("job=%d n=%" PRIu64 " total=%" PRIu64 " bytes=%" PRIu64, job, n, p.total, zgpu::inflate_batch_ws_bytes(job, n));
        for (int r = 0; r < zgpu::kBatchWsRegions; r++) {
            const zgpu::BatchWsRegion &g = zgpu::batch_ws_region(p, r);
            printf(" %s=%" PRIu64 ":%" PRIu64 ":%" PRIu64, zgpu::batch_ws_region_name(r), g.off, g.bytes, g.align);
        }
        printf("\n");
    }
    return 0;
}
