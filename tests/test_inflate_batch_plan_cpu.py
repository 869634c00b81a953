"""The caller-owned workspace of the stream-ordered batch inflate calls (zlib_amd/csrc/zgpu_inflate_batch_plan.h) as a function of plain numbers.
tests/tools/inflate_batch_plan_model.cpp includes the plan header and prints the layout of every job; it is built for the host only, with the host
sanitizers, makes no HIP call and is run as a program, never loaded into Python.  The expected sizes below are worked out from the records the regions
hold (zgpu_common.h, zamd_gpu.h), not from a run: 4 x uint64 per item of the segment table, BatchItemState 64 bytes, InfStatus 16, ChunkMeta 32,
zgpu_inflate_item 32, one uint64 per item and one more for the packed layout's ends, 256 bytes of counters."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE, SIZES, VERIFY, PACKED = 0, 1, 2, 3
JOBS = (DECODE, SIZES, VERIFY, PACKED)
NS = (0, 1, 255, 256, 257, 65536, 65537, 2 ** 32 - 1)
# bytes per item (and per call) of every region, and the alignment its type wants
RECORD = {"seg": (32, 0, 8), "states": (64, 0, 8), "status": (16, 0, 4), "cnt": (0, 256, 8), "meta": (32, 0, 4), "hi": (8, 8, 8), "items2": (32, 0, 8)}
HAS = {DECODE: ("seg", "states", "status", "cnt", "meta"), SIZES: ("seg", "states", "status", "cnt"), VERIFY: ("seg", "states", "status", "cnt", "meta"),
       PACKED: ("seg", "states", "status", "cnt", "meta", "hi", "items2")}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "inflate_batch_plan_model")
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "inflate_batch_plan_model.cpp")], check=True, timeout=300)
    args = [str(v) for job in JOBS for n in NS for v in (job, n)] + ["4", "1", "-1", "1", "0", str(2 ** 32)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    table = {}
    for line in out.stdout.splitlines():
        f = dict(w.split("=", 1) for w in line.split())
        regions = {k: tuple(int(x) for x in v.split(":")) for k, v in f.items() if ":" in v}
        table[(int(f["job"]), int(f["n"]))] = (int(f["total"]), int(f["bytes"]), regions)
    return table


@pytest.mark.parametrize("job", JOBS)
@pytest.mark.parametrize("n", NS)
def test_regions_lie_inside_are_disjoint_and_aligned(plans, job, n):
    total, nbytes, regions = plans[(job, n)]
    assert total == nbytes and 0 < total < 2 ** 63
    assert sorted(regions) == sorted(RECORD)
    live = []
    for name, (off, size, align) in regions.items():
        per_item, fixed, want_align = RECORD[name]
        assert align == want_align
        if name in HAS[job]:
            assert size == per_item * n + fixed, name  # room for every record, exactly
            assert off % 256 == 0 and off % align == 0, name
            live.append((off, off + size, name))
        else:
            assert size == 0, name
        assert off + size <= total, name
    live.sort()
    for (a0, a1, an), (b0, b1, bn) in zip(live, live[1:]):
        assert a1 <= b0, (an, bn)
    # nothing in the workspace but the regions and their padding to 256 bytes
    assert total == sum((hi - lo + 255) // 256 * 256 for lo, hi, _ in live)


@pytest.mark.parametrize("job", JOBS)
def test_total_is_monotone_and_does_not_wrap(plans, job):
    totals = [plans[(job, n)][0] for n in NS]
    assert totals == sorted(totals)  # (255 and 256 items may need the same: every region is padded to 256 bytes)
    assert totals[0] < totals[1] and totals[3] < totals[4] < totals[5] < totals[6] < totals[7]
    per_item = sum(RECORD[name][0] for name in HAS[job])
    assert per_item * (2 ** 32 - 1) <= totals[-1] < 2 ** 40  # (what the sum is in unbounded arithmetic: no 64-bit wrap on the way)


def test_what_is_no_job_has_no_workspace(plans):
    assert plans[(4, 1)][0] == 0 and plans[(-1, 1)][0] == 0 and plans[(0, 2 ** 32)][0] == 0


def test_the_library_answers_what_the_header_says(plans):
    import zlib_amd
    L = zlib_amd.load_library()
    for (job, n), (total, _, _) in plans.items():
        assert L.zgpu_inflate_batch_workspace_bytes(job, n) == total, (job, n)
