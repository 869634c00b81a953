"""The caller-owned workspace of the stream-ordered batch deflate calls (zlib_amd/csrc/zgpu_deflate_batch_plan.h) as a function of plain numbers.
tests/tools/deflate_batch_plan_model.cpp includes the plan header and prints the layout; it is built for the host only, with the host sanitizers, makes
no HIP call and is run as a program, never loaded into Python.  The expected sizes below are worked out from what the regions hold (zgpu_common.h,
zgpu_lz_sorted.h), not from a run.  Nothing is per item of the call.  Per item of a round, which is min(n, batch_items) items with batch_items == 0
standing for 4096: a uint64 for where its input begins, a uint64 for where it begins in the staging buffer (and one more, the round's end), a uint32 of
state, 65536 bytes of staging buffer (256 more once), the sorted buckets' workspace -- S (65536 + 8) u16, the ranks 65536 u16, the head bits
and heads_below (2048 + 512) u32, the records 65536 x 8 bytes, ir 65536 u32: 1,058,832 bytes, once more a header of 256 and a margin of 1024 --, 65536
tokens of four bytes, a slot of 65536 + 256 bytes, a ChunkMeta of 32.  And 256 bytes of counters."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (0, 1, 255, 256, 257, 65537, 2 ** 32 - 1)
BATCHES = (0, 1, 4, 4096)
SORTED_CHUNK = (65536 + 8) * 2 + 65536 * 2 + (2048 + 512) * 4 + 65536 * 8 + 65536 * 4
# name: (bytes per item of the call, bytes per item of a round, fixed bytes, the alignment its type wants)
RECORD = {"cnt": (0, 0, 256, 8), "lo": (0, 8, 0, 8), "pre": (0, 8, 8, 8), "state": (0, 4, 0, 4), "stage": (0, 65536, 256, 256), "sorted": (0, SORTED_CHUNK, 256 + 1024, 256),
          "tokens": (0, 65536 * 4, 0, 4), "slots": (0, 65536 + 256, 0, 4), "meta": (0, 32, 0, 4)}


def _round(n, batch):
    return min(n, batch if batch else 4096)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "deflate_batch_plan_model")
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "deflate_batch_plan_model.cpp")], check=True, timeout=300)
    args = [str(v) for n in NS for b in BATCHES for v in (n, b)] + [str(2 ** 32), "0", str(2 ** 32), "4096", str(2 ** 32 - 1), str(2 ** 32 - 1)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    table = {}
    for line in out.stdout.splitlines():
        f = dict(w.split("=", 1) for w in line.split())
        regions = {k: tuple(int(x) for x in v.split(":")) for k, v in f.items() if ":" in v}
        table[(int(f["n"]), int(f["batch"]))] = (int(f["total"]), int(f["bytes"]), int(f["round"]), regions)
    return table


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("n", NS)
def test_regions_lie_inside_are_disjoint_and_aligned(plans, n, batch):
    total, nbytes, rnd, regions = plans[(n, batch)]
    assert total == nbytes and 0 < total < 2 ** 63
    assert rnd == _round(n, batch)
    assert sorted(regions) == sorted(RECORD)
    live = []
    for name, (off, size, align) in regions.items():
        per_item, per_round, fixed, want_align = RECORD[name]
        assert align == want_align
        assert size == per_item * n + per_round * rnd + fixed, name  # room for every record, exactly
        assert off % 256 == 0 and off % align == 0, name
        assert off + size <= total, name
        live.append((off, off + size, name))
    live.sort()
    for (a0, a1, an), (b0, b1, bn) in zip(live, live[1:]):
        assert a1 <= b0, (an, bn)
    # nothing in the workspace but the regions and their padding to 256 bytes
    assert total == sum((hi - lo + 255) // 256 * 256 for lo, hi, _ in live)


def test_total_is_monotone_in_both_arguments_and_does_not_wrap(plans):
    for batch in BATCHES:
        totals = [plans[(n, batch)][0] for n in NS]
        assert totals == sorted(totals), batch
        for (n1, t1), (n2, t2) in zip(zip(NS, totals), zip(NS[1:], totals[1:])):  # it grows with the round, and with nothing else
            assert (t1 < t2) if _round(n1, batch) < _round(n2, batch) else (t1 == t2), (batch, n1, n2)
    for n in NS:
        totals = [plans[(n, b)][0] for b in (1, 4, 4096)]
        assert totals == sorted(totals), n
        assert plans[(n, 0)][0] == plans[(n, 4096)][0]  # 0 stands for 4096
    # the largest there is: every item of 2^32 - 1 in one round.  What the sum is in unbounded arithmetic: no 64-bit wrap on the way
    n = 2 ** 32 - 1
    per_item = sum(r[0] + r[1] for r in RECORD.values())
    assert per_item * n <= plans[(n, n)][0] < per_item * n + 9 * 256 + 256 + 256 + 1024 + 256 + 8 < 2 ** 63


def test_too_many_items_have_no_workspace(plans):
    assert plans[(2 ** 32, 0)][0] == 0 and plans[(2 ** 32, 4096)][0] == 0


def test_the_library_answers_what_the_header_says(plans):
    import zlib_amd
    L = zlib_amd.load_library()
    for (n, batch), (total, _, _, _) in plans.items():
        assert L.zgpu_deflate_batch_workspace_bytes(n, batch) == total, (n, batch)
