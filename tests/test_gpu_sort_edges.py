"""sort4_kernel (zgpu_lz_sort.hip, K1c) keeps a lane's positions in registers through all its passes: turns of 512 positions handed round the
sixteen waves, ranks and S indices of 16 bits beside a marker for "no position, or not in the chains", two 16-bit counts to an LDS word, S
assembled in two halves.  Passes A and C0 have two forms of a turn: a straight one for a turn of which every position exists, has four bytes to
load and is in the chains (whole_turn: no flush point in the chunk and 512 T + 515 <= n), and the general one for the rest.  These inputs sit on
the edges of that bookkeeping: lengths around a 64-lane step, the end of a turn (514 bytes: turn 0 takes the general form; 515: the straight
one), half a round and a whole round of the waves with the last turn general and the others straight (4098, 8194), the two halves of S; one
bucket with ranks up to 65533, next to 0xffff; both halves of one count word with counts above 255; buckets of one or two entries; chunk starts
at every alignment; calls that take several launches; tiles of a continuous stream with positions that have three bytes and are in no chain,
which keep to the general form while their neighbours take the straight one.

Every case goes through the default path on one fresh engine at levels 6 (walk_kernel reads S and ir) and 1 (fastwin_kernel does), is compared
byte for byte with the CPU oracle, and ends by asking the engine whether the sort's self-check ever failed (zgpu_debug_sort_fallback): a wrong
fast sort that pass V caught and the ballot-ranked sort repaired would give the right bytes too.

The stream with a flush point goes through the host library, as the sync_at rows of test_gpu_continuous.py do (bytes only: that library keeps
its engine to itself), and through the feed interface on this test's engine (scripts/cont_feed.py, as test_gpu_continuous.py's feed test), where
the accessor is asked."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

from oracle import cases, oracle_py as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 65536
LEVELS = (6, 1)

# one chunk of n bytes: no position (0, 1, 2), one (3); the 64-lane step (66 and 67 bytes are 64 and 65 positions); a turn of 512 positions ends
# (513, 514, 515: at 515 turn 0 is a whole turn); eight and sixteen turns, the last one not whole (4098, 8194); S's first half is one short, full, one over (32769, 32770, 32771); the longest
LENGTHS = [0, 1, 2, 3, 66, 67, 513, 514, 515, 4098, 8194, 32769, 32770, 32771, 65535, 65536]


def alternating(n):
    """hash3(0,0,0) = 0 and hash3(0,0,1) = 1: zeros with every FOURTH byte 1 put a quarter of the positions each into buckets 0, 1, 32 and 1024 --
    both 16-bit halves of count word 0 are in use, by turns, with counts far above 255.  (With every third byte 1 no position has three zeros in
    front of it and bucket 0 stays empty.)"""
    d = bytearray(n)
    d[3::4] = b"\x01" * len(d[3::4])
    return bytes(d)


CONTENTS = {
    "zeros-65536": bytes(CHUNK),           # one bucket: ranks 0..65533, the largest next to the marker; pass V runs over a whole half without a head
    "zeros-65535": bytes(CHUNK - 1),
    "alternating": alternating(CHUNK),
    "rand": cases.make("rand", CHUNK, 4),  # every bucket has one or two entries
    "text": cases.make("text", CHUNK, 3),
    "run-then-rand": b"r" * 8192 + cases.make("rand", CHUNK - 8192, 9),
}

# (chunk size, bytes): chunk starts fall at every alignment mod 4, and the last positions of a chunk read their three bytes unaligned
GEOMETRY = [(3, 3 * 41 + 2), (4099, 4099 * 5 + 77), (65535, 65535 * 2 + 1000)]


def sort_fallback(e):
    e.L.zgpu_debug_sort_fallback.argtypes = [C.c_void_p]
    e.L.zgpu_debug_sort_fallback.restype = C.c_int
    return e.L.zgpu_debug_sort_fallback(e.h)


@pytest.fixture()
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


def check(e, data, chunk=CHUNK, what=None):
    for level in LEVELS:
        got = e.deflate_host(data, level, chunk_size=chunk)
        want = O.deflate_stream(data, level, chunk)
        assert got == want, (what, level, chunk, len(data), len(got), len(want))


def test_lengths_of_a_single_chunk(eng):
    for n in LENGTHS:
        check(eng, cases.make("text", n, 3), what="len-%d" % n)
    assert sort_fallback(eng) == 0


@pytest.mark.parametrize("name", list(CONTENTS))
def test_contents(eng, name):
    check(eng, CONTENTS[name], what=name)
    assert sort_fallback(eng) == 0


def test_alternating_input_is_what_it_claims():
    d = alternating(CHUNK)
    hashes = [((d[p] << 10) ^ (d[p + 1] << 5) ^ d[p + 2]) & 32767 for p in range(CHUNK - 2)]
    assert sorted(set(hashes)) == [0, 1, 32, 1024] and hashes.count(0) > 16000 and hashes.count(1) > 16000
    assert hashes[:8] == [0, 1, 32, 1024, 0, 1, 32, 1024]


@pytest.mark.parametrize("chunk,nbytes", GEOMETRY)
def test_several_chunks_per_call(eng, chunk, nbytes):
    check(eng, cases.make("text", nbytes, 5), chunk, what="geometry")
    assert sort_fallback(eng) == 0


CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from oracle import cases, oracle_py as O
import zlib_amd
e = zlib_amd.Engine(0)
data = cases.make("text", 20 * 65536 + 4321, 6)
ok = {str(lvl): e.deflate_host(data, lvl) == O.deflate_stream(data, lvl, 65536) for lvl in (6, 1)}
e.L.zgpu_debug_sort_fallback.argtypes = [C.c_void_p]
e.L.zgpu_debug_sort_fallback.restype = C.c_int
print("RESULT " + json.dumps({"ok": ok, "fallback": e.L.zgpu_debug_sort_fallback(e.h)}))
e.close()
""" % ROOT


def test_a_call_of_several_launches():
    """ZGPU_BATCH_CHUNKS is read once per process: 21 chunks, seven to a launch, in a child."""
    env = dict(os.environ)
    for k in ("ZGPU_SORT", "ZGPU_PARSE"):
        env.pop(k, None)
    env["ZGPU_BATCH_CHUNKS"] = "7"
    p = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res == {"ok": {"6": True, "1": True}, "fallback": 0}


def test_continuous_stream_with_a_flush_point(eng):
    """100 000 bytes, one Z_SYNC_FLUSH in the middle: the tiles' sorts see positions in front of the flush point that have three bytes and are in
    no chain, and must carry the marker through all passes.  Through the host library (bytes), and through the feed interface on this engine with
    the excluded positions filled in (bytes and the accessor); the un-flushed stream beside them."""
    import zhost as Z
    from zlib_amd import gpu
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import cont_feed as CF
    data = cases.make("text", 100000, 7)
    for level in LEVELS:
        z, codes, info = Z.deflate_stream(data, level, [(50000, Z.Z_SYNC_FLUSH), (len(data) - 50000, Z.Z_FINISH)])
        assert z == O.cont_stream(data, level, [(50000, Z.Z_SYNC_FLUSH)]), level
        assert CF.stream(eng, data, level, [(50000, 2)]) == O.deflate_cont(data, level, [(50000, 2)]), level
        one = eng.deflate_host(data, level, flags=gpu.F_FINAL | gpu.F_ZLIB_WRAP | gpu.F_CONTINUOUS)
        assert one == O.cont_stream(data, level), level
    assert sort_fallback(eng) == 0


def test_the_accessor_reports_the_fallback(eng):
    """An injected fault of the self-check: the bytes are still the oracle's (sort_kernel's), and the accessor says so."""
    data = CONTENTS["text"] + CONTENTS["rand"][:1000]
    assert sort_fallback(eng) == 0
    eng.L.zgpu_debug_inject_sort_fault.restype = None
    eng.L.zgpu_debug_inject_sort_fault()
    assert eng.deflate_host(data, 6) == O.deflate_stream(data, 6, CHUNK)
    assert sort_fallback(eng) != 0
    assert eng.deflate_host(data, 1) == O.deflate_stream(data, 1, CHUNK)
