"""GPU: huffman_kernel (zlib_amd/csrc/zgpu_huffman.hip) on the histograms of oracle/treecases.py -- trees that overflow 15 bits and are repaired
(literal tree, distance tree, both in one block), the 15-bit control, histograms made of ties, and the block-type choice at its equalities -- against the
compiled reference's streams in tests/golden/tree_kat.json (length + sha256; tests/test_trees_cpu.py shows that the rows reach the branches they name).

Every row of the fixture runs at every level it lists through every entry that ends in huffman_kernel, nothing is sampled:
  chunk mode (huffman_kernel<false>): Engine.deflate_host with the level's default LZ path, and for strategy-2 rows also the other paths that serve them
      (ZGPU_LZ_SERIAL and ZGPU_LZ_SORTED = match3 + parse2 at levels 4-9, where the default is ZGPU_LZ_SORTED); overflow rows also behind deflatePrime bits 0..7;
  one continuous stream (huffman_kernel<true>): Engine.deflate_host(F_CONTINUOUS | F_FINAL), compress2() and deflateInit2() + deflate() of libzamd_z.so
      with the row's strategy; overflow rows also behind deflatePrime(bits 0..7): the repaired block starts at each of the eight bit phases;
  the batch entry: one zamd_compress2_batch call per level with all default-strategy rows of at most 64 KiB as items, and -- zgpu_deflate_segments_host
      DOES take a strategy -- one Engine.deflate_batch_host(strategy=2) call per level with all strategy-2 rows of at most 64 KiB.
Each stream is inflated again by the product (uncompress(), the device's stream inflate, the batch inflate).  A mismatch names the row and the first
differing bit (the expected bytes then come from the CPU restatement, which tests/test_trees_cpu.py pins to the same fixture)."""
import ctypes as C
import hashlib
import json
import os

import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_py as O, treecases as T  # noqa: E402
import zhost as Z  # noqa: E402

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "tree_kat.json")))
ROWS = {(r["name"], r["level"]): r for r in KAT["rows"]}
CASES = list(T.all_cases())
OVERFLOW = ("lit", "dist", "both", "control")


def sha(b):
    return hashlib.sha256(b).hexdigest()[:24]


def first_diff_bit(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return 8 * i + ((a ^ b) & -(a ^ b)).bit_length() - 1
    return 8 * min(len(got), len(want))


def expected_bytes(c, level, what, bits=0, value=0):
    """For the report of a mismatch only: the restatement's bytes of the same stream (a primed stream is not restated: None)."""
    if bits:
        return None
    if what == "cont":
        return O.deflate_cont(c.data, level, (), c.strategy)
    n = max(1, (len(c.data) + 65535) // 65536)
    return b"".join(O.deflate_chunk(c.data[k * 65536:(k + 1) * 65536], level, k + 1 == n, strategy=c.strategy) for k in range(n))


def check(bad, got, want_len, want_sha, c, level, entry, what, bits=0):
    if len(got) != want_len or sha(got) != want_sha:
        exp = expected_bytes(c, level, what, bits)
        bad.append("%s level %d via %s: %d bytes, the reference has %d; first differing bit %s" %
                   (c.name, level, entry, len(got), want_len, first_diff_bit(got, exp) if exp is not None else "n/a (primed)"))


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


def test_every_row_has_its_case():
    assert sorted(ROWS) == sorted((c.name, lv) for c in CASES for lv in c.levels)


def test_chunk_mode(eng):
    from zlib_amd import gpu
    bad = []
    for c in CASES:
        for lv in c.levels:
            r = ROWS[(c.name, lv)]
            impls = [("auto", gpu.LZ_AUTO)]
            if c.strategy == 2 and lv >= 4:
                impls += [("sorted", gpu.LZ_SORTED), ("serial", gpu.LZ_SERIAL)]
            elif c.strategy == 0 and lv >= 4:
                impls += [("sorted", gpu.LZ_SORTED)]
            for tag, impl in impls:
                z = eng.deflate_host(c.data, lv, flags=gpu.F_FINAL, lz_impl=impl, strategy=c.strategy)
                check(bad, z, r["chunk_len"], r["chunk_sha"], c, lv, "chunk mode, lz " + tag, "chunk")
            if len(c.data) <= 65536:
                assert bytes(eng.inflate_stream_host(z, len(c.data) + 8)) == c.data, (c.name, lv)
            if "primes" in r and len(c.data) <= 65536:  # one chunk: the primed chunk stream is the primed single stream
                for p in r["primes"]:
                    z = eng.deflate_host(c.data, lv, flags=gpu.F_FINAL, strategy=c.strategy, prime=(p["bits"], p["value"]))
                    check(bad, z, p["len"], p["sha"], c, lv, "chunk mode behind %d primed bits" % p["bits"], "chunk", p["bits"])
    assert not bad, "\n".join(bad[:20])


def test_continuous_stream_engine(eng):
    from zlib_amd import gpu
    bad = []
    for c in CASES:
        for lv in c.levels:
            r = ROWS[(c.name, lv)]
            z = eng.deflate_host(c.data, lv, flags=gpu.F_FINAL | gpu.F_CONTINUOUS, strategy=c.strategy)
            check(bad, z, r["cont_len"], r["cont_sha"], c, lv, "the engine's continuous stream", "cont")
            assert bytes(eng.inflate_stream_host(z, len(c.data) + 8)) == c.data, (c.name, lv)
    assert not bad, "\n".join(bad[:20])


def _host_primed(L, data, level, strategy, bits, value):
    s = Z.ZStream()
    assert L.deflateInit2_(C.byref(s), level, 8, -15, 8, strategy, b"1.2.3", C.sizeof(Z.ZStream)) == Z.Z_OK
    assert L.deflatePrime(C.byref(s), bits, value) == Z.Z_OK
    cap = len(data) + (len(data) >> 3) + 1024
    out = C.create_string_buffer(cap)
    inb = C.create_string_buffer(data, max(len(data), 1))
    s.next_in = C.addressof(inb); s.avail_in = len(data); s.next_out = C.addressof(out); s.avail_out = cap
    assert L.deflate(C.byref(s), Z.Z_FINISH) == Z.Z_STREAM_END
    z = out.raw[: s.total_out]
    assert L.deflateEnd(C.byref(s)) == Z.Z_OK
    return z


def test_continuous_stream_host_api():
    L = Z.lib()
    L.deflatePrime.argtypes = [C.POINTER(Z.ZStream), C.c_int, C.c_int]
    bad = []
    for c in CASES:
        for lv in c.levels:
            r = ROWS[(c.name, lv)]
            z, _, _ = Z.deflate_stream(c.data, lv, [(len(c.data), Z.Z_FINISH)], window_bits=-15, strategy=c.strategy)
            check(bad, z, r["cont_len"], r["cont_sha"], c, lv, "deflateInit2 + deflate", "cont")
            assert Z.inflate_stream(z, len(c.data) + 8, window_bits=-15)[:2] == (Z.Z_STREAM_END, c.data), (c.name, lv)
            if c.strategy == 0:  # compress2() has no strategy argument
                rc, z = Z.compress2(c.data, lv)
                assert rc == Z.Z_OK and z[-4:] == O.adler32(c.data).to_bytes(4, "big"), (c.name, lv)
                check(bad, z[2:-4], r["cont_len"], r["cont_sha"], c, lv, "compress2", "cont")
                assert Z.uncompress(z, len(c.data)) == (Z.Z_OK, c.data), (c.name, lv)
            for p in r.get("primes", ()):
                z = _host_primed(L, c.data, lv, c.strategy, p["bits"], p["value"])
                check(bad, z, p["len"], p["sha"], c, lv, "deflate behind deflatePrime(%d)" % p["bits"], "cont", p["bits"])
    assert not bad, "\n".join(bad[:20])


def test_batch_entries(eng):
    L = Z.lib()
    P, U = C.POINTER(C.c_void_p), C.POINTER(C.c_ulong)
    L.zamd_compress2_batch.argtypes = [P, U, P, U, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]
    bad, seen = [], 0
    for lv in (1, 3, 4, 6, 9):
        for strategy in (0, 2):
            items = [c for c in CASES if c.strategy == strategy and lv in c.levels and len(c.data) <= 65536]
            if not items:
                continue
            seen += len(items)
            if strategy == 0:  # the zlib-style entry: what compress2() gives for each item
                n = len(items)
                caps = [int(L.compressBound(len(c.data))) for c in items]
                src = [C.create_string_buffer(c.data, len(c.data)) for c in items]
                dst = [C.create_string_buffer(cap) for cap in caps]
                A = C.c_void_p * n
                dl, st = (C.c_ulong * n)(*caps), (C.c_int * n)()
                rc = L.zamd_compress2_batch(A(*[C.addressof(d) for d in dst]), dl, A(*[C.addressof(s) for s in src]), (C.c_ulong * n)(*[len(c.data) for c in items]), n, lv, 15, st)
                assert rc == Z.Z_OK and all(st[k] == Z.Z_OK for k in range(n)), (lv, rc)
                outs = [dst[k].raw[2: dl[k] - 4] for k in range(n)]
                for k, c in enumerate(items):
                    assert dst[k].raw[dl[k] - 4: dl[k]] == O.adler32(c.data).to_bytes(4, "big"), (c.name, lv)
            else:
                outs = eng.deflate_batch_host([c.data for c in items], lv, wrap="raw", strategy=2)
            for c, z in zip(items, outs):
                r = ROWS[(c.name, lv)]
                check(bad, z, r["cont_len"], r["cont_sha"], c, lv, "the batch entry (strategy %d)" % strategy, "cont")
            back = eng.inflate_batch_host(outs, [len(c.data) + 8 for c in items], wrap="raw")
            for c, b in zip(items, back):
                assert b[0] == 0 and b[2] == c.data, (c.name, lv, b[0], b[1])
    assert seen == sum(1 for c in CASES for lv in c.levels if len(c.data) <= 65536)
    assert not bad, "\n".join(bad[:20])
