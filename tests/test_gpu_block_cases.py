"""GPU: the block layer of one continuous stream -- chains 2-4 of zlib_amd/csrc/zgpu_cont.hip (cont_tokscan_kernel, cont_compact_kernel, cont_table_kernel,
cont_bitscan_kernel, cont_edges_kernel, cont_stitch_kernel, cont_carry_kernel) and the CONT side of huffman_kernel -- on every row of
oracle/blockcases.py: stored blocks that start at every bit phase, segments whose last token fills a block, block cuts on tile and batch edges, more than
1024 blocks in a batch.  Every row goes through every entry it has and owes the compiled reference's bytes (tests/golden/block_kat.json;
tests/test_block_cases_cpu.py shows that the rows are what they say and that the restatement gives the same bytes), and the stream inflates back.

Entries:
  engine      Engine.deflate_host(F_FINAL | F_CONTINUOUS) -- the rows without a flush or a cut
  host        libzamd_z.so's deflate() driven by the row's calls, with ample space (zhost.deflate_stream)
  host-steps  the same, handed over in pieces of 30011 bytes and drained 4099 bytes at a time
  feed        the feed interface zgpu_deflate_cont_host as scripts/cont_feed.py drives it (raw streams: compared with the row's stream less its wrapper)
A row with `feed` set runs with ZAMD_FEED_BYTES = feed (cont_feed: more_at = feed), so its Z_NO_FLUSH call is a feed of its own.  The full and edge rows run
under ZGPU_CONT_BATCH_TILES = 1 (a batch ends with every tile) and its default, ZGPU_CONT_PIPE = 0 and 2.
Only the edge rows are longer than one tile, so only for them do these settings move a batch's end; the full rows are the same single-tile work under all four.

One test per family, entry and setting; every failure of it in one report: the row's name and the first block that differs, read with oracle/blockwalk.py."""
import hashlib
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

from oracle import blockcases as BC, blockwalk as BW  # noqa: E402
import zhost as Z  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "block_kat.json")))["cases"]
ENTRIES = ("engine", "host", "host-steps", "feed")
KNOBS = ((None, None), ("1", "0"), ("1", "2"), (None, "2"))  # (ZGPU_CONT_BATCH_TILES, ZGPU_CONT_PIPE); None: not set


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


_restated = {}


def restated(c):
    """the row's stream by the restatement, made once (the fixture's bytes: tests/test_block_cases_cpu.py)"""
    if c.name not in _restated:
        _restated[c.name] = BC.restated(c)
    return _restated[c.name]


def has_entry(c, entry):
    return entry != "engine" or not c.calls


def run(eng, c, entry):
    """the row's stream by the product (`feed`: the raw stream)"""
    if entry == "engine":
        from zlib_amd import gpu
        wrap = 0 if c.wbits < 0 else gpu.F_GZIP_WRAP if c.wbits > 15 else gpu.F_ZLIB_WRAP
        return eng.deflate_host(c.data, c.level, flags=gpu.F_FINAL | gpu.F_CONTINUOUS | wrap, strategy=c.strategy)
    if entry == "feed":
        import cont_feed as CF
        return CF.stream(eng, c.data, c.level, list(c.calls), strategy=c.strategy, more_at=c.feed or 1 << 62)
    plan, pos = [], 0
    for upto, flush in list(c.calls) + [(len(c.data), Z.Z_FINISH)]:
        plan.append((upto - pos, flush))
        pos = upto
    in_step, out_step = (30011, 4099) if entry == "host-steps" else (None, None)
    return Z.deflate_stream(c.data, c.level, plan, in_step=in_step, out_step=out_step, window_bits=c.wbits, strategy=c.strategy)[0]


def owes(bad, eng, c, entry):
    z = run(eng, c, entry)
    want = KAT[c.name]
    if entry == "feed" and c.wbits >= 0:
        ref = restated(c)
        assert (len(ref), h16(ref)) == (want["len"], want["sha"]), c.name
        same, wrapped = z == BC.raw_of(c, ref), None
    else:
        same, wrapped = (len(z), h16(z)) == (want["len"], want["sha"]), z
    if not same:
        raw = z if wrapped is None else BC.raw_of(c, z)
        bad.append("%s [%s]: %s" % (c.name, entry, BW.first_difference(raw, BC.raw_of(c, restated(c)))))
    if wrapped is None:
        rc, back = Z.inflate_stream(z, len(c.data) + 8, window_bits=-15)[:2]
    else:
        rc, back = Z.inflate_stream(z, len(c.data) + 8, window_bits=c.wbits)[:2]
    if (rc, back) != (Z.Z_STREAM_END, c.data):
        bad.append("%s [%s]: the product's inflate of the stream: rc %d, %d bytes of %d" % (c.name, entry, rc, len(back), len(c.data)))


def play(eng, monkeypatch, rows, entry, knobs=(None, None)):
    assert rows
    for name, v in zip(("ZGPU_CONT_BATCH_TILES", "ZGPU_CONT_PIPE"), knobs):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    bad = []
    for c in rows:
        if c.feed is None:
            monkeypatch.delenv("ZAMD_FEED_BYTES", raising=False)
        else:
            monkeypatch.setenv("ZAMD_FEED_BYTES", str(c.feed))
        owes(bad, eng, c, entry)
    assert not bad, "%d failures\n" % len(bad) + "\n".join(bad[:40])


def rows_of(family, entry):
    """(the catalogue is built when the first test asks for it, not when this file is collected)"""
    return [c for c in BC.catalogue() if c.family == family and has_entry(c, entry)]


def test_every_row_has_every_entry_it_can_have():
    """Nothing is left out: a row with a flush or a cut cannot be one engine call, every other (row, entry) is played below."""
    for c in BC.catalogue():
        assert [e for e in ENTRIES if has_entry(c, e)] == ([] if c.calls else ["engine"]) + ["host", "host-steps", "feed"], c.name
    for family in BC.SITUATIONS:
        assert rows_of(family, "engine"), family
    # compress2()'s path sees a segment of every count that ends with Z_FINISH, reached by a literal and by a match
    assert {c.name.rsplit("-", 1)[0] for c in rows_of("full", "engine")} == {"full-k%d%s-%s-finish" % (k, BC.ETAG[e], kind) for k in (1, 2) for e in (-1, 0, 1) for kind in ("lit", "match")}


@pytest.mark.parametrize("entry", ENTRIES)
def test_phase(eng, monkeypatch, entry):
    play(eng, monkeypatch, rows_of("phase", entry), entry)


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "tiles%s-pipe%s" % k)
@pytest.mark.parametrize("entry", ENTRIES)
def test_full(eng, monkeypatch, entry, knobs):
    play(eng, monkeypatch, rows_of("full", entry), entry, knobs)


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "tiles%s-pipe%s" % k)
@pytest.mark.parametrize("entry", ENTRIES)
def test_edge(eng, monkeypatch, entry, knobs):
    play(eng, monkeypatch, rows_of("edge", entry), entry, knobs)


@pytest.mark.parametrize("entry", ENTRIES)
def test_many(eng, monkeypatch, entry):
    play(eng, monkeypatch, rows_of("many", entry), entry)
