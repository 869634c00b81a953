"""The hand-built DEFLATE catalogue (oracle/handmade.py) on the CPU: it still builds the streams the golden file names, every valid one
decodes to expand()'s bytes through the interpreter's zlib, and -- where the compiled reference is present -- the reference's verdicts are
the golden ones."""
import zlib

import pytest

from oracle import deflate_writer as W, handmade as H, refzlib as R


@pytest.fixture(scope="module")
def cat():
    return H.catalogue()


@pytest.fixture(scope="module")
def gold(golden):
    return golden("handmade_inflate.json")["cases"]


def test_catalogue_builds_the_golden_streams(cat, gold):
    assert sorted(c.name for c in cat) == sorted(gold)
    for c in cat:
        assert [len(c.stream), H.sha16(c.stream)] == gold[c.name]["stream"], c.name


def test_valid_streams_decode_to_expand_through_system_zlib(cat, gold):
    for c in cat:
        if c.kind not in ("ok", "trailing"):
            assert c.expect is None
            continue
        d = zlib.decompressobj(-15, zdict=c.dictionary) if c.dictionary else zlib.decompressobj(-15)
        assert d.decompress(c.stream) == c.expect, c.name
        assert d.eof, c.name
        assert (len(d.unused_data) != 0) == (c.kind == "trailing"), c.name
        g = gold[c.name]
        assert g["rc"] == 1 and g["out"] == [len(c.expect), H.sha16(c.expect)], c.name


def test_invalid_streams_are_refused_by_system_zlib(cat):
    for c in cat:
        if c.kind in ("ok", "trailing"):
            continue
        d = zlib.decompressobj(-15, zdict=c.dictionary) if c.dictionary else zlib.decompressobj(-15)
        try:
            d.decompress(c.stream)
            assert c.kind == "cut" and not d.eof, c.name
        except zlib.error:
            pass


def test_catalogue_reaches_what_the_issue_names(cat, gold):
    """The edges the device paths must see: a valid distance of 32768 on every path (whole stream, segments of at most 64 KiB, the
    pieces decoder, and the zlib API, which takes all of them), a 65536-byte segment, the pieces cases and the one big block."""
    ok = [c for c in cat if c.kind == "ok"]
    assert any(c.maxdist == 32768 for c in ok)                                                            # whole stream / zlib API
    assert any(c.maxdist == 32768 and len(c.expect) <= 65536 and not c.dictionary for c in ok)           # segments, small rings
    assert any(c.maxdist == 32768 and c.dictionary and len(c.dictionary) == 32768 for c in ok)
    assert any(c.maxdist == 32768 and c.pieces for c in ok)                                               # the pieces decoder
    assert any(c.pieces is False and len(c.expect) >= 4 << 20 for c in ok)
    assert any(len(c.segs) > 2 for c in ok)
    two = [c for c in cat if len(c.segs) > 2][0]
    d = zlib.decompressobj(-15)
    assert len(d.decompress(two.stream[two.segs[0]: two.segs[1]])) == 65536 and not d.eof  # (the first segment on its own: exactly 64 KiB)
    msgs = {gold[c.name]["msg"] for c in cat if gold[c.name]["rc"] == -3}
    assert {"invalid distance too far back", "invalid literal/length code", "invalid distance code", "too many length or distance symbols",
            "invalid bit length repeat", "invalid literal/lengths set", "invalid distances set", "invalid code lengths set",
            "invalid stored block lengths", "invalid block type"} <= msgs


def test_writer_round_trips_random_tokens():
    """The writer against the interpreter's zlib on tokens of every kind, fixed and dynamic, behind a dictionary."""
    import numpy as np
    r = H.rint(30000, 0, 1 << 30, 4242)
    kind = (r % 3 == 0).astype(np.int8)
    a = np.where(kind == 1, 3 + (r >> 3) % 256, (r >> 3) & 255)
    b = np.where(kind == 1, 1 + (r >> 11) % 32768, 0)
    t = W.Tokens(kind, a, b)
    d = H.rnd(32768, 4243).tobytes()
    want = W.expand(t, d)
    for blk in (W.fixed, W.dynamic):
        s = W.stream([blk(t, final=True)])
        assert zlib.decompressobj(-15, zdict=d).decompress(s) == want


@pytest.mark.skipif(not R.available(), reason="compiled reference not built (oracle/_ref/libzref.so)")
def test_reference_verdicts_match_golden(cat, gold):
    for c in cat:
        g = gold[c.name]
        cap = len(c.expect) if c.expect is not None else 1 << 20
        rc, out, used, msg = R.inflate_raw_dict(c.stream, cap + 64, c.dictionary)
        assert [rc, msg, [len(out), H.sha16(out)], used] == [g["rc"], g["msg"], g["out"], g["used"]], c.name
