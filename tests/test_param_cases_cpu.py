"""The catalogue of stream lives (oracle/paramcases.py: deflateParams at every transition, deflateTune, deflateReset, short output space, deflateBound) on
the CPU: the catalogue still builds the rows tests/golden/params_kat.json names; the restatement (oracle_py.deflate_cont with params=) gives the fixture's
bytes for every row it can express; where the compiled reference is at hand it reproduces the fixture; the carry rows have the shape they are for; and
the catalogue leaves out nothing but what it says.

Fixture-only families (the restatement has no entry for them): space (a call with avail_out 0 or 7), bound (deflateBound as the output space) and tune
(deflateTune on one continuous stream; deflateReset -- all of tune's rows but the untuned ones the others are compared with).  The GPU side is tests/test_gpu_param_cases.py."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import oracle_py as O, paramcases as PC, refzlib as R

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "params_kat.json")))["cases"]


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


@pytest.fixture(scope="module")
def cases():
    return PC.catalogue()


def test_the_catalogue_builds_the_rows_of_the_fixture(cases):
    assert sorted(c.name for c in cases) == sorted(KAT)
    for c in cases:
        r = KAT[c.name]
        assert (r["family"], r["data"]) == (c.family, [len(c.data), h16(c.data)]), c.name
        assert len(r["streams"]) == 1 + sum(1 for st in c.steps if st[0] == "reset"), c.name
        assert len(r["codes"]) == (c.dictionary is not None) + sum(1 for st in c.steps if st[0] in ("deflate", "params", "tune", "reset")), c.name
        if c.like is not None:
            assert c.like in KAT, c.name
    assert all(len(c.data) <= PC.N for c in cases)
    by_feed = [c.feed for c in cases if c.family in ("matrix", "twice", "wraps", "space", "strategy")]
    assert abs(by_feed.count(1024) - by_feed.count(None)) <= len(by_feed) // 5  # (half of the rows leave collected-but-unparsed input at the switch)


def test_the_stated_exclusion_is_the_only_one(cases):
    """matrix = 9 pairs x 6 kinds of preceding call x 2 corpora, less the same-function pairs behind a Z_NO_FLUSH slice (plain or behind a dictionary)."""
    have = {tuple(c.name.split("-")[1:]) for c in cases if c.family == "matrix"}
    want = {("%dto%d" % (a, b), h, kind) for a, b in PC.PAIRS for h in PC.BEHIND for kind in ("sil", "txt") if (a, b, h) not in PC.EXCLUDED}
    assert have == want
    assert PC.EXCLUDED == {(a, b, h) for a, b in ((0, 0), (1, 3), (6, 9)) for h in ("noflush", "dict")}
    assert {(PC.func_of(a), PC.func_of(b)) for a, b in PC.PAIRS} == {(f, g) for f in range(3) for g in range(3)}
    for c in cases:  # nowhere else does a row switch between two levels of one function with unflushed input waiting
        if c.expect != "ref":
            continue
        level, last_flush, total_in = c.level, None, 0
        for st in c.steps:
            if st[0] == "deflate":
                last_flush, total_in = st[2], st[1]
            elif st[0] == "params":
                if PC.func_of(st[1]) == PC.func_of(level) and total_in:
                    assert last_flush != PC.Z_NO_FLUSH, c.name
                level = st[1]


def test_the_restatement_gives_the_fixtures_bytes(cases):
    seen, bad = set(), []
    for c in cases:
        z = PC.restated(c)
        if z is None:
            continue
        seen.add(c.family)
        r = KAT[c.name]["streams"][0]
        if (len(z), h16(z)) != (r["len"], r["sha"]):
            bad.append((c.name, len(z), r["len"]))
    assert seen == {"matrix", "strategy", "twice", "wraps", "carry", "tune"}  # (of tune: the rows without a deflateTune call)
    assert not bad, bad[:20]


@pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref) is not here")
def test_the_compiled_reference_reproduces_the_fixture(cases):
    for c in cases:
        codes, streams, bound = R.play_steps(c)
        r = KAT[c.name]
        assert codes == r["codes"] and bound == r.get("bound"), c.name
        assert [(len(s["z"]), h16(s["z"]), s["total_in"], s["total_out"], s["adler"], s["valid"]) for s in streams] == \
               [(s["len"], s["sha"], s["total_in"], s["total_out"], s["adler"], s["ref_valid"]) for s in r["streams"]], c.name


def test_rows_the_product_owes_the_references_bytes_are_valid_reference_streams(cases):
    """expect == "ref": the reference's stream is complete and inflates to the input.  The rows whose reference stream does not are the ones the
    catalogue says: avail_out == 0 at the switch, and a gzip stream finished into deflateBound() bytes (zlib 1.2.3 answers compressBound())."""
    for c in cases:
        ok = all(s["ref_valid"] for s in KAT[c.name]["streams"])
        if c.expect == "ref" or c.family == "carry":
            assert ok and KAT[c.name]["codes"][-1] == PC.Z_STREAM_END, c.name
        if not ok:
            assert (c.family == "space" and ("avail_out", 0) in c.steps) or (c.family == "bound" and c.wbits == 31), c.name
    for c in cases:  # a switch right behind a flush: the reference answers Z_BUF_ERROR and switches all the same
        if c.family == "matrix" and c.name.split("-")[2] in ("partial", "sync", "full"):
            a, b = c.level, c.steps[1][1]
            assert KAT[c.name]["codes"][1] == (PC.Z_BUF_ERROR if PC.func_of(a) != PC.func_of(b) else PC.Z_OK), c.name


def test_carry_rows_fill_a_block_that_has_left_the_window():
    """At the finish the block that is filling holds at least 12500 tokens and began more than 65536 + 512 bytes back (blocks are cut every 16383 tokens from
    the stream's start, deflate.h:313), nearly all of them matches of length 6 at 16385 bytes or more."""
    for c in PC.carry():
        assert c.strategy == PC.Z_FIXED and c.wbits == -15 and c.feed == 1024
        assert c.steps == (("deflate", len(c.data), PC.Z_NO_FLUSH), ("deflate", len(c.data), PC.Z_FINISH))
        z, t = O.deflate_cont_tokens(c.data, c.level, c.strategy)
        last = len(t) % 16383
        tail = t[len(t) - last:]
        span = int(np.where(tail["dist"] > 0, tail["lc"].astype(np.int64) + 3, 1).sum())
        far6 = int(((tail["dist"] >= 16385) & (tail["lc"] == 3)).sum())
        assert last >= 12500 and span > 65536 + 512 and far6 >= 12500, (c.name, last, span, far6)
        assert far6 * 25 // 8 > 38400  # 7 + 5 + 13 bits a match: more than a feed sized from the 33 KiB window alone has room for (n + n/8 + n/64 + framing)
