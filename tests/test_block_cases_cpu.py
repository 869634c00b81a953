"""The block-layer catalogue (oracle/blockcases.py: stored blocks at every bit phase, segments that end on a full block, block cuts on tile edges, more
than 1024 blocks in a batch) on the CPU: the catalogue still builds the rows tests/golden/block_kat.json names and holds every situation it promises;
each row's claims and each pair hold on the restatement's stream, read block by block with oracle/blockwalk.py; the restatement gives the fixture's
bytes; where the compiled reference is at hand it reproduces the fixture; and blockwalk decodes every stream back to its input.
The GPU side is tests/test_gpu_block_cases.py."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import blockcases as BC, blockwalk as BW, deflate_writer as W, oracle_py as O, refzlib as R

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "block_kat.json")))["cases"]


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


@pytest.fixture(scope="module")
def cases():
    return BC.catalogue()


@pytest.fixture(scope="module")
def walked(cases):
    """{name: (the restatement's stream, its block table, what blockwalk decoded, the bytes of the raw stream it used)} -- made once, left unchanged"""
    out = {}
    for c in cases:
        z = BC.restated(c)
        raw = BC.raw_of(c, z)
        blocks, back, used = BW.walk(raw)
        out[c.name] = (z, blocks, back == c.data, used == len(raw))
    return out


def test_the_catalogue_builds_the_rows_of_the_fixture(cases):
    assert sorted(c.name for c in cases) == sorted(KAT)
    for c in cases:
        r = KAT[c.name]
        assert (r["family"], r["data"]) == (c.family, [len(c.data), h16(c.data)]), c.name
        assert c.family == "many" or len(c.data) <= 130 * 1024, c.name
        assert all(0 < u <= len(c.data) for u, _ in c.calls) and [u for u, _ in c.calls] == sorted(u for u, _ in c.calls), c.name
        assert (c.feed is not None) == any(f == BC.Z_NO_FLUSH for _, f in c.calls), c.name


def claimed_phase(c):
    """the phase a phase row names: of its first stored block with bytes, or (14 nine-bit literals) of the static block in its place"""
    for want in (("stored", 0), ("block", -1)):
        for cl in c.claims:
            if cl[:2] == want:
                return cl[2] if want[0] == "stored" else cl[3]


def test_every_situation_of_every_family_is_there(cases):
    for fam, sits in BC.SITUATIONS.items():
        assert {c.situation for c in cases if c.family == fam} == set(sits), fam
    for level in BC.LEVELS:
        mine = [c for c in cases if c.level == level]
        # phase: eight phases per situation (the claim names the stored block's phase; small: on either side of its threshold)
        for sit in BC.SITUATIONS["phase"]:
            rows = [c for c in mine if c.family == "phase" and c.situation == sit]
            for n in ((14, 15) if sit == "small" else (None,)):
                sel = [c for c in rows if n is None or c.name.startswith("phase-small%d-" % n)]
                phases = sorted(claimed_phase(c) for c in sel)
                assert phases == list(range(8)), (level, sit, n, phases)
        # full: every k, offset, kind and ending; the second segment behind every flush; the feeds
        have = {tuple(c.name.split("-")[1:4]) for c in mine if c.family == "full" and c.situation in ("lit", "match")}
        assert have == {("k%d%s" % (k, BC.ETAG[e]), kind, f) for k in (1, 2) for e in (-1, 0, 1) for kind in ("lit", "match") for f in list(BC.FLUSHES) + ["finish"]}, level
        for c in mine:
            if c.family == "full" and c.situation in ("lit", "match") and c.name.split("-")[3] == "finish":  # Z_FINISH ends the one segment: no other call
                assert c.calls == () and c.feed is None, c.name
            elif c.family == "full" and c.situation in ("lit", "match"):
                assert len(c.calls) == 1 and c.calls[0][1] == BC.FLUSHES[c.name.split("-")[3]] and len(c.data) > c.calls[0][0], c.name
        assert {c.name for c in mine if c.situation.startswith("feed-")} == {"full-feed-last1-k1-L%d" % level, "full-feed-last1-k2-L%d" % level,
                                                                               "full-feed-carry16382-L%d" % level, "full-feed-carry0-L%d" % level}
        # edge: both edges x three offsets x both kinds of token (the match 129 bytes over the edge as well), the Z_HUFFMAN_ONLY rows
        have = {(cl[2], cl[3]) for c in mine if c.family == "edge" for cl in c.claims if cl[0] == "end"}
        assert have == {(edge + e, ll) for edge, _ in BC.TILE_EDGES for e in (-1, 0, 1) for ll in (1, 258)} | {(edge + 129, 258) for edge, _ in BC.TILE_EDGES}, level
        assert sum(1 for c in mine if c.family == "edge" and c.strategy == BC.Z_HUFFMAN_ONLY) == 2
    assert [c.name for c in cases if c.family == "many"] == ["many-huff-L6"]
    assert {c.wbits for c in cases if c.family == "phase"} == {-15, 15, 31}


def test_the_inputs_parse_into_the_tokens_they_are_built_for(cases):
    """The token list of the restatement (compress2's, so: of a row's first segment alone) has the count and the last token the builders promise."""
    seen = set()
    for c in cases:
        if c.family == "full" and c.situation in ("lit", "match"):
            seg = c.data[: c.calls[0][0]] if c.calls else c.data
            key = (c.level, seg)
            if key in seen:
                continue
            seen.add(key)
            tag = c.name.split("-")[1]
            k, e = int(tag[1]), {v: q for q, v in BC.ETAG.items()}[tag[2:]]
            t = O.deflate_cont_tokens(seg, c.level)[1]
            assert len(t) == BC.NTOK * k + e, c.name
            assert (int(t["dist"][-1]), int(t["lc"][-1]) + 3) == (5000, 50) if c.situation == "match" else t["dist"][-1] == 0, c.name
            assert int((t["dist"] > 0).sum()) == (c.situation == "match"), c.name
        elif c.family == "edge" and c.situation in ("lit", "match"):
            t = O.deflate_cont_tokens(c.data, c.level)[1]
            end = np.cumsum(np.where(t["dist"] > 0, t["lc"].astype(np.int64) + 3, 1))
            (_, i, want_end, want_len), = [cl for cl in c.claims if cl[0] == "end"]
            q = BC.NTOK * (i + 1) - 1
            assert int(end[q]) == want_end and (int(t["lc"][q]) + 3 if t["dist"][q] else 1) == want_len, c.name
            assert all(int(d) == 1 for d in t["dist"][: q + 1][t["dist"][: q + 1] > 0]), c.name
        elif c.strategy == BC.Z_HUFFMAN_ONLY and c.family == "edge":
            assert len(O.deflate_cont_tokens(c.data, c.level, c.strategy)[1]) == len(c.data), c.name


def test_blockwalk_decodes_every_stream_back_to_its_input(cases, walked):
    for c in cases:
        z, blocks, same, used_all = walked[c.name]
        assert same and used_all, c.name
        assert blocks[0].bit == 0 and all(a.end_bit == b.bit and a.end_pos == b.pos for a, b in zip(blocks, blocks[1:])), c.name
        rc, back = O.inflate_raw(BC.raw_of(c, z), len(c.data) + 8)[:2]  # (the restatement's own inflate agrees)
        assert rc == 1 and back == c.data, c.name


def test_blockwalk_reads_what_the_writer_wrote():
    """blockwalk against oracle/deflate_writer.py on streams no encoder of the catalogue emits: a stored block at every phase behind raw bits, a match that
    overlaps itself, static and dynamic blocks with distances, an empty dynamic block; and it refuses what is not a stream."""
    toks = [65, 66, 67, (5, 3), (258, 1), 200, 255, (3, 9)]
    plain = W.expand(toks)
    for ph in range(8):
        z = W.stream([W.fixed(toks)] + [W.fixed([])] * ph + [W.stored(b"xyz" * 5), W.dynamic(toks + [(10, 20)]), W.dynamic([]), W.stored(b"", final=True)])
        blocks, back, used = BW.walk(z)
        assert back == plain + b"xyz" * 5 + W.expand(toks + [(10, 20)], plain + b"xyz" * 5) and used == len(z)
        st = blocks[1 + ph]
        assert (st.btype, st.nbytes, st.ntok, st.last_len) == (BW.STORED, 15, None, None)
        assert st.bit == blocks[0].end_bit + 10 * ph and st.phase == st.bit & 7 and st.end_bit % 8 == 0
        assert [(b.btype, b.ntok, b.nbytes, b.last_len, b.final) for b in blocks[2 + ph:]] == [(2, 9, len(plain) + 10, 10, 0), (2, 0, 0, None, 0), (0, None, 0, None, 1)]
        assert (blocks[0].ntok, blocks[0].nbytes, blocks[0].last_len) == (8, len(plain), 3)
    good = W.stream([W.fixed(toks, final=True)])
    for broken in (good[:-2], W.stream([W.raw_bits(7, 3)]), W.stream([W.stored(b"ab", final=True, nlength=0)]), W.stream([W.fixed([65, (3, 2)], final=True)])):
        with pytest.raises(ValueError):
            BW.walk(broken)


def test_claims_hold_on_the_restatements_streams(cases, walked):
    bad = []
    for c in cases:
        assert c.claims, c.name
        bad += BC.check(c, walked[c.name][1])
    assert not bad, bad[:20]


def test_pairs_differ_the_way_they_say(cases, walked):
    groups = {}
    for c in cases:
        if c.pair:
            groups.setdefault(c.pair[0], {})[c.pair[1]] = c
    assert len(groups) == 40 + 16  # (small: 8 phases x 5 levels; full: k x (three flushes, Z_FINISH alone) x the level pairs 4 / 1 and 6 / 3)
    for g, sides in groups.items():
        assert sorted(sides) == [0, 1] and sides[0].pair[2] == sides[1].pair[2], g
        a, b = sides[0], sides[1]
        assert a.calls == b.calls and (a.data == b.data or a.pair[2] == "stored"), g
        assert BC.pair_holds(a.pair[2], walked[a.name][1], walked[b.name][1], segments=len(a.calls) + 1), g


def test_the_restatement_gives_the_fixtures_bytes(cases, walked):
    bad = [(c.name, len(walked[c.name][0]), KAT[c.name]["len"]) for c in cases if (len(walked[c.name][0]), h16(walked[c.name][0])) != (KAT[c.name]["len"], KAT[c.name]["sha"])]
    assert not bad, bad[:20]


@pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref) is not here")
def test_the_compiled_reference_reproduces_the_fixture(cases):
    for c in cases:
        z = R.deflate_calls(c.data, c.level, list(c.calls), wbits=c.wbits, strategy=c.strategy)
        assert (len(z), h16(z)) == (KAT[c.name]["len"], KAT[c.name]["sha"]), c.name


def test_slicing_the_input_does_not_change_the_stream(cases):
    """tests/test_gpu_block_cases.py also hands a row over in pieces of 30011 bytes with Z_NO_FLUSH: the reference's stream is the same (shown here on the
    restatement, for one row of every situation)."""
    seen = set()
    for c in cases:
        if (c.family, c.situation) in seen or c.family == "many":
            continue
        seen.add((c.family, c.situation))
        cuts = sorted(set(c.calls) | {(q, BC.Z_NO_FLUSH) for q in range(30011, len(c.data), 30011) if q not in [u for u, _ in c.calls]})
        assert O.cont_stream(c.data, c.level, cuts, wbits=c.wbits, strategy=c.strategy) == BC.restated(c), c.name
