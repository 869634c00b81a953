"""GPU: the hand-over between the feeds of one continuous stream (zlib_amd/host/zamd_zlib.c deflate / deflateParams / deflateTune / deflateReset /
deflateBound carrying the block that is filling, the chains' bits, the list of positions that are in no chain, cs.entry / block_start / floor_pos, the
running checks and a feed's output capacity into zgpu_deflate_cont_host and the zgpu_cont.hip kernels) on every row of oracle/paramcases.py, played
through libzamd_z.so by zhost.play_steps against the compiled reference's record in tests/golden/params_kat.json (tests/test_param_cases_cpu.py shows
that the rows are what they say and that the restatement and the reference agree on them).

What a row owes (Case.expect):
  ref     the fixture's return codes call by call (the Z_BUF_ERROR of a switch right behind a flush included), its bytes bit for bit, strm->adler,
          total_in, total_out; the stream inflates back through the product.
  like    space rows.  avail_out == 0: deflateParams answers Z_BUF_ERROR and CHANGES NOTHING, the same call with space then answers what the ample-space
          row's call answers, and the finished stream is that row's, byte for byte.  This is later zlib's contract, not 1.2.3's: the reference sets the
          new level all the same, its stream depends on where its loop stood and for 0 > 1-9 does not inflate (ref_valid false) -- DESIGN.md section 2.
          avail_out == 7: the flush's output stays pending, the call answers Z_OK, the stream is the ample-space row's.
  error   the product refuses the call with Z_STREAM_ERROR and the stream goes on untouched: deflateParams to Z_RLE at levels 1-3 (served in chunks
          only), and -- the choice made here for a deflateTune in the middle of a level 1-3 continuous stream, which the engine cannot serve
          bit-exactly -- deflateTune itself answers the error and the stream finishes to the untuned row's bytes.
  bound   deflate(Z_FINISH) into exactly deflateBound() bytes answers Z_STREAM_END, deflateBound is never below the reference's figure, and where the
          reference's own stream fitted (it does not in a gzip wrapper, 18 bytes of framing against the 6 it counts) the bytes are the reference's.
  chunks  deflateTune before the first byte of a level 1-3 stream: served in independent 64 KiB chunks ("Not modelled"), checked
          against the restatement's chunk streams with the tuned row; the stream behind deflateReset is the reference's continuous one again.

One test per family, every failure of the family in one report: the row's name and the first differing bit.

Found by these rows beyond the host library: a switch from a level 4-9 to a level 1-3 whose flushed part ended on a match.  The reference's deflate_fast then
searches with the prev_length of 0 deflate_slow left behind (deflate.c:1035, 1630-1636) and takes a first candidate only if the byte in front of it equals the
byte in front of the string; 16 rows (all matrix rows 6>1 behind input, twice-1to9sync1-txt-*, space-6to1-*) gave valid but smaller streams, e.g.
matrix-6to1-noflush-sil 108567 bytes for 116482, first differing bit 259072, until fastwin_tile_kernel learnt it (zgpu_deflate_cont_set_stale)."""
import hashlib
import json
import os

import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_py as O, paramcases as PC  # noqa: E402
import zhost as Z  # noqa: E402

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "params_kat.json")))["cases"]
CASES = {c.name: c for c in PC.catalogue()}


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


def first_diff_bit(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return 8 * i + ((a ^ b) & -(a ^ b)).bit_length() - 1
    return 8 * min(len(got), len(want))


def family(name):
    return [c for c in CASES.values() if c.family == name]


def same_stream(bad, c, what, z, want_row, expected):
    """z against a fixture stream record; `expected`: the same bytes from the restatement where it has them, for the report only"""
    if (len(z), h16(z)) != (want_row["len"], want_row["sha"]):
        where = first_diff_bit(z, expected) if expected is not None and (len(expected), h16(expected)) == (want_row["len"], want_row["sha"]) else "n/a"
        bad.append("%s: %s: %d bytes, expected %d; first differing bit %s" % (c.name, what, len(z), want_row["len"], where))
        return False
    return True


def inflates(bad, c, z, data):
    rc, back = Z.inflate_stream(z, len(data) + 8, window_bits=c.wbits, dictionary=c.dictionary if c.wbits < 0 else None)[:2]
    if (rc, back) != (Z.Z_STREAM_END, data):
        bad.append("%s: the product's inflate of the stream: rc %d, %d bytes of %d" % (c.name, rc, len(back), len(data)))


def owes_ref(bad, c, got=None):
    """expect == "ref": codes, bytes, totals and the way back"""
    codes, streams, _ = got or Z.play_steps(c)
    r = KAT[c.name]
    assert all(s["ref_valid"] for s in r["streams"]), c.name
    if codes != r["codes"]:
        bad.append("%s: return codes %s, the reference's %s" % (c.name, codes, r["codes"]))
    for k, (s, w) in enumerate(zip(streams, r["streams"])):
        data = c.data if k == 0 else c.data2
        same_stream(bad, c, "stream %d" % k, s["z"], w, PC.restated(c) if k == 0 else None)
        if (s["total_in"], s["total_out"], s["adler"]) != (w["total_in"], w["total_out"], w["adler"]):
            bad.append("%s: total_in, total_out, adler = %s, the reference's %s" % (c.name, (s["total_in"], s["total_out"], s["adler"]), (w["total_in"], w["total_out"], w["adler"])))
        if s["z"]:
            inflates(bad, c, s["z"], data)


def report(bad):
    assert not bad, "%d failures\n" % len(bad) + "\n".join(bad[:40])


def test_matrix():
    bad = []
    for c in family("matrix"):
        owes_ref(bad, c)
    report(bad)


def test_strategy():
    bad = []
    for c in family("strategy"):
        if c.expect == "ref":
            owes_ref(bad, c)
            continue
        codes, streams, _ = Z.play_steps(c)  # Z_RLE at levels 1-3: refused, nothing changes
        want = list(KAT[c.name]["codes"])
        want[1] = Z.Z_STREAM_ERROR
        if codes != want:
            bad.append("%s: return codes %s, expected %s" % (c.name, codes, want))
        untouched = PC.restated(c, with_params=False)
        if streams[0]["z"] != untouched:
            bad.append("%s: not the stream of the same calls without deflateParams: %d bytes against %d, first differing bit %d" %
                       (c.name, len(streams[0]["z"]), len(untouched), first_diff_bit(streams[0]["z"], untouched)))
        inflates(bad, c, streams[0]["z"], c.data)
    report(bad)


def test_twice():
    bad = []
    for c in family("twice"):
        owes_ref(bad, c)
    report(bad)


def test_wraps():
    bad = []
    for c in family("wraps"):
        owes_ref(bad, c)
    report(bad)


def owes_like(bad, c):
    """expect == "like" (family space)"""
    like = KAT[c.like]
    assert CASES[c.like].expect == "ref" and all(s["ref_valid"] for s in like["streams"]), c.name
    codes, streams, _ = Z.play_steps(c)
    if ("avail_out", 0) in c.steps:  # [the call in front, the refused switch, the switch, the finish]
        want = [like["codes"][0], Z.Z_BUF_ERROR] + like["codes"][1:]
    else:
        want = list(like["codes"])
        assert want[1] == Z.Z_OK, c.name
    if codes != want:
        bad.append("%s: return codes %s, expected %s" % (c.name, codes, want))
    w = like["streams"][0]
    same_stream(bad, c, "against " + c.like, streams[0]["z"], w, PC.restated(c, lenient=True))
    s = streams[0]
    if (s["total_in"], s["total_out"], s["adler"]) != (w["total_in"], w["total_out"], w["adler"]):
        bad.append("%s: total_in, total_out, adler = %s, expected %s" % (c.name, (s["total_in"], s["total_out"], s["adler"]), (w["total_in"], w["total_out"], w["adler"])))
    inflates(bad, c, s["z"], c.data)


def test_space():
    bad = []
    for c in family("space"):
        owes_like(bad, c)
    report(bad)


def test_carry():
    bad = []
    for c in family("carry"):
        owes_ref(bad, c)
    report(bad)


def test_bound():
    bad = []
    for c in family("bound"):
        r = KAT[c.name]
        codes, streams, said = Z.play_steps(c)
        s = streams[0]
        if codes != [Z.Z_STREAM_END]:
            bad.append("%s: deflate(Z_FINISH) into deflateBound() = %d bytes answers %s with %d bytes out" % (c.name, said, codes, s["total_out"]))
            continue
        if s["total_out"] > said or said < r["bound"]:
            bad.append("%s: deflateBound %d, the reference's %d, the stream %d" % (c.name, said, r["bound"], s["total_out"]))
        if r["streams"][0]["ref_valid"]:
            same_stream(bad, c, "the stream", s["z"], r["streams"][0], PC.restated(c, lenient=True))
        inflates(bad, c, s["z"], c.data)
    report(bad)


def chunk_streams(data, level, tune):
    n = max(1, (len(data) + 65535) // 65536)
    return b"".join(O.deflate_chunk(data[k * 65536:(k + 1) * 65536], level, k + 1 == n, tune=tune) for k in range(n))


def test_tune():
    bad = []
    for c in family("tune"):
        r = KAT[c.name]
        if c.expect == "ref":
            owes_ref(bad, c)
        elif c.expect == "error":  # deflateTune in the middle of a level 1-3 continuous stream: refused, the stream is the untuned row's
            codes, streams, _ = Z.play_steps(c)
            like = KAT[c.like]
            want = list(r["codes"])
            want[1] = Z.Z_STREAM_ERROR
            if codes != want:
                bad.append("%s: return codes %s, expected %s" % (c.name, codes, want))
            same_stream(bad, c, "against " + c.like, streams[0]["z"], like["streams"][0], PC.restated(CASES[c.like]))
            inflates(bad, c, streams[0]["z"], c.data)
        else:  # "chunks": the tuned level 1-3 stream in chunks, the stream behind deflateReset the reference's
            codes, streams, _ = Z.play_steps(c)
            if codes != r["codes"]:
                bad.append("%s: return codes %s, the reference's %s" % (c.name, codes, r["codes"]))
            want = chunk_streams(c.data, c.level, PC.TUNE)
            if streams[0]["z"] != want:
                bad.append("%s: the tuned stream is not the chunk streams': %d bytes against %d, first differing bit %d" %
                           (c.name, len(streams[0]["z"]), len(want), first_diff_bit(streams[0]["z"], want)))
            inflates(bad, c, streams[0]["z"], c.data)
            if len(streams) > 1:
                s, w = streams[1], r["streams"][1]
                same_stream(bad, c, "the stream behind deflateReset", s["z"], w, O.deflate_cont(c.data2, c.level, [(50000, 0)]))
                if (s["total_in"], s["total_out"], s["adler"]) != (w["total_in"], w["total_out"], w["adler"]):
                    bad.append("%s: behind deflateReset total_in, total_out, adler = %s, the reference's %s" %
                               (c.name, (s["total_in"], s["total_out"], s["adler"]), (w["total_in"], w["total_out"], w["adler"])))
                inflates(bad, c, s["z"], c.data2)
    report(bad)
