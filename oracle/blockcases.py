"""Inputs that put the BLOCK LAYER of one continuous stream on its thresholds: what turns a stream's tokens into blocks and bits (the reference:
qcsrc/deflate.c FLUSH_BLOCK :1364-1381, the ends of deflate_fast :1544 and deflate_slow :1667-1672, trees.c _tr_flush_block :921-1021,
_tr_stored_block :867-879, _tr_align :892-915; the product: chains 2-4 of zlib_amd/csrc/zgpu_cont.hip and the CONT side of huffman_kernel).
TEST INFRASTRUCTURE, pure Python + numpy, deterministic.

Shared by oracle/gen_golden_blocks.py and the tests.  catalogue() returns Case rows:

  name       unique
  family     phase | full | edge | many
  situation  what the row is an instance of (the CPU test asserts that every situation of a family is there, see SITUATIONS)
  data       the input
  level, strategy, wbits    deflateInit2's arguments (memLevel 8)
  calls      [(upto, flush), ...] as oracle_py.deflate_cont / cont_stream and refzlib.deflate_calls take them; the Z_FINISH call is implied
  feed       ZAMD_FEED_BYTES for the product's host library (None: its default): with 1024 a Z_NO_FLUSH call of `calls` is handed to the engine at once,
             which parses up to 512 bytes in front of the call's end and carries the tokens of the block that is filling to the next feed
  claims     statements about the block table of the REFERENCE's stream, checked with oracle/blockwalk.py by check():
               ("stored", n, phase, final)    the n-th stored block that holds bytes starts at that bit phase and has that BFINAL
               ("stored_bytes", n)            there are exactly n stored blocks that hold bytes
               ("block", i, btype, phase)     block i (negative: from the end) has that type and starts at that phase (None: at any)
               ("ntok", i, n)                 block i holds n tokens
               ("end", i, end_pos, last_len)  block i ends behind input position end_pos, and its last token is last_len bytes long
               ("ends", [end_pos, ...])       the blocks that cover bytes end at these positions, in order, the last one at the input's end
               ("behind_stored", n)           the block behind the n-th stored block with bytes is a coded one and starts inside a 32-bit word
               ("layout", [...])              the whole table: per segment the token counts of its coded blocks, between two segments the marker of
                                              the flush: "partial" (one or two empty static blocks, trees.c:892-915) or "stored" (an empty stored block)
               ("count", n)                   the stream has n blocks
               ("layout_marker", i)           block i is a flush's empty stored block
               ("many", blocks, stored, phases)  more than `blocks` blocks, at least `stored` stored ones at no fewer than `phases` distinct phases
  pair       (group, side, how) or None: the two sides of a group sit on either side of ONE threshold; how their block tables must differ:
               "one more"  side 1 has, per segment, exactly one block more than side 0, an empty static one (the fast levels' flush behind a block that
                           has just been flushed full, against deflate_slow's last literal that fills the block behind the loop)
               "stored"    side 0's last block is static, side 1's stored (15 nine-bit literals: 15 + 4 <= (3 + 9 * 15 + 7 + 7) >> 3, trees.c:972)

How an input is put together.
  FILL     parsecases.FILLER: 102000 bytes of 0..131 in which no trigram occurs twice -- every token is a literal at every level, so a token count is a
           byte count; its blocks are dynamic ones of about 5.8 bits a byte.
  rnd      SHAKE-256 bytes: blocks of them are stored.
  runs     one byte of 132..255, then m more of it: a literal and ONE match (distance 1, length m, 3 <= m <= 258) at every level -- deflate_slow finds the
           match one position behind the literal and, m being the whole rest of the run, nothing longer one position on.  The same byte returns only after
           124 other runs, more than MAX_DIST on.
  nine     bytes of 200 and up: nine bits each in a static block.

Families (every row at the slow levels 4, 6, 9 and the fast levels 1, 3, except where a family says otherwise).
  phase    a stored block that starts at every bit phase 0..7.  i nine-bit bytes, one "a" and Z_PARTIAL_FLUSH put the next block at phase
           (3 + 9 i + 8 + 7 + 10) & 7 = (4 + i) & 7.  Situations:
             partial      17000 random bytes behind the flush: the feed's first block is stored, at the phase, not final; the last is stored at phase 0;
             final        2000 random bytes behind it: the one stored block is the stream's last;
             then-coded   2000 + r random bytes, another Z_PARTIAL_FLUSH (coded: its marker), filler: r is chosen so that the stored block ends 1, 2 or 3
                          bytes into a 32-bit word.  The marker is written by the host side, so for the kernels this is once more a feed that starts
                          inside a word (the filler's block), now behind a stored block; a coded block STITCHED behind a stored one inside one batch
                          is situation cut-then-coded (and many);
             small        15 nine-bit bytes behind the flush: the smallest stored block there is (see "left out"); 14 of them are a static block (pair);
             cut          no flush: 16383 filler literals, a dynamic block cut by its 16383rd token, then 17000 random bytes.  FILL[j: j + 16383] for
                          j = 0, 1, 2, ... gives the dynamic block other code lengths: the j that ends it at each phase is searched, all eight are found;
             cut-then-coded  the same with 3000 filler bytes behind the random ones: dynamic, stored at the phase, and in one batch a dynamic block that
                          starts in the stored block's last word (j is searched per level and phase so that the stored block ends 1, 2 or 3 bytes into
                          a word: how many bytes its 16383 tokens cover depends on the level's few matches in random bytes).
           wbits: -15 at levels 1, 4, 9, 15 at level 3 and 31 at level 6 -- the stream's header stands in the first word of the output.
  full     a segment whose token count at its end is 16383 k - 1, 16383 k, 16383 k + 1 (k = 1, 2), reached by a literal ("lit") or by a match ("match":
           the segment's last 50 bytes are a copy from 5000 back).  "finish" rows are that one segment and no call but Z_FINISH: compress2()'s stream, whose
           final block is the full block or the empty one behind it.  The other rows have two segments: the first ends with Z_PARTIAL_FLUSH, Z_SYNC_FLUSH
           or Z_FULL_FLUSH, the second (k = 1, the same offset and kind, the count starts again at the flush) with Z_FINISH.  layout says what
           gen_golden_fullblock.py found for chunks: deflate_slow tallies a last literal behind its loop, so a block that this literal fills is the
           segment's last; every other way to 16383 k tokens is followed by an empty static block.
             feed-last1       the last byte of 16383 k literals arrives in a call of its own, the bytes in front with Z_NO_FLUSH and feed = 1024: the
                              block that the last feed closes stands in the carry but for its last 513 tokens;
             feed-carry16382  32766 literals, the first call hands over 16382 + 512: 16382 tokens are carried, the next feed's first token fills the block;
             feed-carry0      32766 literals, the first call hands over 16383 + 512: the first feed emits a full block and carries nothing.
           (A feed never parses nearer than 512 bytes to its input's end, so the last byte alone cannot be all that a feed adds to 16382 carried tokens.)
           No full row is longer than one tile (49249 bytes at the most), so the batch settings of the GPU test change nothing for this family.
  edge     the 16383 k-th token ends at a tile edge - 1, at it, + 1, for the edges 65024 (k = 3) and 97536 (k = 5); filler with evenly spread runs makes up
           the bytes.  "lit": that token is a literal, random bytes follow (the next tile, and with one tile per batch the next batch, begins with a stored
           block at whatever phase the block leaves).  "match": it is a run's match of 258 bytes, which starts in front of the edge; + 129 as well, so the next
           tile is entered deep inside it; filler follows.  Z_HUFFMAN_ONLY rows (every byte a token; filler, then random bytes: dynamic and stored blocks):
             huff-cuts       the first call hands over 16382 + 512 bytes (feed = 1024): 16382 tokens are carried.  The next feed's first tile parses the
                             positions 16382 .. 65023 (a feed's first tile ends at position 65024 of its buffer, wherever it is entered), 48642 tokens:
                             three cuts, at its tokens 0, 16383 and 32766.  (Three is the most a tile can hold with every byte a token: 65024 < 4 * 16383.)
             huff-tile-last  Z_SYNC_FLUSH at 65024 - 3 * 16383 = 15875 starts the token count again: the next feed's first tile parses 15875 .. 65023,
                             49149 tokens with nothing carried -- three cuts, the third is the tile's last token.  Without a flush block ends are multiples
                             of 16383 under Z_HUFFMAN_ONLY and never meet 65024 or 97536; at the other levels edge-65024+0-lit and edge-97536+0-lit are this
                             situation (the block's last token is a literal that ends the tile).
  many     one row, level 6, Z_HUFFMAN_ONLY, 17.1 MB: stretches of random bytes (150000 .. 250000) and of letters drawn with a text's frequencies
           (10000 .. 35000), so that more than 1024 blocks -- stored, and dynamic ones of changing length -- stand in one batch; the last block holds 30
           letters and is a static one (a block of 16383 literals never is: a dynamic code is always shorter there).

Left out, and why.
  * The stored-block veto (k.nostore, cont_slides, cont_special).  At windowBits 15 it cannot decide a byte of output: it needs a block that starts more
    than 32506 bytes in front of where the loop stands when the block is flushed, which with at most 16383 tokens is at least two bytes a token.  Such a
    block's code stays well below its stored size: a literal costs at most nine bits for eight, a match of three bytes or more costs under 24 bits even at
    a distance with 13 extra bits (7 + 5 + 13 = 25 bits for length 3 is the one exception, and deflate_slow drops it: TOO_FAR), and half the tokens must be
    matches.  Z_FIXED does not help: trees.c:972 compares the stored size with the smaller of the dynamic and the static size and only then forces
    static; 32508 bytes of mostly nine-bit literals under Z_FIXED come out as static blocks.  Small windows are the geometry path's business.
  * A stored block of 65535 bytes, and one of 1 byte.  Levels 1-9 cannot write either.  65535 bytes in 16383 tokens are four bytes a token, 32 bits stored;
    a token costs at most 31 bits in a static block (a literal 9, a match 8 + 5 for the length and 5 + 13 for the distance).
    A stored block of n bytes needs n + 4 <= (3 + bits + 7) >> 3 with at most 9 n + 7 static bits: n >= 15 (the pair of situation small).
    Level 0 writes blocks of up to 65531 bytes (65536 - 5, deflate.c:1397-1402) and of 1 byte, but in the host library (zamd_zlib.c cont_stored), not in
    the kernels this catalogue is for; tests/test_gpu_continuous.py and the paramcases rows 0>x cover it.
  * carry_n == 16382 in front of a feed that brings only the segment's last byte: see family full.
  * deflateParams in the middle: oracle/paramcases.py."""
import hashlib
from collections import namedtuple

from oracle import blockwalk as BW
from oracle import cases
from oracle import parsecases as PA

Z_NO_FLUSH, Z_PARTIAL_FLUSH, Z_SYNC_FLUSH, Z_FULL_FLUSH, Z_FINISH = 0, 1, 2, 3, 4
Z_HUFFMAN_ONLY = 2
NTOK = 16383                       # lit_bufsize - 1 at memLevel 8 (deflate.h:313)
TILE_EDGES = ((65024, 3), (97536, 5))  # (edge, the k whose block ends there)
SLOW, FAST = (4, 6, 9), (1, 3)
LEVELS = SLOW + FAST
ETAG = {-1: "m1", 0: "e0", 1: "p1"}  # (in a full row's name: 16383 k - 1, 16383 k, 16383 k + 1 tokens)
FLUSHES = {"partial": Z_PARTIAL_FLUSH, "sync": Z_SYNC_FLUSH, "full": Z_FULL_FLUSH}
PHASE_WBITS = {1: -15, 3: 15, 4: -15, 6: 31, 9: -15}
FILL = PA.FILLER.tobytes()

SITUATIONS = {
    "phase": ("partial", "final", "then-coded", "small", "cut", "cut-then-coded"),
    "full": ("lit", "match", "feed-last1", "feed-carry16382", "feed-carry0"),
    "edge": ("lit", "match", "huff-cuts", "huff-tile-last"),
    "many": ("many",),
}

Case = namedtuple("Case", "name family situation data level strategy wbits calls feed claims pair")


def rnd(n, seed=0):
    """n bytes no compressor gets anything out of"""
    return hashlib.shake_256(b"blockcases %d" % seed).digest(n)


def nine(i, base=200):
    return bytes(base + j for j in range(i))


def phase_of(i):
    """the phase behind i nine-bit literals, an eight-bit one, the end-of-block and Z_PARTIAL_FLUSH's marker (static codes: 3 + 9 i + 8 + 7, + 10)"""
    return (3 + 9 * i + 8 + 7 + 10) & 7


def _case(name, family, situation, data, level, claims, calls=(), strategy=0, wbits=-15, feed=None, pair=None):
    return Case(name, family, situation, data, level, strategy, wbits, tuple(calls), feed, list(claims), pair)


# ---- reading a row's stream ----
def restated(case):
    """the row's stream by the CPU restatement"""
    from oracle import oracle_py as O
    return O.cont_stream(case.data, case.level, list(case.calls), wbits=case.wbits, strategy=case.strategy)


def raw_of(case, z):
    """the raw deflate stream inside the row's wrapper"""
    return z if case.wbits < 0 else z[10:-8] if case.wbits > 15 else z[2:-4]


def expected_blocks(ntok, last_is_literal, slow):
    """The token counts of the coded blocks of a segment of ntok tokens (see family full)."""
    out = [NTOK] * (ntok // NTOK)
    if ntok % NTOK:
        out.append(ntok % NTOK)
    elif not (slow and last_is_literal):
        out.append(0)
    return out


def check(case, blocks):
    """The row's claims against a block table (blockwalk.walk(...)[0]): a list of what does not hold."""
    bad = []
    with_bytes = [k for k, b in enumerate(blocks) if b.btype == BW.STORED and b.nbytes]
    for c in case.claims:
        what = c[0]
        try:
            if what == "stored":
                b = blocks[with_bytes[c[1]]]
                ok = (b.phase, bool(b.final)) == (c[2], c[3])
            elif what == "stored_bytes":
                ok = len(with_bytes) == c[1]
            elif what == "block":
                b = blocks[c[1]]
                ok = b.btype == c[2] and c[3] in (None, b.phase)
            elif what == "ntok":
                ok = blocks[c[1]].ntok == c[2]
            elif what == "end":
                b = blocks[c[1]]
                ok = (b.end_pos, b.last_len) == (c[2], c[3])
            elif what == "ends":
                ok = [b.end_pos for b in blocks if b.nbytes] == list(c[1])
            elif what == "behind_stored":
                b, nxt = blocks[with_bytes[c[1]]], blocks[with_bytes[c[1]] + 1]
                ok = nxt.btype != BW.STORED and nxt.bit == b.end_bit and nxt.bit % 32 != 0
            elif what == "layout":
                ok = _layout_holds(blocks, c[1])
            elif what == "count":
                ok = len(blocks) == c[1]
            elif what == "layout_marker":
                b = blocks[c[1]]
                ok = (b.btype, b.nbytes, bool(b.final)) == (BW.STORED, 0, False)
            elif what == "many":
                st = [b for b in blocks if b.btype == BW.STORED]
                ok = len(blocks) > c[1] and len(st) >= c[2] and len({b.phase for b in st}) >= c[3]
            else:
                raise ValueError(what)
        except IndexError:
            ok = False
        if not ok:
            bad.append("%s: %r does not hold" % (case.name, c))
    if not blocks or not blocks[-1].final or any(b.final for b in blocks[:-1]) or blocks[-1].end_pos != len(case.data):
        bad.append("%s: the table does not end with the one final block at the input's end" % case.name)
    return bad


def _layout_holds(blocks, layout):
    i = 0
    for part in layout:
        if part == "stored":
            if not (i < len(blocks) and blocks[i].btype == BW.STORED and blocks[i].nbytes == 0 and not blocks[i].final):
                return False
            i += 1
        elif part == "partial":
            if not (i < len(blocks) and (blocks[i].btype, blocks[i].ntok) == (BW.STATIC, 0)):
                return False
            i += 1
            if i + 1 < len(blocks) and (blocks[i].btype, blocks[i].ntok) == (BW.STATIC, 0) and blocks[i + 1].ntok:  # (the marker twice: trees.c:906-913)
                i += 1
        else:
            for n in part:
                if not (i < len(blocks) and blocks[i].btype != BW.STORED and blocks[i].ntok == n and (n or blocks[i].btype == BW.STATIC)):
                    return False
                i += 1
    return i == len(blocks)


def pair_holds(how, side0, side1, segments=1):
    """side0, side1: the block tables of a pair's two rows; segments: how many segments (flushes + 1) each row has"""
    if how == "one more":
        empty = [sum(1 for b in t if (b.btype, b.ntok) == (BW.STATIC, 0)) for t in (side0, side1)]
        return len(side1) == len(side0) + segments and empty[1] == empty[0] + segments and [b.ntok for b in side0 if b.ntok] == [b.ntok for b in side1 if b.ntok]
    if how == "stored":
        return side0[-1].btype == BW.STATIC and side1[-1].btype == BW.STORED and side0[-1].phase == side1[-1].phase
    raise ValueError(how)


# ---- phase ----
_memo = {}


def _first_blocks(data, level, calls=(), n=None):
    from oracle import oracle_py as O
    return BW.walk(O.deflate_cont(data, level, list(calls)), max_blocks=n)[0]


def then_coded_r(i):
    """how many random bytes put the end of the stored block 1 + i % 3 bytes into a word (the stored block's place does not depend on the level: the
    blocks in front of it hold literals only)"""
    if ("r", i) not in _memo:
        for r in range(2000, 2004):
            d = nine(i) + b"a" + rnd(r, 200 + i) + FILL[:3000]
            st = [b for b in _first_blocks(d, 6, [(i + 1, Z_PARTIAL_FLUSH), (i + 1 + r, Z_PARTIAL_FLUSH)]) if b.btype == BW.STORED and b.nbytes]
            if st[0].end_bit % 32 == 8 * (1 + i % 3):
                _memo["r", i] = r
                break
    return _memo["r", i]


def cut_offsets():
    """{phase: j}: FILL[j: j + 16383] as the stream's first block ends at that phase (all-literal, so at every level)."""
    if "cut" not in _memo:
        found = {}
        for j in range(200):
            b = _first_blocks(FILL[j: j + NTOK] + rnd(64, 300), 6, n=1)[0]
            assert (b.btype, b.ntok) == (BW.DYNAMIC, NTOK)
            found.setdefault(b.end_bit & 7, j)
            if len(found) == 8:
                break
        assert sorted(found) == list(range(8)), found
        _memo["cut"] = found
    return _memo["cut"]


def cut_coded_data(j):
    return FILL[j: j + NTOK] + rnd(17000, 500) + FILL[30000: 33000]


def cut_coded_offsets(level):
    """{phase: j}: in cut_coded_data(j) at this level the stored block starts at that phase and ends inside a 32-bit word"""
    if ("cutc", level) not in _memo:
        found = {}
        for j in range(400):
            b = _first_blocks(cut_coded_data(j), level, n=3)
            if (b[0].ntok, b[1].btype) == (NTOK, BW.STORED) and b[2].btype != BW.STORED and b[1].end_bit % 32 and b[1].phase not in found:
                found[b[1].phase] = j
                if len(found) == 8:
                    break
        assert sorted(found) == list(range(8)), (level, found)
        _memo["cutc", level] = found
    return _memo["cutc", level]


def phase():
    out = []
    for level in LEVELS:
        wbits = PHASE_WBITS[level]
        for i in range(8):
            p = phase_of(i)
            head, flush = nine(i) + b"a", [(i + 1, Z_PARTIAL_FLUSH)]
            tag = "p%d-L%d" % (p, level)
            out.append(_case("phase-partial-" + tag, "phase", "partial", head + rnd(17000, i), level,
                             [("stored", 0, p, False), ("stored", -1, 0, True), ("block", 1, BW.STATIC, (p - 10) & 7)], flush, wbits=wbits))
            out.append(_case("phase-final-" + tag, "phase", "final", head + rnd(2000, 100 + i), level,
                             [("stored", 0, p, True), ("stored_bytes", 1)], flush, wbits=wbits))
            r = then_coded_r(i)
            out.append(_case("phase-then-coded-" + tag, "phase", "then-coded", head + rnd(r, 200 + i) + FILL[:3000], level,
                             [("stored", 0, p, False), ("stored_bytes", 1), ("behind_stored", 0)], flush + [(i + 1 + r, Z_PARTIAL_FLUSH)], wbits=wbits))
            for n in (14, 15):
                out.append(_case("phase-small%d-%s" % (n, tag), "phase", "small", head + nine(n, 230), level,
                                 [("stored", 0, p, True), ("stored_bytes", 1)] if n == 15 else [("stored_bytes", 0), ("block", -1, BW.STATIC, p)], flush,
                                 wbits=wbits, pair=("small-" + tag, n - 14, "stored")))
        for p, j in sorted(cut_offsets().items()):
            out.append(_case("phase-cut-p%d-L%d" % (p, level), "phase", "cut", FILL[j: j + NTOK] + rnd(17000, 300 + p), level,
                             [("block", 0, BW.DYNAMIC, 0), ("ntok", 0, NTOK), ("stored", 0, p, False), ("stored", -1, 0, True)], wbits=wbits))
        for p, j in sorted(cut_coded_offsets(level).items()):
            out.append(_case("phase-cut-then-coded-p%d-L%d" % (p, level), "phase", "cut-then-coded", cut_coded_data(j), level,
                             [("block", 0, BW.DYNAMIC, 0), ("ntok", 0, NTOK), ("stored", 0, p, False), ("stored_bytes", 1), ("behind_stored", 0), ("count", 3)], wbits=wbits))
    return out


# ---- full ----
def segment(kind, ntok, o):
    """ntok tokens at every level, the last one a literal ("lit") or a match of 50 bytes from 5000 back"""
    if kind == "lit":
        return FILL[o: o + ntok]
    m = ntok - 1
    return FILL[o: o + m] + FILL[o + m - 5000: o + m - 5000 + 50]


def full():
    out = []
    for level in LEVELS:
        slow = level in SLOW
        for k in (1, 2):
            for e in (-1, 0, 1):
                for kind in ("lit", "match"):
                    for fname, flush in FLUSHES.items():
                        s1, s2 = segment(kind, NTOK * k + e, 0), segment(kind, NTOK + e, 40000)
                        lay = [expected_blocks(NTOK * k + e, kind == "lit", slow), "partial" if fname == "partial" else "stored", expected_blocks(NTOK + e, kind == "lit", slow)]
                        pair = None
                        if e == 0 and kind == "lit" and level in (4, 1, 6, 3):
                            pair = ("full-k%d-%s-L%s" % (k, fname, "4v1" if level in (4, 1) else "6v3"), int(not slow), "one more")
                        claims = [("layout", lay)]
                        if fname != "partial":
                            claims.append(("count", len(lay[0]) + 1 + len(lay[2])))
                        out.append(_case("full-k%d%s-%s-%s-L%d" % (k, ETAG[e], kind, fname, level), "full", kind, s1 + s2, level, claims, [(len(s1), flush)], pair=pair))
                    # one segment, no flush: what compress2() makes of it -- the full block (or the empty one behind it) is the stream's final block
                    lay = expected_blocks(NTOK * k + e, kind == "lit", slow)
                    pair = None
                    if e == 0 and kind == "lit" and level in (4, 1, 6, 3):
                        pair = ("full-k%d-finish-L%s" % (k, "4v1" if level in (4, 1) else "6v3"), int(not slow), "one more")
                    out.append(_case("full-k%d%s-%s-finish-L%d" % (k, ETAG[e], kind, level), "full", kind, segment(kind, NTOK * k + e, 0), level,
                                     [("layout", [lay]), ("count", len(lay))], pair=pair))
        for k in (1, 2):
            n = NTOK * k
            lay = expected_blocks(n, True, slow)
            out.append(_case("full-feed-last1-k%d-L%d" % (k, level), "full", "feed-last1", FILL[:n], level, [("layout", [lay]), ("count", len(lay))], [(n - 1, Z_NO_FLUSH)], feed=1024))
        lay = expected_blocks(2 * NTOK, True, slow)
        for sit, upto in (("feed-carry16382", NTOK - 1 + 512), ("feed-carry0", NTOK + 512)):
            out.append(_case("full-%s-L%d" % (sit, level), "full", sit, FILL[: 2 * NTOK], level, [("layout", [lay]), ("count", len(lay))], [(upto, Z_NO_FLUSH)], feed=1024))
    return out


# ---- edge ----
def run_lengths(extra):
    """match lengths (3..258 each) whose runs cover `extra` bytes more than they have tokens: a run of 1 + m bytes is two tokens"""
    a, b = divmod(extra, 257)
    lens = [258] * a
    if b >= 2:
        lens.append(b + 1)
    elif b == 1:
        lens[-1:] = [257, 3]
    return lens


def tokens_to(ntok, nbytes, last):
    """Bytes that are ntok tokens over nbytes bytes at every level: filler literals and evenly spread runs; the last token is a literal, or
    ("match") the 258 bytes of a run."""
    lens = run_lengths(nbytes - ntok)
    lens.sort()  # (the short ones first: a 258 is last)
    nlit = ntok - 2 * len(lens)
    gaps = len(lens) + (1 if last == "lit" else 0)
    base, more = divmod(nlit, gaps)
    out, o = bytearray(), 0
    for q, m in enumerate(lens):
        g = base + (1 if q < more else 0)
        out += FILL[o: o + g]
        o += g
        out += bytes([132 + q % 124]) * (1 + m)
    if last == "lit":
        out += FILL[o: o + base]
        o += base
    else:
        assert lens[-1] == 258
    assert len(out) == nbytes and o == nlit
    return bytes(out), o


def edge():
    out = []
    for level in LEVELS:
        for edge_pos, k in TILE_EDGES:
            for kind in ("lit", "match"):
                for e in (-1, 0, 1) + ((129,) if kind == "match" else ()):
                    body, o = tokens_to(NTOK * k, edge_pos + e, kind)
                    tail = rnd(3000, edge_pos + e) if kind == "lit" else FILL[o: o + 3000]
                    claims = [("ntok", k - 1, NTOK), ("end", k - 1, edge_pos + e, 1 if kind == "lit" else 258)]
                    if kind == "lit":
                        claims.append(("stored_bytes", 1))
                    out.append(_case("edge-%d%+d-%s-L%d" % (edge_pos, e, kind, level), "edge", kind, body + tail, level, claims))
        n = 50000
        d = FILL[:n] + rnd(90000 - n, 400)
        ends = [NTOK * (q + 1) for q in range(len(d) // NTOK)] + [len(d)]
        out.append(_case("edge-huff-cuts-L%d" % level, "edge", "huff-cuts", d, level, [("ends", ends)], [(NTOK - 1 + 512, Z_NO_FLUSH)], strategy=Z_HUFFMAN_ONLY, feed=1024))
        at = 65024 - 3 * NTOK
        ends = [at] + [at + NTOK * (q + 1) for q in range((len(d) - at) // NTOK)] + [len(d)]
        out.append(_case("edge-huff-tile-last-L%d" % level, "edge", "huff-tile-last", d, level, [("ends", ends), ("layout_marker", 1)], [(at, Z_SYNC_FLUSH)],
                         strategy=Z_HUFFMAN_ONLY))
    return out


# ---- many ----
def letters(n, seed):
    """n bytes drawn with a text's letter frequencies (per 256: space 45, e 26, t 19, a 17, ...)"""
    freq = (" " * 45 + "e" * 26 + "t" * 19 + "a" * 17 + "o" * 16 + "i" * 15 + "n" * 15 + "s" * 13 + "h" * 13 + "r" * 12 + "d" * 9 + "l" * 8 + "c" * 6 + "u" * 6 +
            "m" * 5 + "w" * 5 + "f" * 5 + "g" * 4 + "y" * 4 + "p" * 4 + "b" * 3 + "v" * 2 + "k" * 1 + ".,\n")
    assert len(freq) == 256
    return rnd(n, seed).translate(freq.encode())


def many():
    g = cases.Lcg(7)
    parts, total, q = [], 0, 0
    while total < 1045 * NTOK:
        a, b = 150000 + g.below(100000), 10000 + g.below(25000)
        parts += [rnd(a, 1000 + q), letters(b, 2000 + q)]
        total += a + b
        q += 1
    parts.append(letters((30 - total) % NTOK, 3000))  # (the last block: 30 letters, a static one)
    return [_case("many-huff-L6", "many", "many", b"".join(parts), 6, [("many", 1024, 100, 4), ("block", -1, BW.STATIC, None), ("ntok", -1, 30)], strategy=Z_HUFFMAN_ONLY)]


FAMILIES = (phase, full, edge, many)
_catalogue = None


def catalogue():
    global _catalogue
    if _catalogue is None:
        out = [c for f in FAMILIES for c in f()]
        assert len({c.name for c in out}) == len(out)
        _catalogue = out
    return _catalogue
