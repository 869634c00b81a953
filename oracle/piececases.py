"""A deterministic catalogue of hand-built LONG batch items (oracle/deflate_writer.py) for the piece path of the blocking batch decode
(zlib_amd/csrc/zgpu_inflate_batch_pieces.hip): the shapes zlib's encoder never writes at these sizes.

TEST INFRASTRUCTURE ONLY.  Every case is laid out for ZGPU_BATCH_PIECES_MIN_BYTES=49153, the smallest body that can be long: spacing 32768, finders 16384
bytes apart, a piece start 24576 bytes or more behind the one before it and more than 8192 bytes before the item's end.  A finder reports only the first
dynamic start and the first vouched stored start of its 16 KiB region, so the blocks are laid out for every intended start to be the first of its kind
in its region, wherever in a buffer (and behind which wrapper's header) the item lies: tests/test_piece_cases_cpu.py checks that without a GPU.

`catalogue()` returns the cases in a fixed order; each has
    name    unique
    stream  the raw deflate bytes (bytes behind the final block included, where a case has them)
    expect  the bytes a decoder must produce (None: not a valid stream)
    kind    "ok" | "bad" (a data error) | "cut" (ends before its final block)
    msg     zlib's message for a bad case ("" otherwise)
    starts  [(bit, "d" | "s")]: the block starts the case means to have selected as piece starts behind the first -- "d": the first header bit of a
            dynamic block, "s": the first bit of the LEN of a stored block -- counted from the first bit of the stream
    went    (1, 0): decoded in pieces; (0, 1): falls back to the one-workgroup decoder; None: either
    tail    bytes of the item behind the stream (`stream` ends with them; wrapped() puts them behind the trailer)
    wraps   the wrappers the case is laid out for
    blocks, block_bits, block_out   the block list, the bit every block starts at (and the bit the last one ends at), the bytes every block decodes to
    planted [bit]: dynamic block headers that are data (inside a stored block): what a finder reports besides the true starts
    group   "P1" ... "P7", "pool"
`pool()` returns ok cases of graded length for the many-item tests.  Seeded bytes come from handmade.rnd / rint; nothing is stored.
"""
import struct
import zlib

import numpy as np

from oracle import deflate_writer as W
from oracle.deflate_writer import dynamic, fixed, literals, stored, tokens
from oracle.handmade import rint, rnd

MIN_BYTES = 49153        # what the tests set ZGPU_BATCH_PIECES_MIN_BYTES to
SPACING, FSPACING = 32768, 16384
APART, BEFORE_END = SPACING * 6 // 8, SPACING * 2 // 8   # bytes between two piece starts at least; a start lies more than this before the end


class PieceCase:
    def __init__(self, name, group, blocks, toks, starts, went, kind="ok", msg="", tail=b"", planted=(), wraps=("raw", "zlib", "gzip")):
        self.name, self.group, self.kind, self.msg, self.went, self.tail, self.wraps = name, group, kind, msg, went, tail, wraps
        self.blocks = blocks
        self.block_bits = W.block_starts(blocks)
        self.deflate_bytes = (self.block_bits[-1] + 7) // 8   # where the final block ends, in whole bytes
        self.stream = W.stream(blocks) + tail
        self.expect = W.expand(toks) if kind == "ok" else None
        self.starts = [(self.start_of(i), k) for i, k in starts]
        self.start_blocks = [i for i, _ in starts]
        self.block_out = [len(b["data"]) if b["t"] == "stored" else int((b["toks"].kind == W.LIT).sum() + b["toks"].a[b["toks"].kind == W.MATCH].sum()) for b in blocks]
        self.planted = list(planted)

    def wrapped(self, wrap):
        """the item in the wrapper `wrap`: header, deflate data, trailer (of a bad case: that of no bytes), then the bytes that are none of the stream's"""
        data = self.expect or b""
        body = self.stream[: self.deflate_bytes]
        if wrap == "zlib":
            return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(data)) + self.tail
        if wrap == "gzip":
            return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF) + self.tail
        return self.stream

    def start_of(self, i):
        """the bit a piece that begins with block i starts at: a stored block's LEN, a dynamic block's first header bit"""
        b = self.block_bits[i]
        return (b + 3 + 7) // 8 * 8 if self.blocks[i]["t"] == "stored" else b


# ---------------------------------------------------------------------------- building blocks
_PAD_N = {}


def skewed(n, seed):
    """n seeded bytes, about a fifth of them from eight values: incompressible but for a few per cent, and their Huffman codes have several lengths"""
    b, c = rnd(n, seed), rnd(n, seed + 7777)
    return np.where(c < 48, b & 7, b).astype(np.uint8)


def head_for_pad(seed, base_n, pad, at_bit=0):
    """skewed literals, base_n or a few more, whose dynamic block -- begun at bit `at_bit` -- ends where a stored header has `pad` padding bits behind its
    three bits (the literals' codes differ in length, so a few more of them reach every bit of the byte)"""
    key = (seed, base_n)
    if key not in _PAD_N:
        data, found = skewed(base_n + 400, seed), {}
        for n in range(base_n, base_n + 400):
            found.setdefault(W.block_starts([dynamic(literals(data[:n]))])[-1] % 8, n)
            if len(found) == 8:
                break
        assert len(found) == 8, (seed, base_n, sorted(found))
        _PAD_N[key] = found
    return skewed(base_n + 400, seed)[: _PAD_N[key][(-(at_bit + 3 + pad)) % 8]]


def far_tail(seed, first, nlit=300):
    """tokens of a small block that begins with `first` (matches that reach far back), then random literals and a few more far matches"""
    lit = rnd(nlit, seed)
    r = rint(4, 0, 1 << 30, seed + 1)
    out = list(first) + [int(x) for x in lit[: nlit // 2]]
    for i in range(4):
        out += [(3 + int(r[i]) % 256, 32768 - int(r[i]) % 300), int(lit[nlit // 2 + i])]
    out += [int(x) for x in lit[nlit // 2 + 4:]]
    return tokens(out)


FAR3 = [(258, 32768), (3, 32767), (258, 1)]


# ---------------------------------------------------------------------------- P1: a stored start behind p padding bits
def p1_blocks(seed, pad, padval=0, s1=17408, s2=8192, final=None):
    head = head_for_pad(seed, 27200, pad)
    d1, d2 = rnd(s1, seed + 1), rnd(s2, seed + 2)
    blocks = [dynamic(literals(head)), stored(d1.tobytes(), pad=padval), stored(d2.tobytes())]
    toks = literals(head) + literals(d1) + literals(d2)
    if final is None:
        t = far_tail(seed + 3, FAR3)
        blocks.append(dynamic(t, final=True))
        toks = toks + t
    else:
        blocks.append(final[0])
        toks = toks + final[1]
    assert (W.block_starts(blocks)[1] + 3 + pad) % 8 == 0
    return blocks, toks


def p1():
    cs = []
    for p in range(8):
        b, t = p1_blocks(1100 + 10 * p, p)
        cs.append(PieceCase("p1_pad%d" % p, "P1", b, t, [(1, "s")], (1, 0)))
    for p in range(4, 8):  # the lowest padding bit set: the sieve vouches (the byte's top three bits are zero), the chain's link rule refuses
        b, t = p1_blocks(1200 + 10 * p, p, padval=1)
        cs.append(PieceCase("p1_pad%d_low_bit_set" % p, "P1", b, t, [(1, "s")], (0, 1)))
    # the highest padding bit set: the sieve does not vouch for the first stored block; it does for the second, which lies far enough behind the start
    p = 5
    b, t = p1_blocks(1300, p, padval=1 << (p - 1))
    cs.append(PieceCase("p1_pad%d_top_bit_set" % p, "P1", b, t, [(2, "s")], None))
    return cs


# ---------------------------------------------------------------------------- P2: pieces shorter than the window
def p2():
    seed = 2000
    head = rnd(8192, seed)
    blocks, toks = [dynamic(literals(head))], literals(head)
    starts = []

    def two_stored(k, final):
        nonlocal toks
        for j in range(2):
            d = rnd(12800, seed + 10 * k + j + 1)
            blocks.append(stored(d.tobytes(), final=final and j == 1))
            toks = toks + literals(d)
    two_stored(0, False)
    for k in range(1, 5):
        lit = rnd(520, seed + 10 * k + 5)
        first = []
        for j, d in enumerate((32768, 32767, 25601, 1)):
            first += [(40 + j, d), int(lit[j])]
        t = tokens(first + [int(x) for x in lit[4:]] + [(258, 30000 - 7 * j) for j in range(5)] + [int(lit[0])])
        starts.append((len(blocks), "d"))
        blocks.append(dynamic(t))
        toks = toks + t
        two_stored(k, k == 4)
    return [PieceCase("p2_short_pieces", "P2", blocks, toks, starts, (1, 0))]


# ---------------------------------------------------------------------------- P3: how far the second piece may reach back
def p3():
    cs = []
    for name, n, dist, ok in (("p3_25200_reach_25200", 25200, 25200, True), ("p3_25200_reach_25201", 25200, 25201, False),
                              ("p3_32768_reach_32768", 32768, 32768, True), ("p3_32767_reach_32768", 32767, 32768, False)):
        seed = 3000 + 10 * len(cs)
        head = rnd(n, seed)
        second = tokens([(3, dist)]) + literals(rnd(20000, seed + 1))
        last = literals(rnd(9000, seed + 2)) + tokens([(258, 32768), 5])
        toks = literals(head) + second + last
        blocks = [dynamic(literals(head)), dynamic(second), dynamic(last, final=True)]
        cs.append(PieceCase(name, "P3", blocks, toks, [(1, "d")], (1, 0) if ok else (0, 1), kind="ok" if ok else "bad",
                            msg="" if ok else "invalid distance too far back"))
    return cs


# ---------------------------------------------------------------------------- P4: marker floods
FLOOD = 8000


def p4():
    cs = []
    for dist in (1, 7):
        seed = 4000 + dist
        head, mid, end = rnd(25000, seed), rnd(700, seed + 1), rnd(25000, seed + 2)
        flood = tokens([(258, dist)] * FLOOD) + literals(mid)
        toks = literals(head) + flood + literals(end)
        blocks = [dynamic(literals(head)), dynamic(flood), dynamic(literals(end), final=True)]
        cs.append(PieceCase("p4_flood_dist%d" % dist, "P4", blocks, toks, [(1, "d")], (1, 0)))
    return cs


# ---------------------------------------------------------------------------- P6: the final block ends at bit k of its byte
def p6():
    cs = []
    for k in range(8):
        # a fixed block behind a stored one begins a byte: 3 header bits, 8 per literal below 144, 9 per literal from 144 on, 7 for the end of the block
        nine = (k - 10) % 8
        lits = [65 + k, 66, 67] + [200 + j for j in range(nine)]
        t = tokens(lits)
        b, toks = p1_blocks(6000 + 10 * k, k, final=(fixed(t, final=True), t))
        c = PieceCase("p6_final_ends_at_bit%d" % k, "P6", b, toks, [(1, "s")], (1, 0), tail=b"\xa5\x5a\xc3")
        assert c.block_bits[-1] % 8 == k
        cs.append(c)
    return cs


# ---------------------------------------------------------------------------- P7: finder decoys
def p7():
    cs = []
    # a: bytes behind the final stored block that read as a stored header: the sieve vouches for the final block's LEN as for any other
    seed = 7000
    a, d = rnd(25000, seed), rnd(12288, seed + 2)
    # (three padding bits in front of the final block's LEN: its BFINAL bit stays out of the top three bits of that byte, which the sieve wants zero)
    b2 = head_for_pad(seed + 1, 28000, 3, at_bit=W.block_starts([dynamic(literals(a))])[-1])
    blocks = [dynamic(literals(a)), dynamic(literals(b2)), stored(d.tobytes(), final=True)]
    toks = literals(a) + literals(b2) + literals(d)
    cs.append(PieceCase("p7_decoy_header_behind_final_stored", "P7", blocks, toks, [(1, "d"), (2, "s")], None, tail=b"\x00\x10\x00\xef\xff",
                        wraps=("raw",)))
    # b: a whole dynamic block, header and all, as data of a vouched stored block; the true dynamic start behind the stored block is the one to select
    seed = 7100
    a = rnd(17000, seed)
    inner = W.stream([dynamic(literals(rnd(600, seed + 1)))])
    data = bytearray(rnd(32900, seed + 2).tobytes())
    at = 19000
    data[at: at + len(inner)] = inner
    c2, tail = rnd(25000, seed + 3), far_tail(seed + 4, FAR3)
    blocks = [dynamic(literals(a)), stored(bytes(data)), dynamic(literals(c2)), dynamic(tail, final=True)]
    toks = literals(a) + literals(bytes(data)) + literals(c2) + tail
    c = PieceCase("p7_dynamic_block_inside_stored", "P7", blocks, toks, [(2, "d")], (1, 0))
    c.planted = [c.start_of(1) + 32 + 8 * at]
    cs.append(c)
    return cs


# ---------------------------------------------------------------------------- pool
POOL_BODIES = (49153, 52801, 57000, 61999, 66000, 70500, 74001, 78000, 82000)


def pool_case(i, length):
    """an ok case whose raw deflate stream has exactly `length` bytes: literals, a stored block that is selected, for the longer ones a further dynamic
    block that is selected, a small block of far matches, a final stored block that fills up"""
    seed = 8000 + 100 * i
    head = head_for_pad(seed, 27200, i % 8)
    d1 = rnd(17408, seed + 1)
    blocks = [dynamic(literals(head)), stored(d1.tobytes())]
    toks = literals(head) + literals(d1)
    starts = [(1, "s")]
    if length >= 70000:
        l1 = literals(rnd(8000, seed + 2))
        l2 = tokens([(258, 1), (3, 32768)]) + literals(rnd(10000, seed + 3))
        starts.append((3, "d"))
        blocks += [dynamic(l1), dynamic(l2)]
        toks = toks + l1 + l2
    t = far_tail(seed + 4, FAR3)
    blocks.append(dynamic(t))
    toks = toks + t
    len_at = (W.block_starts(blocks)[-1] + 3 + 7) // 8
    fill = rnd(length - len_at - 4, seed + 5)
    blocks.append(stored(fill.tobytes(), final=True))
    toks = toks + literals(fill)
    c = PieceCase("pool%d_%d" % (i, length), "pool", blocks, toks, starts, (1, 0))
    assert len(c.stream) == length
    return c


_CACHE = {}


def catalogue():
    if "cat" not in _CACHE:
        cs = p1() + p2() + p3() + p4() + p6() + p7()
        names = [c.name for c in cs]
        assert len(set(names)) == len(names), "duplicate case names"
        _CACHE["cat"] = cs
    return _CACHE["cat"]


def pool():
    if "pool" not in _CACHE:
        _CACHE["pool"] = [pool_case(i, n) for i, n in enumerate(POOL_BODIES)]
    return _CACHE["pool"]


def by_name(name):
    return next(c for c in catalogue() + pool() if c.name == name)
