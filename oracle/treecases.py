"""Inputs that steer zlib's Huffman tree construction (qcsrc/trees.c:434-701) where ordinary data never takes it.  TEST INFRASTRUCTURE.

Shared by oracle/gen_golden_trees.py and the tests; integer arithmetic on cases.Lcg, so the inputs are the same everywhere.  Every family yields
Case(name, data, strategy, levels, family): `family` says what the row is for --

  lit      the literal/length tree overflows 15 bits in at least one block and goes through gen_bitlen's repair (trees.c:525-566)
  dist     the distance tree does
  both     both trees of ONE block do
  control  the literal tree reaches 15 bits exactly and is NOT repaired
  tie      many equal frequencies: the order in which equal keys leave the heap (trees.c:434-478) decides the lengths
  btype    short inputs on which the stored / static / dynamic choice (trees.c:921-1016) flips, some of them at an equality

How the overflow is made.  A Huffman tree is deeper than 15 only when its frequencies grow like Fibonacci numbers; with plain Fibonacci numbers
zlib's tie-break (equal frequency: the shallower subtree first) flattens the tree again, so the ladder is a(1) = a(2) = 1, a(k) = a(k-1) + a(k-2) + 1:
no internal node ever ties with a leaf.  Sixteen ladder symbols plus the end-of-block symbol (frequency 1) already overflow by 2.

Under Z_HUFFMAN_ONLY (strategy 2) every token is a literal and a block is cut every 16383 tokens, so the literal histogram of block k is the byte
histogram of data[16383 k : 16383 (k + 1)] plus one end-of-block: a test hands the kernel any literal histogram it likes.

For the distance tree the tokens have to be matches the reference's own search finds.  The first block is cases.nomatch(16383): 16383 literals, no
three-byte string twice.  Behind it come copies of four bytes, each of a string of the prefix that is copied once only ("unit" u = prefix[2u : 2u + 4],
two units share no three-byte string), so the one candidate of the search is the original and the distance is the one asked for.  A copy is kept from
growing past four bytes by what follows it (the next unit is chosen to start with another byte than the original goes on with, or a literal >= 0xC0,
which the prefix does not contain, sits in between)."""
from collections import namedtuple

from oracle import cases

Case = namedtuple("Case", "name data strategy levels family")

BLOCK = 16383  # tokens per block: lit_bufsize - 1 (h/deflate.h:308-324)
S2_LEVELS = (1, 6, 9)
DIST_LEVELS = (1, 3, 4, 6, 9)
DIST_BASE = [0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192, 12288, 16384, 24576]
MAX_DIST = 32506


def ladder(k, percent=100):
    """a(1) = a(2) = 1, a(n) = a(n-1) + a(n-2) + 1, every term scaled to `percent` (never below 1), ascending."""
    a = [1, 1]
    while len(a) < k:
        a.append(a[-1] + a[-2] + 1)
    return sorted(max(1, v * percent // 100) for v in a[:k])


def shuffled(counts, seed):
    """counts: [(byte value, count), ...] -> the bytes in a seeded Fisher-Yates order."""
    out = bytearray()
    for b, c in counts:
        out += bytes([b]) * c
    g = cases.Lcg(seed)
    for i in range(len(out) - 1, 0, -1):
        j = g.below(i + 1)
        out[i], out[j] = out[j], out[i]
    return bytes(out)


def pick_symbols(where, k, seed):
    """k distinct byte values: "low" 0.., "high" 144.. (9-bit static codes), "edge" the k values up to 255 (next to end-of-block, 256),
    "spread" seeded over all 256; the order (which value carries which count) is seeded as well."""
    if where == "low":
        vals = list(range(k))
    elif where == "high":
        vals = list(range(144, 144 + k))
    elif where == "edge":
        vals = list(range(256 - k, 256))
    else:
        pool, g = list(range(256)), cases.Lcg(seed + 77)
        vals = [pool.pop(g.below(len(pool))) for _ in range(k)]
    g = cases.Lcg(seed)
    for i in range(k - 1, 0, -1):
        j = g.below(i + 1)
        vals[i], vals[j] = vals[j], vals[i]
    return vals


def ladder_block(where, k, seed, percent=100):
    return shuffled(list(zip(pick_symbols(where, k, seed), ladder(k, percent))), seed)


def filler(n, seed):
    return cases.make("text", n, seed)


def lit_overflow_cases():
    s = 100
    for k in (16, 17, 18):
        for where in ("low", "high", "edge", "spread"):
            s += 1
            yield Case("lit-%d-%s" % (k, where), ladder_block(where, k, s), 2, S2_LEVELS, "lit")
    # 19 symbols fit a block only when scaled (the unscaled ladder has 21871 bytes)
    yield Case("lit-19-spread-70pc", ladder_block("spread", 19, 120, 70), 2, S2_LEVELS, "lit")
    yield Case("lit-19-high-60pc", ladder_block("high", 19, 121, 60), 2, S2_LEVELS, "lit")
    # (two ladders side by side do NOT overflow: their symbols interleave into one shallower tree.  What makes the repair loop run several times is
    #  a longer ladder: 16, 17, 18, 19 symbols overflow by 2, 4, 6, 8.)  A ladder whose five smallest terms (1, 1, 3, 5, 9) are 19 symbols of count 1:
    vals = pick_symbols("spread", 19 + 13, 125)
    yield Case("lit-18-flat-bottom", shuffled(list(zip(vals, [1] * 19 + ladder(18)[5:])), 125), 2, S2_LEVELS, "lit")
    # the position of the repaired block in a stream of several (a block is 16383 bytes here)
    lad18, lad17, lad16 = ladder_block("spread", 18, 131), ladder_block("edge", 17, 132), ladder_block("high", 16, 133)
    top18 = bytes([max(set(lad18), key=lad18.count)])
    full18 = lad18 + top18 * (BLOCK - len(lad18))  # a whole block: the most frequent symbol takes the rest
    yield Case("lit-pos-whole-block", full18, 2, S2_LEVELS, "lit")
    yield Case("lit-pos-2of2-last", filler(BLOCK, 1) + lad17, 2, S2_LEVELS, "lit")
    yield Case("lit-pos-1of3", full18 + filler(BLOCK + 5000, 2), 2, S2_LEVELS, "lit")
    yield Case("lit-pos-2of3", filler(BLOCK, 3) + full18 + filler(7000, 4), 2, S2_LEVELS, "lit")
    yield Case("lit-pos-3of4", filler(2 * BLOCK, 5) + full18 + filler(1, 6), 2, S2_LEVELS, "lit")
    yield Case("lit-pos-3of3-last", filler(2 * BLOCK, 7) + lad16, 2, S2_LEVELS, "lit")
    yield Case("lit-pos-1-and-3of4-64k", full18 + filler(BLOCK, 8) + full18 + lad16 + bytes(65536 - 3 * BLOCK - len(lad16)), 2, S2_LEVELS, "lit")
    # longer than a chunk: the continuous stream meets the repaired block at block 6 and as the last one, chunk mode in chunks of their own
    yield Case("lit-pos-long", filler(5 * BLOCK, 9) + full18 + filler(3 * BLOCK, 10) + lad17, 2, S2_LEVELS, "lit")


def control_cases():
    """Fifteen ladder symbols and the end-of-block symbol: the longest code is 15 bits and nothing overflows."""
    yield Case("control-15-low", ladder_block("low", 15, 141), 2, S2_LEVELS, "control")
    yield Case("control-15-edge", ladder_block("edge", 15, 142), 2, S2_LEVELS, "control")


class _Copies:
    """The copy region behind a nomatch prefix of one or two blocks."""

    def __init__(self, prefix_blocks):
        self.text = bytearray(cases.nomatch(BLOCK * prefix_blocks))
        self.plen = len(self.text)
        self.used = set()
        self.avoid = -1  # the byte the next unit must not start with (the one the last original goes on with)
        self.bucket = {}  # hash of three bytes (deflate.c:170) -> the positions that have it, oldest first: the chains of a search that inserts every position
        self.hashed = 0

    def _hash(self, p):
        t = self.text
        return ((t[p] << 10) ^ (t[p + 1] << 5) ^ t[p + 2]) & 0x7fff

    def _insert_upto(self, q):
        while self.hashed < q and self.hashed + 3 <= len(self.text):
            self.bucket.setdefault(self._hash(self.hashed), []).append(self.hashed)
            self.hashed += 1

    def literal(self, b):
        assert b >= 0xC0
        self.text.append(b)
        self.avoid = -1

    def copy(self, code):
        """Append a four-byte copy whose distance has this distance code; False when no unused unit is in reach."""
        q = len(self.text)
        self._insert_upto(q - 2)
        lo, hi = DIST_BASE[code] + 1, min(DIST_BASE[code + 1] if code < 29 else 32768, MAX_DIST)
        s_hi, s_lo = min(q - lo, self.plen - 6), max(q - hi, 2)  # (position 0 is never a candidate: NIL)
        s = s_lo + (s_lo & 1)
        while s <= s_hi:  # the farthest unit first: the region grows away from it, the near ones stay in reach of later copies
            # (level 1 looks at four candidates of the hash chain and no further, deflate.c:137-149: the original has to be one of them)
            if s not in self.used and self.text[s] != self.avoid and s in self.bucket.get(self._hash(s), ())[-4:]:
                self.used.add(s)
                self.text += self.text[s:s + 4]
                self.avoid = self.text[s + 4]
                return True
            s += 2
        return False


def copy_region(prefix_blocks, codes_counts, literals=(), seed=1):
    """codes_counts: [(distance code, count), ...]; literals: [(byte >= 0xC0, count), ...] spread between the copies, never two in a row.
    The order of the copies is planned (least slack first): a code can be served only while the region has not grown past its distances."""
    c = _Copies(prefix_blocks)
    left = dict(codes_counts)
    lits = bytearray(shuffled(list(literals), seed)) if literals else bytearray()
    total = sum(left.values())
    assert len(lits) <= total
    g = cases.Lcg(seed)
    done = 0
    while left:
        if lits and g.below(total - done) < len(lits):
            c.literal(lits.pop())
        # least slack first: code c can be served only while the region is shorter than its largest distance; what is left of it needs room
        x, step = len(c.text) - c.plen, 5 if literals else 4
        for code in sorted(left, key=lambda k: ((min(DIST_BASE[k + 1] if k < 29 else 32768, MAX_DIST) - x) // step - left[k], k)):
            if c.copy(code):
                left[code] -= 1
                if left[code] == 0:
                    del left[code]
                break
        else:
            raise ValueError("no unit in reach for codes %r at %d" % (sorted(left), len(c.text)))
        done += 1
    for b in lits:  # (whatever the draw left over: one behind the last copy, the rest cannot be placed)
        c.literal(b)
        break
    return bytes(c.text)


def dist_overflow_cases():
    # 17 codes (13..29), the ladder ascending with the code: the rare small distances come first, while the prefix is still near.  The ladder is
    # scaled so that the region stays in reach of the prefix (distances end at 32506) and the whole input fits one 64 KiB chunk.
    for pc in (60, 70):
        yield Case("dist-17-top29-%dpc" % pc, copy_region(1, list(zip(range(13, 30), ladder(17, pc))), seed=17 + pc), 0, DIST_LEVELS, "dist")


def both_cases():
    """The copy block with a literal (values 239..255: none of them in the prefix) in front of some of the copies: 17 literal values, the length code of
    the copies and end-of-block make the literal/length ladder, the 17 distance codes the other one."""
    for lpc in (50, 45):
        lit = list(zip(pick_symbols("edge", 17, 151), ladder(17, lpc)))
        yield Case("both-17dist-17lit-%dpc" % lpc, copy_region(1, list(zip(range(13, 30), ladder(17, 60))), lit, seed=152), 0, DIST_LEVELS, "both")


def _hist_block(vals, counts, seed, cap=BLOCK):
    """A strategy-2 block with these counts, scaled down when they do not fit a block."""
    tot = sum(counts)
    if tot > cap:
        counts = [max(1, c * cap // tot - 1) for c in counts]
    return shuffled(list(zip(vals, counts)), seed)


def tie_cases():
    yield Case("tie-all256-equal", shuffled([(b, 63) for b in range(256)], 201), 2, S2_LEVELS, "tie")
    yield Case("tie-all256-once", bytes(range(256)), 2, S2_LEVELS, "tie")
    s = 210
    for nvals, nsym in ((2, 30), (2, 256), (3, 77), (3, 200), (5, 130), (5, 256)):
        s += 1
        g = cases.Lcg(s)
        base = [1 + g.below(12) for _ in range(nvals)]
        vals = pick_symbols("spread", nsym, s)
        yield Case("tie-%dvalues-%dsyms" % (nvals, nsym), _hist_block(vals, [base[g.below(nvals)] * 4 for _ in range(nsym)], s), 2, S2_LEVELS, "tie")
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    yield Case("tie-fibonacci-19", shuffled(list(zip(pick_symbols("spread", 19, 221), fib)), 221), 2, S2_LEVELS, "tie")
    yield Case("tie-fibonacci-18-high", shuffled(list(zip(pick_symbols("high", 18, 222), fib[:18])), 222), 2, S2_LEVELS, "tie")
    yield Case("tie-powers-of-two-13", shuffled(list(zip(pick_symbols("spread", 13, 223), [1 << i for i in range(13)])), 223), 2, S2_LEVELS, "tie")
    yield Case("tie-powers-of-two-14-full", shuffled(list(zip(pick_symbols("low", 14, 224), [1, 1] + [1 << i for i in range(1, 13)] + [8191])), 224), 2, S2_LEVELS, "tie")
    yield Case("tie-pairs-of-powers", shuffled(list(zip(pick_symbols("spread", 24, 225), [1 << (i // 2) for i in range(24)])), 225), 2, S2_LEVELS, "tie")
    # one or two symbols only: heap_len < 2, the forced codes of trees.c:640-646
    yield Case("tie-one-symbol-0", bytes(1), 2, S2_LEVELS, "tie")
    yield Case("tie-one-symbol-0-run", bytes(300), 2, S2_LEVELS, "tie")
    yield Case("tie-one-symbol-1-run", b"\x01" * 300, 2, S2_LEVELS, "tie")
    yield Case("tie-one-symbol-255-block", b"\xff" * (BLOCK + 9), 2, S2_LEVELS, "tie")
    yield Case("tie-two-symbols", shuffled([(7, 500), (200, 500)], 226), 2, S2_LEVELS, "tie")
    yield Case("tie-two-symbols-1-and-many", shuffled([(0, 1), (255, 4000)], 227), 2, S2_LEVELS, "tie")
    # seeded histograms whose counts come from a small set: ties dominate
    for i in range(200):
        g = cases.Lcg(1000 + i)
        nsym = 3 + g.below(254) if i % 4 else 3 + g.below(40)
        pool = [[1, 2], [1, 2, 3], [1, 2, 4, 8], [3, 5], [1, 1, 1, 2, 16], [2, 3, 5, 8, 13], [7], [1, 64]][g.below(8)]
        mult = 1 + g.below(6)
        vals = pick_symbols("spread", nsym, 1000 + i)
        yield Case("tie-random-%03d" % i, _hist_block(vals, [pool[g.below(len(pool))] * mult for _ in range(nsym)], 1000 + i, cap=6000), 2, (1, 6, 9)[i % 3:i % 3 + 1], "tie")


def btype_cases():
    """Short inputs over small alphabets: the stored / static / dynamic choice flips with the length."""
    lengths = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 23, 26, 30, 35, 40, 48, 56, 64, 80, 100, 128, 160, 200, 256, 330, 420, 512, 700, 1000, 1400, 2000]
    for alpha in (2, 16, 64, 256):
        for strategy in (2, 0):
            for n in lengths:
                g = cases.Lcg(alpha * 100003 + n * 7 + strategy)
                first = g.below(257 - alpha)
                data = bytes(first + g.below(alpha) for _ in range(n))
                yield Case("btype-a%d-s%d-n%d" % (alpha, strategy, n), data, strategy, ((1, 6, 9)[(n + alpha) % 3],), "btype")


FAMILIES = (lit_overflow_cases, control_cases, dist_overflow_cases, both_cases, tie_cases, btype_cases)


def all_cases():
    for fam in FAMILIES:
        yield from fam()
