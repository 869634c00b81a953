"""A reader of a raw DEFLATE stream (RFC 1951) that reports its BLOCKS: where each one's header stands, what kind it is, how many tokens and bytes
it holds, how long its last token is, where the bits behind its end-of-block stand.  TEST INFRASTRUCTURE ONLY, pure Python, written from the RFC
with the tables of oracle/deflate_writer.py.

walk(z) returns (blocks, data, used): one Block per block up to and including the one with BFINAL set, the bytes the stream decodes to, and how
many bytes of z were read.

  bit       bit offset of the header's first bit (BFINAL); bit & 7 is the phase the block starts at
  final     BFINAL
  btype     0 stored, 1 static, 2 dynamic
  ntok      tokens in front of the end-of-block (None for a stored block: it has bytes, no tokens)
  nbytes    bytes the block covers
  last_len  bytes of its last token (1: a literal; None for a stored block or a block with no token)
  end_bit   bit offset behind the end-of-block (behind the last byte of a stored block)
  pos       bytes of output in front of the block; end_pos = pos + nbytes

Between two blocks nothing is skipped: a block's header stands where the one in front ended (walk asserts nothing about it, it is how the
stream is read).  Bits behind the final block (a last byte's padding, a trailer) are left alone; walk reports how many bytes it used."""
from collections import namedtuple

import numpy as np

from oracle import deflate_writer as W

STORED, STATIC, DYNAMIC = 0, 1, 2
NAMES = {STORED: "stored", STATIC: "static", DYNAMIC: "dynamic"}


class Block(namedtuple("Block", "bit final btype ntok nbytes last_len end_bit pos")):
    __slots__ = ()

    @property
    def phase(self):
        return self.bit & 7

    @property
    def end_pos(self):
        return self.pos + self.nbytes

    def __str__(self):
        return "%s%s at bit %d (phase %d): bytes %d..%d, %s tokens, last %s, ends at bit %d" % (
            NAMES[self.btype], " final" if self.final else "", self.bit, self.bit & 7, self.pos, self.end_pos, self.ntok, self.last_len, self.end_bit)


def _table(lens):
    """Lookup by the next `bits` bits of the stream (LSB first): (symbol << 4) | code length, 0 where no code begins."""
    lens = [int(x) for x in lens]
    bits = max(lens) if lens else 0
    if bits == 0:
        return [0], 0
    if sum(1 << (bits - l) for l in lens if l) > (1 << bits):
        raise ValueError("over-subscribed code")
    codes = W.canonical_codes(lens)  # (bit-reversed: the value as it stands in the stream)
    t = np.zeros(1 << bits, dtype=np.int64)
    for s, l in enumerate(lens):
        if l:
            t[codes[s]:: 1 << l] = (s << 4) | l
    return t.tolist(), bits


_FIXED = None


def _fixed_tables():
    global _FIXED
    if _FIXED is None:
        _FIXED = _table(W.FIXED_LIT) + _table(W.FIXED_DIST[:30] + [0, 0])
    return _FIXED


def _peek(z, pos):
    """at least 56 bits of the stream from bit `pos` on"""
    b = pos >> 3
    return int.from_bytes(z[b: b + 8], "little") >> (pos & 7)


def _code_lengths(z, pos):
    """The header of a dynamic block behind its three type bits: (literal/length lengths, distance lengths, bit offset behind them)."""
    v = _peek(z, pos)
    hlit, hdist, hclen = (v & 31) + 257, ((v >> 5) & 31) + 1, ((v >> 10) & 15) + 4
    pos += 14
    cl = [0] * 19
    for i in range(hclen):
        cl[W.CL_ORDER[i]] = _peek(z, pos) & 7
        pos += 3
    tab, bits = _table(cl)
    mask = (1 << bits) - 1
    lens = []
    while len(lens) < hlit + hdist:
        v = _peek(z, pos)
        e = tab[v & mask]
        if not e & 15:
            raise ValueError("no code-length code at bit %d" % pos)
        pos += e & 15
        s = e >> 4
        v >>= e & 15
        if s < 16:
            lens.append(s)
        elif s == 16:
            if not lens:
                raise ValueError("repeat with nothing in front at bit %d" % pos)
            lens += [lens[-1]] * (3 + (v & 3))
            pos += 2
        elif s == 17:
            lens += [0] * (3 + (v & 7))
            pos += 3
        else:
            lens += [0] * (11 + (v & 127))
            pos += 7
    if len(lens) != hlit + hdist:
        raise ValueError("a run of code lengths goes past HLIT + HDIST")
    return lens[:hlit], lens[hlit:], pos


def _coded(z, pos, out, ltab, lbits, dtab, dbits, toks=None):
    """The tokens of a coded block from bit `pos` on, appended to `out`: (tokens, length of the last one, bit offset behind the end-of-block).
    toks: a list that receives every token as (position, dist, length), a literal as (position, 0, 1)."""
    lmask, dmask = (1 << lbits) - 1, (1 << dbits) - 1
    lbase, lext, dbase, dext = W.LEN_BASE, W.LEN_EXTRA, W.DIST_BASE, W.DIST_EXTRA
    from_bytes = int.from_bytes
    ntok, last, nz = 0, None, 8 * len(z)
    while True:
        b = pos >> 3
        v = from_bytes(z[b: b + 8], "little") >> (pos & 7)
        e = ltab[v & lmask]
        n = e & 15
        s = e >> 4
        if n == 0 or pos + n > nz:
            raise ValueError("no literal/length code at bit %d" % pos)
        if s < 256:
            if toks is not None:
                toks.append((len(out), 0, 1))
            out.append(s)
            pos += n
            ntok += 1
            last = 1
            continue
        if s == 256:
            return ntok, last, pos + n
        if s > 285:
            raise ValueError("length symbol %d at bit %d" % (s, pos))
        v >>= n
        x = lext[s - 257]
        length = lbase[s - 257] + (v & ((1 << x) - 1))
        v >>= x
        used = n + x
        e = dtab[v & dmask]
        n = e & 15
        if n == 0 or (e >> 4) > 29:
            raise ValueError("no distance code at bit %d" % (pos + used))
        v >>= n
        x = dext[e >> 4]
        dist = dbase[e >> 4] + (v & ((1 << x) - 1))
        pos += used + n + x
        if dist > len(out):
            raise ValueError("distance %d with %d bytes in front, at bit %d" % (dist, len(out), pos))
        if toks is not None:
            toks.append((len(out), dist, length))
        if dist >= length:
            o = len(out) - dist
            out += out[o: o + length]
        else:
            piece = bytes(out[len(out) - dist:])
            out += (piece * (length // dist + 1))[:length]
        ntok += 1
        last = length
        if pos > nz:
            raise ValueError("the stream ends inside a token")


def walk(z, max_blocks=None, toks=None):
    """(blocks, data, bytes of z used) -- see the module's text.  Raises ValueError on a stream that is not valid or ends before a final block.
    toks: a list that receives the tokens of the coded blocks, (position, dist, length) each."""
    z = bytes(z)
    out = bytearray()
    blocks = []
    pos = 0
    while True:
        if pos + 3 > 8 * len(z):
            raise ValueError("the stream ends in front of a block header at bit %d" % pos)
        v = _peek(z, pos)
        final, btype = v & 1, (v >> 1) & 3
        start, at = len(out), pos
        if btype == STORED:
            p = (pos + 3 + 7) >> 3
            if p + 4 > len(z):
                raise ValueError("the stream ends inside a stored block's header at bit %d" % pos)
            n, nn = z[p] | (z[p + 1] << 8), z[p + 2] | (z[p + 3] << 8)
            if n ^ nn != 0xFFFF:
                raise ValueError("LEN / NLEN of the stored block at bit %d" % pos)
            if p + 4 + n > len(z):
                raise ValueError("the stream ends inside the stored block at bit %d" % pos)
            out += z[p + 4: p + 4 + n]
            pos = 8 * (p + 4 + n)
            blocks.append(Block(at, final, btype, None, n, None, pos, start))
        elif btype == 3:
            raise ValueError("block type 3 at bit %d" % pos)
        else:
            if btype == STATIC:
                ltab, lbits, dtab, dbits = _fixed_tables()
                p = pos + 3
            else:
                ll, dl, p = _code_lengths(z, pos + 3)
                if ll[256] == 0:
                    raise ValueError("no end-of-block code in the block at bit %d" % pos)
                ltab, lbits = _table(ll)
                dtab, dbits = _table(dl)
            ntok, last, pos = _coded(z, p, out, ltab, lbits, dtab, dbits, toks)
            blocks.append(Block(at, final, btype, ntok, len(out) - start, last, pos, start))
        if final or (max_blocks is not None and len(blocks) >= max_blocks):
            return blocks, bytes(out), (pos + 7) >> 3


def first_difference(got, want):
    """For a report: the first block of `want` (a valid stream) that `got` does not share bit for bit, as text."""
    n = min(len(got), len(want))
    k = next((i for i in range(n) if got[i] != want[i]), n)
    bit = 8 * k + (((got[k] ^ want[k]) & -(got[k] ^ want[k])).bit_length() - 1 if k < n else 0)
    blocks = walk(want)[0]
    for i, b in enumerate(blocks):
        if bit < b.end_bit or i + 1 == len(blocks):
            return "%d bytes for %d, first differing bit %d, in block %d of %d: %s" % (len(got), len(want), bit, i, len(blocks), b)


def first_token_difference(got, want_tokens):
    """For a report: the first token of `got` (a raw stream, valid or not) that is not the one of want_tokens (a list of (position, dist, length)), as text."""
    toks = []
    try:
        walk(got, toks=toks)
        err = ""
    except ValueError as e:
        err = " (then: %s)" % e
    for i, w in enumerate(want_tokens):
        if i >= len(toks):
            return "%d tokens for %d, the first %d agree%s" % (len(toks), len(want_tokens), i, err)
        if tuple(toks[i]) != tuple(w):
            return "token %d at position %d: (dist %d, len %d), the reference has (dist %d, len %d) at %d%s" % ((i, toks[i][0], toks[i][1], toks[i][2], w[1], w[2], w[0], err))
    return "the first %d tokens agree, %d follow%s" % (len(want_tokens), len(toks) - len(want_tokens), err)
