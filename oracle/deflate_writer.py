"""A DEFLATE bit writer (RFC 1951) for hand-built test streams.

TEST INFRASTRUCTURE ONLY.  Written from the RFC: it exists to write what a zlib encoder never does -- distances of
32 507 ... 32 768, length 258 as symbol 284 with 31 extra bits, codes of up to 15 bits, any HLIT / HDIST / HCLEN, any
run-length coding of the code lengths, raw header fields (invalid streams need those), stored blocks anywhere.

Tokens are held as three arrays (see `Tokens`); a list of
    int 0..255              a literal
    (length, dist)          a match
    (258, dist, 284)        a match whose length symbol is forced (here: 258 as 284 + 31 extra bits)
    ("L", sym)              a raw literal/length symbol without extra bits (286 / 287 in a fixed block ...)
    ("D", sym)              a raw distance symbol without extra bits (30 / 31 ...)
becomes one with `tokens()`.  Blocks are dicts made by `stored()`, `fixed()`, `dynamic()` and `raw_bits()`; `stream()` packs
a list of them.  The bits are packed with numpy, so streams of a few MiB take well under a second.
"""
import heapq

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

# symbol of every length 3..258 and of every distance 1..32768 (RFC 1951 3.2.5)
_LSYM = np.zeros(259, dtype=np.int32)
for _s in range(28, -1, -1):
    _LSYM[LEN_BASE[_s]: LEN_BASE[_s] + (1 << LEN_EXTRA[_s])] = 257 + _s
_LSYM[258] = 285
_DSYM = np.zeros(32769, dtype=np.int32)
for _s in range(30):
    _DSYM[DIST_BASE[_s]: DIST_BASE[_s] + (1 << DIST_EXTRA[_s])] = _s
_LBASE = np.array([0] * 257 + LEN_BASE + [0, 0], dtype=np.int64)
_LEXT = np.array([0] * 257 + LEN_EXTRA + [0, 0], dtype=np.int64)
_DBASE = np.array(DIST_BASE + [0, 0], dtype=np.int64)
_DEXT = np.array(DIST_EXTRA + [0, 0], dtype=np.int64)

LIT, MATCH, RAW_L, RAW_D = 0, 1, 2, 3


class Tokens:
    """kind (LIT / MATCH / RAW_L / RAW_D), a (literal byte, match length or raw symbol), b (distance), lsym (forced length symbol, 0: natural)."""

    def __init__(self, kind, a, b, lsym=None):
        self.kind = np.asarray(kind, dtype=np.int8)
        self.a = np.asarray(a, dtype=np.int32)
        self.b = np.asarray(b, dtype=np.int32)
        self.lsym = np.zeros(len(self.kind), dtype=np.int32) if lsym is None else np.asarray(lsym, dtype=np.int32)

    def __len__(self):
        return len(self.kind)

    def __add__(self, other):
        return Tokens(np.concatenate([self.kind, other.kind]), np.concatenate([self.a, other.a]), np.concatenate([self.b, other.b]),
                      np.concatenate([self.lsym, other.lsym]))


def tokens(seq):
    if isinstance(seq, Tokens):
        return seq
    kind, a, b, ls = [], [], [], []
    for t in seq:
        if isinstance(t, (int, np.integer)):
            kind.append(LIT); a.append(int(t)); b.append(0); ls.append(0)
        elif t[0] == "L":
            kind.append(RAW_L); a.append(t[1]); b.append(0); ls.append(0)
        elif t[0] == "D":
            kind.append(RAW_D); a.append(t[1]); b.append(0); ls.append(0)
        else:
            kind.append(MATCH); a.append(t[0]); b.append(t[1]); ls.append(t[2] if len(t) > 2 else 0)
    return Tokens(kind, a, b, ls)


def literals(data):
    d = np.frombuffer(bytes(data), dtype=np.uint8)
    return Tokens(np.zeros(len(d), dtype=np.int8), d.astype(np.int32), np.zeros(len(d), dtype=np.int32))


def expand(toks, dictionary=b""):
    """The plain reference: apply the tokens one after the other to a window that starts with `dictionary`.  A match copies byte
    by byte (an overlapping one repeats what it has just written).  Raises ValueError on a distance beyond the window."""
    t = tokens(toks)
    out = bytearray(dictionary)
    lits = t.a.astype(np.uint8)
    ms = np.flatnonzero(t.kind != LIT)
    prev = 0
    for i in ms.tolist():
        if i > prev:
            out += lits[prev:i].tobytes()
        prev = i + 1
        if t.kind[i] != MATCH:
            raise ValueError("raw symbol: no plain meaning")
        n, d = int(t.a[i]), int(t.b[i])
        if not (3 <= n <= 258 and 1 <= d <= 32768) or d > len(out):
            raise ValueError("match (%d, %d) at %d" % (n, d, len(out)))
        if d >= n:
            out += out[len(out) - d: len(out) - d + n]
        else:
            piece = out[len(out) - d:]
            out += (piece * (n // d + 1))[:n]
    if prev < len(t):
        out += lits[prev:].tobytes()
    return bytes(out[len(dictionary):])


# ---------------------------------------------------------------------------- codes
def huffman_lengths(freq, limit):
    """Code lengths of a Huffman code for the frequencies, no longer than `limit` (frequencies are halved until it fits).
    One used symbol gets a one-bit code (RFC 1951 3.2.7: one distance code of one bit)."""
    f = [int(x) for x in freq]
    while True:
        used = [i for i, x in enumerate(f) if x]
        lens = [0] * len(f)
        if len(used) == 1:
            lens[used[0]] = 1
            return lens
        if not used:
            return lens
        heap = [(f[i], i, (i,)) for i in used]
        heapq.heapify(heap)
        k = len(f)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                lens[s] += 1
            heapq.heappush(heap, (a[0] + b[0], k, a[2] + b[2]))
            k += 1
        if max(lens) <= limit:
            return lens
        f = [(x + 1) // 2 if x else 0 for x in f]


def canonical_codes(lens):
    """RFC 1951 3.2.2; returns the codes bit-reversed (DEFLATE sends a Huffman code from its most significant bit: packed LSB first, that is
    the reversed value)."""
    lens = [int(x) for x in lens]
    mx = max(lens) if lens else 0
    bl_count = [0] * (mx + 2)
    for l in lens:
        if l:
            bl_count[l] += 1
    code, next_code = 0, [0] * (mx + 2)
    for b in range(1, mx + 1):
        code = (code + bl_count[b - 1]) << 1
        next_code[b] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            c = next_code[l]; next_code[l] += 1
            out[s] = int("{:0{w}b}".format(c, w=l)[::-1], 2)
    return out


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def symbol_counts(toks):
    t = tokens(toks)
    lf = np.zeros(288, dtype=np.int64)
    df = np.zeros(32, dtype=np.int64)
    k = t.kind
    np.add.at(lf, t.a[k == LIT], 1)
    m = k == MATCH
    ls = np.where(t.lsym[m] != 0, t.lsym[m], _LSYM[t.a[m]])
    np.add.at(lf, ls, 1)
    np.add.at(df, _DSYM[t.b[m]], 1)
    np.add.at(lf, t.a[k == RAW_L], 1)
    np.add.at(df, t.a[k == RAW_D], 1)
    return lf, df


def rle_lengths(lens):
    """The usual run-length coding of a sequence of code lengths (runs may cross from the literal/length lengths into the distance lengths):
    list of (symbol, extra value)."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138); out.append((18, k - 11)); run -= k
            if run >= 3:
                out.append((17, run - 3)); run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                k = min(run, 6); out.append((16, k - 3)); run -= k
            out += [(v, 0)] * run
        i = j
    return out


_CL_EXTRA = {16: 2, 17: 3, 18: 7}


# ---------------------------------------------------------------------------- blocks
def raw_bits(value, nbits):
    """Arbitrary bits in the stream (LSB first): a block type 3, a header cut short, ..."""
    return {"t": "bits", "v": value, "n": nbits}


def stored(data, final=False, pad=0, length=None, nlength=None):
    """Stored block; `pad`: the value of the bits that fill up the byte behind the header (the RFC says ignore them)."""
    return {"t": "stored", "data": bytes(data), "final": final, "pad": pad, "len": length, "nlen": nlength}


def fixed(toks, final=False, eob=True):
    return {"t": "fixed", "toks": tokens(toks), "final": final, "eob": eob}


def dynamic(toks, final=False, eob=True, litlens=None, distlens=None, hlit=None, hdist=None, cl_syms=None, cl_lens=None, hclen=None,
            fields=None):
    """Dynamic block.  litlens / distlens: the code lengths (default: Huffman of the tokens, 15 bits at most); hlit / hdist: how many of them
    are sent (default: up to the last non-zero one, at least 257 / 1); cl_syms: the code-length sequence as (symbol, extra) pairs (default:
    rle_lengths), cl_lens: the code-length code's lengths (default: Huffman, 7 bits), hclen: how many of those are sent (default: up to the last
    non-zero in CL_ORDER, at least 4); fields: raw values that replace what is written for "HLIT" (5 bits), "HDIST" (5), "HCLEN" (4)."""
    return {"t": "dynamic", "toks": tokens(toks), "final": final, "eob": eob, "litlens": litlens, "distlens": distlens, "hlit": hlit,
            "hdist": hdist, "cl_syms": cl_syms, "cl_lens": cl_lens, "hclen": hclen, "fields": fields or {}}


class _Bits:
    def __init__(self):
        self.vals, self.lens = [], []
        self.nbits = 0

    def put(self, v, n):
        self.vals.append(np.array([v], dtype=np.uint64)); self.lens.append(np.array([n], dtype=np.int64)); self.nbits += n

    def put_arrays(self, v, n):
        self.vals.append(np.asarray(v, dtype=np.uint64).ravel()); self.lens.append(np.asarray(n, dtype=np.int64).ravel()); self.nbits += int(np.sum(n))

    def pack(self):
        v = np.concatenate(self.vals) if self.vals else np.zeros(0, np.uint64)
        n = np.concatenate(self.lens) if self.lens else np.zeros(0, np.int64)
        pos = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
        total = int(n.sum())
        nwords = (total + 31) // 32 + 1
        sh = (pos & 31).astype(np.uint64)
        x = (v & ((np.uint64(1) << n.astype(np.uint64)) - np.uint64(1))) << sh  # (fields are at most 32 bits wide)
        w = pos >> 5
        # fields never share a bit, so adding them is or-ing them; every word's sum stays below 2**32 (exact in float64)
        lo = np.bincount(w, weights=(x & np.uint64(0xFFFFFFFF)).astype(np.float64), minlength=nwords)
        hi = np.bincount(w + 1, weights=(x >> np.uint64(32)).astype(np.float64), minlength=nwords + 1)[:nwords]
        words = (lo + hi).astype(np.uint64).astype("<u4")
        return words.tobytes()[: (total + 7) // 8]


def _put_tokens(bits, t, lcode, llen, dcode, dlen, eob):
    """The tokens as fields: (code, extra) of the length / literal, (code, extra) of the distance."""
    k, a, b = t.kind, t.a.astype(np.int64), t.b.astype(np.int64)
    m = k == MATCH
    lsym = np.where(k == LIT, a, 0)
    lsym = np.where(m, np.where(t.lsym != 0, t.lsym, _LSYM[np.clip(a, 0, 258)]), lsym)
    lsym = np.where(k == RAW_L, a, lsym)
    has_l = k != RAW_D
    dsym = np.where(m, _DSYM[np.clip(b, 0, 32768)], np.where(k == RAW_D, a, 0))
    has_d = m | (k == RAW_D)
    lcode, llen, dcode, dlen = (np.asarray(x, dtype=np.int64) for x in (lcode, llen, dcode, dlen))
    if np.any(has_l & (llen[lsym] == 0)) or np.any(has_d & (dlen[dsym] == 0)):
        raise ValueError("a token's symbol has no code")
    f = np.zeros((len(k), 4), dtype=np.int64)
    n = np.zeros((len(k), 4), dtype=np.int64)
    f[:, 0] = np.where(has_l, lcode[lsym], 0); n[:, 0] = np.where(has_l, llen[lsym], 0)
    f[:, 1] = np.where(m, a - _LBASE[lsym], 0); n[:, 1] = np.where(m, _LEXT[lsym], 0)
    f[:, 2] = np.where(has_d, dcode[dsym], 0); n[:, 2] = np.where(has_d, dlen[dsym], 0)
    f[:, 3] = np.where(m, b - _DBASE[dsym], 0); n[:, 3] = np.where(m, _DEXT[dsym], 0)
    if np.any(f[:, 1] < 0) or np.any(f[:, 1] >= (1 << n[:, 1])) or np.any(f[:, 3] < 0) or np.any(f[:, 3] >= (1 << n[:, 3])):
        raise ValueError("a length or distance does not fit its symbol")
    bits.put_arrays(f, n)
    if eob:
        bits.put(int(lcode[256]), int(llen[256]))


def _dynamic(bits, blk):
    t = blk["toks"]
    lf, df = symbol_counts(t)
    if blk["eob"]:
        lf[256] += 1
    litlens = list(blk["litlens"]) if blk["litlens"] is not None else huffman_lengths(lf[:286], 15)
    distlens = list(blk["distlens"]) if blk["distlens"] is not None else huffman_lengths(df[:30], 15)
    hlit = blk["hlit"] or max(257, max([i + 1 for i, l in enumerate(litlens) if l] + [0]))
    hdist = blk["hdist"] or max(1, max([i + 1 for i, l in enumerate(distlens) if l] + [0]))
    seq = (litlens + [0] * 320)[:hlit] + (distlens + [0] * 32)[:hdist]
    cl_syms = blk["cl_syms"] if blk["cl_syms"] is not None else rle_lengths(seq)
    if blk["cl_lens"] is not None:
        cl_lens = list(blk["cl_lens"])
    else:
        cf = [0] * 19
        for s, _ in cl_syms:
            cf[s] += 1
        cl_lens = huffman_lengths(cf, 7)
    hclen = blk["hclen"] or max(4, max([i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]] + [0]))
    fl = blk["fields"]
    bits.put(fl.get("HLIT", hlit - 257), 5)
    bits.put(fl.get("HDIST", hdist - 1), 5)
    bits.put(fl.get("HCLEN", hclen - 4), 4)
    bits.put_arrays([cl_lens[CL_ORDER[i]] for i in range(hclen)], [3] * hclen)
    cc = canonical_codes(cl_lens)
    for s, e in cl_syms:
        bits.put(cc[s], cl_lens[s])
        if s in _CL_EXTRA:
            bits.put(e, _CL_EXTRA[s])
    lpad = (litlens + [0] * 288)[:288]
    dpad = (distlens + [0] * 32)[:32]
    _put_tokens(bits, t, canonical_codes(lpad), lpad, canonical_codes(dpad), dpad, blk["eob"])


def _emit(blocks):
    """The blocks as fields, and the bit at which each block starts"""
    bits = _Bits()
    starts = []
    for blk in blocks:
        starts.append(bits.nbits)
        ty = blk["t"]
        if ty == "bits":
            bits.put(blk["v"], blk["n"])
        elif ty == "stored":
            bits.put(int(blk["final"]), 1); bits.put(0, 2)
            pad = (-bits.nbits) % 8
            if pad:
                bits.put(blk["pad"] & ((1 << pad) - 1), pad)
            n = len(blk["data"])
            ln = n if blk["len"] is None else blk["len"]
            nl = (~ln & 0xFFFF) if blk["nlen"] is None else blk["nlen"]
            bits.put(ln, 16); bits.put(nl, 16)
            if n:
                bits.put_arrays(np.frombuffer(blk["data"], dtype=np.uint8), np.full(n, 8))
        elif ty == "fixed":
            bits.put(int(blk["final"]), 1); bits.put(1, 2)
            _put_tokens(bits, blk["toks"], canonical_codes(FIXED_LIT), FIXED_LIT, canonical_codes(FIXED_DIST), FIXED_DIST, blk["eob"])
        elif ty == "dynamic":
            bits.put(int(blk["final"]), 1); bits.put(2, 2)
            _dynamic(bits, blk)
        else:
            raise ValueError(ty)
    return bits, starts


def stream(blocks):
    """Pack the blocks (in order) into bytes; the last byte is filled up with zeros."""
    return _emit(blocks)[0].pack()


def block_starts(blocks):
    """The bit of `stream(blocks)` at which every block starts (a stored block: its three header bits, the padding and LEN follow), and behind them
    the bit at which the last block ends."""
    bits, starts = _emit(blocks)
    return starts + [bits.nbits]
