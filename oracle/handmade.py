"""A deterministic catalogue of hand-built DEFLATE streams (oracle/deflate_writer.py): what zlib's encoder never writes.

TEST INFRASTRUCTURE ONLY.  `catalogue()` returns the cases in a fixed order; each has
    name        unique
    stream      the raw deflate bytes
    dictionary  preset dictionary (b"": none)
    expect      the bytes a decoder must produce (None: the stream is not a valid one)
    kind        "ok" | "bad" (a data error) | "cut" (ends before its final block) | "trailing" (bytes behind the final block)
    maxdist     the farthest distance of its matches (valid cases)
    segs        byte offsets of the independent segments it is made of (the chunked layout of the library's own streams)
    pieces      True: long enough and shaped for the pieces decoder of a stream without a side table; False: one block with no start
                to find; None: small
Nothing is stored: tests/golden/handmade_inflate.json holds each stream's SHA-256 and the reference's verdict, the streams are built again.
"""
import hashlib

import numpy as np

from oracle import deflate_writer as W
from oracle.deflate_writer import dynamic, fixed, literals, raw_bits, stored, tokens


class Case:
    def __init__(self, name, blocks=None, stream=None, dictionary=b"", toks=None, kind="ok", segs=None, pieces=None, tail=b""):
        self.name, self.dictionary, self.kind, self.pieces = name, bytes(dictionary), kind, pieces
        self.stream = (W.stream(blocks) if stream is None else stream) + tail
        self.expect = None
        self.maxdist = 0
        if toks is not None and kind in ("ok", "trailing"):
            t = toks if isinstance(toks, W.Tokens) else W.tokens(toks)
            self.expect = W.expand(t, self.dictionary)
            m = t.kind == W.MATCH
            self.maxdist = int(t.b[m].max()) if m.any() else 0
        self.segs = segs or [0, len(self.stream)]


def rnd(n, seed):
    """n deterministic bytes (SHAKE-256 of the seed)"""
    return np.frombuffer(hashlib.shake_256(b"handmade:%d" % seed).digest(max(n, 1)), dtype=np.uint8)[:n].copy()


def rint(n, lo, hi, seed):
    """n deterministic integers in [lo, hi)"""
    r = np.frombuffer(hashlib.shake_256(b"handmade-int:%d" % seed).digest(4 * max(n, 1)), dtype="<u4")[:n].astype(np.int64)
    return lo + r % (hi - lo)


def _all_blocks(toks, final, dyn):
    return [dynamic(toks, final=final) if dyn else fixed(toks, final=final)]


# ---------------------------------------------------------------------------- window edge
FAR_DISTS = (32506, 32507, 32767, 32768)
FAR_LENS = (3, 4, 31, 32, 33, 64, 65, 257, 258)


def edge_pass(seed):
    """Tokens of a few reader passes (64 tokens each): every far distance x every length, overlapping matches (distance 1 with length 258
    among them), literals right behind the 32768 matches; then 64 matches at distance 32768 in a row."""
    items = [(n, d) for d in FAR_DISTS for n in FAR_LENS] + [(258, 1), (258, 2), (100, 7), (33, 32), (64, 63), (258, 257), (3, 1)]
    order = np.argsort(rint(len(items), 0, 1 << 30, seed), kind="stable")
    lit = rnd(600, seed + 1)
    out, k = [], 0
    for i in order.tolist():
        n, d = items[i]
        out.append((n, d))
        if d == 32768 or i % 3 == 0:
            for _ in range(1 + (i % 2)):
                out.append(int(lit[k])); k += 1
    for j in range(64):
        out.append((FAR_LENS[j % len(FAR_LENS)], 32768))
    out += [int(x) for x in lit[k: k + 5]]
    return tokens(out)


def window_edge():
    cs = []
    n = 0
    for ring in (4096, 8192, 16384):
        k = -(-32770 // ring)
        for delta in (-1, 0, 1):
            pos = k * ring + delta
            t = literals(rnd(pos, 100 + n)) + edge_pass(200 + n)
            cs.append(Case("edge_r%d_%+d" % (ring, delta), _all_blocks(t, True, n % 2 == 0), toks=t))
            n += 1
    # behind a 32 KiB dictionary the far matches start at outputs 0, 1, 4095 and 32767 (ring - 1)
    d = rnd(32768, 300).tobytes()
    for pos in (0, 1, 4095, 32767):
        t = literals(rnd(pos, 310 + pos)) + edge_pass(320 + pos)
        cs.append(Case("edge_dict32k_at%d" % pos, _all_blocks(t, True, pos % 2 == 1), dictionary=d, toks=t))
    # two independent segments, the first decoding to exactly 65536 bytes (its blocks not final, a flush marker behind them)
    head = literals(rnd(40000, 330)) + edge_pass(331)
    fill = 65536 - len(W.expand(head))
    t1 = head + literals(rnd(fill, 332))
    assert len(W.expand(t1)) == 65536
    s1 = W.stream([dynamic(t1), stored(b"")])
    t2 = literals(rnd(33000, 333)) + edge_pass(334)
    s2 = W.stream([fixed(t2, final=True)])
    cs.append(Case("edge_two_segments_64k", stream=s1 + s2, toks=t1 + t2, segs=[0, len(s1), len(s1) + len(s2)]))
    return cs


# ---------------------------------------------------------------------------- reach
def reach():
    cs = []
    for dl in (0, 1, 100, 32768):
        d = rnd(dl, 400 + dl).tobytes()
        for n in ((0, 1, 2, 3, 100, 32767, 32768) if dl else (1, 2, 3, 100, 32767, 32768)):
            pre = literals(rnd(n, 410 + n))
            far = dl + n
            if far <= 32768:
                t = pre + tokens([(258 if far < 300 else 3, far), 7, (3, 1)])
                cs.append(Case("reach_d%d_o%d_ok" % (dl, n), [fixed(t, final=True)], dictionary=d, toks=t))
            if far + 1 <= 32768:
                t = pre + tokens([(3, far + 1), 7])
                cs.append(Case("reach_d%d_o%d_far" % (dl, n), [fixed(t, final=True)], dictionary=d, kind="bad"))
    return cs


# ---------------------------------------------------------------------------- codes
def every_symbol(seed):
    """each length symbol 257..285 and each distance symbol 0..29 at its smallest and its largest extra bits; 258 both ways"""
    ls = []
    for s in range(29):
        b, e = W.LEN_BASE[s], W.LEN_EXTRA[s]
        ls += [b, b + (1 << e) - 1]
    ls = [min(x, 257) if x > 258 else x for x in ls]
    ds = []
    for s in range(30):
        b, e = W.DIST_BASE[s], W.DIST_EXTRA[s]
        ds += [b, b + (1 << e) - 1]
    out = []
    for i in range(max(len(ls), len(ds))):
        out.append((ls[i % len(ls)], ds[i % len(ds)]))
        out.append(i & 255)
    out += [(258, 32768, 284), (258, 32768), (258, 1, 284), (258, 1)]
    return literals(rnd(32768, seed)) + tokens(out)


def fill_lengths(n, fixed_lens, fillers):
    """Code lengths for n symbols: the given ones, then the fillers take the lengths that make the code complete (one per set bit of what is left)."""
    lens = [0] * n
    for s, l in fixed_lens.items():
        lens[s] = l
    left = 32768 - sum(32768 >> l for l in lens if l)
    assert left >= 0
    fl = [15 - b for b in range(15, -1, -1) if (left >> b) & 1]
    assert len(fl) <= len(fillers), (len(fl), len(fillers))
    for s, l in zip(fillers, fl):
        assert lens[s] == 0
        lens[s] = l
    return lens


def chain(syms):
    """lengths 1, 2, ..., 14, 15, 15 (complete) on 16 symbols"""
    return {s: min(i + 1, 15) for i, s in enumerate(syms)}


def long_codes(seed, rev):
    """codes of 1 ... 15 bits in both alphabets (9 and 10 and 15 past the decoders' 9-bit first-level tables)"""
    lsyms = [97, 257, 98, 258, 99, 265, 100, 270, 101, 273, 102, 277, 103, 281, 285, 256]
    dsyms = [0, 29, 3, 28, 10, 27, 15, 26, 20, 25, 5, 24, 8, 23, 12, 22]
    if rev:
        lsyms, dsyms = lsyms[::-1], dsyms[::-1]
    ll = [0] * 286
    for s, l in chain(lsyms).items():
        ll[s] = l
    dl = [0] * 30
    for s, l in chain(dsyms).items():
        dl[s] = l
    lits = [s for s in lsyms if s < 256]
    lens_of = {257: 3, 258: 4, 265: 11, 270: 23, 273: 35, 277: 67, 281: 131, 285: 258}
    r = rint(40000, 0, 1 << 30, seed)
    out = [lits[int(x) % len(lits)] for x in r[:33000]]
    pos = len(out)
    k = 33000
    for rep in range(3):
        for ls in lens_of:
            for ds in dsyms:
                lo, e = W.DIST_BASE[ds], W.DIST_EXTRA[ds]
                d = min(lo + int(r[k]) % (1 << e) if e else lo, pos)
                out.append((lens_of[ls], d)); pos += lens_of[ls]; k += 1
                out.append(lits[int(r[k]) % len(lits)]); pos += 1; k += 1
    t = tokens(out)
    return [dynamic(t, final=True, litlens=ll, distlens=dl)], t


def codes():
    cs = []
    for dyn in (False, True):
        t = every_symbol(500 + dyn)
        cs.append(Case("codes_every_symbol_%s" % ("dynamic" if dyn else "fixed"), _all_blocks(t, True, dyn), toks=t))
    for rev in (False, True):
        blocks, t = long_codes(510 + rev, rev)
        cs.append(Case("codes_1_to_15_bits%s" % ("_rev" if rev else ""), blocks, toks=t))
    # one distance code of one bit (symbol 29: 24577..32768, or symbol 0: distance 1); no distance code at all
    base = literals(rnd(33000, 520))
    far = tokens([(n, 32768 - (i * 977) % 8192) for i, n in enumerate((3, 258, 31, 32, 33, 100) * 4)])
    t = base + far
    cs.append(Case("codes_one_dist_code_29", [dynamic(t, final=True, distlens=[0] * 29 + [1])], toks=t))
    t = literals(rnd(300, 521)) + tokens([(258, 1), 5, (3, 1)])
    cs.append(Case("codes_one_dist_code_0", [dynamic(t, final=True, distlens=[1])], toks=t))
    t = literals(rnd(3000, 522))
    cs.append(Case("codes_no_dist_codes", [dynamic(t, final=True, distlens=[0], hdist=1)], toks=t))
    # HLIT 286, HDIST 30, HCLEN 19 (and HCLEN 4: only 16 17 18 0 can be sent, so no code at all -- invalid as soon as a symbol is read)
    t = every_symbol(530)
    cs.append(Case("codes_hlit286_hdist30_hclen19", [dynamic(t, final=True, hlit=286, hdist=30, hclen=19)], toks=t))
    t = literals(rnd(50, 531))
    cs.append(Case("codes_hclen4", [dynamic(tokens([]), final=True, eob=False, litlens=[0] * 257, distlens=[0], hdist=1, hlit=257,
                                            cl_syms=[(18, 127), (18, 109)], cl_lens=[0] * 17 + [1, 1], hclen=4), raw_bits(0, 16)],
                   kind="bad"))
    cs += repeats()
    cs += bad_codes()
    return cs


def crosses(cl, hlit, sym, run=None):
    """does a repeat `sym` (of `run` lengths) cover both length hlit - 1 and length hlit"""
    at = 0
    for s, e in cl:
        n = 1 if s < 16 else (3 + e if s < 18 else 11 + e)
        if s == sym and at < hlit < at + n and (run is None or n == run):
            return True
        at += n
    return False


def repeats():
    """code 16 across the boundary between the two sets of lengths, 17 and 18 across it, 18 at 138"""
    cs = []
    # 16: lengths 257..259 and distance 0..2 are all 5: one run of six
    ll = fill_lengths(260, {257: 5, 258: 5, 259: 5, 256: 5}, [65, 66, 67])
    dl = fill_lengths(30, {0: 5, 1: 5, 2: 5}, [3, 4, 5, 6])
    seq = ll + dl[:7]
    cl = W.rle_lengths(seq)
    assert crosses(cl, 260, 16)
    lits = [s for s in (65, 66, 67) if ll[s]]
    t = tokens([65, 66, 67, 65, (3, 1), (4, 2), (5, 3), 66, (3, 4), (4, 5), (5, 7), (3, 9), 67])
    cs.append(Case("rep16_across", [dynamic(t, final=True, litlens=ll, distlens=dl[:7], hlit=260, hdist=7, cl_syms=cl)], toks=t))
    # 17: lengths 262..269 (HLIT 270) and distance 0..1 are zero: a run of ten; 18: 257..285 and distance 0..9 zero (39); 18 at 138: literals 100..237
    for name, lzero, dzero in (("rep17_across", range(262, 286), range(0, 2)), ("rep18_across_and_138", range(257, 286), range(0, 10))):
        used = set(range(0, 100)) | set(range(238, 257)) | (set(range(257, 286)) - set(lzero))
        ll = W.huffman_lengths([1 if i in used else 0 for i in range(286)], 15)
        dl = W.huffman_lengths([0 if i in dzero else 1 for i in range(30)], 15)
        hlit = 270 if name == "rep17_across" else 286  # (rep17: lengths 262..269 are sent, all zero)
        seq = ll[:hlit] + dl
        cl = W.rle_lengths(seq)
        assert crosses(cl, hlit, 17 if name == "rep17_across" else 18)
        assert name == "rep17_across" or (18, 127) in cl
        lits = [s for s in range(256) if ll[s]]
        lsy = [s for s in range(257, 286) if ll[s]]
        dsy = [s for s in range(30) if dl[s]]
        r = rint(5000, 0, 1 << 30, 540 + len(cs))
        out = [lits[int(x) % len(lits)] for x in r[:2000]]
        k = 2000
        for ls in lsy:
            for ds in dsy[:6]:
                out.append((W.LEN_BASE[ls - 257], W.DIST_BASE[ds])); out.append(lits[int(r[k]) % len(lits)]); k += 1
        t = tokens(out)
        cs.append(Case(name, [dynamic(t, final=True, litlens=ll[:hlit], distlens=dl, hlit=hlit, hdist=30, cl_syms=cl)], toks=t))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return cs


def bad_codes():
    cs = []
    pre = list(rnd(40, 560))
    for s in (286, 287):
        cs.append(Case("bad_fixed_sym%d" % s, [fixed(tokens(pre + [("L", s)]), final=True, eob=False)], kind="bad"))
    for s in (30, 31):
        cs.append(Case("bad_fixed_dist%d" % s, [fixed(tokens(pre + [("L", 257), ("D", s)]), final=True, eob=False)], kind="bad"))
    t = literals(rnd(20, 561))
    for f in (30, 31):
        cs.append(Case("bad_hdist%d" % (f + 1), [dynamic(t, final=True, fields={"HDIST": f})], kind="bad"))
        cs.append(Case("bad_hlit%d" % (f + 257), [dynamic(t, final=True, fields={"HLIT": f})], kind="bad"))
    # a first length that is a repeat of the previous one (there is none)
    ll = W.huffman_lengths(W.symbol_counts(t)[0][:286] + np.eye(286, dtype=np.int64)[256], 15)
    cl = [(16, 0)] + W.rle_lengths(ll + [1])
    cs.append(Case("bad_first_length_repeat", [dynamic(t, final=True, cl_syms=cl, litlens=ll, distlens=[1])], kind="bad"))
    # a repeat that runs past HLIT + HDIST
    cs.append(Case("bad_repeat_too_long", [dynamic(t, final=True, cl_syms=W.rle_lengths(ll) + [(18, 100)], litlens=ll, distlens=[1])], kind="bad"))
    # a literal/length code without an end-of-block symbol (complete, so zlib 1.2.3 takes the table): the block never ends
    ll2 = [0] * 286
    for s in range(256):
        ll2[s] = 8
    cs.append(Case("bad_no_eob_code", [dynamic(t, final=True, eob=False, litlens=ll2, distlens=[1])], kind="cut"))
    # over-subscribed and incomplete codes (more than one symbol), literal/length and distance; an over-subscribed code-length code
    lls = [2, 2, 2] + [0] * 253 + [1]
    cs.append(Case("bad_litlen_oversubscribed", [dynamic(tokens([0]), final=True, litlens=lls, distlens=[1])], kind="bad"))
    lli = [2] + [0] * 255 + [2]
    cs.append(Case("bad_litlen_incomplete", [dynamic(tokens([0]), final=True, litlens=lli, distlens=[1])], kind="bad"))
    lla = [1] + [0] * 255 + [1]
    cs.append(Case("bad_dist_oversubscribed", [dynamic(tokens([0]), final=True, litlens=lla, distlens=[1, 1, 1])], kind="bad"))
    cs.append(Case("bad_dist_incomplete", [dynamic(tokens([0]), final=True, litlens=lla, distlens=[2, 0, 2])], kind="bad"))
    cs.append(Case("bad_codelen_oversubscribed", [dynamic(tokens([0]), final=True, litlens=lla, distlens=[1], cl_lens=[1] * 19)], kind="bad"))
    return cs


# ---------------------------------------------------------------------------- blocks
def blocks():
    cs = []
    cs.append(Case("stored_empty_final", [stored(b"", final=True)], toks=tokens([])))
    d = rnd(65535, 600)
    cs.append(Case("stored_65535", [stored(d.tobytes(), final=True)], toks=literals(d)))
    for b in range(8):
        # a fixed block whose length leaves the stored header at bit offset b; the padding behind the header all ones; a match across it
        head = literals((rnd(20, 610 + b) % 144).tolist() + [200] * ((b - 2) % 8))  # (3 + 20 * 8 + 9 * k + 7 bits)
        body = rnd(300 + b, 620 + b)
        tail = tokens([(258, 300 + b + 5), (40, 1), 9])
        t = head + literals(body) + tail
        cs.append(Case("stored_at_bit%d" % b, [fixed(head), stored(body.tobytes(), pad=0xFF), fixed(tail, final=True)], toks=t))
    cs.append(Case("bad_stored_nlen", [fixed(literals(b"ab")), stored(b"xyz", final=True, nlength=0x1234)], kind="bad"))
    cs.append(Case("bad_btype3", [fixed(literals(b"ab")), raw_bits(1 | (3 << 1), 3), raw_bits(0, 13)], kind="bad"))
    empt = [fixed(tokens([]))] * 1000
    t = literals(rnd(100, 630)) + tokens([(50, 100), (258, 1)])
    cs.append(Case("empty_fixed_x1000", [fixed(literals(rnd(100, 630)))] + empt + [fixed(tokens([(50, 100), (258, 1)]), final=True)], toks=t))
    t = literals(rnd(500, 640)) + tokens([(100, 400)])
    cs.append(Case("trailing_bytes", [dynamic(t, final=True)], toks=t, kind="trailing", tail=b"\x00\xffjunk"))
    t = literals(rnd(500, 650))
    cs.append(Case("cut_before_final", [dynamic(t), fixed(tokens([1, 2, 3]))], kind="cut"))
    return cs


# ---------------------------------------------------------------------------- large: the pieces decoder
def random_block_tokens(nbytes, first, seed):
    """~nbytes of output: `first` token, random literals, a far match every ~2 KiB"""
    lit = rnd(nbytes, seed)
    r = rint(nbytes // 2048 + 2, 0, 1 << 30, seed + 1)
    out = [first]
    step = 2048
    t = tokens(out)
    parts = [t]
    for i in range(0, nbytes, step):
        parts.append(literals(lit[i: i + step]))
        parts.append(tokens([(3 + int(r[i // step]) % 256, 32768 - int(r[i // step]) % 300)]))
    return sum(parts[1:], parts[0])


def big():
    cs = []
    # dynamic blocks of 16..64 KiB whose first token is a match at distance 32768 or 1 (a piece found there starts with a reach into the unknown window)
    sizes = rint(64, 16384, 65536, 700)
    toks, blks = literals(rnd(32768, 701)), []
    blks.append(fixed(toks))
    for i, n in enumerate(sizes.tolist()):
        t = random_block_tokens(n, (258, 32768) if i % 2 == 0 else (258, 1), 710 + i)
        blks.append(dynamic(t, final=i == len(sizes) - 1))
        toks = toks + t
    cs.append(Case("pieces_first_match_far_or_1", blks, toks=toks, pieces=True))
    # real flush markers (an empty stored block) followed by matches across them at distance 1 and 32768
    toks, blks = literals(rnd(32768, 800)), []
    blks.append(dynamic(toks))
    for i in range(60):
        t = random_block_tokens(int(rint(1, 20000, 40000, 801 + i)[0]), (3 + i, 1 if i % 2 else 32768), 810 + i)
        blks += [stored(b""), dynamic(t, final=i == 59)]
        toks = toks + t
    cs.append(Case("pieces_sync_markers_crossed", blks, toks=toks, pieces=True))
    # stored blocks full of 00 00 FF FF between dynamic blocks: more fake markers than the repair passes take
    toks, blks = literals(rnd(32768, 900)), []
    blks.append(dynamic(toks))
    for i in range(40):
        sd = bytearray(rnd(int(rint(1, 2000, 12000, 901 + i)[0]), 902 + i).tobytes())
        for j in range(8):
            at = (j * 997 + 13 * i) % (len(sd) - 4)
            sd[at: at + 4] = b"\x00\x00\xff\xff"
        t = random_block_tokens(int(rint(1, 20000, 40000, 950 + i)[0]), (40, 32768), 960 + i)
        blks += [stored(bytes(sd)), dynamic(t, final=i == 39)]
        toks = toks + literals(sd) + t
    cs.append(Case("pieces_fake_markers_in_stored", blks, toks=toks, pieces=True))
    # one dynamic block: >= 4 MiB of output, >= 10**6 tokens, no block start to find
    n = 1200000
    kind = (rint(n, 0, 2, 1000) == 0).astype(np.int8)
    kind[:1000] = 0
    a = np.where(kind == 1, rint(n, 3, 11, 1001), rnd(n, 1002))
    b = np.where(kind == 1, rint(n, 1, 32769, 1003), 0)
    b[:40000] = np.minimum(b[:40000], 900)
    t = W.Tokens(kind, a, b)
    cs.append(Case("one_block_4mib_1m_tokens", [dynamic(t, final=True)], toks=t, pieces=False))
    return cs


_CACHE = None


def catalogue():
    global _CACHE
    if _CACHE is None:
        cs = window_edge() + reach() + codes() + blocks() + big()
        names = [c.name for c in cs]
        assert len(set(names)) == len(names), "duplicate case names"
        _CACHE = cs
    return _CACHE


def sha16(b):
    return hashlib.sha256(b).hexdigest()[:16]
