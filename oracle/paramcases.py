"""Lives of ONE deflate stream across its hand-overs: deflateParams / deflateTune / deflateReset between the deflate() calls, output space that runs out
at the switch, a finish that has only the carried block left, deflateBound as the output space.  TEST INFRASTRUCTURE, pure Python, deterministic.

Shared by oracle/gen_golden_params.py and the tests.  catalogue() returns Case rows:

  name        unique
  family      matrix | strategy | twice | wraps | space | carry | bound | tune
  data        the input (data2: the input of the second stream of a row that calls deflateReset)
  level, strategy, wbits    deflateInit2's arguments (memLevel 8)
  dictionary  bytes for deflateSetDictionary right behind deflateInit2, or None
  steps       what the caller does, in order:
                ("deflate", upto, flush)   deflate() is handed data[fed:upto] with that flush value
                ("params", level, strategy)  deflateParams()
                ("tune", good_length, max_lazy, nice_length, max_chain)  deflateTune()
                ("reset",)                 deflateReset(); the deflate steps behind it hand over data2
                ("avail_out", k)           the next call (deflateParams or deflate) has avail_out = k; every other call has ample space
                ("bound",)                 the next call has avail_out = deflateBound(strm, len(data)), which is recorded
  feed        ZAMD_FEED_BYTES for the product (None: its default, 16 MiB): with 1024 a Z_NO_FLUSH slice is handed to the engine at once and leaves
              collected-but-unparsed input behind (the 512 bytes in front of its end); with the default the whole slice is still waiting at the switch
  like        space rows: the name of the row that makes the same calls with ample space;  tune rows at levels 1-3: the row without the deflateTune call
  expect      what the product owes on this row: "ref" the reference's codes and bytes; "like" the bytes of row `like`; "error" (the call is refused with
              Z_STREAM_ERROR and the stream goes on as row `like`, or -- no `like` -- still finishes to the input); "bound"; "chunks" (see family tune)

play(L, ZStream, case) plays the steps on a library with zlib's ABI (the compiled reference, refzlib.play_steps; the product, tests/zhost.play_steps)
and returns every call's return code and, per stream, the bytes, total_in, total_out and strm->adler.

Inputs: 300001 bytes of both synthetic corpora -- the smallest length at which switches at 100000 and 150000 sit behind a window that has slid, so the
window arithmetic of the chain conversions is live.  Level 1 leaves many positions out of its chains on the text corpus.

Families.
  matrix    every ordered pair of compress functions -- stored (0), fast (1-3), slow (4-9): 0>0 0>1 0>6 1>0 1>3 1>9 6>0 6>1 6>9 -- behind every kind of
            preceding call: none (before any input), a Z_NO_FLUSH slice, Z_PARTIAL_FLUSH, Z_SYNC_FLUSH, Z_FULL_FLUSH, deflateSetDictionary + a slice;
            raw streams, both corpora.  THE ONE EXCLUSION (EXCLUDED): a same-function pair behind a Z_NO_FLUSH slice (with or without the dictionary) --
            the reference switches the parameters where its loop happens to stand, the product where the parse of its next feed begins.
  strategy  the level stays, the strategy changes (the same function, so: behind a Z_SYNC_FLUSH): 0>1 0>2 0>4 4>0 at levels 1 and 6, 0>3 at levels 4, 6, 9.
            0>3 at levels 1 and 3: the product does not serve Z_RLE there on a continuous stream, deflateParams answers Z_STREAM_ERROR and changes nothing.
  twice     1>9>0>6, 6>0>6, and 1>9>1 with a Z_SYNC_FLUSH between the switches.
  wraps     matrix rows at windowBits 15 and 31 (matrix itself is -15): the trailer's Adler-32 / CRC-32 pass through the hand-over.
  space     the switch with avail_out == 0 (refused: Z_BUF_ERROR, nothing changes, a second call with space switches -- the product's contract, not the
            reference's, whose stream is not required here and for 0 > 1-9 is not even valid) and with avail_out == 7 (the flush's output stays pending).
  carry     Z_FIXED, raw, levels 1 and 6: 32 KiB of random bytes, then 6-byte pieces copied from 16385 .. 32506 bytes back, each followed in its source by
            another byte than the one that follows it here -- one match of length 6 and a far distance per piece, about 25 bits each.  Handed over with
            Z_NO_FLUSH, finished by a Z_FINISH call with avail_in == 0: the block that is filling holds more than 12500 tokens and began more than
            65536 + 512 bytes back, so its bytes have left the window the product keeps and its code is larger than that window's bound.
  bound     random bytes, n in BOUND_N x levels 0 1 6 9 x windowBits -15 15 31: deflate(Z_FINISH) into exactly deflateBound() bytes.
  tune      levels 1, 3, 6: deflateTune before the first byte; the same, then deflateReset and a second stream of other data; deflateTune behind a
            Z_SYNC_FLUSH at 100000.  The product serves a tuned deflate_fast in independent 64 KiB chunks ("Not modelled"): at
            levels 1 and 3 the tuned stream is not the reference's ("chunks": the restatement's chunk streams with the tuned row), the stream behind
            deflateReset is; in the middle of such a stream deflateTune is refused ("error")."""
import ctypes as C
import hashlib
from collections import namedtuple

from oracle import corpus_py as CP

Z_NO_FLUSH, Z_PARTIAL_FLUSH, Z_SYNC_FLUSH, Z_FULL_FLUSH, Z_FINISH = 0, 1, 2, 3, 4
Z_OK, Z_STREAM_END, Z_STREAM_ERROR, Z_BUF_ERROR = 0, 1, -2, -5
Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 1, 2, 3, 4
N = 300001
PAIRS = ((0, 0), (0, 1), (0, 6), (1, 0), (1, 3), (1, 9), (6, 0), (6, 1), (6, 9))
BEHIND = ("none", "noflush", "partial", "sync", "full", "dict")
FLUSH_OF = {"noflush": Z_NO_FLUSH, "partial": Z_PARTIAL_FLUSH, "sync": Z_SYNC_FLUSH, "full": Z_FULL_FLUSH, "dict": Z_NO_FLUSH}
BOUND_N = (0, 1, 1000, 16383, 16384, 65535, 65536, 100000)
TUNE = (5, 9, 37, 13)

Case = namedtuple("Case", "name family data data2 level strategy wbits dictionary steps feed like expect")


def func_of(level):
    return 0 if level == 0 else 1 if level <= 3 else 2


EXCLUDED = {(a, b, h) for a, b in PAIRS if func_of(a) == func_of(b) for h in ("noflush", "dict")}

_memo = {}


def corpus(kind):
    if kind not in _memo:
        _memo[kind] = {"sil": lambda: CP.chunks(0, 11, 5).tobytes()[:N], "txt": lambda: CP.chunks(1, 11, 5).tobytes()[:N],
                       "sil2": lambda: CP.chunks(0, 40, 2).tobytes()[:100001], "txt2": lambda: CP.chunks(1, 40, 2).tobytes()[:100001]}[kind]()
    return _memo[kind]


def random_bytes(n, seed=0):
    """n bytes no compressor gets anything out of (SHA-256 in counter mode)."""
    out = b"".join(hashlib.sha256(b"paramcases %d %d" % (seed, i)).digest() for i in range((n + 31) // 32))
    return out[:n]


def far_pieces(npieces=13500):
    """The carry family's input (see the module's text).  A source behind the random part is the start of an earlier piece: deflate_fast puts only a
    match's first position into its chains at level 1.  13500 pieces: the filling block's code (25 bits a token) stays behind the tokens it is read from
    in the reference's pending buffer, which 1.2.3 lets it overtake from about 14560 such tokens on (the block would come out corrupt)."""
    if "far" in _memo:
        return _memo["far"]
    d = bytearray(random_bytes(32768, 1))
    x, seen = 12345, {}   # seen: where each piece's bytes were written last -- a nearer copy would be the match the search takes
    for _ in range(npieces):
        p = len(d)
        while True:
            x = (x * 1103515245 + 12345) & 0x7FFFFFFF
            s = p - 32500 + x % (32500 - 16385 - 8)   # p - s in 16393 .. 32500
            if s > 32768 - 7:
                s = max(s - (s - 32768) % 6, 32768)
            if d[s - 1] != d[p - 1] and (p == 32768 or d[s] != follow) and p - seen.get(bytes(d[s:s + 6]), -32768) >= 16385:
                break  # (no match that begins a byte early, none that runs on from the piece in front, none nearer than 16385)
        seen[bytes(d[s:s + 6])] = p
        d += d[s:s + 6]
        follow = d[s + 6]
    d += bytes([follow ^ 0x55])
    _memo["far"] = bytes(d)
    return _memo["far"]


def D(upto, flush):
    return ("deflate", upto, flush)


def P(level, strategy=0):
    return ("params", level, strategy)


def _case(name, family, data, level, steps, strategy=0, wbits=-15, dictionary=None, feed=None, like=None, expect="ref", data2=None):
    return Case(name, family, data, data2, level, strategy, wbits, dictionary, tuple(steps), feed, like, expect)


def _switch_steps(a, b, behind, at=100000, strategy=0):
    """the life of a matrix row: [the preceding call,] deflateParams(b), the rest with Z_FINISH"""
    pre = [] if behind == "none" else [D(at, FLUSH_OF[behind])]
    return pre + [P(b, strategy), D(N, Z_FINISH)]


def matrix():
    out = []
    for i, (a, b) in enumerate(PAIRS):
        for j, behind in enumerate(BEHIND):
            if (a, b, behind) in EXCLUDED:
                continue
            for k, kind in enumerate(("sil", "txt")):
                d = corpus(kind)
                out.append(_case("matrix-%dto%d-%s-%s" % (a, b, behind, kind), "matrix", d, a, _switch_steps(a, b, behind),
                                 dictionary=d[200000:220000] if behind == "dict" else None, feed=1024 if (i + j + k) % 2 else None))
    return out


def strategy():
    out = []
    n = 0
    for level in (1, 6):
        for s0, s1 in ((0, Z_FILTERED), (0, Z_HUFFMAN_ONLY), (0, Z_FIXED), (Z_FIXED, 0)):
            n += 1
            out.append(_case("strategy-L%d-%dto%d" % (level, s0, s1), "strategy", corpus("txt" if level == 1 else "sil"), level,
                             [D(100000, Z_SYNC_FLUSH), P(level, s1), D(N, Z_FINISH)], strategy=s0, feed=1024 if n % 2 else None))
    for level in (4, 6, 9):
        out.append(_case("strategy-L%d-0to3" % level, "strategy", corpus("sil"), level, [D(150000, Z_SYNC_FLUSH), P(level, Z_RLE), D(N, Z_FINISH)],
                         feed=1024 if level == 6 else None))
    for level in (1, 3):  # refused by the product (Z_RLE at levels 1-3 is served in chunks only): nothing changes
        out.append(_case("strategy-L%d-0to3-sync" % level, "strategy", corpus("txt"), level, [D(100000, Z_SYNC_FLUSH), P(level, Z_RLE), D(N, Z_FINISH)],
                         feed=1024 if level == 1 else None, expect="error"))
        out.append(_case("strategy-L%d-0to3-noflush" % level, "strategy", corpus("txt"), level, [D(100000, Z_NO_FLUSH), P(level, Z_RLE), D(N, Z_FINISH)],
                         feed=1024 if level == 3 else None, expect="error"))
    return out


def twice():
    out = []
    for k, kind in enumerate(("sil", "txt")):
        d = corpus(kind)
        for f, feed in enumerate((None, 1024)):
            tag = "%s-%s" % (kind, "feed1k" if feed else "feed16m")
            out.append(_case("twice-1to9to0to6-" + tag, "twice", d, 1, [D(100000, Z_NO_FLUSH), P(9), D(150000, Z_NO_FLUSH), P(0), D(200000, Z_NO_FLUSH), P(6), D(N, Z_FINISH)], feed=feed))
            out.append(_case("twice-6to0to6-" + tag, "twice", d, 6, [D(100000, Z_NO_FLUSH), P(0), D(150000, Z_NO_FLUSH), P(6), D(N, Z_FINISH)], feed=feed))
            out.append(_case("twice-1to9sync1-" + tag, "twice", d, 1, [D(100000, Z_NO_FLUSH), P(9), D(150000, Z_SYNC_FLUSH), P(1), D(N, Z_FINISH)], feed=feed))
    return out


def wraps():
    out = []
    n = 0
    for a, b in ((1, 9), (6, 1), (6, 0), (0, 6), (0, 1), (1, 0)):
        for behind in ("noflush", "sync"):
            for wbits in (15, 31):
                n += 1
                out.append(_case("wraps-%dto%d-%s-w%d" % (a, b, behind, wbits), "wraps", corpus("txt" if a == 1 else "sil"), a, _switch_steps(a, b, behind, at=150000),
                                 wbits=wbits, feed=1024 if n % 3 else None))
    return out


def space():
    out = []
    n = 0
    for a, b in ((1, 9), (6, 1), (6, 0), (0, 6), (1, 0), (0, 1)):
        kind = "txt" if a == 1 else "sil"
        for k in (0, 7):
            for feed in (None, 1024):
                steps = [D(100000, Z_NO_FLUSH), ("avail_out", k), P(b)] + ([P(b)] if k == 0 else []) + [D(N, Z_FINISH)]
                out.append(_case("space-%dto%d-out%d-%s" % (a, b, k, "feed1k" if feed else "feed16m"), "space", corpus(kind), a, steps, feed=feed,
                                 like="matrix-%dto%d-noflush-%s" % (a, b, kind), expect="like"))
    for a, b in ((1, 9), (6, 0)):  # behind a flush, where the second call is refused for another reason (nothing to flush) and switches all the same
        n += 1
        kind = "txt" if a == 1 else "sil"
        out.append(_case("space-%dto%d-out0-sync" % (a, b), "space", corpus(kind), a, [D(100000, Z_SYNC_FLUSH), ("avail_out", 0), P(b), P(b), D(N, Z_FINISH)],
                         feed=1024 if n % 2 else None, like="matrix-%dto%d-sync-%s" % (a, b, kind), expect="like"))
    for a, b, wbits in ((6, 0, 15), (0, 6, 31), (6, 0, 31), (0, 6, 15)):  # ... with the trailer's checksum at stake (`checked` overwritten)
        for k in (0, 7):
            steps = [D(150000, Z_NO_FLUSH), ("avail_out", k), P(b)] + ([P(b)] if k == 0 else []) + [D(N, Z_FINISH)]
            out.append(_case("space-%dto%d-out%d-w%d" % (a, b, k, wbits), "space", corpus("sil"), a, steps, wbits=wbits, feed=1024 if wbits == 15 else None,
                             like="wraps-%dto%d-noflush-w%d" % (a, b, wbits), expect="like"))
    return out


def carry():
    d = far_pieces()
    return [_case("carry-L%d-fixed" % level, "carry", d, level, [D(len(d), Z_NO_FLUSH), D(len(d), Z_FINISH)], strategy=Z_FIXED, feed=1024) for level in (1, 6)]


def bound():
    out = []
    for n in BOUND_N:
        d = random_bytes(n, 2)
        for level in (0, 1, 6, 9):
            for wbits in (-15, 15, 31):
                out.append(_case("bound-n%d-L%d-w%d" % (n, level, wbits), "bound", d, level, [("bound",), D(n, Z_FINISH)], wbits=wbits, expect="bound"))
    return out


def tune():
    out = []
    for i, level in enumerate((1, 3, 6)):
        kind, fast = ("txt", "sil")[i % 2], level <= 3
        d, d2 = corpus(kind), corpus(kind + "2")
        T = ("tune",) + TUNE
        feed = 1024 if i % 2 else None
        out.append(_case("tune-L%d-plain" % level, "tune", d, level, [D(100000, Z_SYNC_FLUSH), D(N, Z_FINISH)], feed=feed))
        out.append(_case("tune-L%d-first" % level, "tune", d, level, [T, D(100000, Z_NO_FLUSH), D(N, Z_FINISH)], feed=feed, expect="chunks" if fast else "ref"))
        out.append(_case("tune-L%d-first-reset" % level, "tune", d, level, [T, D(N, Z_FINISH), ("reset",), D(50000, Z_NO_FLUSH), D(len(d2), Z_FINISH)], data2=d2, feed=feed,
                         expect="chunks" if fast else "ref"))
        out.append(_case("tune-L%d-mid" % level, "tune", d, level, [D(100000, Z_SYNC_FLUSH), T, D(N, Z_FINISH)], feed=feed,
                         like="tune-L%d-plain" % level if fast else None, expect="error" if fast else "ref"))
    return out


FAMILIES = (matrix, strategy, twice, wraps, space, carry, bound, tune)


def catalogue():
    out = [c for f in FAMILIES for c in f()]
    assert len({c.name for c in out}) == len(out)
    return out


def restatement_calls(case, lenient=False):
    """(calls, params) for oracle_py.deflate_cont when the restatement can express the row -- deflate and deflateParams steps, ample space, at most one
    deflateParams in front of a call --, else None (the families space, bound and tune are fixture-only but for tune's untuned rows).
    lenient: steps that only set the output space are passed over, and so is a deflateParams that repeats the one in front of it (for the report of a
    mismatch: the bytes a space or bound row is expected to share with its ample-space row)."""
    calls, params = [], {}
    for st in case.steps:
        if st[0] == "deflate":
            calls.append((st[1], st[2]))
        elif st[0] == "params" and (len(calls) not in params or (lenient and params[len(calls)] == (st[1], st[2]))):
            params[len(calls)] = (st[1], st[2])
        elif not (lenient and st[0] in ("avail_out", "bound")):
            return None
    if not calls or calls[-1] != (len(case.data), Z_FINISH):
        return None
    return calls[:-1], params


def restated(case, lenient=False, with_params=True):
    """The row's stream by the CPU restatement (oracle/deflate_oracle.c ora_deflate_cont_p) with the header and trailer deflate() writes for the level and
    strategy in force at its first call (deflate.c:578-649, 833-855); None when restatement_calls() says so.  with_params=False: the same calls without
    the deflateParams ones."""
    from oracle import oracle_py as O
    cp = restatement_calls(case, lenient)
    if cp is None:
        return None
    calls, params = cp
    if not with_params:
        params = {}
    d = case.data
    raw = O.deflate_cont(d, case.level, calls, strategy=case.strategy, dictionary=case.dictionary or b"", params=params or None)
    level, strat = params.get(0, (case.level, case.strategy))
    if case.wbits < 0:
        return raw
    if case.wbits > 15:
        xfl = 2 if level == 9 else 4 if (strat >= 2 or level < 2) else 0
        return bytes([31, 139, 8, 0, 0, 0, 0, 0, xfl, 3]) + raw + O.crc32(d).to_bytes(4, "little") + (len(d) & 0xFFFFFFFF).to_bytes(4, "little")
    hdr = (8 + (7 << 4)) << 8
    hdr |= (0 if (strat >= 2 or level < 2) else 1 if level < 6 else 2 if level == 6 else 3) << 6
    hdr += 31 - hdr % 31
    return bytes([hdr >> 8, hdr & 255]) + raw + O.adler32(d).to_bytes(4, "big")


def play(L, ZStream, case):
    """Plays the steps on the library L (zlib's ABI).  Returns (codes, streams, bound): one return code per call (deflateSetDictionary first when there is a
    dictionary), per stream a dict with z, total_in, total_out, adler, and what deflateBound said (None without a "bound" step)."""
    P_ = C.POINTER(ZStream)
    L.deflateInit2_.argtypes = [P_, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.deflateParams.argtypes = [P_, C.c_int, C.c_int]
    L.deflateTune.argtypes = [P_, C.c_int, C.c_int, C.c_int, C.c_int]
    L.deflateSetDictionary.argtypes = [P_, C.c_char_p, C.c_uint]
    L.deflateBound.argtypes = [P_, C.c_ulong]
    L.deflateBound.restype = C.c_ulong
    L.deflate.argtypes = [P_, C.c_int]
    L.deflateReset.argtypes = [P_]
    L.deflateEnd.argtypes = [P_]
    s = ZStream()
    rc = L.deflateInit2_(C.byref(s), case.level, 8, case.wbits, 8, case.strategy, b"1.2.3", C.sizeof(ZStream))
    assert rc == Z_OK, (case.name, rc)
    codes, streams, bound_said = [], [], None
    if case.dictionary is not None:
        codes.append(L.deflateSetDictionary(C.byref(s), case.dictionary, len(case.dictionary)))
    data = case.data
    longest = max(len(case.data), len(case.data2 or b""))
    cap = longest + (longest >> 3) + 64 * len(case.steps) + 1024
    inb = C.create_string_buffer(data, max(len(data), 1))
    out = C.create_string_buffer(cap)
    opos, fed, limit = 0, 0, None

    def record():
        return dict(z=out.raw[:opos], total_in=s.total_in, total_out=s.total_out, adler=s.adler & 0xFFFFFFFF)

    for st in case.steps:
        room = cap - opos if limit is None else min(limit, cap - opos)
        s.next_out = C.addressof(out) + opos
        s.avail_out = room
        if st[0] == "deflate":
            s.next_in = C.addressof(inb) + fed
            s.avail_in = st[1] - fed
            codes.append(L.deflate(C.byref(s), st[2]))
            fed = st[1] - s.avail_in
        elif st[0] == "params":
            s.next_in = C.addressof(inb) + fed
            s.avail_in = 0
            codes.append(L.deflateParams(C.byref(s), st[1], st[2]))
        elif st[0] == "tune":
            codes.append(L.deflateTune(C.byref(s), *st[1:]))
        elif st[0] == "reset":
            streams.append(record())
            codes.append(L.deflateReset(C.byref(s)))
            data = case.data2
            inb = C.create_string_buffer(data, max(len(data), 1))
            opos, fed, limit = 0, 0, None
            continue
        elif st[0] == "avail_out":
            limit = st[1]
            continue
        elif st[0] == "bound":
            bound_said = limit = int(L.deflateBound(C.byref(s), len(data)))
            continue
        else:
            raise ValueError(st)
        opos += room - s.avail_out
        limit = None
    streams.append(record())
    L.deflateEnd(C.byref(s))
    return codes, streams, bound_said
