"""Shared by tests/test_piece_cases_cpu.py and tests/test_gpu_batch_pieces_built.py: Python zlib's verdict on an item, and what an IDEAL block finder would
report of an item of oracle/piececases.py that lies somewhere in a buffer -- worked out from the block list, not from a search."""
import zlib

from oracle import piececases as P

OK, DATA_ERROR, BUF_ERROR = 0, -3, -5
ROUND_BYTES = 131072
HDR = {"raw": 0, "zlib": 2, "gzip": 10}
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
FSPACING, SPACING = 16384, 32768


def zlib_verdict(item, wrap):
    """(ok, message, bytes, in_used) of Python's zlib for the item in wrapper `wrap`; a stream that ends before its final block: message "cut"."""
    d = zlib.decompressobj(WBITS[wrap])
    try:
        out = d.decompress(item)
    except zlib.error as e:
        return False, str(e).split(": ", 1)[-1], b"", 0
    if not d.eof:
        return False, "cut", out, 0
    return True, "", out, len(item) - len(d.unused_data)


def target_lo(body_lo, t):
    return ((body_lo + t * FSPACING) & ~15) * 8


def ideal_finder(case, buf, body_lo, end):
    """(dyn, sto, lens) as tests/tools/inflate_pieces_plan_model.cpp's `select` takes them: per finder region the first true dynamic start (a block that is
    not final, whose code-length code lies inside the region as the finder's second sieve asks; the case's planted headers count as starts) and the
    first true stored LEN the stored sieve vouches for -- the byte in front of it has zero top bits, and behind the block stands a stored header that holds
    (LEN, ~LEN, zero padding) or a true dynamic block.  The item's body is buf[body_lo:end]; its deflate data begins at body_lo."""
    body = end - body_lo
    ntargets = (body - 1) // FSPACING
    bit0 = body_lo * 8

    def bits(at, n):
        v = int.from_bytes(buf[at >> 3: (at >> 3) + 4], "little") >> (at & 7)
        return v & ((1 << n) - 1)
    dyn_all = sorted([bit0 + case.block_bits[i] for i, b in enumerate(case.blocks) if b["t"] == "dynamic" and not b["final"]] + [bit0 + p for p in case.planted])
    dyn_true = {bit0 + case.block_bits[i] for i, b in enumerate(case.blocks) if b["t"] == "dynamic"}
    sto_all = [(body_lo + case.start_of(i) // 8, len(b["data"])) for i, b in enumerate(case.blocks) if b["t"] == "stored"]
    dyn, sto, lens = [], [], []
    for t in range(1, ntargets + 1):
        lo, hi = target_lo(body_lo, t), end * 8 if t >= ntargets else target_lo(body_lo, t + 1)
        d = next((b for b in dyn_all if lo <= b < hi and b + 17 + 3 * (bits(b + 13, 4) + 4) < hi), None)
        s = None
        for B, n in sto_all:
            if not (lo >> 3 <= B < hi >> 3) or buf[B - 1] >> 5 or B + 4 > end:
                continue
            N = B + 4 + n
            if N + 5 > end:
                continue
            hb, ty = buf[N], (buf[N] >> 1) & 3
            if ty == 0:
                good = (int.from_bytes(buf[N + 1: N + 3], "little") ^ int.from_bytes(buf[N + 3: N + 5], "little")) == 0xFFFF and hb >> 3 == 0
            else:
                good = ty == 2 and N * 8 in dyn_true
            if good:
                s = B
                lens.append((B, n))
                break
        dyn.append(d); sto.append(s)
    return dyn, sto, lens


def rounds_batch(wrap):
    """The seven items of the rounds test, as (bytes, room, plaintext or None, code, message or None, went, name): items 1, 3 and 4 are a room one byte too
    small, a stream cut at two thirds and a reach one byte in front of the item; item 6 has four times its room.  With ROUND_BYTES of output room to a
    round no three of the rooms fit one round."""
    pool = P.pool()

    def good(c, times=1):
        return (c.wrapped(wrap), times * len(c.expect), c.expect, OK, None, (1, 0), c.name)
    small, cut, far = pool[3], pool[8], P.by_name("p3_25200_reach_25201")
    cut_bytes = cut.wrapped(wrap)[: len(cut.wrapped(wrap)) * 2 // 3]
    return [good(pool[0]),
            (small.wrapped(wrap), len(small.expect) - 1, None, BUF_ERROR, None, (0, 1), small.name + " (room - 1)"),
            good(pool[2]),
            (cut_bytes, len(cut.expect), None, DATA_ERROR, None, (0, 1), cut.name + " (cut)"),
            (far.wrapped(wrap), 65536, None, DATA_ERROR, far.msg, (0, 1), far.name),
            good(pool[5]),
            good(pool[6], 4)]
