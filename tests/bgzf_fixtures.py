"""BGZF files for the tests, made with Python's zlib (a foreign producer): a block writer, a header chase (the index oracle) and the catalogue of
well-formed and malformed files.  gzip.decompress reads multi-member files and is the data oracle.  Test helper."""
import functools
import struct
import zlib

from oracle import cases

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK = 65280


def header(total, front=b"", si=b"BC"):
    """the gzip header of a block of `total` bytes: FEXTRA, XFL 0, OS 255, the subfields `front` and then si (BSIZE = total - 1)"""
    return bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", len(front) + 6) + front + si + struct.pack("<HH", 2, total - 1)


def block(data, level=6, front=b"", si=b"BC", body=None):
    if body is None:
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(data) + c.flush()
    total = 12 + len(front) + 6 + len(body) + 8
    assert total <= 65536
    return header(total, front, si) + body + struct.pack("<II", zlib.crc32(data), len(data))


def write(data, level=6, size=BLOCK, eof=True):
    return b"".join(block(data[i: i + size], level) for i in range(0, len(data), size)) + (EOF_BLOCK if eof else b"")


def chase(f):
    """(block starts + [len(f)], exclusive sums of ISIZE + [total], ends with the end block), or None when the blocks do not chain from byte 0 to
    exactly len(f)"""
    pos, upos, co, uo = 0, 0, [], []
    while pos < len(f):
        if len(f) - pos < 12 or f[pos: pos + 3] != b"\x1f\x8b\x08" or not f[pos + 3] & 4:
            return None
        xend, q, bsize = pos + 12 + struct.unpack_from("<H", f, pos + 10)[0], pos + 12, None
        if xend > len(f):
            return None
        while q + 4 <= xend and bsize is None:
            slen = struct.unpack_from("<H", f, q + 2)[0]
            if f[q: q + 2] == b"BC" and slen == 2:
                if q + 6 > xend:
                    return None
                bsize = struct.unpack_from("<H", f, q + 4)[0]
            q += 4 + slen
        if bsize is None or pos + bsize + 1 > len(f) or bsize + 1 < xend - pos + 2 + 8:
            return None
        isize = struct.unpack_from("<I", f, pos + bsize + 1 - 4)[0]
        if isize > 65536:
            return None
        co.append(pos); uo.append(upos)
        pos += bsize + 1; upos += isize
    return co + [len(f)], uo + [upos], len(co) > 0 and f[co[-1]:] == EOF_BLOCK


def _stored(payload):
    return block(payload, 0)


def _many():
    base = cases.make("text", 64 * 1024, 31)
    out, at = [], 0
    for k in range(1500):
        n = 1 + (k * 7919) % 40
        out.append(base[at: at + n]); at += n
    return out


MANY_PIECES = _many()
SIX = [cases.make("mix", 3000 + 500 * i, 60 + i) for i in range(6)]


def six_blocks():
    return [block(d, 6) for d in SIX]


def _decoy_inner():
    inner = write(cases.make("text", 5000, 41), 6, 2000)  # three blocks and the end block, all inside one stored block's payload
    return _stored(b"front" + inner + b"back") + block(cases.make("mix", 3000, 42)) + EOF_BLOCK


def _decoy_join():
    """a stored block whose payload holds an 18-byte BGZF header that points exactly at the next true block's start"""
    front, back = b"A" * 100, b"B" * 200
    total = 18 + 5 + len(front) + 18 + len(back) + 8   # header, stored-block header, payload, trailer
    at = 18 + 5 + len(front)                           # where the false header sits in the block
    payload = front + header(total - at) + back
    b = _stored(payload)
    assert len(b) == total and chase(b[at:] + EOF_BLOCK) is not None  # the false candidate chains into the true chain
    return b + block(cases.make("text", 4000, 43)) + EOF_BLOCK


@functools.lru_cache(maxsize=None)
def well_formed():
    """name -> file"""
    mix = cases.make("mix", 20000, 44)
    a, b = write(cases.make("text", 70000, 45)), write(cases.make("runs", 9000, 46), 1)
    return {
        "one": write(cases.make("text", 5000, 47)),
        "levels": b"".join(block(mix[5000 * i: 5000 * (i + 1)], lv) for i, lv in enumerate((0, 1, 6, 9))) + EOF_BLOCK,
        "full": block(bytes(65536), 6) + EOF_BLOCK,
        "xlen10": block(mix[:7000], 6, front=b"XY\x00\x00") + block(mix[7000:9000], 6, front=b"Q\x01\x00\x00") + EOF_BLOCK,
        "concat": a + b,
        "noeof": write(cases.make("mix", 150000, 48), 6, eof=False),
        "three": write(cases.make("mix", 3 * BLOCK - 1000, 49)),
        "many": b"".join(block(p, 6) for p in MANY_PIECES) + EOF_BLOCK,
        "decoy_inner": _decoy_inner(),
        "decoy_join": _decoy_join(),
        "empty_file": b"",
        "eof_only": EOF_BLOCK,
        "smallest": EOF_BLOCK * 300,  # as many blocks as a file of its length can hold
    }


@functools.lru_cache(maxsize=None)
def malformed():
    """name -> file whose blocks do not chain from byte 0 to exactly its end"""
    blocks = six_blocks()
    good = b"".join(blocks) + EOF_BLOCK
    b3 = blocks[3]
    bumped = b3[:16] + struct.pack("<H", struct.unpack_from("<H", b3, 16)[0] + 1) + b3[18:]
    return {
        "cut": good[:-1],
        "appended": good + b"\x00",
        "bsize_plus_one": b"".join(blocks[:3]) + bumped + b"".join(blocks[4:]) + EOF_BLOCK,
        "first_byte": b"\x1e" + good[1:],
        "no_bc": block(SIX[0], 6, si=b"XY") + EOF_BLOCK,
        "isize_large": blocks[0][:-4] + struct.pack("<I", 65537) + EOF_BLOCK,
        "no_body": block(b"", body=b"") * 40 + EOF_BLOCK,  # 26-byte blocks: a header and a trailer with no deflate data between them
    }


def mutations(count=120, seed=5):
    """files one byte away from a well-formed one, the byte inside a header or a trailer: most do not chain any more, some still do"""
    import random
    rng = random.Random(seed)
    wf = well_formed()
    out = []
    for i in range(count):
        f = bytearray(wf[("xlen10", "decoy_join", "levels", "concat")[i % 4]])
        co = chase(bytes(f))[0]
        k = rng.randrange(len(co) - 1)
        at = co[k] + rng.randrange(0, 24) if i % 3 else co[k + 1] - 1 - rng.randrange(0, 4)
        f[at] = rng.randrange(256) if i % 2 else f[at] ^ (1 << rng.randrange(8))
        out.append(bytes(f))
    return out
