"""What tests/test_gpu_deflate_streams.py and tests/test_gpu_deflate_streams_enqueue.py share for the one shape at which the 256-lane scans of the batched
block layer (kBatchScan, zlib_amd/csrc/zgpu_cont.hip) give a lane more than one tile and more than one block: six items, the fourth of 9,786,113 bytes =
301 tiles, its first 6,000,000 bytes byte-random (about 366 blocks of 16383 literals, stored ones among them), the rest `mix`.  The list has 307 tiles and
the long item holds tiles 3..304, so a batch of 259 tiles gives its first part exactly 256 tiles (every lane one) and a batch of 260 gives it 257 (two
tiles a lane, the tail lanes empty); one batch gives a part of 301.  The yardstick is the product's own one-call continuous stream of each item, which
runs the 1024-lane one-stream kernels and which the continuous suites pin to the reference.  Built once per session."""
import functools
import zlib

import numpy as np

from oracle import cases

LONG, LONG_RANDOM = 9786113, 6000000
BATCH_TILES = (0, 259, 260)  # 0: the call's default, one batch
OK = 0


def ntiles(n):
    return 0 if n == 0 else 1 if n <= 65024 else -(-(n - 65024) // 32512) + 1


@functools.lru_cache(maxsize=None)
def items():
    long_item = np.random.RandomState(12).randint(0, 256, LONG_RANDOM, dtype=np.uint8).tobytes() + cases.make("mix", LONG - LONG_RANDOM, 12)
    out = (cases.make("mix", 1, 1), b"", cases.make("mix", 65025, 2), long_item, cases.make("mix", 1, 3), cases.make("mix", 65025, 4))
    assert [len(d) for d in out] == [1, 0, 65025, LONG, 1, 65025]
    tiles = [ntiles(len(d)) for d in out]
    assert tiles == [1, 0, 2, 301, 1, 2] and sum(tiles[:3]) == 3  # the long item: tiles 3..304 of 307
    return out


_one_call = []


def one_call_streams(eng):
    """[(stream, adler32)] of items(): deflate_host(d, 6, F_FINAL | F_CONTINUOUS | F_ZLIB_WRAP), made once"""
    from zlib_amd import gpu
    if not _one_call:
        for d in items():
            z = eng.deflate_host(d, 6, flags=gpu.F_FINAL | gpu.F_CONTINUOUS | gpu.F_ZLIB_WRAP)
            _one_call.append((z, eng.last.adler32))
            if len(d) == LONG:  # a block is 16383 tokens: more than 256 blocks lie in the random bytes alone, which the first 256 tiles of the item cover
                assert eng.last.ntokens // 16383 > 256 and LONG_RANDOM < 256 * 32512
    return _one_call


def check(streams, records):
    """streams: the six streams of a call; records: (code, adler32) per item"""
    its = items()
    for k, (d, (z, adler)) in enumerate(zip(its, _one_call)):
        assert records[k] == (OK, zlib.adler32(d)) and adler == zlib.adler32(d), (k, records[k])
        assert streams[k] == z, (k, len(d), len(streams[k]), len(z))
        assert zlib.decompress(streams[k]) == d, k
