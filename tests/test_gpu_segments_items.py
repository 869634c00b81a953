"""Per-segment records of the segment compressor (zgpu_deflate_segments_items_host): the bytes are those of zgpu_deflate_segments_host, and record k
says where segment k's stream lies, the checksums of its input and strm->data_type after its first block."""
import zlib

import pytest

pytestmark = pytest.mark.gpu

from oracle import cases  # noqa: E402
from zlib_amd import gpu  # noqa: E402

SEGMENTS = [cases.make(kind, n, 40 + i) for i, (kind, n) in enumerate(
    [("text", 0), ("text", 1), ("text", 100), ("text", 4096), ("text", 65536), ("rand", 1), ("rand", 4096), ("rand", 65536), ("runs", 100), ("runs", 65536)])]
WRAPS = {"raw": (0, -15), "zlib": (gpu.F_ZLIB_WRAP, 15), "gzip": (gpu.F_GZIP_WRAP, 31)}


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data_types():
    """strm->data_type of a one-item deflate() of each segment through the host library, per level"""
    from tests import zhost
    return {level: [zhost.deflate_stream(d, level, [(len(d), zhost.Z_FINISH)], window_bits=-15)[2]["data_type"] for d in SEGMENTS] for level in (1, 6)}


def _check(segs, items, plain, flags, want_types):
    assert segs == plain
    at = 0
    for d, z, (out_lo, out_bytes, in_bytes, data_type, adler, crc), want_type in zip(SEGMENTS, plain, items, want_types):
        assert (out_lo, out_bytes) == (at, len(z))
        at += len(z)
        assert in_bytes == len(d)
        assert adler == zlib.adler32(d)
        assert crc == (zlib.crc32(d) if flags & (gpu.F_GZIP_WRAP | gpu.F_CRC32) else 0)
        assert data_type == want_type


@pytest.mark.parametrize("wrap", sorted(WRAPS))
@pytest.mark.parametrize("level", [1, 6])
def test_records_describe_the_segments(eng, data_types, level, wrap):
    flags = gpu.F_FINAL | WRAPS[wrap][0]
    plain = eng.deflate_segments_host(SEGMENTS, level, flags=flags)
    segs, items = eng.deflate_segments_host(SEGMENTS, level, flags=flags, want_items=True)
    _check(segs, items, plain, flags, data_types[level])
    assert data_types[level][0] == 2 and items[0][3] == 2  # the empty segment: Z_UNKNOWN


def test_crc_flag_without_a_wrapper_and_records_written_batch_by_batch(eng, data_types, monkeypatch):
    flags = gpu.F_FINAL | gpu.F_CRC32
    plain = eng.deflate_segments_host(SEGMENTS, 6, flags=flags)
    monkeypatch.setenv("ZGPU_BATCH_CHUNKS", "4")  # ten segments in three launches
    segs, items = eng.deflate_segments_host(SEGMENTS, 6, flags=flags, want_items=True)
    _check(segs, items, plain, flags, data_types[6])
