"""Batch checksums (zgpu_checksum_batch_host / _device, zamd_crc32_batch / zamd_adler32_batch) against Python's zlib.crc32 / zlib.adler32: items of
every size at which the kernels take another way (empty, below and above a word, a wave's 64 lanes, the 4096 bytes a wave serves, one 64 KiB piece,
several), packed back to back so that most of them start unaligned."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from zlib_amd import gpu  # noqa: E402

SIZES = [0, 1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 65535, 65536, 65537, 200001]
STREAM_ERROR = -2


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


def _pack(items):
    offs = np.zeros(len(items) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(b) for b in items])
    return b"".join(items), offs


def _want(items, checks):
    return [(zlib.adler32(b) if checks & 1 else 1, zlib.crc32(b) if checks & 2 else 0) for b in items]


def _device(eng, blob, offs, checks, refused=False):
    """the device entry on records filled with 0x55555555; refused: the call must fail with ZGPU_STREAM_ERROR -- the records as they are then"""
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.frombuffer(bytearray(blob + b"\0"), dtype=torch.uint8).to(dev)
    d_off = torch.from_numpy(np.asarray(offs, dtype=np.uint64).astype(np.int64)).to(dev)
    n = len(offs) - 1
    d_items = torch.full((max(n, 1), 2), 0x55555555, dtype=torch.int32, device=dev)
    if refused:
        with pytest.raises(gpu.EngineError) as ei:
            eng.checksum_batch_device(d_in.data_ptr(), len(blob), d_off.data_ptr(), n, d_items.data_ptr(), checks)
        assert ei.value.code == STREAM_ERROR
    else:
        eng.checksum_batch_device(d_in.data_ptr(), len(blob), d_off.data_ptr(), n, d_items.data_ptr(), checks)
    got = d_items.cpu().numpy().view(np.uint32)
    return [(int(a), int(c)) for a, c in got[:n]]


@pytest.fixture(scope="module")
def mixed():
    rnd = random.Random(4101)
    items = [rnd.randbytes(n) for n in SIZES]
    return items, _pack(items)


@pytest.mark.parametrize("checks", [1, 2, 3], ids=["adler", "crc", "both"])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_every_path_in_one_call(eng, mixed, checks, entry):
    items, (blob, offs) = mixed
    got = eng.checksum_batch_host(blob, offs, checks) if entry == "host" else _device(eng, blob, offs, checks)
    assert got == _want(items, checks)


@pytest.mark.parametrize("entry", ["host", "device"])
def test_adler_sums_stay_in_range_on_ff_bytes(eng, entry):
    items = [b"\xff" * n for n in SIZES]
    blob, offs = _pack(items)
    got = eng.checksum_batch_host(blob, offs, 3) if entry == "host" else _device(eng, blob, offs, 3)
    assert got == _want(items, 3)


def test_three_thousand_short_items_and_the_last_partial_workgroup(eng):
    rnd = random.Random(4102)
    items = [rnd.randbytes(rnd.randint(1, 300)) for _ in range(3000)]
    blob, offs = _pack(items)
    assert eng.checksum_batch_host(blob, offs, 3) == _want(items, 3)
    assert _device(eng, blob, offs, 3) == _want(items, 3)


def test_the_threshold_between_wave_and_pieces_at_every_alignment(eng):
    rnd = random.Random(4103)
    items = []
    for pad in range(4):  # 4096 is a wave's, 4097 a piece's; a pad byte in front moves both through the alignments of a word
        items += [rnd.randbytes(pad), rnd.randbytes(4096), rnd.randbytes(4097)]
    blob, offs = _pack(items)
    assert eng.checksum_batch_host(blob, offs, 3) == _want(items, 3)


def test_piece_join_between_empty_neighbours(eng):
    big = random.Random(4104).randbytes(5 * 1024 * 1024 + 1)
    items = [b"", big, b""]
    blob, offs = _pack(items)
    assert eng.checksum_batch_host(blob, offs, 3) == _want(items, 3)
    assert _device(eng, blob, offs, 3) == _want(items, 3)


def test_bad_offset_tables_are_refused_with_nothing_written(eng):
    blob = bytes(range(256)) * 4
    for offs in ([0, 100, 50, 200], [0, 100, 200, len(blob) + 1]):
        items = (gpu.CheckItem * 3)()
        for it in items:
            it.adler32, it.crc32 = 0x1234, 0x5678
        with pytest.raises(gpu.EngineError) as ei:
            eng.checksum_batch_host(blob, offs, 3, items=items)
        assert ei.value.code == STREAM_ERROR
        assert [(it.adler32, it.crc32) for it in items] == [(0x1234, 0x5678)] * 3
        # the device entry: the plan kernel refuses the table before any kernel writes a record
        assert _device(eng, blob, offs, 3, refused=True) == [(0x55555555, 0x55555555)] * 3
    # the engine goes on working
    assert eng.checksum_batch_host(blob, [0, 100, 200, len(blob)], 3) == _want([blob[:100], blob[100:200], blob[200:]], 3)


def test_host_library_folds_running_values_in():
    from tests import zhost
    L = zhost.lib()
    L.zamd_crc32_batch.argtypes = [C.POINTER(C.c_ulong), C.POINTER(C.c_char_p), C.POINTER(C.c_ulong), C.c_size_t]
    L.zamd_adler32_batch.argtypes = [C.POINTER(C.c_ulong), C.POINTER(C.c_char_p), C.POINTER(C.c_ulong), C.c_size_t]
    rnd = random.Random(4105)
    items = [rnd.randbytes(n) for n in (0, 1, 300, 4096, 70000)]
    heads = [rnd.randbytes(n) for n in (5, 0, 17, 1000, 3)]  # what each running value has seen so far
    n = len(items)
    bufs = (C.c_char_p * n)(*items)
    lens = (C.c_ulong * n)(*[len(b) for b in items])
    crc = (C.c_ulong * n)(*[zlib.crc32(h) for h in heads])
    adler = (C.c_ulong * n)(*[zlib.adler32(h) for h in heads])
    assert L.zamd_crc32_batch(crc, bufs, lens, n) == 0
    assert L.zamd_adler32_batch(adler, bufs, lens, n) == 0
    assert list(crc) == [zlib.crc32(b, zlib.crc32(h)) for b, h in zip(items, heads)]
    assert list(adler) == [zlib.adler32(b, zlib.adler32(h)) for b, h in zip(items, heads)]
