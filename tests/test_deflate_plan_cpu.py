"""What a compress call decides before it touches the device (zlib_amd/csrc/zgpu_deflate_plan.h): the LZ77 implementation, the batch, the steps in which
host input's batches grow, the tiles and batches of a feed of the continuous stream, the phases of round 0 at levels 1-3.  tests/tools/deflate_plan_model.cpp
calls the plan functions as the engine does, with the engine's state, the environment knobs and the free device memory given as numbers; it is built for the
host only, with the host sanitizers, makes no HIP call and is not loaded into Python.  Every expected value below is a literal worked out from the thresholds
and comments of the code, none was produced by running it.  Unless a row says otherwise: ZGPU_LZ_AUTO, the default geometry, no knob set, memory not known."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINAL, ZLIB, POS0, POS0_ALL, GZIP, CRC32, CONTINUOUS, BGZF = 1, 2, 4, 8, 16, 32, 64, 128
SERIAL, PARALLEL, SORTED, WALK, FAST, FASTWIN = 1, 2, 3, 4, 5, 6
MORE, FLUSH, FINISH = 0, 1, 2
STREAM_ERROR = -2
GIB = 1 << 30


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "deflate_plan_model")
    # host code only, with the host sanitizers: the program makes no HIP call
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "tools", "deflate_plan_model.cpp")], check=True, timeout=300)

    def run(kind, rows):
        """rows: [(inputs, expected)]; every expected key must be in the program's line for the row, with that value"""
        out = subprocess.run([exe] + ["%s %s" % (kind, " ".join("%s=%s" % kv for kv in inp.items())) for inp, _ in rows], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = out.stdout.splitlines()
        assert len(lines) == len(rows)
        for (inp, want), line in zip(rows, lines):
            if "msg" in want:  # (a refusal's text has blanks in it)
                head, _, msg = line.partition(" msg=")
                got = dict(w.split("=", 1) for w in head.split())
                got["msg"] = msg
            else:
                got = dict(w.split("=", 1) for w in line.split())
            assert {k: got.get(k) for k in want} == {k: str(v) for k, v in want.items()}, (inp, line)
    return run


def test_levels_4_to_9_walk_at_every_size(model):
    chains = {4: 16, 5: 32, 6: 128, 7: 256, 8: 1024, 9: 4096}
    model("deflate", [(dict(level=lv, nchunks=n), dict(rc=0, impl="WALK", serial=0, hand_on=0, geo=0, check_sort=1, chain=chains[lv], slow=1, nchunks=n, batch=n, first=n, nbatches=1,
                                                       block_tokens=16383, head=0, tail=0, with_crc=0, seg_wrap=0))
                      for lv in range(4, 10) for n in (1, 16384, 65536)])


def test_strategies_that_are_chain_budgets_stay_with_the_all_position_search(model):
    model("deflate", [(dict(level=6, strategy=3), dict(rc=0, impl="SORTED", chain=1, check_sort=1)),   # Z_RLE
                      (dict(level=6, strategy=2), dict(rc=0, impl="SORTED", chain=0, check_sort=1)),   # Z_HUFFMAN_ONLY
                      (dict(level=6, strategy=1), dict(rc=0, impl="WALK", chain=128)),                 # Z_FILTERED
                      (dict(level=6, strategy=4), dict(rc=0, impl="WALK", chain=128))])                # Z_FIXED


def test_levels_1_to_3_cross_over_to_the_loop_with_its_hand_on(model):
    rows = []
    for level, upto, chain in ((1, 61440, 4), (2, 45056, 8), (3, 10240, 32)):
        rows.append((dict(level=level, nchunks=upto), dict(rc=0, impl="FASTWIN", serial=0, hand_on=0, hand_piece=0, check_sort=1, chain=chain, slow=0, batch=upto)))
        rows.append((dict(level=level, nchunks=upto + 1), dict(rc=0, impl="SERIAL", serial=1, hand_on=1, check_sort=1, batch=upto + 1)))
        # (the per-launch cap of 65536 applies before the comparison: 200000 chunks are launches of 65536)
        rows.append((dict(level=level, nchunks=200000), dict(rc=0, impl="SERIAL", serial=1, hand_on=1, check_sort=1, batch=65536, hand_piece=16384, nbatches=4)))
    rows.append((dict(level=1, nchunks=61441), dict(hand_piece=15360)))
    # a segment table counts by its segments
    rows.append((dict(level=1, seg=1, nseg=61440, in_bytes=1000000), dict(rc=0, impl="FASTWIN", nchunks=61440)))
    rows.append((dict(level=1, seg=1, nseg=61441, in_bytes=1000000), dict(rc=0, impl="SERIAL", hand_on=1, nchunks=61441)))
    # ZGPU_BATCH_CHUNKS is the launch: 100000 chunks in launches of 1000 are the waves'
    rows.append((dict(level=1, nchunks=100000, batch_chunks=1000), dict(rc=0, impl="FASTWIN", batch=1000, nbatches=100)))
    # levels 1-3 with Z_HUFFMAN_ONLY / Z_RLE: the loop, nothing handed on
    rows.append((dict(level=1, strategy=2, nchunks=65536), dict(rc=0, impl="SERIAL", hand_on=0, check_sort=0)))
    rows.append((dict(level=2, strategy=3, nchunks=100), dict(rc=0, impl="SERIAL", hand_on=0, check_sort=0)))
    # deflateTune'd parameters the waves do not serve
    rows.append((dict(level=1, nchunks=100, tune_good=4, tune_lazy=4, tune_nice=8, tune_chain=5), dict(rc=0, impl="SERIAL", hand_on=0, chain=5)))
    model("deflate", rows)


def test_dictionary_chunk_and_geometry_go_to_the_loop(model):
    model("deflate", [(dict(level=6, in_bytes=40000, skip0=1000), dict(rc=0, impl="SERIAL", serial=1, hand_on=0, check_sort=0, nchunks=1, batch=1)),
                      (dict(level=1, in_bytes=65536, skip0=32506), dict(rc=0, impl="SERIAL", hand_on=0, check_sort=0)),
                      (dict(level=6, geo_w=12, geo_m=5), dict(rc=0, impl="SERIAL", serial=1, geo=1, hand_on=0, check_sort=0, block_tokens=2047, w_bits=12, hash_bits=12)),
                      (dict(level=1, geo_w=15, geo_m=9, nchunks=65536), dict(rc=0, impl="SERIAL", geo=1, hand_on=0, block_tokens=32767, w_bits=15, hash_bits=16)),
                      (dict(level=6, geo_w=9, geo_m=1, lz_impl=SERIAL), dict(rc=0, impl="SERIAL", geo=1, block_tokens=127, w_bits=9, hash_bits=8)),
                      (dict(level=6), dict(w_bits=0, hash_bits=0)),
                      # a dictionary may be as long as the geometry's window reaches: 2^12 - 262
                      (dict(level=6, geo_w=12, geo_m=5, in_bytes=40000, skip0=3834), dict(rc=0, impl="SERIAL"))])


def test_every_refusal(model):
    bgzf_only = "BGZF blocks: segment calls only, with FINAL and no other wrapper"
    fastwin = "ZGPU_LZ_FASTWIN serves levels 1..3 with their own parameters, not Z_HUFFMAN_ONLY / Z_RLE, no dictionary chunk"
    fast = "ZGPU_LZ_FAST serves levels 1..3, not Z_HUFFMAN_ONLY / Z_RLE, no dictionary chunk"
    dictionary = "dictionary chunk: 3..32506 dictionary bytes + data <= 65536, no wrapper"
    segment = "segment mode: nseg >= 1, a wrapper needs FINAL (one of zlib / gzip)"
    rows = [(dict(args=0), "null argument"),
            (dict(level=0), "level must be 1..9"), (dict(level=10), "level must be 1..9"), (dict(level=-1), "level must be 1..9"),
            (dict(chunk_size=65537), "chunk_size must be 1..65536"),
            (dict(flags=ZLIB), "a wrapper needs FINAL"), (dict(flags=GZIP), "a wrapper needs FINAL"),
            (dict(flags=FINAL | ZLIB | GZIP), "one wrapper at a time"),
            (dict(prime=17 << 16), "prime: at most 16 bits, no wrapper"), (dict(prime=(3 << 16) | 5, flags=FINAL | ZLIB), "prime: at most 16 bits, no wrapper"),
            (dict(flags=FINAL | BGZF), bgzf_only), (dict(flags=BGZF, seg=1, nseg=4), bgzf_only), (dict(flags=FINAL | BGZF | GZIP, seg=1, nseg=4), bgzf_only),
            (dict(flags=FINAL | BGZF | CONTINUOUS, seg=1, nseg=4), bgzf_only), (dict(flags=FINAL | BGZF, seg=1, nseg=4, prime=(3 << 16) | 5), bgzf_only),
            (dict(flags=FINAL | BGZF, seg=1, nseg=4, geo_w=12), "BGZF blocks need the default geometry (windowBits 15, memLevel 8)"),
            (dict(flags=FINAL | BGZF, seg=1, nseg=4, geo_m=9), "BGZF blocks need the default geometry (windowBits 15, memLevel 8)"),
            (dict(strategy=5), "strategy must be 0..4"), (dict(strategy=-1), "strategy must be 0..4"),
            (dict(geo_w=12, lz_impl=WALK), "a non-default windowBits / memLevel is served by ZGPU_LZ_SERIAL only"),
            (dict(level=1, lz_impl=WALK), "parallel LZ77 serves levels 4..9 only"), (dict(level=3, lz_impl=SORTED), "parallel LZ77 serves levels 4..9 only"),
            (dict(level=2, lz_impl=PARALLEL), "parallel LZ77 serves levels 4..9 only"), (dict(level=6, lz_impl=WALK, lz_parallel=0), "parallel LZ77 serves levels 4..9 only"),
            (dict(level=6, lz_impl=FAST), fast), (dict(level=1, lz_impl=FAST, strategy=3), fast), (dict(level=1, lz_impl=FAST, in_bytes=40000, skip0=100), fast),
            (dict(level=6, lz_impl=FASTWIN), fastwin), (dict(level=1, lz_impl=FASTWIN, strategy=2), fastwin), (dict(level=1, lz_impl=FASTWIN, in_bytes=40000, skip0=100), fastwin),
            (dict(level=1, lz_impl=FASTWIN, tune_good=4, tune_lazy=4, tune_nice=8, tune_chain=5), fastwin),
            (dict(lz_impl=7), "unknown lz_impl"), (dict(lz_impl=-1), "unknown lz_impl"),
            (dict(level=6, lz_impl=PARALLEL, strategy=1), "ZGPU_LZ_PARALLEL serves the default strategy only"),
            (dict(level=6, lz_impl=WALK, strategy=3), "ZGPU_LZ_WALK does not serve Z_HUFFMAN_ONLY / Z_RLE"), (dict(level=6, lz_impl=WALK, strategy=2), "ZGPU_LZ_WALK does not serve Z_HUFFMAN_ONLY / Z_RLE"),
            (dict(in_bytes=1000, skip0=2), dictionary), (dict(in_bytes=70000, skip0=1000), dictionary), (dict(in_bytes=40000, skip0=32507), dictionary),
            (dict(in_bytes=500, skip0=501), dictionary), (dict(in_bytes=40000, skip0=100, flags=FINAL | ZLIB), dictionary), (dict(in_bytes=40000, skip0=100, flags=POS0), dictionary),
            (dict(in_bytes=40000, skip0=100, seg=1, nseg=1), dictionary), (dict(geo_w=12, geo_m=5, in_bytes=40000, skip0=3835), dictionary),
            (dict(flags=FINAL, seg=1, nseg=0), segment)]
    model("deflate", [(inp, dict(rc=STREAM_ERROR, msg=msg)) for inp, msg in rows])


def tune(good, lazy, nice, chain):
    return dict(tune_good=good, tune_lazy=lazy, tune_nice=nice, tune_chain=chain)


def test_deflateTune_rows_no_levels_row_resembles(model):
    """Relations between the four parameters that hold in all nine rows of the level table and that an implementation rests on: where deflateTune breaks one,
    an explicit request for that implementation is refused with a message of its own, and ZGPU_LZ_AUTO -- whatever ZGPU_LZ_DEFAULT says -- serves the row."""
    quarter0 = "ZGPU_LZ_SORTED / ZGPU_LZ_PARALLEL do not serve a max_chain below 4 (deflateTune): its quarter budget never runs out"
    lazy_nice = "ZGPU_LZ_SORTED / ZGPU_LZ_PARALLEL do not serve max_lazy > nice_length (deflateTune)"
    deep = "ZGPU_LZ_SORTED does not serve a max_chain above 4096 (deflateTune)"
    insert = "ZGPU_LZ_FAST does not serve a max_insert_length above 7 (deflateTune)"
    good2 = "ZGPU_LZ_FAST does not serve a good_length below 3 (deflateTune): every search of deflate_fast is quartered"
    fastwin = "ZGPU_LZ_FASTWIN serves levels 1..3 with their own parameters, not Z_HUFFMAN_ONLY / Z_RLE, no dictionary chunk"
    refused, served = [], []
    for impl in (SORTED, PARALLEL):
        refused += [(dict(level=6, lz_impl=impl, **tune(4, 16, 32, c)), quarter0) for c in (1, 2, 3)]
        refused += [(dict(level=lv, lz_impl=impl, **tune(4, 16, 32, 3)), quarter0) for lv in (4, 9)]
        refused += [(dict(level=6, lz_impl=impl, **tune(8, 258, 32, 128)), lazy_nice), (dict(level=6, lz_impl=impl, **tune(4, 64, 8, 32)), lazy_nice),
                    (dict(level=6, lz_impl=impl, **tune(8, 33, 32, 128)), lazy_nice), (dict(level=6, lz_impl=impl, **tune(8, 16, 3, 128)), lazy_nice)]
        if impl == SORTED:  # (match3_kernel's keys; the link ring counts in a register)
            refused += [(dict(level=6, lz_impl=impl, **tune(8, 16, 128, c)), deep) for c in (0, 4097, 65535, 70000)]
        else:
            served += [(dict(level=6, lz_impl=impl, **tune(8, 16, 128, c)), dict(rc=0, impl="PARALLEL", chain=c or 0xffffffff)) for c in (0, 4097, 65535, 70000)]
        # on either side of each relation: served
        served += [(dict(level=6, lz_impl=impl, **tune(4, 16, 32, 4)), dict(rc=0, chain=4)), (dict(level=6, lz_impl=impl, **tune(8, 32, 32, 128)), dict(rc=0, lazy=32, nice=32)),
                   (dict(level=6, lz_impl=impl, **tune(8, 16, 128, 4096)), dict(rc=0, chain=4096)),
                   (dict(level=6, lz_impl=impl, **tune(32, 1000, 258, 4096)), dict(rc=0, lazy=1000, nice=258)),  # (258 bytes in hand: nothing is longer)
                   (dict(level=6, lz_impl=impl, **tune(32, 1000, 1000, 4096)), dict(rc=0, nice=258)),
                   (dict(level=6, lz_impl=impl, **tune(0, 16, 128, 128)), dict(rc=0, good=0)), (dict(level=6, lz_impl=impl, **tune(300, 0, 128, 128)), dict(rc=0, good=300, lazy=0))]
    # Z_RLE and Z_HUFFMAN_ONLY are chain budgets of their own (1 and 0, no quarter): the all-position search keeps them whatever max_chain says
    served += [(dict(level=6, strategy=3, **tune(4, 16, 32, 3)), dict(rc=0, impl="SORTED", chain=1)), (dict(level=6, strategy=2, **tune(8, 16, 128, 0)), dict(rc=0, impl="SORTED", chain=0)),
               (dict(level=6, strategy=3, lz_impl=SORTED, **tune(8, 258, 32, 70000)), dict(rc=0, impl="SORTED", chain=1))]
    # the walkers and the lane-per-chunk loop play the reference's own loop: every row
    for t in (tune(4, 16, 32, 3), tune(4, 16, 32, 1), tune(8, 258, 32, 128), tune(8, 16, 128, 0), tune(8, 16, 128, 70000), tune(0, 0, 0, 0)):
        served += [(dict(level=6, **t), dict(rc=0, impl="WALK")), (dict(level=6, lz_impl=WALK, **t), dict(rc=0, impl="WALK")), (dict(level=6, lz_impl=SERIAL, **t), dict(rc=0, impl="SERIAL")),
                   (dict(level=6, lz_default=3, **t), dict(rc=0, impl="WALK"))]  # ZGPU_LZ_DEFAULT=3 does not send the default path into a refusal
    # max_chain is kept whole (the quarter of 70000 is 17500); 0, which never runs out, is the largest budget there is
    served += [(dict(level=6, **tune(8, 16, 128, 0)), dict(rc=0, chain=0xffffffff)), (dict(level=6, **tune(8, 16, 128, 70000)), dict(rc=0, chain=70000)),
               (dict(level=6, **tune(8, 16, 128, 65535)), dict(rc=0, chain=65535)), (dict(level=1, nchunks=100, **tune(4, 4, 8, 0)), dict(rc=0, impl="SERIAL", chain=0xffffffff)),
               (dict(level=6, lz_default=3, **tune(8, 16, 32, 33)), dict(rc=0, impl="SORTED"))]
    # levels 1-3.  The waves: the level's good_length, nice_length and max_chain, and max_insert_length BELOW nice_length
    for lv, nice, chain in ((1, 8, 4), (2, 16, 8), (3, 32, 32)):
        served += [(dict(level=lv, nchunks=100, **tune(4, mi, nice, chain)), dict(rc=0, impl="FASTWIN", lazy=mi)) for mi in (0, 3, nice - 1)]
        served += [(dict(level=lv, nchunks=100, lz_impl=FASTWIN, **tune(4, nice - 1, nice, chain)), dict(rc=0, impl="FASTWIN"))]
        for mi in (nice, nice + 1, 258):
            served += [(dict(level=lv, nchunks=100, **tune(4, mi, nice, chain)), dict(rc=0, impl="SERIAL", hand_on=0, lazy=mi)),
                       (dict(level=lv, nchunks=100000, **tune(4, mi, nice, chain)), dict(rc=0, impl="SERIAL", hand_on=0))]  # (no hand-on to the waves either)
            refused += [(dict(level=lv, lz_impl=FASTWIN, **tune(4, mi, nice, chain)), fastwin)]
    refused += [(dict(level=1, lz_impl=FASTWIN, **tune(2, 4, 8, 4)), fastwin), (dict(level=1, lz_impl=FASTWIN, **tune(2, 4, 8, 3)), fastwin)]
    served += [(dict(level=1, nchunks=100, **tune(2, 4, 8, 4)), dict(rc=0, impl="SERIAL", hand_on=0)), (dict(level=1, nchunks=100, **tune(2, 4, 8, 3)), dict(rc=0, impl="SERIAL", chain=3))]
    # deflate_fast on the sorted buckets: max_insert_length up to 7, good_length above 2
    served += [(dict(level=1, lz_impl=FAST, **tune(4, mi, 8, 4)), dict(rc=0, impl="FAST", lazy=mi)) for mi in (0, 3, 7)]
    served += [(dict(level=1, lz_impl=FAST, **tune(3, 4, 8, 4)), dict(rc=0, impl="FAST")), (dict(level=1, nchunks=100, lz_default=5, **tune(4, 7, 8, 4)), dict(rc=0, impl="FAST"))]
    refused += [(dict(level=1, lz_impl=FAST, **tune(4, mi, 8, 4)), insert) for mi in (8, 258)] + [(dict(level=3, lz_impl=FAST, **tune(4, 31, 32, 32)), insert)]
    refused += [(dict(level=1, lz_impl=FAST, **tune(g, 4, 8, 4)), good2) for g in (0, 2)]
    served += [(dict(level=1, nchunks=100, lz_default=5, **tune(4, 8, 8, 4)), dict(rc=0, impl="SERIAL")), (dict(level=1, nchunks=100, lz_default=5, **tune(2, 4, 8, 3)), dict(rc=0, impl="SERIAL"))]
    model("deflate", [(inp, dict(rc=STREAM_ERROR, msg=msg)) for inp, msg in refused] + served)


def test_framing(model):
    model("deflate", [(dict(flags=FINAL), dict(rc=0, head=0, tail=0, with_crc=0, seg_wrap=0)),
                      (dict(flags=FINAL | ZLIB), dict(rc=0, head=2, tail=4, with_crc=0, seg_wrap=0)),
                      (dict(flags=FINAL | GZIP), dict(rc=0, head=10, tail=8, with_crc=1, seg_wrap=0)),
                      (dict(flags=FINAL | CRC32), dict(rc=0, head=0, tail=0, with_crc=1, seg_wrap=0)),
                      (dict(flags=FINAL | ZLIB, seg=1, nseg=7), dict(rc=0, head=0, tail=0, with_crc=0, seg_wrap=1, nchunks=7, batch=7)),
                      (dict(flags=FINAL | GZIP, seg=1, nseg=7), dict(rc=0, head=0, tail=0, with_crc=1, seg_wrap=1)),
                      (dict(flags=FINAL | BGZF, seg=1, nseg=7), dict(rc=0, head=0, tail=0, with_crc=1, seg_wrap=1, impl="WALK")),
                      (dict(flags=FINAL, seg=1, nseg=7), dict(rc=0, seg_wrap=0)),
                      (dict(in_bytes=0), dict(rc=0, nchunks=1, batch=1)),
                      (dict(in_bytes=100001, chunk_size=1000), dict(rc=0, nchunks=101, batch=101))])


def test_knobs(model):
    model("deflate", [(dict(level=1, nchunks=1000, lz_default=1), dict(rc=0, impl="SERIAL", hand_on=0, check_sort=0)),       # ZGPU_LZ_DEFAULT=1 keeps the loop
                      (dict(level=6, nchunks=1000, lz_default=1), dict(rc=0, impl="WALK")),
                      (dict(level=6, nchunks=1000, lz_default=3), dict(rc=0, impl="SORTED", chain=128, check_sort=1)),      # the all-position search
                      (dict(level=1, nchunks=1000, lz_default=5), dict(rc=0, impl="FAST", serial=0, hand_on=0, check_sort=1)),
                      (dict(level=1, nchunks=1000, lz_default=5, in_bytes=40000, skip0=100), dict(rc=0, impl="SERIAL")),
                      (dict(level=1, nchunks=65536, lz_default=6), dict(rc=0, impl="FASTWIN", hand_on=0)),                   # the waves whatever the size
                      (dict(level=1, nchunks=65536, hand_on=0), dict(rc=0, impl="SERIAL", hand_on=0, hand_piece=0, check_sort=0)),  # ZGPU_HAND_ON=0: the loop keeps every chunk
                      (dict(level=1, nchunks=1000, hand_on=0), dict(rc=0, impl="FASTWIN")),
                      (dict(level=1, nchunks=1000, hand_on=2), dict(rc=0, impl="SERIAL", hand_on=1, hand_piece=1000, check_sort=1)),  # =2: the loop + hand-on at any size
                      (dict(level=1, nchunks=1000, hand_on=2, lz_default=6), dict(rc=0, impl="FASTWIN", hand_on=0)),
                      (dict(level=1, nchunks=1000, hand_on=2, lz_impl=SERIAL), dict(rc=0, impl="SERIAL", hand_on=0)),         # (AUTO only)
                      (dict(level=6, nchunks=1000, hand_on=2), dict(rc=0, impl="WALK", hand_on=0)),
                      (dict(level=6, nchunks=1000, exact_sort=1), dict(rc=0, impl="WALK", check_sort=0)),                    # the self-check has failed once: the exact sort is not checked
                      (dict(level=6, nchunks=1000, batch_chunks=300, steps=1), dict(rc=0, batch=300, first=300, nbatches=4, steps="300,300,300,100"))])  # ZGPU_BATCH_CHUNKS


def test_hand_piece_is_a_quarter_of_the_batch_and_at_least_4096(model):
    model("deflate", [(dict(level=1, nchunks=n, hand_on=2), dict(rc=0, hand_on=1, batch=min(n, 65536), hand_piece=hp)) for n, hp in ((1000, 1000), (4095, 4095), (4096, 4096), (8000, 4096),
                                                                                                                                  (16384, 4096), (16388, 4097), (65536, 16384), (100000, 16384))])


def test_host_input_ramps_up_at_levels_4_to_9_only(model):
    model("deflate", [(dict(level=6, nchunks=65536, host=1, steps=1), dict(rc=0, impl="WALK", batch=16384, first=2048, nbatches=7, steps="2048,4096,8192,16384,16384,16384,2048")),
                      (dict(level=6, nchunks=65536, steps=1), dict(rc=0, batch=65536, first=65536, nbatches=1, steps="65536")),          # device input: one launch
                      (dict(level=6, nchunks=16384, host=1, steps=1), dict(rc=0, batch=16384, first=2048, steps="2048,4096,8192,2048")),
                      (dict(level=6, nchunks=4096, host=1, steps=1), dict(rc=0, batch=4096, first=2048, steps="2048,2048")),
                      (dict(level=6, nchunks=4095, host=1, steps=1), dict(rc=0, batch=4095, first=4095, steps="4095")),                  # (a batch below two first ones: no ramp)
                      (dict(level=6, nchunks=8193, host=1, steps=1), dict(rc=0, batch=8193, first=2048, steps="2048,4096,2049")),
                      (dict(level=6, nchunks=65536, host=1, host_batch=8192, first_batch=1024, steps=1), dict(rc=0, batch=8192, first=1024, steps="1024,2048,4096" + ",8192" * 7 + ",1024")),
                      # levels 1-3: no ramp and no cut to 16384; the crossover sees a launch of 65536
                      (dict(level=1, nchunks=65536, host=1, steps=1), dict(rc=0, impl="SERIAL", hand_on=1, batch=65536, first=65536, nbatches=1, steps="65536")),
                      (dict(level=1, nchunks=61440, host=1, steps=1), dict(rc=0, impl="FASTWIN", batch=61440, first=61440, steps="61440")),
                      (dict(level=1, nchunks=200000, host=1, host_batch=16384), dict(rc=0, impl="FASTWIN", batch=16384, first=16384, nbatches=13)),
                      (dict(level=3, nchunks=65536, host=1), dict(rc=0, impl="SERIAL", hand_on=1, batch=65536, first=65536))])


def test_memory_cap(model):
    # levels 4-9: 4 * 65536 of tokens + a slot of 65792 + the sorted buckets (given: 1000000) = 1327936 bytes a chunk; six tenths of what is free (and held) count
    per = 4 * 65536 + 65792 + 1000000
    assert per == 1327936
    free = 22132266670  # free // 10 * 6 = 13279360002 = 10000 * per + 2
    serial = 4 * 65536 + 65792 + 65536 * 16  # the loop: tables of 65536 uint4 instead
    model("deflate", [(dict(level=6, nchunks=65536, sws=1000000, free=free), dict(rc=0, batch=10000, first=10000, nbatches=7)),
                      (dict(level=6, nchunks=65536, sws=1000000, free=free - 20), dict(rc=0, batch=9999)),
                      (dict(level=6, nchunks=65536, sws=1000000, free=free - 5000 * per, batch_cap=5000), dict(rc=0, batch=10000)),  # what the engine holds is counted as free
                      (dict(level=6, nchunks=5000, sws=1000000, free=free), dict(rc=0, batch=5000)),
                      (dict(level=6, nchunks=65536, sws=1000000, free=1000000), dict(rc=0, batch=256, nbatches=256)),               # never below 256
                      (dict(level=6, nchunks=100, sws=1000000, free=1000000), dict(rc=0, batch=100)),
                      (dict(level=6, nchunks=65536, sws=1000000, free=10 * ((300 * serial + 5) // 6 + 1), lz_impl=SERIAL), dict(rc=0, impl="SERIAL", batch=300)),
                      (dict(level=6, nchunks=65536, sws=1000000), dict(rc=0, batch=65536))])                                          # free = 0: not known, no cap


def test_continuous_feed_tiles(model):
    rows = [  # a feed that parses nothing: ZGPU_CONT_MORE holds back kTileSlack = 512 bytes
        (dict(level=6, buf=512, mode=MORE), dict(fast_lz=0, e0=0, w0=0, end=0, ntiles=0, batch=1)),
        (dict(level=6, buf=1000, entry=600, mode=MORE), dict(e0=600, end=488, ntiles=0, batch=1)),
        (dict(level=6, buf=0, mode=FINISH), dict(end=0, ntiles=0, batch=1)),
        (dict(level=6, buf=513, mode=MORE), dict(end=1, ntiles=1, batch=1)),
        # one tile up to w0 + kTileH1 = 65024, a second one from there
        (dict(level=6, buf=1, mode=FINISH), dict(end=1, ntiles=1, pipe=0, batch=1, nbatches=1)),
        (dict(level=6, buf=65024, mode=FINISH), dict(end=65024, ntiles=1)),
        (dict(level=6, buf=65025, mode=FLUSH), dict(end=65025, ntiles=2, batch=2)),
        (dict(level=6, buf=65024 + 32512, mode=FINISH), dict(ntiles=2)),
        (dict(level=6, buf=65024 + 32512 + 1, mode=FINISH), dict(ntiles=3)),
        # a stream that stands at 1040000 with a buffer from 1000000: the first tile starts 32512 in front of the entry
        (dict(level=6, abs0=1000000, entry=1040000, buf=72512, mode=FINISH), dict(e0=40000, w0=7488, end=72512, ntiles=1)),
        (dict(level=6, abs0=1000000, entry=1040000, buf=72513, mode=FINISH), dict(e0=40000, w0=7488, ntiles=2)),
        (dict(level=6, abs0=1000000, entry=1010000, buf=72513, mode=FINISH), dict(e0=10000, w0=0, ntiles=2)),
        (dict(level=6, buf=100000, mode=MORE), dict(end=99488, ntiles=3, batch=3)),
        (dict(level=6, buf=100000, mode=FLUSH), dict(end=100000, ntiles=3)),
        (dict(level=6, buf=65024 + 512, mode=MORE), dict(end=65024, ntiles=1)),
        # levels 1-3 go by rounds, but for Z_HUFFMAN_ONLY
        (dict(level=1, buf=65025), dict(fast_lz=1, ntiles=2)), (dict(level=3, buf=65025), dict(fast_lz=1)), (dict(level=4, buf=65025), dict(fast_lz=0)),
        (dict(level=1, strategy=2, buf=65025), dict(fast_lz=0, ntiles=2))]
    model("cont", rows)


def test_continuous_feed_batches(model):
    per_tile = 1000000 + 4 * 65536 + 4 * (32512 + 512) + 4 * 65792  # the buckets (given), tokens, the stream's tokens, four slots
    assert per_tile == 1657408
    tiles = lambda n: 65024 + (n - 1) * 32512  # the longest buffer of n tiles: one byte more is one tile more
    rows = [  # levels 1-3: no short batch at the end
        (dict(level=1, buf=2 * GIB), dict(fast_lz=1, ntiles=66052, batch=66052, nbatches=1)),
        (dict(level=1, buf=4 * GIB), dict(ntiles=132104, batch=66052, nbatches=2)),
        (dict(level=1, buf=4 * GIB, sws=1000000, free=200 * 10 ** 9), dict(ntiles=132104, batch=66052, nbatches=2)),  # memory admits 72402 tiles
        (dict(level=1, buf=4 * GIB, sws=1000000, free=180 * 10 ** 9), dict(ntiles=132104, batch=65161, nbatches=3)),  # ... 65161: not the even batches
        (dict(level=1, buf=2 * GIB, batch_tiles=65536), dict(batch=65536, nbatches=2)),                               # ZGPU_CONT_BATCH_TILES is taken at its word
        (dict(level=1, buf=tiles(65536 + 8192)), dict(ntiles=73728, batch=36864, nbatches=2)),                        # a remainder of an eighth of a batch and more stays a batch: two of one size
        (dict(level=1, buf=tiles(65536 + 8191)), dict(ntiles=73727, batch=73727, nbatches=1)),
        (dict(level=1, buf=tiles(65536)), dict(ntiles=65536, batch=65536, nbatches=1)),
        # levels 4-9: batches of 32768
        (dict(level=6, buf=4 * GIB), dict(fast_lz=0, ntiles=132104, pipe=0, batch=32768, nbatches=5)),
        (dict(level=6, buf=4 * GIB, sws=1000000, free=10 ** 9), dict(batch=362)),
        (dict(level=6, buf=4 * GIB, sws=1000000, free=10 ** 6), dict(batch=64)),                                      # never below 64
        (dict(level=6, buf=4 * GIB, sws=1000000, free=10 ** 6, batch_cap=1000, par_cap=1000, ct_tiles=1000), dict(batch=600)),  # what the engine holds (1000 tiles' worth) would be used again
        # ZGPU_CONT_PIPE: 2 whatever the size, 1 from 2048 tiles; half batches, at least four of them
        (dict(level=6, buf=tiles(1), pipe=2), dict(ntiles=1, pipe=0, batch=1)),
        (dict(level=6, buf=tiles(1) + 1, pipe=2), dict(ntiles=2, pipe=1, batch=2)),
        (dict(level=6, buf=tiles(2047), pipe=1), dict(ntiles=2047, pipe=0, batch=2047, nbatches=1)),
        (dict(level=6, buf=tiles(2048), pipe=1), dict(ntiles=2048, pipe=1, batch=2048, nbatches=1)),
        (dict(level=6, buf=tiles(8192), pipe=1), dict(ntiles=8192, pipe=1, batch=2048, nbatches=4)),
        (dict(level=6, buf=4 * GIB, pipe=1), dict(ntiles=132104, pipe=1, batch=16384, nbatches=9)),
        (dict(level=6, buf=4 * GIB, pipe=0), dict(pipe=0, batch=32768)),
        (dict(level=1, buf=4 * GIB, pipe=2), dict(fast_lz=1, pipe=0, batch=66052))]                                   # (levels 4-9 only)
    model("cont", rows)


def test_round0_phases(model):
    # tiles / 256 up to 16, and no phase over the 2816 tiles the chip holds at once (eleven workgroups on each of 256 CUs): 4 GiB at level 1 are two
    # batches of 66 052 tiles in 24 phases each, the count measured best there
    model("phases", [(dict(nb=n), dict(K=k)) for n, k in ((1, 1), (255, 1), (256, 1), (511, 1), (512, 2), (4095, 15), (4096, 16), (4128, 16), (45056, 16), (45057, 17), (65536, 24), (66052, 24), (67584, 24), (67585, 25))] +
          # ZGPU_FAST_RUN is taken at its word, up to 64
          [(dict(nb=n, fast_run=r), dict(K=k)) for n, r, k in ((4096, 1, 1), (4096, 3, 3), (66052, 16, 16), (100, 64, 64), (100, 100, 64))])

