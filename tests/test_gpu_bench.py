"""bench.py as it is run for every change: a plain run prints the one line with the headline's fields and nothing of --full, --steps sets the
number of timed steps, and --dump-outputs writes what the last timed step gave its caller -- here checked against the CPU oracle's bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    from oracle import corpus_py as CP, oracle_py as O
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--gib", "0.125", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "GiB/s" and j["higher_is_better"] is True and j["dtype"] == "u8" and j["metric"].startswith("GiB/s raw input compressed")
    assert "extra" not in j and "cpu_baseline" not in j and j["config"]["chunks_checked_against_reference_hashes"] is None

    nchunks = (1 << 27) // 65536
    stream_bytes, adler = np.load(out / "result.npy").astype(np.int64).tolist()
    offs = np.load(out / "chunk_offsets.npy").astype(np.int64)
    assert stream_bytes == j["config"]["stream_bytes"]
    assert len(offs) == nchunks + 1 and offs[0] == 2 and offs[-1] + 4 == stream_bytes and (np.diff(offs) > 0).all()
    sample = np.load(out / "stream.npy")
    at = np.load(out / "stream_at.npy").astype(np.int64)
    digest = np.load(out / "stream_digest.npy")
    assert sample.dtype == np.float32 and digest.dtype == np.float64
    assert len(at) == 128 and at[0] == 0 and at[-1] == (stream_bytes - 1) // 65536 * 65536 and len(digest) == -(-stream_bytes // 65536)
    assert len(sample) == 127 * 65536 + stream_bytes - at[-1]
    z = sample.astype(np.uint8).tobytes()
    # the first window: zlib header and chunk 0 as the oracle writes it; its digest; the last window ends with the Adler-32 of the input
    data0 = CP.chunk(CP.KIND_SILESIA, 0)
    assert z[:2] == O.deflate_stream(data0, 6)[:2]
    assert z[offs[0]:offs[1]] == O.deflate_chunk(data0, 6, False)
    assert digest[0] == float((np.frombuffer(z[:65536], dtype=np.uint8).astype(np.int64) * np.arange(1, 65537)).sum())
    assert int.from_bytes(z[-4:], "big") == adler
