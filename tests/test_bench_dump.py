"""bench.py --dump-outputs: what the last timed step computed, as float32 /
float64 .npy files under 64 MB in all, the same elements for the same
arguments; and the plain run's result line (parity and the CPU baseline are
--full's)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, str(REPO / "bench.py"), *argv], env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_dump_indices_full_size_budget():
    """The full-size workloads' element choice: fixed by the seed, sorted, in
    range, and under 64 MB once written (8 bytes per table element, 4 per
    stream byte) even for config 3's six tables."""
    import bench
    n, nm = 1 << 20, 1 << 18
    tables = {"packed_off": nm + n + 1, "seg_word_off": n + 1, "seg_in_off": n + 1,
              "seg_status": n, "msg_seg_off": nm + 1, "msg_status": nm}
    streams = {"packed": 79_000_000_123, "decoded": 82_000_000_000}
    a = bench.dump_indices(np.random.default_rng(bench.SEED), tables, streams)
    b = bench.dump_indices(np.random.default_rng(bench.SEED), tables, streams)
    size = dict(tables, **streams)
    for k in size:
        assert np.array_equal(a[k], b[k])
        assert a[k][0] >= 0 and a[k][-1] < size[k] and (np.diff(a[k]) >= 0).all()
    assert all(len(np.unique(a[k])) == len(a[k]) for k in tables)
    assert len(a["msg_status"]) == nm and len(a["seg_status"]) == bench.DUMP_TABLE_MAX
    assert len(a["packed"]) == bench.DUMP_CHUNKS * bench.DUMP_CHUNK_BYTES
    assert 8 * sum(len(a[k]) for k in tables) + 4 * sum(len(a[k]) for k in streams) <= 64 * 10 ** 6


def test_stub_dump_outputs(oracle, tmp_path):
    """The CPU rehearsal writes the oracle's own round trip: small arrays
    whole, identical from run to run."""
    argv = ["--gpus", "1", "--stub", "--config", "2", "--segments", "48", "--seg-words", "512", "--steps", "2"]
    _bench(*argv, "--dump-outputs", str(tmp_path / "a"))
    _bench(*argv, "--dump-outputs", str(tmp_path / "b"))
    swo = np.arange(0, 49 * 512, 512, dtype=np.uint64)
    data = oracle.generate(oracle.preset(2), swo)
    pk, off = oracle.pack_batch(data, swo)
    want = {"packed": pk, "packed_off": off, "decoded": data, "piece_status": np.zeros(48)}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(f"{k}.npy" for k in want)
    for k, w in want.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        assert got.dtype == (np.float64 if k == "packed_off" else np.float32)
        assert np.array_equal(got, w.astype(got.dtype))
        assert np.array_equal(got, np.load(tmp_path / "b" / f"{k}.npy"))


@pytest.mark.gpu
def test_plain_run_dumps_last_step(oracle, tmp_path):
    """A plain one-GPU run (256 pieces x 64 KiB: the byte streams are sampled,
    the tables whole): --steps sets the timed steps, the line says so and holds
    ms_per_step, nothing of --full is in it, and the dumped elements equal the
    oracle's pack of the same generated data."""
    import bench
    line = _bench("--gpus", "1", "--config", "2", "--segments", "256", "--steps", "3", "--warmup", "1",
                  "--dump-outputs", str(tmp_path))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] > 0 and line["unit"] == "GiB/s" and line["higher_is_better"] is True
    assert line["parity"] is None and line["cpu_baseline"] is None
    swo = np.arange(0, 257 * 8192, 8192, dtype=np.uint64)
    data = oracle.generate(oracle.preset(2), swo)
    pk, off = oracle.pack_batch(data, swo, threads=8)
    assert line["config"]["packed_bytes_per_gpu"] == len(pk)
    idx = bench.dump_indices(np.random.default_rng(bench.SEED), {"packed_off": 257, "piece_status": 256},
                             {"packed": len(pk), "decoded": len(data)})
    assert len(idx["decoded"]) < len(data) and len(idx["packed"]) < len(pk)
    want = {"packed": pk, "packed_off": off, "decoded": data, "piece_status": np.zeros(256)}
    for k, w in want.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == (np.float64 if k == "packed_off" else np.float32)
        assert np.array_equal(got, w[idx[k]].astype(got.dtype)), k
