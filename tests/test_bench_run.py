"""bench.py as a program on the GPU, at a small size (2048 x 32 KiB blocks).

* the plain run (`--gpus 1 --steps K --warmup W`) prints one JSON line with
  the headline fields and nothing that takes runs of its own; `--steps` is
  the number of timed steps; `--dump-outputs DIR` writes the digests the last
  timed step returned, every one of which the oracle confirms on the host
  over the config-2 bytes regenerated from the seed;
* `--full` adds the parity checks and the live VALU ceiling.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import ROOT

pytestmark = pytest.mark.gpu

BS, NBLK = 32768, 2048


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--blocks", str(NBLK), "--block-size", str(BS)] + args,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_digests(gpu, oracle, tmp_path):
    out = str(tmp_path / "dump")
    rec = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", out])
    assert rec["metric"] == bench.METRIC and rec["unit"] == "GiB/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "u64"
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["ms_per_step"] > 0
    # value is the bytes of the timed steps over their time
    assert rec["value"] == pytest.approx(NBLK * BS / (rec["ms_per_step"] / 1e3) / bench.GIB,
                                         rel=1e-2)
    assert "secondary" not in rec and "cpu_baseline" not in rec
    assert rec["roofline"]["valu_ceiling_ms"] is None
    assert rec["parity"] == bench.PARITY_NOT_CHECKED

    got = np.load(os.path.join(out, "digests.npy"))
    idx = np.load(os.path.join(out, "digests_blocks.npy"))
    assert got.dtype == np.float32 and got.shape == (NBLK, 32)
    assert idx.dtype == np.float64 and idx.tolist() == list(range(NBLK))
    # the config-2 bytes on the host: splitmix64 words, blocks 0-15 zero,
    # blocks 16-31 bytes(range(256)) repeated
    words = np.empty(NBLK * BS // 8, dtype=np.uint64)
    oracle.oracle_splitmix64_fill(words.ctypes.data, 0, words.size, bench.SEED_C2, 0, 0)
    host = words.view(np.uint8)
    host[:16 * BS] = 0
    host[16 * BS:32 * BS] = np.tile(np.arange(256, dtype=np.uint8), 16 * BS // 256)
    want = np.empty(NBLK * 32, dtype=np.uint8)
    oracle.oracle_hash_chunks(host.ctypes.data, NBLK * BS, BS, want.ctypes.data, 4)
    assert np.array_equal(got, want.reshape(NBLK, 32).astype(np.float32))


def test_full_run_checks_parity_and_times_the_valu_ceiling(gpu):
    rec = _bench(["--steps", "2", "--warmup", "1", "--full", "--no-secondary",
                  "--no-cpu-baseline"])
    assert rec["parity"] == "ok" and rec["parity_checked_blocks"] == 32
    assert rec["roofline"]["valu_ceiling_ms"] > 0
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0
