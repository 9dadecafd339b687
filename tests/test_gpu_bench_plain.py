"""A plain bench.py run (no --full: the headline only) at a small size: --steps sets the number of timed steps, the line holds ms_per_step,
and --dump-outputs writes what the last step computed as float .npy files, at most 64 MB in all, which a second run with the same
arguments reproduces value for value."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps):
    env = dict(os.environ, MEME_BENCH_MBP="64", MEME_BENCH_READS="200000")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, env=env, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(tmp_path):
    runs = [(tmp_path / "a", 3), (tmp_path / "b", 2)]
    lines = [_run(d, steps) for d, steps in runs]
    for (d, steps), line in zip(runs, lines):
        assert line["metric"] == "seeding_reads_per_sec" and line["unit"] == "reads/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
        assert line["steps"] == steps and line["ms_per_step"] > 0
        assert abs(line["value"] - 200000 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-6
        assert "roofline" not in line and "cpu_baseline" not in line and "e2e" not in line          # the extras are --full's
    names = sorted(os.listdir(runs[0][0]))
    assert names == sorted(os.listdir(runs[1][0])) and "seed_smems.npy" in names and "seed_hits.npy" in names
    total = 0
    for name in names:
        x, y = np.load(runs[0][0] / name), np.load(runs[1][0] / name)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
        total += os.path.getsize(runs[0][0] / name)
    assert total <= 64 << 20
    smems, counts = np.load(runs[0][0] / "seed_smems.npy"), np.load(runs[0][0] / "seed_smem_count.npy")
    assert smems.shape == (counts.sum(), 5) and counts.sum() > 0
    assert np.load(runs[0][0] / "seed_hits.npy").shape[0] == smems[:, 3].sum()
