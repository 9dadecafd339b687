"""bench.py samples its batch on host threads (sample_reads): the reads must be workload.make_reads_fast's, byte for byte -- they are the
benchmark's input, and runs of two builds are compared output for output on them.  In a child process: importing bench.py sets
GPU_MAX_HW_QUEUES for the process that imports it."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench
from pymeme import synth, workload
g = synth.make_genome(3000000, seed=11)
for n, seed, chunk in ((70000, 1000, 1 << 14), (5000, 7, 1 << 20), (1, 3, 1 << 20)):
    a = bench.sample_reads(g, n, 150, seed, chunk=chunk)
    b = workload.make_reads_fast(g, n, 150, seed, chunk=chunk)
    assert np.array_equal(a, b), (n, seed, chunk)
print("ok")
"""


def test_threaded_sampler_equals_make_reads_fast():
    r = subprocess.run([sys.executable, "-c", CODE, REPO], capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]
