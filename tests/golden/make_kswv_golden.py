#!/usr/bin/env python3
"""Generates tests/golden/kswv_golden.npz: the kswr_t records (score, te, qe, score2, te2, tb, qb) the COMPILED REFERENCE's mate-rescue batch
(sort_classify + mem_sam_pe_batch with the AVX-512 kswv kernels, src/bwamem.cpp:1798-1825, src/bwamem_pair.cpp:719-818, src/kswv.cpp, through
oracle/_ref/libstage_ref.so) gives for the jobs of tests/common.py kswv_workload(), under the scoring parameters of KSWV_GOLDEN_SETS: three general
sets and three whose int8 lanes saturate.  Runs in the build container (no GPU).  Data only: the reference's outputs; the inputs are regenerated
from seeds by the tests.

The reference leaves score2 / te2 unwritten for a 64-lane vector in which EVERY job saturates (getScores8 returns at live == 0, src/kswv.cpp:607,
before it writes them).  The generator refuses to record such a vector: every saturated record must carry score2 == te2 == -1."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "bwa-meme_amd"))
import ref_py  # noqa: E402
from common import KSWV_GOLDEN_SETS, KSWV_SAT_SETS, kswv_workload  # noqa: E402

SCORE, TE, QE, SCORE2, TE2, TB, QB = range(7)


def main(out):
    committed = os.path.join(HERE, "kswv_golden.npz")
    old = dict(np.load(committed)) if os.path.exists(committed) else {}
    data = {}
    for name, kw, pen in KSWV_GOLDEN_SETS:
        jobs, ref, qer = kswv_workload(**kw)
        r = ref_py.kswv_batch(jobs, ref, qer, **pen)
        data[name] = r.view(np.int32).reshape(-1, 7)
        sat = data[name][data[name][:, SCORE] == 255]
        print(name, "jobs", r.shape[0], "int8 class", int(((jobs["xtra"] & 0x10000) != 0).sum()), "with start", int((r["tb"] >= 0).sum()), "with a second-best score",
              int((r["score2"] > 0).sum()), "saturated", sat.shape[0])
        if name in KSWV_SAT_SETS:
            assert ((jobs["xtra"] & 0x10000) != 0).all(), (name, "holds int16 jobs: a score of 255 would not mean saturation")
            assert sat.shape[0] >= 200, (name, "saturated records", sat.shape[0])
            assert (sat[:, SCORE2] == -1).all() and (sat[:, TE2] == -1).all(), (name, "a reference vector was all-saturated: score2 / te2 are not defined")
            assert (sat[:, TB] == -1).all() and (sat[:, QB] == -1).all(), (name, "a saturated record with a start")
        else:
            assert name in old and np.array_equal(old[name], data[name]), (name, "differs from the committed array")
    np.savez_compressed(out, **data)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "kswv_golden.npz"))
