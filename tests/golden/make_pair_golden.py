"""Writes tests/golden/pair_golden.npz: what the COMPILED REFERENCE's mem_pair (tests/ref_pair.py) returns for every pair of the workload of
tests/pair_gen.py under default options -- score (the return value), sub, n_sub and z, the batches one after the other.  Outputs only: the tests
regenerate the inputs.

A candidate's q is (int)(scores + .721 * log(2 erfc(...)) * a + .499): the logarithm and erfc are the build host's libm, and the reference is compiled
-O3 at the build host's SIMD level, so whether `x * a + s` is one fused multiply-add depends on the box that built it.  The model therefore evaluates
every q again with the penalty moved by 8 ulp either way and with the multiply-add fused, and this script refuses a workload on which any of that changes
a q: the fixture then holds on any box's libm and at any SIMD level.  (A pair that fails: change that synthetic input in pair_gen, do not drop it.)

Run from the repository root with oracle/_ref built:  python tests/golden/make_pair_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "bwa-meme_amd")]

import pair_gen as QG         # noqa: E402
import ref_pair               # noqa: E402


def main():
    W = QG.workload()
    M, C = QG.modelled()
    for k in sorted(C):
        print("%-16s %d" % (k, C[k]))
    print("batches %d, pairs %d, records %d" % (len(W), sum((B["reg_off"].shape[0] - 1) // 2 for B in W), sum(B["regs"].shape[0] for B in W)))
    assert C["n_unstable"] == 0, "%d candidates' q depend on the last bits of the penalty or on whether x * a + s is fused" % C["n_unstable"]
    missed = QG.floors(C, W)
    assert not missed, missed
    R = ref_pair.Reference(QG.CONTIGS, QG.L_PAC)
    got = []
    for B, m in zip(W, M):
        r = R.run(B)
        diff = QG.same(m, r)
        assert diff is None, "model and compiled reference disagree in batch %s: %s" % (B["name"], diff)
        got.append(r)
    out = os.path.join(HERE, "pair_golden.npz")
    np.savez_compressed(out, **{f: np.concatenate([r[f] for r in got]).astype(np.int32) for f in QG.RESULT})
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))
    for g, r in zip(QG.golden(), got):
        assert QG.same(g, r) is None


if __name__ == "__main__":
    main()
