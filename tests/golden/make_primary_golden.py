"""Writes tests/golden/primary_golden.npz: what the COMPILED REFERENCE's mem_mark_primary_se and mem_approx_mapq_se (tests/ref_primary.py) leave
for the workload of tests/primary_gen.py under default options, read r with id ID_BASE + r.  Outputs only: per record of the final order its
index in the workload (`src`), the fields the functions write, the quality; per read n_pri.  The tests regenerate the inputs.

The reference is compiled -O3 at the build host's SIMD level, so whether its `x * y + .499` is one fused multiply-add depends on the box that
built it.  The model therefore evaluates every quality both ways and this script refuses a workload on which the two differ anywhere: the
fixture then holds on every box.  (A record that fails: change that synthetic input in primary_gen._synthetic, do not drop it.)

Run from the repository root with oracle/_ref built:  python tests/golden/make_primary_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "bwa-meme_amd")]

import primary_gen as PG      # noqa: E402
import ref_primary            # noqa: E402


def main():
    W = PG.workload()
    M = PG.modelled()
    C = M["counters"]
    for k in sorted(C):
        print("%-16s %d" % (k, C[k]))
    n = np.diff(W["reg_off"])
    print("reads %d (fixture %d), records %d, most per read %d" % (n.shape[0], W["n_fixture"], W["regs"].shape[0], n.max()))
    assert C["n_fma_differs"] == 0, "%d qualities depend on whether x * y + .499 is fused" % C["n_fma_differs"]
    missed = PG.floors(C, W["reg_off"])
    assert not missed, missed
    R = ref_primary.Reference().run(W["regs"], W["reg_off"], W["ids"])
    assert R["mapq"].min() >= 0 and R["mapq"].max() <= 60
    got = {"regs": R["regs"], "n_pri": R["n_pri"], "mapq": R["mapq"].astype(np.uint8)}
    diff = PG.same(M, got, W["reg_off"])
    assert diff is None, "model and compiled reference disagree: " + diff
    # src: the record's index in the workload (`c` of the synthetic records and the position of the fixture's are distinct per read; matched through the model, which equals the reference)
    src = np.zeros(W["regs"].shape[0], np.int64)
    for r in range(n.shape[0]):
        b, e = int(W["reg_off"][r]), int(W["reg_off"][r + 1])
        h = {PG.hash_64(int(W["ids"][r]) + i): b + i for i in range(e - b)}
        src[b:e] = [h[int(x)] for x in R["regs"]["hash"][b:e]]
    cols = np.stack([R["regs"][f].astype(np.int32) for f in PG.OUT_FIELDS[:-1]], axis=1)
    out = os.path.join(HERE, "primary_golden.npz")
    np.savez_compressed(out, src=src.astype(np.int32), cols=cols, hash=R["regs"]["hash"], n_pri=R["n_pri"], mapq=got["mapq"])
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))
    assert PG.same(PG.golden(), got, W["reg_off"]) is None


if __name__ == "__main__":
    main()
