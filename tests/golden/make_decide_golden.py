"""Writes tests/golden/decide_golden.npz: what the COMPILED REFERENCE's mem_sam_pe (tests/ref_decide.py: MEM_F_NO_RESCUE | MEM_F_ALL) shows for every pair of the
workload of tests/decide_gen.py -- per record sub, secondary and secondary_all behind the call; per read the number of SAM lines, FLAG and MAPQ of the first,
the record it reports and the record its mate fields (RNEXT, PNEXT, the mate-strand bit) point to, which on the no-pairing paths is `which` of the other end.
Outputs only: the tests regenerate the inputs.  path and q_pe are not observable; the model supplies them.

The script refuses to write unless the model (tests/decide_gen.py: chain) agrees with the reference on every observable and on EVERY field of every record,
and unless the workload meets its floors.

Run from the repository root with oracle/_ref built:  python tests/golden/make_decide_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "bwa-meme_amd")]

import decide_gen as DG       # noqa: E402
import ref_decide             # noqa: E402
from pymeme import hipapi     # noqa: E402

REF_FIELDS = {"a": "a", "b": "b", "pen_unpaired": "pen_unpaired", "T": "T"}


def reference_of(B):
    return ref_decide.Reference(no_pairing=B["opt"].get("no_pairing", 0), **{REF_FIELDS[k]: v for k, v in B["opt"].items() if k in REF_FIELDS})


def main():
    W = DG.workload()
    M, C = DG.modelled()
    for k in sorted(C):
        print("%-16s %d" % (k, C[k]))
    print("batches %d, pairs %d, records %d" % (len(W), sum((B["reg_off"].shape[0] - 1) // 2 for B in W), sum(B["regs"].shape[0] for B in W)))
    missed = DG.floors(C, W)
    assert not missed, missed
    obs, marks = [], []
    for B, m in zip(W, M):
        assert not m["decide"]["status"].any(), B["name"]
        o, regs = reference_of(B).run(B)
        diff = DG.observables_agree(B, m, o, regs)
        assert diff is None, "model and compiled reference disagree in batch %s: %s" % (B["name"], diff)
        for f in hipapi.ALNREG.names:
            if not f.startswith("pad") and f != "c":
                assert np.array_equal(regs[f], m["decide"]["regs"][f]), "batch %s: field %s of the records differs from the reference's" % (B["name"], f)
        obs.append(o)
        marks.append(regs)
    print("model vs reference: same")
    out = os.path.join(HERE, "decide_golden.npz")
    data = {f: np.concatenate([o[f] for o in obs]).astype(np.int32) for f in DG.OBS}
    data.update({f: np.concatenate([r[f] for r in marks]).astype(np.int32) for f in DG.MARKS})
    np.savez_compressed(out, **data)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
