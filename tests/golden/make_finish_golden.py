#!/usr/bin/env python3
"""Generates tests/golden/finish_golden.npz: what the COMPILED REFERENCE's own mem_sort_dedup_patch_mate_sort (oracle/_ref/libbwa_pic.so, through
tests/ref_finish.py) with the compaction in front of it and the is_alt loop behind it (reference src/bwamem.cpp:1681-1719) leaves of the records
of tests/finish_gen.py's workload.  Runs in the build container (no GPU).  Data only: the reference's outputs; the inputs are regenerated from
seeds by the tests.  Prints the branch counts of the workload (the Python model's, which must reproduce the file)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "bwa-meme_amd"))
import finish_gen as FG  # noqa: E402
import ref_finish  # noqa: E402
from common import build_index  # noqa: E402
from pymeme import synth  # noqa: E402


def main(out):
    W = FG.workload()
    fa = os.path.join(tempfile.mkdtemp(prefix="fin_"), "c.fa")
    synth.write_fasta(fa, W["genome"], name="cg", contigs=3)
    ref = ref_finish.Reference(build_index(fa, bits=14), alt=(FG.ALT_CONTIG,))
    assert ref.l_pac == W["l_pac"] and ref.contigs == W["contigs"]
    regs, off, ums = ref.finish(W["regs"], W["reg_off"], W["reads"], W["read_off"])
    cols = np.stack([regs[f].astype(np.int64) for f in FG.GOLDEN_FIELDS], 1)
    np.savez_compressed(out, cols=cols, frac_rep_bits=regs["frac_rep"].view(np.uint32), reg_off=off, use_mate_sort=ums)
    m_regs, m_off, m_ums, C = FG.model(W["regs"], W["reg_off"], W["reads"], W["read_off"], W["text"], W["l_pac"], [c[2] for c in W["contigs"]])
    print("reads", off.shape[0] - 1, "records in", int((W["regs"]["qe"] > W["regs"]["qb"]).sum()), "out", regs.shape[0], "counts", C)
    print("model vs reference:", FG.same_records(m_regs, m_off, m_ums, regs, off, ums) or "same")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "finish_golden.npz"))
