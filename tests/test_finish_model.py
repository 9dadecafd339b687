"""Model and fixture of record finishing (CPU only): tests/finish_gen.py's plain-Python restatement of the tail of mem_kernel2_core
(reference src/bwamem.cpp:1681-1719: compaction, mem_sort_dedup_patch_mate_sort, is_alt) reproduces what the compiled reference left in
tests/golden/finish_golden.npz on the whole workload -- every field, the offsets and the useMateSort flag, exactly --, the workload takes
every branch often enough to mean something, and where the compiled reference is at hand the model equals it under other options too."""
import os
import tempfile

import numpy as np
import pytest

import finish_gen as FG
import ref_py
from pymeme import hipapi, synth


@pytest.fixture(scope="module")
def modelled():
    W = FG.workload()
    return W, FG.model(W["regs"], W["reg_off"], W["reads"], W["read_off"], W["text"], W["l_pac"], [c[2] for c in W["contigs"]])


def test_model_reproduces_the_reference_golden(modelled):
    W, (regs, off, ums, _) = modelled
    assert FG.same_records(regs, off, ums, *FG.golden()) is None


def test_workload_takes_every_branch(modelled):
    """the floors the workload was built to meet, counted by the model that reproduces the reference on it"""
    W, (regs, off, ums, C) = modelled
    print(C)
    assert C["n_redundant"] >= 50 and C["n_patch_jobs"] >= 50 and C["n_patched"] >= 50 and C["n_ratio_rejected"] >= 50 and C["n_identical"] >= 50
    assert C["n_ums0"] >= 20 and int((ums == 0).sum()) == C["n_ums0"] and C["n_above_17"] >= 10
    assert C["n_rounds_max"] >= 2                                         # a -> b -> c: a read asks for a second alignment after its first merge
    live = np.diff(np.concatenate([[0], np.cumsum(W["regs"]["qe"] > W["regs"]["qb"])])[W["reg_off"]])
    assert set(FG.SORT_COUNTS) <= set(live.tolist())
    assert (regs["n_comp_is_alt"] >> 30 != 0).any() and (regs["n_comp_is_alt"] & 0x3fffffff > 2).any()      # is_alt set; n_comp accumulated over a chain of merges
    lone = np.nonzero(np.diff(off) == 1)[0]
    assert ((regs["n_comp_is_alt"][off[lone]] & 0x3fffffff) == 0).any()    # the early return: a lone record keeps n_comp == 0


def test_float_boundary_of_the_redundancy_test():
    """0.95f * 100 is exactly 95.0f: an overlap of 95 of 100 bases is NOT redundant in the reference's float arithmetic (in double it would be)"""
    assert not np.float32(95) > np.float32(0.95) * np.float32(100) and 95 > 0.95 * 100 - 1e-9
    regs = np.zeros(2, hipapi.ALNREG)
    for k, (rb, re, qb, qe, sc) in enumerate([(1000, 1100, 0, 60, 50), (1005, 1105, 1, 61, 40)]):
        regs[k]["rb"], regs[k]["re"], regs[k]["qb"], regs[k]["qe"], regs[k]["score"], regs[k]["w"] = rb, re, qb, qe, sc, 100
    text = np.zeros(8000, np.uint8)
    args = (np.array([0, 2]), np.zeros(100, np.uint8), np.array([0, 100]), text, 4000, [0])
    assert FG.model(regs, *args)[1][1] == 2                               # overlap 95: both stay
    regs[1]["rb"], regs[1]["re"] = 1004, 1104
    assert FG.model(regs, *args)[1][1] == 1                               # overlap 96: the lower score goes


OTHER = {"mask-0.5": dict(mask_level_redun=0.5), "gap-100": dict(max_chain_gap=100), "w-10": dict(w=10), "w-40": dict(w=40), "penalties": dict(a=2, b=3, o_del=4, e_del=2, o_ins=5, e_ins=1)}


@pytest.mark.skipif(not (ref_py.have("libstage_ref.so") and ref_py.have("libbwa_pic.so") and ref_py.cpu_can_run()), reason="compiled reference (oracle/_ref) not available on this box")
@pytest.mark.parametrize("name", list(OTHER), ids=list(OTHER))
def test_model_equals_the_compiled_reference_under_other_options(name):
    """the model as the oracle for options the fixture does not cover: the synthetic parts of the workload through the reference's own function"""
    import ref_finish
    from common import build_index
    W = FG.workload()
    fa = os.path.join(tempfile.mkdtemp(prefix="fin_"), "c.fa")
    synth.write_fasta(fa, W["genome"], name="cg", contigs=3)
    ref = ref_finish.Reference(build_index(fa, bits=14), alt=(FG.ALT_CONTIG,), **OTHER[name])
    n = W["first_real"]
    regs, reg_off, read_off = FG.take(W["regs"], np.arange(W["reg_off"][n])), W["reg_off"][:n + 1], W["read_off"][:n + 1]
    want = ref.finish(regs, reg_off, W["reads"], read_off)
    got = FG.model(regs, reg_off, W["reads"], read_off, W["text"], W["l_pac"], [c[2] for c in W["contigs"]], FG.default_opt(**OTHER[name]))
    assert got[3]["n_patch_jobs"] > 20 and got[3]["n_redundant"] > 20
    assert FG.same_records(got[0], got[1], got[2], *want) is None
