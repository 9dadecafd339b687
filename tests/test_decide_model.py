"""Model and fixture of the pairing decision (CPU only): tests/decide_gen.py's plain-Python restatement of what mem_sam_pe does behind mem_pair (reference
src/bwamem_pair.cpp:536-590, :632-648), behind the models of primary marking and pair scoring, reproduces what the compiled reference's mem_sam_pe left in
tests/golden/decide_golden.npz on the whole workload -- sub, secondary and secondary_all of every record, and per end the SAM lines, the first line's FLAG, MAPQ and record
and the record its mate fields name --, the workload takes every branch often enough to mean something, and where the compiled reference is at hand the model equals it
live, on every field of every record."""
import os

import numpy as np
import pytest

import decide_gen as DG
import ref_py
from pymeme import hipapi


def test_model_reproduces_the_reference_golden():
    W, (M, _), G = DG.workload(), DG.modelled(), DG.golden()
    assert len(W) == len(M) == len(G)
    for B, m, (obs, marks) in zip(W, M, G):
        assert DG.observables_agree(B, m, obs, marks) is None, B["name"]
        d = m["decide"]
        assert not d["status"].any(), B["name"]                        # (outside direct() no pair has a status)
        # what the outputs have to satisfy among themselves
        paired = d["path"] >= 2
        assert (d["q_se"][~paired] == 0).all() and (d["q_pe"][~paired] == 0).all() and (d["alt"][~paired] == -1).all()
        assert ((d["flag"] == 1) | (d["flag"] == 3)).all() and (d["flag"][d["path"] == 3] == 3).all() and (d["flag"][d["path"] == 2] == 1).all()
        assert (d["sel"][d["path"] == 2] == 0).all() and (d["sel"][paired] >= 0).all() and (0 <= d["q_pe"]).all() and (d["q_pe"] <= 60).all()
        changed = [f for f in hipapi.ALNREG.names if not np.array_equal(d["regs"][f], m["primary"]["regs"][f])]
        assert set(changed) <= set(DG.MARKS), changed


def test_workload_takes_every_branch():
    """the floors the workload was built to meet, counted by the model that reproduces the reference on it; the third way an ALT record is rejected (its is_alt bit) is
    beyond what the primary step leaves and lives in direct()"""
    W, (_, C) = DG.workload(), DG.modelled()
    print(C)
    assert DG.floors(C, W) == []
    sizes = [(B["reg_off"].shape[0] - 1) // 2 for B in W]
    assert min(sizes) == 1 and 200 <= max(sizes) <= 400
    C2 = DG.counters()
    for D in DG.direct():
        DG.decide(D["regs"], D["reg_off"], D["n_pri"], D["pair"], D["pes"], DG.default_opt(**D["opt"]), C2)
    assert C2["alt_not_alt"] >= 5 and C2["status1"] == 3
    S = DG.direct_modelled()[0]
    assert np.nonzero(S["status"])[0].tolist() == DG.direct()[0]["expect_status1"]


def test_the_float_sum_of_frac_rep_decides_some_q_pe():
    assert DG.modelled()[1]["frac_float"] >= 3


def test_a_pair_by_hand():
    """FR at the mean distance: the penalty is .721 log 2 and o the sum of the scores, 17 above score_un: q_pe 60 (6.02 x 17 clamped), both q_se from mem_approx_mapq_se
    (60) against it, the flag 3; 600 bases further out o falls below score_un and the unpaired alignment is preferred"""
    near = DG.chain(DG._batch("hand", [[[DG.rec(0, 3000, 0, 100)], [DG.rec(0, 3350, 1, 90)]]], DG.PES, 11))
    d = near["decide"]
    assert near["pair"]["score"][0] == 190 and (d["path"][0], d["q_pe"][0], d["flag"][0]) == (3, 60, 3) and d["sel"][0].tolist() == [0, 0] and d["q_se"][0].tolist() == [60, 60]
    far = DG.chain(DG._batch("hand", [[[DG.rec(0, 3000, 0, 100)], [DG.rec(0, 3850, 1, 90)]]], DG.PES, 11))
    d = far["decide"]
    assert 0 < far["pair"]["score"][0] <= 173 and (d["path"][0], d["q_pe"][0], d["flag"][0]) == (2, 0, 1) and d["q_se"][0].tolist() == [60, 60]


@pytest.mark.skipif(not os.path.exists(os.path.join(ref_py.REF_DIR, "libbwa_pic.so")), reason="the compiled reference is not built here")
def test_model_equals_the_live_reference():
    import ref_decide
    for B, m in zip(DG.workload(), DG.modelled()[0]):
        R = ref_decide.Reference(no_pairing=B["opt"].get("no_pairing", 0), **{k: v for k, v in B["opt"].items() if k != "no_pairing"})
        obs, regs = R.run(B)
        assert DG.observables_agree(B, m, obs, regs) is None, B["name"]
        for f in hipapi.ALNREG.names:
            if not f.startswith("pad") and f != "c":
                assert np.array_equal(regs[f], m["decide"]["regs"][f]), (B["name"], f)
