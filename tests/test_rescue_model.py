"""The model of mate rescue's record updates (tests/rescue_gen.py: mem_sam_pe_batch_post in front of the primary marking, reference src/bwamem_pair.cpp:851-921 with the two
post functions) against the fixture the compiled reference wrote (tests/golden/rescue_golden.npz: every field of every record right behind rescue, the gar, the job
offsets and the results; for family A every record and SAM observable behind the reference's WHOLE mem_sam_pe_batch_post, which the chain rescue model -> primary -> pair
-> decide models has to reproduce), and, where oracle/_ref is built, against the live reference both ways: its own posing and its post functions called piecewise, and the
whole call (tests/ref_rescue.py).
The workload meets its floors, and no walk of a parity batch asks for a result gar does not hold."""
import os

import numpy as np
import pytest

import ref_py
import rescue_gen as RG


def test_model_equals_the_fixture_on_every_field_of_every_record():
    G, W, (M, _) = RG.golden(), RG.workload(), RG.modelled()
    at_k = at_r = 0
    for B, m in zip(W, M):
        k, n = m["regs"].shape[0], m["reg_off"].shape[0]
        assert np.array_equal(m["reg_off"], G["reg_off"][at_r:at_r + n]), B["name"]
        for c, f in enumerate(RG.FIELDS):
            assert np.array_equal(m["regs"][f].astype(np.int64), G["cols"][at_k:at_k + k, c]), (B["name"], f)
        for f in ("gar", "gar_off", "job_off"):
            assert np.array_equal(B[f], G["%s_%s" % (f, B["name"])]), (B["name"], f)
        assert np.array_equal(np.stack([B["res"][f] for f in RG.KSWR.names], 1), G["res_" + B["name"]]), B["name"]
        at_k += k
        at_r += n
    assert at_k == G["cols"].shape[0] and at_r == G["reg_off"].shape[0], "the fixture is not of this workload"


def test_chained_models_equal_the_whole_reference_call_of_the_fixture():
    """rescue model -> primary -> pair -> decide models on family A = every record and every observable behind mem_sam_pe_batch_post itself"""
    GW = RG.golden_whole()
    assert sorted(GW) == sorted(RG.FAMILY_A)
    for B, m in zip(RG.workload(), RG.modelled()[0]):
        if B["name"] in RG.FAMILY_A:
            obs, whole = GW[B["name"]]
            assert RG.whole_agrees(B, m, obs, whole) is None, B["name"]
            assert whole["regs"].shape[0] > B["regs"].shape[0]                   # (rescue pushed records: the call is not the decide fixture's over again)


def test_workload_meets_its_floors():
    W, (M, C) = RG.workload(), RG.modelled()
    assert RG.floors(C, W) == []
    G = RG.golden()
    assert [int(x) for x in G["counters"]] == [C[k] for k in sorted(C)]


def test_no_walk_of_the_parity_batches_asks_for_a_missing_result():
    for B in RG.workload():
        m = RG.model(B, walk_all=True)               # (lists the stage does not walk included: they must come out as they went in)
        assert not m["status"].any(), B["name"]
    assert RG.modelled()[1]["status1"] == 0


def test_lists_without_a_posed_result_are_not_walked_and_report_0():
    """posed == 0 but the reference's walk reaches a job (gar was not posed from these records): off the mate-sort path, and on it with at most one record, the stage
    reports 0 and hands the list back with flg = 0; a full walk of the same list asks for the missing result"""
    B, m = next((B, m) for B, m in zip(RG.direct(), RG.direct_modelled()) if B["name"] == "unposed")
    full = RG.model(B, walk_all_status=True)
    quiet = [r for r in B["unposed"] if m["status"][r] == 0]
    assert len(quiet) >= 3 and all(full["status"][r] == 1 for r in quiet)
    for r in quiet:
        b, e = int(B["reg_off"][r]), int(B["reg_off"][r + 1])
        want = RG.take(B["regs"], np.arange(b, e))
        want["flg"] = 0
        assert m["regs"][int(m["reg_off"][r]):int(m["reg_off"][r + 1])].tobytes() == want.tobytes()


def test_status_1_batches_hit_what_they_aim_at():
    for B, m in zip(RG.direct(), RG.direct_modelled()):
        if B["name"] != "status1":
            continue
        hit = np.nonzero(m["status"] == 1)[0]
        assert hit.size >= 3
        for r in hit:                                # the list comes back as it went in, flg included; its mate's list is walked as usual
            b, e = int(B["reg_off"][r]), int(B["reg_off"][r + 1])
            assert m["reg_off"][r + 1] - m["reg_off"][r] == e - b
            assert m["regs"][int(m["reg_off"][r]):int(m["reg_off"][r + 1])].tobytes() == RG.take(B["regs"], np.arange(b, e)).tobytes()


@pytest.mark.skipif(not os.path.exists(os.path.join(ref_py.REF_DIR, "libbwa_pic.so")), reason="the compiled reference is not built")
def test_model_equals_the_live_reference_piecewise():
    import ref_rescue
    R = ref_rescue.Reference()
    for B, m in zip(RG.workload(), RG.modelled()[0]):
        assert RG.same(m, R.run(B)) is None, B["name"]
        if B["name"] in RG.FAMILY_A:
            gar, gar_off, job_off, parts = ref_rescue.pose(B)
            assert np.array_equal(gar, B["gar"]) and np.array_equal(gar_off, B["gar_off"]) and np.array_equal(job_off, B["job_off"]), B["name"]
            assert ref_rescue.kswv(parts).tobytes() == B["res"].tobytes(), B["name"]


@pytest.mark.skipif(not os.path.exists(os.path.join(ref_py.REF_DIR, "libbwa_pic.so")), reason="the compiled reference is not built")
def test_chained_models_equal_the_live_reference_whole():
    import ref_rescue
    R = ref_rescue.Reference()
    GW = RG.golden_whole()
    for B, m in zip(RG.workload(), RG.modelled()[0]):
        if B["name"] in RG.FAMILY_A:
            obs, whole = R.run_whole(B)
            assert RG.whole_agrees(B, m, obs, whole) is None, B["name"]
            assert RG.same(whole, GW[B["name"]][1]) is None and all(np.array_equal(obs[f], GW[B["name"]][0][f]) for f in RG.DG.OBS), B["name"]
