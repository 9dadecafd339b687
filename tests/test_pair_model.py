"""Model and fixture of pair scoring (CPU only): tests/pair_gen.py's plain-Python restatement of mem_pair (reference src/bwamem_pair.cpp:372-433)
reproduces what the compiled reference left in tests/golden/pair_golden.npz on the whole workload -- score, sub, n_sub and z of every pair, exactly --,
the workload takes every branch often enough to mean something, no q of it depends on the last bits of the host libm's log and erfc or on whether a
compiler fuses `x * a + s`, and where the compiled reference is at hand the model equals it under other options too."""
import ctypes

import numpy as np
import pytest

import pair_gen as QG
import ref_py
from pymeme import hipapi


def test_model_reproduces_the_reference_golden():
    W, (M, _), G = QG.workload(), QG.modelled(), QG.golden()
    assert len(W) == len(M) == len(G)
    for B, m, g in zip(W, M, G):
        assert QG.same(m, g) is None, B["name"]
        assert not m["status"].any()
        # what the outputs have to satisfy among themselves
        assert ((m["n_cand"] == 0) == (m["z"][:, 0] < 0)).all() and ((m["z"][:, 0] < 0) == (m["z"][:, 1] < 0)).all()
        assert (m["sub"] <= m["score"]).all() and (m["n_sub"] <= np.maximum(m["n_cand"] - 1, 0)).all() and ((m["n_cand"] > 1) | (m["sub"] == 0)).all()
        n0, n1 = B["n_pri"][0::2], B["n_pri"][1::2]
        assert (m["z"][:, 0] < n0).all() and (m["z"][:, 1] < n1).all()


def test_workload_takes_every_branch():
    """the floors the workload was built to meet, counted by the model that reproduces the reference on it"""
    W, (_, C) = QG.workload(), QG.modelled()
    print(C)
    assert QG.floors(C, W) == []
    assert 1400 <= sum((B["reg_off"].shape[0] - 1) // 2 for B in W) <= 3200


def test_no_q_depends_on_the_libm_or_on_contraction():
    """8 ulp either way on the penalty, `x * a + s` as one fused multiply-add: no candidate's q of the workload changes, so the fixture holds on every box"""
    assert QG.modelled()[1]["n_unstable"] == 0


def test_two_candidates_of_equal_q_and_equal_hash_word_exist():
    """the two pairs built for it: best and second have the same x, and (k, i) orders them"""
    W, (M, C) = QG.workload(), QG.modelled()
    assert C["n_tie_hash"] == len(QG.EQUAL_HASH) == 2
    for B, m in zip(W, M):
        if B["name"].startswith("equal-hash-"):
            pair_id = int(B["name"].split("-")[-1])
            p = pair_id - B["id_base"]
            (k1, i1), (k2, i2) = QG.EQUAL_HASH[pair_id]
            y1, y2 = k1 << 32 | i1, k2 << 32 | i2
            assert QG.PG.hash_64(y1 ^ QG.idx_of(pair_id)) & 0xffffffff == QG.PG.hash_64(y2 ^ QG.idx_of(pair_id)) & 0xffffffff
            assert m["n_cand"][p] == 2 and m["score"][p] == m["sub"][p] == 130 and m["n_sub"][p] == 1


def test_a_single_pair_by_hand():
    """FR at the mean distance: the penalty is .721 log 2 and q the sum of the scores; a second mate 7 below is counted in n_sub, one 8 below is not"""
    for third, n_sub in ((43, 3), (42, 2)):                   # (the second itself and its equal are within tmp of sub)
        B = QG._batch("hand", [[[QG.rec(0, 3000, 0, 50)], [QG.rec(0, 3350, 1, 60), QG.rec(0, 3350, 1, 50), QG.rec(0, 3350, 1, third), QG.rec(0, 3350, 1, 50)]]], QG.PES, 11)
        m = QG.model(B)
        assert (m["score"][0], m["sub"][0], m["n_sub"][0], m["n_cand"][0]) == (110, 100, n_sub, 4) and m["z"][0].tolist() == [0, 0]


def test_structures_have_their_sizes():
    assert ctypes.sizeof(hipapi.PairPes) == 32 and ctypes.sizeof(hipapi.PairOpt) == 24 and ctypes.sizeof(hipapi.PairHost) == 72 and ctypes.sizeof(hipapi.PairDeviceOut) == 56
    assert hipapi.PairPes.avg.offset == 16 and hipapi.PairHost.n_heavy.offset == 56 and hipapi.PairHost.kernel_ms.offset == 64
    o, d = hipapi.default_pair_opt(), QG.default_opt()
    assert all(getattr(o, k) == d[k] for k in d)
    assert QG.CONTIGS == QG.PG.FG.workload()["contigs"] and QG.L_PAC == QG.PG.FG.workload()["l_pac"]


@pytest.mark.skipif(not (ref_py.have("libstage_ref.so") and ref_py.have("libbwa_pic.so") and ref_py.cpu_can_run()), reason="compiled reference (oracle/_ref) not available on this box")
@pytest.mark.parametrize("name", list(QG.OTHER), ids=list(QG.OTHER))
def test_model_equals_the_compiled_reference_under_other_options(name):
    import ref_pair
    kw = QG.OTHER[name]
    R = ref_pair.Reference(QG.CONTIGS, QG.L_PAC, **kw)
    C = QG.counters()
    differs = False
    for B, base in zip(QG.workload(), QG.modelled()[0]):
        got = QG.model(B, QG.default_opt(**kw), check=True, C=C)
        assert QG.same(got, R.run(B)) is None, B["name"]
        differs = differs or QG.same(got, base) is not None
    assert C["n_unstable"] == 0                          # (else the comparison above would depend on the box that built the reference)
    assert differs                                       # the options show
