"""The rules of record finishing (bwa-meme_amd/csrc/meme_finish_rules.h: the two orders through klib's introsort, the float redundancy test, the bars of
mem_patch_reg in double, the merge, the useMateSort scan, the identical-hit pass, the is_alt bit and the sequential driver finish_read that
meme_finish.hip runs on every lane of a wavefront) on the CPU: the header is compiled with g++ into a scalar driver (tests/finish_rules_driver.h) that
gives finish_read the header's own scalar patch score, and has to reproduce the compiled reference's records of tests/golden/finish_golden.npz on the
whole workload, the model of tests/finish_gen.py under other options and on three zero-slack merges the fixture lacks, and the score of the oracle's
bwa_gen_cigar2 -- every field, the offsets and the flag, exactly.  (The kernels are checked in tests/test_gpu_finish.py.)"""
import numpy as np
import pytest

import finish_cases as FC
import finish_gen as FG
import oracle_py as O
from common import gencig_workload
from pymeme import hipapi
from test_finish_model import OTHER


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return FC.build_driver(tmp_path_factory.mktemp("finish_rules"))


@pytest.fixture(scope="module")
def W():
    return FG.workload()


def test_driver_reproduces_the_reference_golden_on_the_whole_workload(driver, W):
    got = driver(W, W)
    assert FC.same(got, FG.golden()) is None
    assert not got["status"].any()                                         # no patch of the workload is one the reference's function rejects
    C = FC.model(W, W)[3]
    assert (got["n_patch_jobs"], got["n_patched"]) == (C["n_patch_jobs"], C["n_patched"]) == (404, 236)


@pytest.mark.parametrize("name", list(OTHER), ids=list(OTHER))
def test_driver_equals_the_model_under_other_options(driver, W, name):
    B = FC.subset(W, np.arange(W["first_real"]))
    want = FC.model(W, B, **OTHER[name])
    got = driver(W, B, **OTHER[name])
    assert FC.same(got, want) is None and not got["status"].any()
    assert (got["n_patch_jobs"], got["n_patched"]) == (want[3]["n_patch_jobs"], want[3]["n_patched"])


def test_zero_slack_merges(driver, W):
    """abutting pieces: the band is 0 with equal lengths (the gap-free shortcut), on both strands, and 2 through the DP"""
    B, expected = FC.zero_slack_batch(W)
    want = FC.model(W, B)
    got = driver(W, B)
    assert FC.same(got, want) is None
    assert got["reg_off"].tolist() == [0, 1, 2, 3] and got["n_patch_jobs"] == 3 and got["n_patched"] == 3
    assert list(zip(got["regs"]["score"].tolist(), got["regs"]["w"].tolist())) == expected
    assert (got["regs"]["n_comp_is_alt"] & 0x3fffffff).tolist() == [3, 3, 3] and (got["regs"]["qe"] - got["regs"]["qb"]).tolist() == [200, 200, 200]


def test_scalar_patch_score_equals_the_oracles_gen_cigar(driver):
    g, reads, calls = gencig_workload()
    text, l_pac = hipapi.fwd_rc_text(g), g.shape[0]
    dp = 0
    for k, J in enumerate(calls):
        rd, qb, qlen, rb, tlen, w_ = reads[int(J["read"])], int(J["qb"]), int(J["qlen"]), int(J["rb"]), int(J["tlen"]), int(J["w_"])
        want = O.gen_cigar2(text, l_pac, rd[qb:qb + qlen], rb, rb + tlen, w_)
        assert want is not None
        assert driver.score(text, l_pac, rd, qb, qb + qlen, rb, rb + tlen, w_) == (want[0], True), k
        dp += not (qlen == tlen and w_ == 0)
    assert dp > calls.shape[0] // 2
    for pen in (dict(a=2, b=3, o_del=4, e_del=2, o_ins=7, e_ins=1), dict(a=1, b=9, o_del=1, e_del=1, o_ins=1, e_ins=1)):
        for k, J in enumerate(calls[:400]):
            rd, qb, qlen, rb, tlen, w_ = reads[int(J["read"])], int(J["qb"]), int(J["qlen"]), int(J["rb"]), int(J["tlen"]), int(J["w_"])
            want = O.gen_cigar2(text, l_pac, rd[qb:qb + qlen], rb, rb + tlen, w_, **pen)
            assert driver.score(text, l_pac, rd, qb, qb + qlen, rb, rb + tlen, w_, **pen) == (want[0], True), (k, pen)


def test_calls_the_reference_rejects_are_not_posed(driver, W):
    """bwa_gen_cigar2 returns without a score for an empty span and for a target that bridges the strands or leaves the text: finish_read sets the read's status there"""
    text, L, read = W["text"], W["l_pac"], W["reads"][:200]
    for rb, re, qb, qe in ((L - 50, L + 50, 0, 100), (5000, 5000, 0, 100), (5100, 5000, 0, 100), (2 * L - 50, 2 * L + 50, 0, 100), (-10, 90, 0, 100), (5000, 5100, 50, 50),
                           (5000, 5100, 150, 250), (5000, 5100, -1, 99)):
        assert driver.score(text, L, read, qb, qe, rb, re, 10)[1] is False
    assert driver.score(text, L, read, 0, 100, L - 100, L, 10)[1] and driver.score(text, L, read, 0, 100, L, L + 100, 10)[1]
    # two records below l_pac whose patch would end beyond it
    g = W["genome"]
    B = FC.batch_of([g[L - 300:L - 100]], [[dict(rb=L - 300, re=L - 200, qb=0, qe=100, rid=2, score=100, truesc=100, w=0),
                                           dict(rb=L - 200, re=L + 100, qb=100, qe=200, rid=2, score=100, truesc=100, w=0)]])
    got = driver(W, B)
    assert got["status"].tolist() == [1] and got["n_patch_jobs"] == 1 and got["n_patched"] == 0
