"""The rules of primary marking and mapping quality (bwa-meme_amd/csrc/meme_primary_rules.h: the hash and the two orders, the float overlap test, the score
distance, what a hit does to the list member it hits, alt_sc, the remap behind the second order, the primary5 choice and the quality, which both tiers of
meme_primary.hip call) on the CPU: the header is compiled with g++ into a sequential driver (tests/primary_rules_driver.h: klib's introsort for the orders, a
scalar scan for the walk, the host libm's table of logarithms) that has to reproduce the compiled reference's records of tests/golden/primary_golden.npz on
the whole workload and the model of tests/primary_gen.py under other options, on the float boundary, on a grid of qualities and on the smallest reads --
every field, n_pri, every quality and the status, exactly.  (The kernels are checked in tests/test_gpu_primary.py.)"""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import primary_cases as PC
import primary_gen as PG
from pymeme import hipapi


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return PC.build_driver(tmp_path_factory.mktemp("primary_rules"))


@pytest.fixture(scope="module")
def W():
    return PG.workload()


def check(got, want, reg_off, status):
    """every field, n_pri and the qualities (but those of the reads whose status is set), and the status itself"""
    status = np.asarray(status, np.uint8)
    assert PG.same(got, want, reg_off, skip_mapq_of=np.nonzero(status)[0].tolist()) is None
    assert np.array_equal(got["status"], status)


def read_of(W, r):
    """read r of the workload as a batch of its own -> (regs, reg_off, ids)"""
    b, e = int(W["reg_off"][r]), int(W["reg_off"][r + 1])
    return PG.FG.take(W["regs"], np.arange(b, e)), np.array([0, e - b], np.int64), [int(W["ids"][r])]


def test_driver_reproduces_the_reference_golden_on_the_whole_workload(driver, W):
    got = driver(W["regs"], W["reg_off"], PG.ID_BASE)
    status = np.zeros(W["reg_off"].shape[0] - 1, np.uint8)
    status[W["status_read"]] = 1
    check(got, PG.golden(), W["reg_off"], status)
    # the orders are strict and total: klib's introsort leaves what the kernels' ranks by counting leave, which is what the golden holds -- and here it ran
    # once per read with records, twice where ALT and primary-assembly records mix
    C = PG.modelled()["counters"]
    assert got["orders"] == int((np.diff(W["reg_off"]) > 0).sum()) + C["n_alt_and_pri"] and C["n_alt_and_pri"] >= 500


@pytest.mark.parametrize("name", list(PG.OTHER), ids=list(PG.OTHER))
def test_driver_equals_the_model_under_other_options(driver, W, name):
    kw, id_base = PG.split_other(name)
    ids = np.arange(W["reg_off"].shape[0] - 1, dtype=np.int64) + id_base
    want = PG.model(W["regs"], W["reg_off"], ids, PG.default_opt(**kw))
    if name == "primary5":
        assert want["counters"]["n_reordered"] >= 50
    check(driver(W["regs"], W["reg_off"], id_base, **kw), want, W["reg_off"], want["status"])


@pytest.mark.parametrize("pen", [dict(a=1, b=9, o_del=4, e_del=1, o_ins=4, e_ins=1), dict(a=1, b=4, o_del=9, e_del=2, o_ins=3, e_ins=1), dict(a=1, b=4, o_del=3, e_del=1, o_ins=9, e_ins=2)],
                         ids=["mismatch", "deletion", "insertion"])
def test_each_term_of_the_score_distance_alone(driver, W, pen):
    """a + b, o_del + e_del and o_ins + e_ins each as the only largest (10 or 11 against 5 and 4): the default penalties and OTHER's tie two of them"""
    want = PG.model(W["regs"], W["reg_off"], W["ids"], PG.default_opt(**pen))
    assert not np.array_equal(want["regs"]["sub_n"], PG.modelled()["regs"]["sub_n"])           # the distance shows
    check(driver(W["regs"], W["reg_off"], PG.ID_BASE, **pen), want, W["reg_off"], want["status"])


def test_primary5_takes_the_earlier_of_two_candidates_that_start_together(driver):
    """spans that start at the same base overlap by the whole of the shorter one, so two candidates of equal qb exist only above mask_level 1: then the earlier record of
    the order is the leftmost (the reference's scan replaces its choice only for a smaller qb)"""
    regs = np.zeros(4, hipapi.ALNREG)
    for k, (qb, qe, sc) in enumerate([(0, 40, 40), (10, 90, 50), (0, 60, 45), (0, 20, 25)]):          # by score: 50 @ 10, 45 @ 0, 40 @ 0; 25 is below T
        regs[k]["qb"], regs[k]["qe"], regs[k]["rb"], regs[k]["re"], regs[k]["score"], regs[k]["c"] = qb, qe, 1000, 1000 + qe - qb, sc, k
    off = np.array([0, 4])
    kw = dict(mask_level=1.5, primary5=1)
    want = PG.model(regs, off, [5], PG.default_opt(**kw))
    assert want["counters"]["n_reordered"] == 1 and want["regs"]["c"].tolist() == [2, 1, 0, 3]
    check(driver(regs, off, 5, **kw), want, off, want["status"])


def test_float_boundary_of_the_overlap_test(driver):
    """the two records of test_primary_model.py's test of the same name: 3 of 10 bases are a significant overlap at mask_level 0.3 in float, not at 0.31"""
    regs = np.zeros(2, hipapi.ALNREG)
    for k, (qb, qe, sc) in enumerate([(0, 10, 50), (7, 40, 40)]):
        regs[k]["qb"], regs[k]["qe"], regs[k]["rb"], regs[k]["re"], regs[k]["score"] = qb, qe, 1000, 1000 + qe - qb, sc
    off = np.array([0, 2])
    for mask_level, secondary in ((0.3, [-1, 0]), (0.31, [-1, -1])):
        want = PG.model(regs, off, [5], PG.default_opt(mask_level=mask_level))
        got = driver(regs, off, 5, mask_level=mask_level)
        check(got, want, off, want["status"])
        assert got["regs"]["secondary"].tolist() == secondary


def test_quality_of_every_record_of_the_modelled_workload(driver, W):
    M = PG.modelled()
    regs, off = M["regs"], W["reg_off"]
    q, beyond = np.zeros(regs.shape[0], np.int64), np.zeros(regs.shape[0], bool)
    for k in range(regs.shape[0]):
        q[k], beyond[k] = driver.mapq(regs[k:k + 1])
    reads = np.searchsorted(off, np.nonzero(beyond)[0], "right") - 1
    assert sorted(set(reads.tolist())) == np.nonzero(M["status"])[0].tolist() == [W["status_read"]]
    assert q.min() >= 0 and q.max() <= 60
    assert np.array_equal(q[~beyond], M["mapq"][~beyond])


def test_quality_on_a_grid_the_workload_does_not_hold(driver):
    """lengths on both sides of mapQ_coef_len and at the table's last entry, with sub_n up to the table's last entry; beyond the table only the flag means anything"""
    o = PG.default_opt()
    n = n_beyond = 0
    for l, score_of, sub_n, frac in itertools.product((49, 50, 51, 65535, 65536), (0, 1, None), (0, 1, 65533, 65534, 65535), (0.0, 0.5)):
        score = l if score_of is None else score_of
        for on_ref in (False, True):                                     # the length from the query span, from the reference span
            qe, re = (10, 1000 + l) if on_ref else (l, 1000 + 10)
            reg = np.zeros(1, hipapi.ALNREG)
            reg["qe"], reg["rb"], reg["re"], reg["score"], reg["sub_n"], reg["frac_rep"] = qe, 1000, re, score, sub_n, frac
            p = SimpleNamespace(qb=0, qe=qe, rb=1000, re=re, score=score, sub=0, csub=0, sub_n=sub_n, frac_rep=frac)
            sub = max(o["min_seed_len"] * o["a"], p.csub)
            want_beyond = bool(sub < score and ((not PG.F32(l) < PG.F32(o["mapQ_coef_len"]) and l >= PG.LOG_TABLE) or (sub_n > 0 and sub_n + 1 >= PG.LOG_TABLE)))      # the condition of PG.model's status
            q, beyond = driver.mapq(reg)
            assert beyond == want_beyond, (l, score, sub_n, frac)
            if not beyond:
                assert q == PG.mapq_se(o, p), (l, score, sub_n, frac)
            n += 1
            n_beyond += beyond
    assert n == 300 and 0 < n_beyond < n // 2


def test_smallest_reads_one_per_call(driver, W):
    """reads of 0, 1 and 2 records, a read whose records are all ALT (n_pri 0, no second order) and one that mixes ALT and primary-assembly records (two orders)"""
    n = np.diff(W["reg_off"])
    alt = np.concatenate([[0], np.cumsum((W["regs"]["n_comp_is_alt"] >> 30) & 3 != 0)])
    n_alt = alt[W["reg_off"][1:]] - alt[W["reg_off"][:-1]]
    picks = {"0": np.nonzero(n == 0)[0], "1": np.nonzero(n == 1)[0], "2": np.nonzero(n == 2)[0], "all ALT": np.nonzero((n >= 3) & (n_alt == n))[0],
             "mixed": np.nonzero((n >= 3) & (n_alt > 0) & (n_alt < n))[0]}
    for what, reads in picks.items():
        assert reads.shape[0] >= 3, what
        for r in reads[:3]:
            regs, off, ids = read_of(W, int(r))
            want = PG.model(regs, off, ids)
            got = driver(regs, off, ids[0])
            check(got, want, off, want["status"])
            assert got["orders"] == int(n[r] > 0) + int(0 < n_alt[r] < n[r]), what            # one order per read with records, a second where the two kinds mix
            assert got["orders"] == {"0": 0, "1": 1, "all ALT": 1, "mixed": 2}.get(what, got["orders"]), what
            if what == "all ALT":
                assert got["n_pri"].tolist() == [0] and (got["regs"]["secondary"][got["regs"]["secondary"] >= 0] == PG.INT_MAX).all()
