"""The rules of pair scoring (bwa-meme_amd/csrc/meme_pair_rules.h: the key and the order of the keys, the candidate test as a predicate, the score from
the host's penalty table, the candidate's key, the top two and what n_sub counts, which both tiers of meme_pair.hip call) on the CPU: the header is
compiled with g++ into a sequential driver (tests/pair_rules_driver.h: klib's introsort for the order, every k < i put to the predicate) that has to
reproduce the compiled reference's outputs of tests/golden/pair_golden.npz on the whole workload and the model of tests/pair_gen.py -- the reference's
backward loop with its break and its y[] array, restated literally -- under other options, with n_cand, exactly.  That is where "the predicate equals
the loop" is tested.  The same driver as a program of its own (scripts/pair_rules_main.cpp) is built with -fsanitize=address,undefined and run over the
whole workload.  (The kernels are checked in tests/test_gpu_pair.py.)"""
import subprocess

import numpy as np
import pytest

import pair_cases as QC
import pair_gen as QG

ALL = QG.RESULT + ("n_cand", "status")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return QC.build_driver(tmp_path_factory.mktemp("pair_rules"))


@pytest.mark.parametrize("exhaustive", [False, True], ids=["reach", "every-k"])
def test_driver_reproduces_the_reference_golden_on_the_whole_workload(driver, exhaustive):
    """every-k: the predicate alone decides, over all k < i -- equal to the loop with its break; reach: stopping the walk where the distance exceeds every live high loses nothing"""
    for B, g, m in zip(QG.workload(), QG.golden(), QG.modelled()[0]):
        got = driver(B, exhaustive=exhaustive)
        assert QG.same(got, g) is None, B["name"]
        assert QG.same(got, m, ALL) is None, B["name"]


@pytest.mark.parametrize("name", list(QG.OTHER), ids=list(QG.OTHER))
def test_driver_equals_the_model_under_other_options(driver, name):
    kw = QG.OTHER[name]
    for B in QG.workload():
        assert QG.same(driver(B, **kw), QG.model(B, QG.default_opt(**kw)), ALL) is None, B["name"]


def test_predicate_equals_the_loop_on_dense_random_pairs(driver):
    """keys packed into a few hundred bases on both strands of two contigs, narrow and wide orientations, some failed: many keys of every `which` between a key and its candidates"""
    rng = np.random.default_rng(5)
    n_cand = 0
    for it in range(40):
        pes = [(int(lo), int(lo + w), int(rng.random() < 0.25), float(lo + w / 2), float(rng.choice([1.0, 20.0, 200.0]))) for lo, w in zip(rng.integers(0, 60, 4), rng.integers(0, 250, 4))]
        pairs = [QG._random_pair(rng, int(rng.integers(4, 21)), int(rng.integers(4, 21)), int(rng.choice([30, 150])), rids=(0, 1) if it % 3 == 0 else (0,)) for _ in range(12)]
        B = QG._batch("dense", pairs, pes, int(rng.integers(0, 1 << 33)))
        want = QG.model(B)
        for exhaustive in (False, True):
            assert QG.same(driver(B, exhaustive=exhaustive), want, ALL) is None
        n_cand += int(want["n_cand"].sum())
    assert n_cand > 5000                                 # (480 pairs of about 12 x 12 keys of different ends: some 70 000 tests, of which a few in ten are in range)


def test_status_and_refusals(driver):
    W = QG.workload()
    B = dict(QG.piece(W[-1], 0, 5))
    for field, value in (("rid", 3), ("rid", -1), ("score", -1)):
        regs = B["regs"].copy()
        k = int(B["reg_off"][4])                         # the first record of pair 2
        regs[field][k] = value
        got = driver(dict(B, regs=regs))
        want = QG.model(B)
        assert got["status"].tolist() == [0, 0, 1, 0, 0]
        assert (got["score"][2], got["sub"][2], got["n_sub"][2], got["n_cand"][2]) == (0, 0, 0, 0) and got["z"][2].tolist() == [-1, -1]
        keep = np.array([0, 1, 3, 4])
        assert QG.same({f: got[f][keep] for f in ALL}, {f: want[f][keep] for f in ALL}, ALL) is None
    wide = [(0, 1 << 20, 0, 300.0, 50.0)] + list(QG.PES[1:])
    assert driver(dict(B, pes=wide)) is None             # 2^20 + 1 distances
    wide[0] = (0, 1 << 20, 1, 300.0, 50.0)
    assert driver(dict(B, pes=wide)) is not None         # ... of a failed orientation: no table


def test_the_driver_as_a_program_is_clean_under_the_sanitizers(tmp_path):
    """address and undefined-behaviour sanitizers on the rules, in a program of its own: the whole workload, both walks"""
    exe = QC.build_program(tmp_path)
    dump = str(tmp_path / "pair.bin")
    QC.dump(dump)
    r = subprocess.run([exe, dump], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert " 0 differences" in r.stdout
