"""The rules of the pairing decision (bwa-meme_amd/csrc/meme_decide_rules.h: whether the paired branch is entered, is_multi, q_pe with the float sum of the two frac_rep,
the two branches of q_se and the cap, the secondary_all swap as a function of one record, the ALT record, `which` and the flag of the no-pairing paths, which
meme_decide.hip's kernel calls) on the CPU: the header is compiled with g++ into a sequential driver (tests/decide_rules_driver.h) that has to reproduce the model of
tests/decide_gen.py -- which reproduces the compiled reference's fixture -- on the whole workload and on the batches built for the status and the is_alt bit, every output and
every byte of every record.  The same driver as a program of its own (scripts/decide_rules_main.cpp) is built with -fsanitize=address,undefined and run over all of it.
(The kernel is checked in tests/test_gpu_decide.py.)"""
import subprocess

import numpy as np
import pytest

import decide_cases as DC
import decide_gen as DG


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return DC.build_driver(tmp_path_factory.mktemp("decide_rules"))


def test_driver_reproduces_the_model_on_the_whole_workload(driver):
    S = DC.stage_inputs()
    assert len(S) == len(DG.workload()) + 2
    for s, m in S:
        assert DC.same(driver(s), m) is None, s["name"]


def test_swap_as_a_function_of_one_record_equals_the_loop(driver):
    """the reference's loop rewrites secondary_all in index order and then sets record z; the header states the result per record: random parents, k and z"""
    rng = np.random.default_rng(3)
    for _ in range(300):
        n = int(rng.integers(1, 40))
        n_pri = int(rng.integers(1, n + 1))
        sa = rng.integers(-1, n, n).tolist()
        z = int(rng.integers(0, n_pri))
        k = sa[z]
        want = list(sa)
        if 0 <= k < n_pri:
            for j in range(n):
                if want[j] == k or j == k:
                    want[j] = z
            want[z] = -1
        got = [(-1 if j == z else z if sa[j] == k or j == k else sa[j]) if 0 <= k < n_pri else sa[j] for j in range(n)]      # dec_swapped, restated
        assert got == want


def test_refusals(driver):
    s, _ = DC.stage_inputs()[0]
    assert driver(dict(s, opt=dict(a=0))) is None
    n_pri = s["n_pri"].copy()
    n_pri[0] = int(s["reg_off"][1]) + 1
    assert driver(dict(s, n_pri=n_pri)) is None


def test_the_driver_as_a_program_is_clean_under_the_sanitizers(tmp_path):
    """address and undefined-behaviour sanitizers on the rules, in a program of its own: the whole workload and the direct batches"""
    exe = DC.build_program(tmp_path)
    dump = str(tmp_path / "decide.bin")
    DC.dump(dump)
    r = subprocess.run([exe, dump], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert " 0 differences" in r.stdout
