"""The rules of mate rescue's record updates (bwa-meme_amd/csrc/meme_rescue_rules.h: the records looked at and their gar entries, the record a result becomes, the two
insertions, the two clean-ups and the driver of one end, which meme_rescue.hip's kernels call) on the CPU: the header is compiled with g++ into a sequential driver
(tests/rescue_rules_driver.h) that has to reproduce the model of tests/rescue_gen.py -- which reproduces the compiled reference's fixture -- on families A and B and
on the batches built for the status: every record, every offset, every counter.  The same driver as a program of its own (scripts/rescue_rules_main.cpp) is built with
-fsanitize=address,undefined and run over all of it.  (The kernels are checked in tests/test_gpu_rescue.py.)"""
import subprocess

import numpy as np
import pytest

import rescue_cases as RC
import rescue_gen as RG


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return RC.build_driver(tmp_path_factory.mktemp("rescue_rules"))


def test_driver_reproduces_the_model_on_the_whole_workload(driver):
    S = RC.stage_inputs()
    assert len(S) == len(RG.workload()) + len(RG.direct())
    for B, m in S:
        got = driver(B)
        assert got is not None and RG.same(got, m) is None, (B["name"], RG.same(got, m))
        assert got["counters"] == RC.counters_of(m), B["name"]


def test_refusals(driver):
    B = RG.workload()[0]
    assert driver(B, opt=dict(B["opt"], max_matesw=-1)) is None
    assert driver(B, opt=dict(B["opt"], batch_reads=3)) is None
    assert driver(B, opt=dict(B["opt"], batch_reads=0)) is None
    assert driver(B, gar_off=B["gar_off"][:-1]) is None                  # (worker batches that do not cover the reads)


def test_the_driver_as_a_program_is_clean_under_the_sanitizers(tmp_path):
    """address and undefined-behaviour sanitizers on the rules, in a program of its own: the whole workload and the direct batches"""
    exe = RC.build_program(tmp_path)
    dump = str(tmp_path / "rescue.bin")
    RC.dump(dump)
    r = subprocess.run([exe, dump], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert " 0 differences" in r.stdout
