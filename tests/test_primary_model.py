"""Model and fixture of primary marking and mapping quality (CPU only): tests/primary_gen.py's plain-Python restatement of mem_mark_primary_se,
mem_reorder_primary5 and mem_approx_mapq_se (reference src/bwamem.cpp:1974-2100) reproduces what the compiled reference left in
tests/golden/primary_golden.npz on the whole workload -- every field of every record, n_pri and every quality, exactly --, the workload takes
every branch often enough to mean something, no quality of it depends on whether a compiler fuses `x * y + .499`, and where the compiled
reference is at hand the model equals it under other options too."""
import ctypes
import os

import numpy as np
import pytest

import primary_gen as PG
import ref_py
from pymeme import hipapi

OTHER, split_other = PG.OTHER, PG.split_other


def test_model_reproduces_the_reference_golden():
    W = PG.workload()
    assert PG.same(PG.modelled(), PG.golden(), W["reg_off"]) is None


def test_golden_is_a_permutation_of_each_reads_records():
    W = PG.workload()
    G = np.load(os.path.join(PG.GOLDEN, "primary_golden.npz"))
    src, off = G["src"].astype(np.int64), W["reg_off"]
    assert src.shape[0] == W["regs"].shape[0] == G["mapq"].shape[0] == G["cols"].shape[0] and G["n_pri"].shape[0] == off.shape[0] - 1
    assert np.array_equal(np.sort(src), np.arange(src.shape[0]))
    read_of = np.searchsorted(off, np.arange(src.shape[0]), "right") - 1
    assert np.array_equal(read_of[src], read_of)


def test_workload_takes_every_branch():
    """the floors the workload was built to meet, counted by the model that reproduces the reference on it"""
    W, C = PG.workload(), PG.modelled()["counters"]
    print(C)
    assert PG.floors(C, W["reg_off"]) == []
    assert C["n_alt_and_pri"] >= 500 and C["n_alt_only"] >= 900 and C["n_alt_sc"] >= 600 and C["n_secondary"] >= 4000 and C["n_boundary"] >= 5
    assert all(C[k] >= 50 for k in C if k.startswith("q_"))
    # every synthetic list length is there: a read whose list of non-overlapping records has m + 1 members (the m tiles and the record behind them)
    first = np.concatenate([[0], np.cumsum(PG.modelled()["regs"]["secondary"] < 0)])[W["reg_off"]]
    members = set(np.diff(first)[W["n_fixture"]:].tolist())
    assert {m + 1 for m in PG.LIST_LENGTHS} <= members


def test_no_quality_depends_on_contraction():
    """the compiled reference may or may not fuse `x * y + .499` (-O3 at the build host's SIMD level): on this workload both give the same qualities, so the fixture holds on every box"""
    assert PG.modelled()["counters"]["n_fma_differs"] == 0


def test_float_boundary_of_the_overlap_test():
    """10 * 0.3f rounds to 3.0f as a float product and is above 3 as a double one: an overlap of 3 of 10 bases IS significant at mask_level 0.3 in the reference's
    arithmetic (int * float is a float multiply), and would not be had the product been taken in double"""
    assert np.float32(3) >= np.float32(10) * np.float32(0.3) and not 3 >= 10 * float(np.float32(0.3))
    regs = np.zeros(2, hipapi.ALNREG)
    for k, (qb, qe, sc) in enumerate([(0, 10, 50), (7, 40, 40)]):
        regs[k]["qb"], regs[k]["qe"], regs[k]["rb"], regs[k]["re"], regs[k]["score"] = qb, qe, 1000, 1000 + qe - qb, sc
    off = np.array([0, 2])
    assert PG.model(regs, off, [5], PG.default_opt(mask_level=0.3))["regs"]["secondary"].tolist() == [-1, 0]
    assert PG.model(regs, off, [5], PG.default_opt(mask_level=0.31))["regs"]["secondary"].tolist() == [-1, -1]


def test_structures_have_their_sizes():
    assert ctypes.sizeof(hipapi.PrimaryOpt) == 48 and ctypes.sizeof(hipapi.PrimaryHost) == 64 and ctypes.sizeof(hipapi.PrimaryDeviceOut) == 40
    assert hipapi.PrimaryOpt.mask_level.offset == 32 and hipapi.PrimaryOpt.primary5.offset == 44 and hipapi.PrimaryHost.kernel_ms.offset == 56
    o = hipapi.default_primary_opt()
    d = PG.default_opt()
    assert all(getattr(o, k) == d[k] for k in d)


@pytest.mark.skipif(not (ref_py.have("libstage_ref.so") and ref_py.have("libbwa_pic.so") and ref_py.cpu_can_run()), reason="compiled reference (oracle/_ref) not available on this box")
@pytest.mark.parametrize("name", list(OTHER), ids=list(OTHER))
def test_model_equals_the_compiled_reference_under_other_options(name):
    import ref_primary
    W = PG.workload()
    kw, id_base = split_other(name)
    ids = np.arange(W["reg_off"].shape[0] - 1, dtype=np.int64) + id_base
    got = PG.model(W["regs"], W["reg_off"], ids, PG.default_opt(**kw), both=True)
    assert got["counters"]["n_fma_differs"] == 0                          # (else the comparison below would depend on the box that built the reference)
    if name == "primary5":
        assert got["counters"]["n_reordered"] >= 50
    fields = {k: v for k, v in kw.items() if k != "primary5"}
    R = ref_primary.Reference(**fields).run(W["regs"], W["reg_off"], ids, primary5=bool(kw.get("primary5")))
    assert R["mapq"].min() >= 0 and R["mapq"].max() <= 255
    want = {"regs": R["regs"], "n_pri": R["n_pri"], "mapq": R["mapq"].astype(np.uint8)}
    assert PG.same(got, want, W["reg_off"]) is None
