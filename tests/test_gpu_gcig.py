"""The CIGAR kernel (meme_global_batch_host = ksw_global2 under bwa_gen_cigar2), through the C ABI, against score and CIGAR of the
compiled reference (tests/golden/gcig_golden.npz) and against the oracle with other penalties."""
import os
import re

import numpy as np
import pytest

import oracle_py as O
from common import GOLDEN, build_index, cjob_band, gcig_workload, gencig_workload
from pymeme import hipapi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=[1, 0], ids=["groups", "wavefront-per-job"])
def _gcig_groups(request, monkeypatch):
    """Round 6: jobs with bands of at most 16 / 32 columns run 4 / 2 to a wavefront (k_gcig_grp); every test of this file runs with that (the default) and with
    one wavefront per job (k_gcig alone) -- the same scores, operations, NM and MD either way."""
    monkeypatch.setenv("MEME_TUNING", "gcig_groups=%d" % request.param)


def _ctx_with_reads(tmp_path, g, reads):
    fa = str(tmp_path / "g.fa")
    synth.write_fasta(fa, g, contigs=2)
    prefix = build_index(fa, bits=14)
    ctx = hipapi.Context(0)
    ctx.load_index_files(prefix)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    ctx.seed_batch_host(np.concatenate(reads), off)            # stages the reads the jobs refer to
    return ctx


def test_device_cigars_equal_reference_golden(tmp_path):
    g, reads, jobs, _ = gcig_workload()
    G = np.load(os.path.join(GOLDEN, "gcig_golden.npz"))
    ctx = _ctx_with_reads(tmp_path, g, reads)
    try:
        res, cig, ms = ctx.global_batch_host(jobs)
    finally:
        ctx.close()
    assert np.array_equal(res["score"], G["score"])
    assert np.array_equal(res["n_cigar"], G["n_cigar"])
    assert np.array_equal(res["cigar_off"], np.concatenate([[0], np.cumsum(G["n_cigar"])])[:-1])
    assert np.array_equal(cig, G["cigars"])


def test_device_cigars_equal_oracle_with_other_penalties(tmp_path):
    g, reads, jobs, seqs = gcig_workload(n=800, seed=91)
    # (the workload's bands are 1, 3, 10, 30, 100, ...: every third job gets one of 33-63 instead -- 67-127 band columns, the two-columns-per-lane kernel of round 6)
    jobs = jobs.copy()
    for k in range(0, jobs.shape[0], 3):
        need = abs(int(jobs["tlen"][k]) - int(jobs["qlen"][k]))
        jobs["w"][k] = max(need, 33 + (7 * k) % 31)
    ctx = _ctx_with_reads(tmp_path, g, reads)
    try:
        for a, b, od, ed, oi, ei in ((2, 3, 4, 2, 7, 1), (1, 9, 1, 1, 1, 1)):
            opt = hipapi.BswOpt(od, ed, oi, ei, 100, 5, a, b)
            res, cig, _ = ctx.global_batch_host(jobs, opt)
            for k, (J, (q, t)) in enumerate(zip(jobs, seqs)):
                sc, cg = O.ksw_global2(q, t, int(J["w"]), a, b, od, ed, oi, ei)
                o0 = int(res["cigar_off"][k])
                assert sc == int(res["score"][k]) and np.array_equal(cg, cig[o0:o0 + int(res["n_cigar"][k])]), (k, a, b, od, ed, oi, ei)
        bad = jobs[:4].copy()
        bad["read"][2] = len(reads) + 5
        with pytest.raises(hipapi.MemeError, match="malformed"):
            ctx.global_batch_host(bad)
        # a band that does not reach the matrix's last cell, and a query span that runs past its read: refused, not computed on garbage
        narrow = jobs[:4].copy()
        narrow["tlen"][1] = narrow["qlen"][1] + 40
        narrow["w"][1] = 10
        with pytest.raises(hipapi.MemeError, match="malformed"):
            ctx.global_batch_host(narrow)
        long_q = jobs[:4].copy()
        long_q["qb"][3] = 5
        long_q["qlen"][3] = len(reads[int(long_q["read"][3])])
        long_q["w"][3] = 500
        with pytest.raises(hipapi.MemeError, match="beyond the end of read"):
            ctx.global_batch_host(long_q)
    finally:
        ctx.close()


def _check_calls(res, cig, md, want):
    """device results of a gen_cigar batch against a list of (score, cigar, nm, md) tuples"""
    assert res.shape[0] == len(want)
    o, m = 0, 0
    for k, (sc, cg, nm, s) in enumerate(want):
        R = res[k]
        assert int(R["cigar_off"]) == o and int(R["md_off"]) == m, k                # packed in job order
        got_md = md[m:m + int(R["md_len"])].tobytes()
        assert md[m + int(R["md_len"])] == 0
        assert (int(R["score"]), int(R["nm"]), got_md) == (sc, nm, s) and np.array_equal(cig[o:o + int(R["n_cigar"])], cg), (k, R, sc, nm, s, got_md)
        o += int(R["n_cigar"]); m += int(R["md_len"]) + 1
    assert o == cig.shape[0] and m == md.shape[0]


def test_device_gen_cigar_equals_reference_golden(tmp_path):
    """meme_gen_cigar_batch_host (bwa_gen_cigar2 whole on the device: shortcut or band + DP + traceback, NM, MD) against what the compiled
    reference's function returned for the same calls (tests/golden/gencig_golden.npz)."""
    g, reads, calls = gencig_workload()
    G = np.load(os.path.join(GOLDEN, "gencig_golden.npz"))
    off = np.concatenate([[0], np.cumsum(G["n_cigar"])])
    mds = G["md"].tobytes().split(b"\0")
    want = [(int(G["score"][k]), G["cigars"][off[k]:off[k + 1]], int(G["nm"][k]), mds[k]) for k in range(calls.shape[0])]
    ctx = _ctx_with_reads(tmp_path, g, reads)
    try:
        res, cig, md, ms = ctx.gen_cigar_batch_host(calls)
        _check_calls(res, cig, md, want)
        # a call the reference's function rejects is refused, not computed: a target across the strand boundary, an empty query
        bad = calls[:3].copy()
        bad["rb"][1] = g.shape[0] - 10; bad["tlen"][1] = 40
        with pytest.raises(hipapi.MemeError, match="malformed"):
            ctx.gen_cigar_batch_host(bad)
        bad = calls[:3].copy()
        bad["qb"][2] = 5; bad["qlen"][2] = len(reads[int(bad["read"][2])])
        with pytest.raises(hipapi.MemeError, match="beyond the end of read"):
            ctx.gen_cigar_batch_host(bad)
        r0 = ctx.gen_cigar_batch_host(calls[:0])
        assert r0[0].shape[0] == 0 and r0[1].shape[0] == 0 and r0[2].shape[0] == 0
    finally:
        ctx.close()


def test_device_gen_cigar_equals_oracle_with_other_penalties(tmp_path):
    g, reads, calls = gencig_workload(n=700, seed=211)
    text = hipapi.fwd_rc_text(g)
    ctx = _ctx_with_reads(tmp_path, g, reads)
    try:
        for a, b, od, ed, oi, ei in ((2, 3, 4, 2, 7, 1), (1, 9, 1, 1, 1, 1), (3, 1, 5, 3, 2, 2)):
            opt = hipapi.BswOpt(od, ed, oi, ei, 100, 5, a, b)
            res, cig, md, _ = ctx.gen_cigar_batch_host(calls, opt)
            want = [O.gen_cigar2(text, g.shape[0], reads[int(J["read"])][int(J["qb"]):int(J["qb"]) + int(J["qlen"])], int(J["rb"]), int(J["rb"]) + int(J["tlen"]),
                                 int(J["w_"]), a, b, od, ed, oi, ei) for J in calls]
            _check_calls(res, cig, md, want)
    finally:
        ctx.close()


# ---- the storage modes, LDS budgets and batch limits that only the batch's SIZE selects: forced through the tuning keys, the host-side model of
# ---- gcig_plan / k_gcig_sizes (csrc/meme_gcig.hip) says before the GPU call which path every job takes ---------------------------------------
_GRP = ((16, 4, 4096, 24 * 1024), (32, 2, 8192, 24 * 1024), (64, 1, 12288, 16 * 1024))      # GCIG_GRP: lanes, jobs per wavefront, zmax, lds_max
_Z_LDS_CAP, _Z_LDS_WINDOW = 8192, 2048


def _groups_on():
    return os.environ["MEME_TUNING"] == "gcig_groups=1"


def _plan(qlen, tlen, w, groups, zcap_key=-1):
    """gcig_plan + k_gcig_sizes on the host.  w < 0: the gap-free shortcut.  Returns (zcap in force, LDS matrix bytes of the three group classes, class per job
    -- 0 / 1 / 4: k_gcig_grp<16 / 32 / 64>, 2: k_gcig_t, 3: k_gcig_nogap, the slots of meme_timings::gcig_class_jobs --, band columns per job)."""
    qlen, tlen, w = (np.asarray(x, np.int64) for x in (qlen, tlen, w))
    qmax, tmax = int(qlen.max()), int(tlen.max())
    qcap, tcap = (qmax + 3) & ~3, (tmax + 3) & ~3
    lds_base = 3 * (qmax + 2) * 4 + qcap + tcap
    zwant = zcap_key if zcap_key >= 0 else (_Z_LDS_CAP if tmax * 33 <= _Z_LDS_CAP else _Z_LDS_WINDOW)
    zcap = zwant if lds_base + zwant <= 32 * 1024 else 0
    grp_z = []
    for lanes, per_wave, zmax, lds_max in _GRP:
        z = min((lanes * tmax + 3) & ~3, zmax) if groups else 0
        if per_wave * (3 * 2 * lanes * 4 + qcap + tcap + z) > lds_max:
            z = 0
        grp_z.append(z)
    n_col = np.minimum(qlen, 2 * w + 1)
    cls = np.full(qlen.shape[0], 3, np.int64)
    left = w >= 0
    for slot, (lanes, _, _, _), z in zip((0, 1, 4), _GRP, grp_z):
        take = left & (n_col <= lanes) & (n_col * tlen <= z)
        cls[take] = slot
        left &= ~take
    cls[left] = 2
    return zcap, grp_z, cls, n_col


def _walks(n_col, tlen, zcap):
    """how k_gcig_t walks a job's matrix back: (whole matrix in LDS, through a window of LDS rows, straight on global memory) masks; rows of the window"""
    in_lds = n_col * tlen <= zcap
    windowed = ~in_lds & (zcap >= 2 * n_col + 8)
    return in_lds, windowed, ~in_lds & ~windowed, np.where(windowed, (zcap - 8) // np.maximum(n_col, 1), 0)


def _class_counts(cls):
    return [int((cls == k).sum()) for k in range(6)]


# matrix in LDS / walked through a window / walked straight on global memory, of the 4 000 jobs of gcig_workload() when all go to k_gcig_t
_ZCAP_SPLIT = {0: (0, 0, 4000), 64: (0, 1183, 2817), 2048: (777, 3223, 0), 8192: (2187, 1813, 0), 24576: (3280, 720, 0)}


@pytest.mark.parametrize("zcap", sorted(_ZCAP_SPLIT))
def test_every_matrix_storage_mode_gives_the_golden_cigars(tmp_path, zcap):
    """Tuning "gcig_zcap": the LDS k_gcig_t keeps per job for its backtrack matrix.  The fixture's targets reach 290 bases, so by default every test of this
    file runs with 2 048 bytes; 8 192 is what 150-bp reads get, 0 and 64 walk the matrix straight on global memory, 64 also through a window of two rows."""
    g, reads, jobs, _ = gcig_workload()
    G = np.load(os.path.join(GOLDEN, "gcig_golden.npz"))
    groups = _groups_on()
    q, t, w = jobs["qlen"], jobs["tlen"], jobs["w"]
    # every job a wavefront: the table of the modes
    zc, _, cls_all, n_col = _plan(q, t, w, False, zcap)
    assert zc == zcap and (cls_all == 2).all()
    in_lds, windowed, straight, rows = _walks(n_col, t.astype(np.int64), zc)
    assert (int(in_lds.sum()), int(windowed.sum()), int(straight.sum())) == _ZCAP_SPLIT[zcap]
    if zcap == 64:
        assert int((rows[windowed] == 2).sum()) > 0
    if zcap == 8192:
        assert int(in_lds.sum()) > jobs.shape[0] // 2
    # the run's own classes: what is left to k_gcig_t, and the modes among that
    zc, _, cls, _ = _plan(q, t, w, groups, zcap)
    mine = cls == 2
    assert mine.sum() > 0 and (groups or mine.all())
    m_lds, m_win, m_str, _ = _walks(n_col[mine], t.astype(np.int64)[mine], zc)
    if zcap in (0, 64):
        assert int(m_str.sum()) > 0
    if zcap >= 2048 or (zcap == 64 and not groups):            # (with groups on, the bands a 64-byte window can hold are the group classes')
        assert int(m_win.sum()) > 0
    ctx = _ctx_with_reads(tmp_path, g, reads)
    try:
        ctx.set_tuning("gcig_zcap", zcap)
        res, cig, ms = ctx.global_batch_host(jobs)
        got_cls = list(ctx.timings().gcig_class_jobs)
    finally:
        ctx.close()
    print("gcig_zcap=%d groups=%d: gcig_class_jobs %s, k_gcig_t jobs in LDS / window / global %d / %d / %d" % (zcap, groups, got_cls, m_lds.sum(), m_win.sum(), m_str.sum()))
    assert got_cls == _class_counts(cls)
    assert got_cls[2] > 0 and (groups or got_cls[2] == jobs.shape[0])
    assert np.array_equal(res["score"], G["score"])
    assert np.array_equal(res["n_cigar"], G["n_cigar"])
    assert np.array_equal(res["cigar_off"], np.concatenate([[0], np.cumsum(G["n_cigar"])])[:-1])
    assert np.array_equal(cig, G["cigars"])


@pytest.mark.parametrize("zcap", sorted(_ZCAP_SPLIT))
def test_every_matrix_storage_mode_gives_the_golden_gen_cigar_results(tmp_path, zcap):
    """The same for meme_gen_cigar_batch_host: NM and MD are read off the operations the walk wrote."""
    g, reads, calls = gencig_workload()
    G = np.load(os.path.join(GOLDEN, "gencig_golden.npz"))
    off = np.concatenate([[0], np.cumsum(G["n_cigar"])])
    mds = G["md"].tobytes().split(b"\0")
    want = [(int(G["score"][k]), G["cigars"][off[k]:off[k + 1]], int(G["nm"][k]), mds[k]) for k in range(calls.shape[0])]
    groups = _groups_on()
    q, t = calls["qlen"], calls["tlen"]
    w = cjob_band(q, t, calls["w_"])
    zc, _, cls, n_col = _plan(q, t, w, groups, zcap)
    mine = cls == 2
    assert zc == zcap and mine.sum() > 0 and (cls == 3).sum() > 0
    m_lds, m_win, m_str, rows = _walks(n_col[mine], t.astype(np.int64)[mine], zc)
    if zcap in (0, 64):
        assert int(m_str.sum()) > 0
    if zcap == 64 and not groups:
        assert int((rows[m_win] == 2).sum()) > 0
    if zcap >= 2048:
        assert int(m_win.sum()) > 0 and (groups or int(m_lds.sum()) > 0)    # (with groups on, the small matrices are mostly the group classes')
    ctx = _ctx_with_reads(tmp_path, g, reads)
    try:
        ctx.set_tuning("gcig_zcap", zcap)
        res, cig, md, ms = ctx.gen_cigar_batch_host(calls)
        got_cls = list(ctx.timings().gcig_class_jobs)
    finally:
        ctx.close()
    print("gen_cigar gcig_zcap=%d groups=%d: gcig_class_jobs %s, k_gcig_t jobs in LDS / window / global %d / %d / %d" % (zcap, groups, got_cls, m_lds.sum(), m_win.sum(), m_str.sum()))
    assert got_cls == _class_counts(cls)
    assert got_cls[2] > 0 and (groups or got_cls[2] == int((w >= 0).sum()))
    _check_calls(res, cig, md, want)


def _check_global(res, cig, jobs, seqs, pen):
    a, b, od, ed, oi, ei = pen
    for k, (J, (q, t)) in enumerate(zip(jobs, seqs)):
        sc, cg = O.ksw_global2(q, t, int(J["w"]), a, b, od, ed, oi, ei)
        o0 = int(res["cigar_off"][k])
        assert sc == int(res["score"][k]) and np.array_equal(cg, cig[o0:o0 + int(res["n_cigar"][k])]), (k, pen)


def test_short_reads_take_the_whole_matrix_mode_by_default(tmp_path):
    """Reads of 40-150 bases -- production's commonest class: the longest target x 33 columns fits 8 192 bytes, so gcig_plan keeps 8 192 bytes per job WITHOUT any
    key (every other test of this file has targets of 290 bases and gets 2 048)."""
    g, reads, jobs, seqs = gcig_workload(n=600, seed=301, read_len=(40, 151))
    assert jobs.shape[0] == 800 and int(jobs["tlen"].max()) * 33 <= _Z_LDS_CAP
    groups = _groups_on()
    zc, _, cls, n_col = _plan(jobs["qlen"], jobs["tlen"], jobs["w"], groups)
    mine = cls == 2
    m_lds, m_win, m_str, _ = _walks(n_col[mine], jobs["tlen"].astype(np.int64)[mine], zc)
    assert zc == _Z_LDS_CAP and int(m_lds.sum()) > 0 and int(m_win.sum()) > 0 and int(m_str.sum()) == 0
    ctx = _ctx_with_reads(tmp_path, g, reads)
    try:
        for pen in ((1, 4, 6, 1, 6, 1), (2, 3, 4, 2, 7, 1)):
            a, b, od, ed, oi, ei = pen
            res, cig, _ = ctx.global_batch_host(jobs, hipapi.BswOpt(od, ed, oi, ei, 100, 5, a, b))
            assert list(ctx.timings().gcig_class_jobs) == _class_counts(cls)
            _check_global(res, cig, jobs, seqs, pen)
    finally:
        ctx.close()
    g, reads, calls = gencig_workload(n=600, seed=303, read_len=(40, 151))
    assert int(calls["tlen"].max()) * 33 <= _Z_LDS_CAP
    w = cjob_band(calls["qlen"], calls["tlen"], calls["w_"])
    zc, _, cls, _ = _plan(calls["qlen"], calls["tlen"], w, groups)
    assert zc == _Z_LDS_CAP and (cls == 2).sum() > 0
    text = hipapi.fwd_rc_text(g)
    (tmp_path / "calls").mkdir()                                   # (another genome: an index of its own)
    ctx = _ctx_with_reads(tmp_path / "calls", g, reads)
    try:
        res, cig, md, _ = ctx.gen_cigar_batch_host(calls)
        assert list(ctx.timings().gcig_class_jobs) == _class_counts(cls)
        want = [O.gen_cigar2(text, g.shape[0], reads[int(J["read"])][int(J["qb"]):int(J["qb"]) + int(J["qlen"])], int(J["rb"]), int(J["rb"]) + int(J["tlen"]), int(J["w_"]))
                for J in calls]
        _check_calls(res, cig, md, want)
    finally:
        ctx.close()


def test_reads_of_251_to_500_bases(tmp_path):
    """Seeding admits reads of 500 bases; the other tests of this file stop at 250.  Bands from 1 to 600 (never below |tlen - qlen| + 3, as the workload does)."""
    bands = (1, 3, 10, 30, 100, 200, 400, 600)
    g, reads, jobs, seqs = gcig_workload(n=300, seed=311, read_len=(251, 501), bands=bands)
    assert jobs.shape[0] == 400 and int(jobs["qlen"].min()) > 235 and int(jobs["qlen"].max()) > 490 and int(jobs["w"].max()) == 600
    groups = _groups_on()
    zc, _, cls, _ = _plan(jobs["qlen"], jobs["tlen"], jobs["w"], groups)
    assert zc == _Z_LDS_WINDOW and (cls == 2).sum() > 0
    ctx = _ctx_with_reads(tmp_path, g, reads)
    try:
        res, cig, _ = ctx.global_batch_host(jobs)
        assert list(ctx.timings().gcig_class_jobs) == _class_counts(cls)
        _check_global(res, cig, jobs, seqs, (1, 4, 6, 1, 6, 1))
    finally:
        ctx.close()
    g, reads, calls = gencig_workload(n=300, seed=313, read_len=(251, 501), bands=(0,) + bands)
    text = hipapi.fwd_rc_text(g)
    w = cjob_band(calls["qlen"], calls["tlen"], calls["w_"])
    _, _, cls, _ = _plan(calls["qlen"], calls["tlen"], w, groups)
    (tmp_path / "calls").mkdir()
    ctx = _ctx_with_reads(tmp_path / "calls", g, reads)
    try:
        res, cig, md, _ = ctx.gen_cigar_batch_host(calls)
        assert list(ctx.timings().gcig_class_jobs) == _class_counts(cls)
        want = [O.gen_cigar2(text, g.shape[0], reads[int(J["read"])][int(J["qb"]):int(J["qb"]) + int(J["qlen"])], int(J["rb"]), int(J["rb"]) + int(J["tlen"]), int(J["w_"]))
                for J in calls]
        assert all(x is not None for x in want)
        _check_calls(res, cig, md, want)
    finally:
        ctx.close()


def test_one_long_target_switches_a_group_class_off_for_the_batch(tmp_path):
    """The group classes' LDS is sized by the batch's longest query and target (grp_lds against GCIG_GRP's lds_max): one job of a 500-base read against a
    1 300-base target -- admissible: the entry points take targets up to 65 535 bases inside the text, a band of at least |tlen - qlen| -- among 300 short
    ones leaves k_gcig_grp<16> without a matrix, and its jobs go to the 32-lane class.  Every job against the oracle."""
    g, reads, jobs, seqs = gcig_workload(n=225, seed=321, read_len=(40, 151), bands=(1, 3, 5, 7, 10, 30))
    assert jobs.shape[0] == 300
    rng = np.random.default_rng(5)
    text = hipapi.fwd_rc_text(g)
    big = rng.integers(0, 4, size=500).astype(np.uint8)
    rb, tl = 20_000, 1300
    big[:400] = text[rb + 100:rb + 500]                             # (related to its target: a real alignment with a long deletion at its end)
    reads = reads + [big]
    out = np.zeros(1, hipapi.GJOB)
    out[0] = (rb, len(reads) - 1, 0, 500, tl, tl - 500 + 3, 0)
    at = 137
    jobs = np.concatenate([jobs[:at], out, jobs[at:]])
    seqs = seqs[:at] + [(big.copy(), text[rb:rb + tl].copy())] + seqs[at:]
    _, z_without, cls_without, _ = _plan(np.delete(jobs["qlen"], at), np.delete(jobs["tlen"], at), np.delete(jobs["w"], at), True)
    zc, z_with, cls, _ = _plan(jobs["qlen"], jobs["tlen"], jobs["w"], _groups_on())
    _, z_grp, cls_grp, _ = _plan(jobs["qlen"], jobs["tlen"], jobs["w"], True)
    assert all(z > 0 for z in z_without) and (cls_without == 0).sum() > 50
    assert z_grp[0] == 0 and z_grp[1] > 0 and z_grp[2] > 0 and (cls_grp == 0).sum() == 0 and (cls_grp == 1).sum() > 50     # the 16-lane class is off, its jobs are the 32-lane class's
    ctx = _ctx_with_reads(tmp_path, g, reads)
    try:
        res, cig, _ = ctx.global_batch_host(jobs)
        assert list(ctx.timings().gcig_class_jobs) == _class_counts(cls)
        _check_global(res, cig, jobs, seqs, (1, 4, 6, 1, 6, 1))
        calls = np.zeros(jobs.shape[0], hipapi.CJOB)
        for f in ("rb", "read", "qb", "qlen", "tlen"):
            calls[f] = jobs[f]
        calls["w_"] = jobs["w"]
        res, cig, md, _ = ctx.gen_cigar_batch_host(calls)
        wc = cjob_band(calls["qlen"], calls["tlen"], calls["w_"])
        assert list(ctx.timings().gcig_class_jobs) == _class_counts(_plan(calls["qlen"], calls["tlen"], wc, _groups_on())[2])
        want = [O.gen_cigar2(text, g.shape[0], reads[int(J["read"])][int(J["qb"]):int(J["qb"]) + int(J["qlen"])], int(J["rb"]), int(J["rb"]) + int(J["tlen"]), int(J["w_"]))
                for J in calls]
        assert all(x is not None for x in want)
        _check_calls(res, cig, md, want)
    finally:
        ctx.close()


def test_max_batch_refuses_more_jobs_and_takes_that_many(tmp_path):
    """Tuning "max_batch" (what the bound aligner sets from its memory budget): both entry points refuse 11 jobs with MEME_E_CAPACITY -- the caller then feeds
    pieces -- and give for 10 what an unrestricted ctx gives."""
    g, reads, jobs, _ = gcig_workload(n=12, seed=331)
    _, _, calls = gencig_workload(n=12, seed=331)
    assert jobs.shape[0] >= 11 and calls.shape[0] >= 11
    free = _ctx_with_reads(tmp_path, g, reads)
    ctx = _ctx_with_reads(tmp_path, g, reads)
    try:
        ctx.set_tuning("max_batch", 10)
        with pytest.raises(hipapi.MemeError, match="exceed the ctx's"):
            ctx.global_batch_host(jobs[:11])
        with pytest.raises(hipapi.MemeError, match="exceed the ctx's"):
            ctx.gen_cigar_batch_host(calls[:11])
        a, b = ctx.global_batch_host(jobs[:10]), free.global_batch_host(jobs[:10])
        assert hipapi.records_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].shape[0] == 10
        a, b = ctx.gen_cigar_batch_host(calls[:10]), free.gen_cigar_batch_host(calls[:10])
        assert hipapi.records_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[0].shape[0] == 10
    finally:
        ctx.close()
        free.close()


# ---- the shapes at which what the DP kernels share can go wrong: the rules of csrc/meme_gcig_rules.h in both kernels' storage, F's scan at every group width and
# ---- across the chunk seam, the NM / MD emitter at every group width ----------------------------------------------------------------------------------------
_EDGE_W = {7: 0, 8: 1, 15: 1, 16: 4, 31: 4, 32: 2}        # band -> 2w + 1 = 15, 17, 31, 33, 63, 65 band columns -> the class with groups on (slot of gcig_class_jobs)
_EDGE_Q = {16: 0, 17: 1, 32: 1, 33: 4, 64: 4, 65: 2}      # the same numbers of columns as the query's length under a band of 100
_MD_W = {0: 3, 7: 0, 15: 1, 31: 4, 100: 2}                # band ARGUMENT of a 150-base call without length difference -> its class (0: the gap-free shortcut)
# mismatch positions of 150-base calls: match runs of exactly G, G + 1 and 2G between them for G = 16, 32, 64 (64: two calls), and mismatches in the last lane of
# a group and the first lane of the next
_MD_RUNS = {16: [(5, 22, 40, 73)], 32: [(5, 38, 72, 137)], 64: [(3, 68, 134), (10, 139)], 0: [(15, 16, 31, 32, 63, 64)]}


class _Posed:
    """Jobs posed in the frame the kernels align in (on the reverse strand both sequences reversed): a target is drawn from the text, the query is built
    against it in that frame, add() stores the read the job names."""

    def __init__(self, g, seed):
        self.text, self.l_pac, self.rng = hipapi.fwd_rc_text(g), g.shape[0], np.random.default_rng(seed)
        self.reads, self.jobs, self.calls, self.seqs = [], [], [], []
        self.want_j, self.want_c, self.n = [], [], 0

    def target(self, tlen):
        self.n += 1                                                  # strands alternate
        rb = int(self.rng.integers(1000, self.l_pac - 1000 - tlen)) + (self.n & 1) * self.l_pac
        t = self.text[rb:rb + tlen]
        return rb, (t[::-1] if self.n & 1 else t).copy()

    def noisy(self, t):
        q = t.copy()
        hit = self.rng.random(q.shape[0]) < 0.02
        q[hit] = (q[hit] + self.rng.integers(1, 4, size=int(hit.sum()))) & 3
        return q

    def fit(self, q, qlen):
        """q cut or filled with random bases to qlen"""
        return np.concatenate([q, self.rng.integers(0, 4, size=max(qlen - q.shape[0], 0)).astype(np.uint8)])[:qlen]

    def add(self, q, rb, t, w, cls, call=False):
        rev = int(rb >= self.l_pac)
        q = np.ascontiguousarray(q, np.uint8)
        assert q.shape[0] <= 150
        self.reads.append(q[::-1].copy() if rev else q)
        if call:
            self.calls.append((rb, len(self.reads) - 1, 0, q.shape[0], t.shape[0], w, 0)); self.want_c.append(cls)
        else:
            self.jobs.append((rb, len(self.reads) - 1, 0, q.shape[0], t.shape[0], w, rev)); self.want_j.append(cls); self.seqs.append((q, t))


def _shared_piece_jobs(g):
    P = _Posed(g, 401)
    rng = P.rng
    # ksw_global2 jobs: the band columns on both sides of every class edge, through the band and through the query's length; tlen - qlen in -3 .. 3
    for edge, reps in ((_EDGE_W, 3), (_EDGE_Q, 2)):
        for x, cls in edge.items():
            for dl in range(-3, 4):
                for _ in range(reps):
                    qlen, w = (int(rng.integers(100, 151)), x) if edge is _EDGE_W else (x, 100)
                    rb, t = P.target(qlen + dl)
                    P.add(P.fit(P.noisy(t), qlen), rb, t, w, cls)
    # two and three chunks of 64 columns per row, with an insertion of 10-40 bases whose run crosses query column 63|64 (w = 64, 100: in a row below w, the
    # chunks start at column 0 and F is carried across the seam)
    for w in (33, 64, 100):
        for dl in range(-3, 4):
            for _ in range(4):
                L = int(rng.integers(10, min(40, w - 6) + 1))
                p = int(rng.integers(64 - L + 3, 61))
                rb, t = P.target(150 - L + dl)
                q = np.concatenate([P.noisy(t[:p]), rng.integers(0, 4, size=L).astype(np.uint8), P.noisy(t[p:])])
                P.add(P.fit(q, 150), rb, t, w, 2)
    # bwa_gen_cigar2 calls for the MD emitter: the runs and lane positions above, through every class
    for G, pats in _MD_RUNS.items():
        for pat in pats:
            for w_, cls in _MD_W.items():
                for _ in range(2):                                   # both strands
                    rb, t = P.target(150)
                    q = t.copy()
                    q[list(pat)] = (q[list(pat)] + 1) & 3
                    P.add(q, rb, t, w_, cls, call=True)
    # deletions longer than a group writes at once, in the class whose group is one base narrower (the band columns are the query's) and in longer queries
    for qlen, D, cls in ((16, 17, 0), (32, 33, 1), (64, 65, 4), (100, 17, None), (100, 33, None), (100, 65, 2)):
        for _ in range(2):
            rb, t = P.target(qlen + D)
            P.add(np.concatenate([t[:qlen // 2], t[qlen // 2 + D:]]), rb, t, 100, cls, call=True)
    # a deletion as the first and as the last operation: not reported
    for w_ in (7, 15, 31, 100):
        for first in (0, 0, 1, 1):
            rb, t = P.target(123)
            P.add(t[3:] if first else t[:120], rb, t, w_, None, call=True)
    return P


def _ops(cg):
    return [(int(c) & 0xf, int(c) >> 4) for c in cg]


def test_shared_rules_scan_and_md_emitter_at_class_edges_and_chunk_seams(tmp_path):
    """What k_gcig_t and k_gcig_grp<16 / 32 / 64> share -- meme_gcig_rules.h, gcig_fscan, gcig_md, gcig_put_num -- at the shapes where a shared piece can go wrong
    in one kernel only: see _shared_piece_jobs.  Score, operations, NM and MD of every job equal the oracle's; which class takes which job is asserted first."""
    g = synth.make_genome(120_000, seed=403, repeat_frac=0.02)
    P = _shared_piece_jobs(g)
    jobs, calls = np.array(P.jobs, dtype=hipapi.GJOB), np.array(P.calls, dtype=hipapi.CJOB)
    groups = _groups_on()
    assert 300 <= jobs.shape[0] + calls.shape[0] <= 600 and max(len(r) for r in P.reads) == 150
    # the classes: as posed with groups on -- every slot populated --, k_gcig_t for every DP job without
    _, _, cls_j, n_col = _plan(jobs["qlen"], jobs["tlen"], jobs["w"], groups)
    assert sorted(set(n_col.tolist()) & {15, 16, 17, 31, 32, 33, 63, 64, 65}) == [15, 16, 17, 31, 32, 33, 63, 64, 65]
    assert set((jobs["tlen"] - jobs["qlen"])[:len(_EDGE_W) * 21 + len(_EDGE_Q) * 14].tolist()) == set(range(-3, 4))
    wc = cjob_band(calls["qlen"], calls["tlen"], calls["w_"])
    _, _, cls_c, _ = _plan(calls["qlen"], calls["tlen"], wc, groups)
    for cls, want in ((cls_j, P.want_j), (cls_c, P.want_c)):
        for k, c in enumerate(want):
            assert c is None or int(cls[k]) == (c if groups or c == 3 else 2), (k, c, int(cls[k]))
        assert not groups or all(_class_counts(cls)[s] > 0 for s in (0, 1, 4, 2))
    # what the oracle's alignments are, against what the jobs were posed for
    pen = (1, 4, 6, 1, 6, 1)
    want_j = [O.ksw_global2(q, t, int(J["w"]), *pen) for J, (q, t) in zip(jobs, P.seqs)]
    seam = 0
    for J, (_, cg) in zip(jobs, want_j):
        x = y = 0
        for op, l in _ops(cg):
            seam += int(op == 1 and l >= 10 and x <= 63 and x + l - 1 >= 64 and y - 1 < int(J["w"]) and int(J["w"]) >= 64)
            x += l if op != 2 else 0
            y += l if op != 1 else 0
    assert seam >= 36, seam
    want_c = [O.gen_cigar2(P.text, P.l_pac, P.reads[int(J["read"])], int(J["rb"]), int(J["rb"]) + int(J["tlen"]), int(J["w_"])) for J in calls]
    assert all(x is not None for x in want_c)
    runs = {c: set() for c in range(5)}
    for c, (_, _, _, md) in zip(cls_c, want_c):
        runs[int(c)] |= {int(x) for x in re.split(rb"[ACGTN^]+", md) if x}
    for G, c in ((16, 0), (32, 1), (64, 4), (64, 2)):
        assert {G, G + 1, 2 * G} <= runs[c if groups else 2], (G, c)
    dels = [l for _, cg, _, _ in want_c for op, l in _ops(cg)[1:-1] if op == 2]
    assert all(dels.count(D) >= 2 for D in (17, 33, 65))
    assert sum(_ops(cg)[0][0] == 2 for _, cg, _, _ in want_c) >= 4 and sum(_ops(cg)[-1][0] == 2 for _, cg, _, _ in want_c) >= 4
    ctx = _ctx_with_reads(tmp_path, g, P.reads)
    try:
        res, cig, _ = ctx.global_batch_host(jobs)
        assert list(ctx.timings().gcig_class_jobs) == _class_counts(cls_j)
        for k, (sc, cg) in enumerate(want_j):
            o0 = int(res["cigar_off"][k])
            assert sc == int(res["score"][k]) and np.array_equal(cg, cig[o0:o0 + int(res["n_cigar"][k])]), (k, jobs[k])
        res, cig, md, _ = ctx.gen_cigar_batch_host(calls)
        assert list(ctx.timings().gcig_class_jobs) == _class_counts(cls_c)
        _check_calls(res, cig, md, want_c)
    finally:
        ctx.close()
