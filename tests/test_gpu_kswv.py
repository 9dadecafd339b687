"""The mate-rescue Smith-Waterman kernel (meme_kswv_batch_host) against the compiled reference's fixture and the oracle."""
import os

import numpy as np
import pytest

import oracle_py as O
from common import (GOLDEN, KSWV_A7_PEN, KSWV_A7_WORKLOAD, KSWV_CLASS_EDGE_BOTH, KSWV_CLASS_EDGE_I16, KSWV_EDGE_WANT, KSWV_GOLDEN_SETS, KSWV_LIMIT_PEN, KSWV_SAT_SETS,
                    kswv_class_edge_jobs, kswv_edge_jobs, kswv_limit_jobs, kswv_saturated_jobs, kswv_workload)
from pymeme import hipapi

pytestmark = pytest.mark.gpu


def _opt(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1):
    o = hipapi.default_bsw_opt()
    o.a, o.b, o.o_del, o.e_del, o.o_ins, o.e_ins = a, b, o_del, e_del, o_ins, e_ins
    return o


# the driver's arithmetic (meme_kswv_run), restated: the padded query length of a job and the LDS size class (= launch) it falls into
KSWV_CLS = (64, 128, 160, 256, 384, 528)
XBYTE, XSTOP, XSUBO, XSTART = O.KSW_XBYTE, O.KSW_XSTOP, O.KSW_XSUBO, O.KSW_XSTART


def _padded(jobs):
    is8 = (jobs["xtra"] & XBYTE) != 0
    L = jobs["len2"].astype(np.int64)
    return np.where(is8, (L + 15) // 16 * 16, (L + 7) // 8 * 8), is8


def _cls(padded):
    return np.searchsorted(np.array(KSWV_CLS), padded, side="left")         # the first class that holds the padded query


def _run(ctx, jobs, ref, qer, **pen):
    return ctx.kswv_batch_host(jobs.view(hipapi.KSWV_JOB), ref, qer, _opt(**pen))[0].view(np.int32).reshape(-1, 7).copy()


def _want(jobs, ref, qer, **pen):
    return O.kswv_batch(jobs, ref, qer, threads=4, **pen)[0].view(np.int32).reshape(-1, 7)


def _same(got, want, jobs, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), jobs[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


def _job(win, q, xtra):
    jobs = np.zeros(1, O.KSWV_JOB_DTYPE)
    jobs[0] = (0, 0, win.shape[0], q.shape[0], xtra, 0)
    pad = np.zeros(8, np.uint8)
    return jobs, np.concatenate([win, pad]), np.concatenate([q, pad])


def test_kswv_kernel_equals_reference_golden():
    """All seven kswr_t fields of 11 500 jobs == what sort_classify + mem_sam_pe_batch of the compiled reference (AVX-512 kswv kernels) gave
    (tests/golden/kswv_golden.npz): int8 and int16 classes, second-best scores, reverse passes, N, low-complexity sequence, other penalties, and
    three sets under large mismatch penalties in which more than 1 000 int8 lanes saturate (score 255, no second-best score, no start)."""
    G = np.load(os.path.join(GOLDEN, "kswv_golden.npz"))
    assert sum(int((G[name][:, 0] == 255).sum()) for name in KSWV_SAT_SETS) > 1000
    assert set(KSWV_SAT_SETS) <= set(name for name, _, _ in KSWV_GOLDEN_SETS)
    ctx = hipapi.Context(0)
    try:
        for name, kw, pen in KSWV_GOLDEN_SETS:
            jobs, ref, qer = kswv_workload(**kw)
            if name in KSWV_SAT_SETS:
                assert ((jobs["xtra"] & XBYTE) != 0).all()                  # (int8 lanes only: 255 means saturated)
            got, ms = ctx.kswv_batch_host(jobs.view(hipapi.KSWV_JOB), ref, qer, _opt(**pen))
            got = got.view(np.int32).reshape(-1, 7)
            bad = np.nonzero((got != G[name]).any(axis=1))[0]
            assert bad.size == 0, (name, int(bad.size), int(bad[0]), jobs[bad[0]].tolist(), got[bad[0]].tolist(), G[name][bad[0]].tolist())
            assert ms > 0
    finally:
        ctx.close()


def test_kswv_kernel_equals_oracle_on_fresh_jobs_and_edges():
    """Fresh seeds and penalties against orc_kswv_batch; plus edge jobs: a one-base window, a window shorter than the read, a query of one
    base, jobs without KSW_XSTART / without KSW_XSUBO, a caller-set KSW_XSTOP, an empty batch; malformed jobs are refused."""
    ctx = hipapi.Context(0)
    try:
        for kw, pen in ((dict(n=3000, seed=33), {}), (dict(n=1500, seed=34, read_len=(19, 140)), dict(a=1, b=9, o_del=1, e_del=1, o_ins=1, e_ins=1)),
                        (dict(n=1500, seed=35, read_len=(240, 500), a=3), dict(a=3, b=5, o_del=7, e_del=2, o_ins=3, e_ins=3))):
            jobs, ref, qer = kswv_workload(**kw)
            want = O.kswv_batch(jobs, ref, qer, **pen)[0].view(np.int32).reshape(-1, 7)
            got = ctx.kswv_batch_host(jobs.view(hipapi.KSWV_JOB), ref, qer, _opt(**pen))[0].view(np.int32).reshape(-1, 7)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (kw, int(bad.size), int(bad[0]), jobs[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
        jobs, rb, qb = kswv_edge_jobs()
        want = O.kswv_batch(jobs, rb, qb)[0].view(np.int32).reshape(-1, 7)
        got = ctx.kswv_batch_host(jobs.view(hipapi.KSWV_JOB), rb, qb)[0].view(np.int32).reshape(-1, 7)
        assert np.array_equal(got, want), (got.tolist(), want.tolist())
        assert np.array_equal(want, np.array(KSWV_EDGE_WANT, np.int32))     # (the compiled reference's records: tests/test_ref_live.py checks them live)
        g, q, X = rb, qb, int(jobs["xtra"][0])
        assert ctx.kswv_batch_host(np.zeros(0, hipapi.KSWV_JOB), g, q)[0].shape[0] == 0
        for bad_job in ((g.shape[0] - 100, 400, 0, 150, X), (0, 400, q.shape[0] - 50, 150, X), (0, 40000, 0, 150, X)):
            jb = np.zeros(1, hipapi.KSWV_JOB)
            jb[0] = (bad_job[0], bad_job[2], bad_job[1], bad_job[3], bad_job[4], 0)
            with pytest.raises(RuntimeError):
                ctx.kswv_batch_host(jb, g, q)
    finally:
        ctx.close()


def test_kswv_saturating_int8_lanes_equal_the_oracle():
    """int8 lanes that stop because score + shift reaches 255 (shift = the mismatch penalty): the three saturating workloads of the fixture under
    other seeds, match 7 / mismatch 120, and wavefronts in which every lane saturates (64 and 130 equal jobs) or all but one do.  A saturated
    record is (255, te, qe, -1, -1, -1, -1) -- also where the reference leaves score2 / te2 unwritten (a vector without a live lane)."""
    ctx = hipapi.Context(0)
    try:
        for n_sat, kw, pen in ((50, dict(n=1000, seed=150, read_len=(236, 250)), dict(b=20)),
                               (50, dict(n=1000, seed=151, read_len=(110, 125), a=2), dict(a=2, b=30, o_del=4, e_del=2, o_ins=5, e_ins=1)),
                               (150, dict(n=1000, seed=152, read_len=(200, 250)), dict(b=60, o_del=1, e_del=1, o_ins=1, e_ins=1)),
                               (100, KSWV_A7_WORKLOAD, KSWV_A7_PEN)):
            jobs, ref, qer = kswv_workload(**kw)
            want = _want(jobs, ref, qer, **pen)
            sat = want[:, 0] == 255
            assert ((jobs["xtra"] & XBYTE) != 0).all() and int(sat.sum()) >= n_sat, (kw, int(sat.sum()))
            near = (want[:, 0] + pen["b"] >= 250) & ~sat                    # (lanes that stop just short of saturating)
            assert kw is KSWV_A7_WORKLOAD or int(near.sum()) >= 5, (kw, int(near.sum()))
            assert (want[sat][:, 3:] == -1).all()
            _same(_run(ctx, jobs, ref, qer, **pen), want, jobs, (kw, pen))
        for n, n_live in ((64, 0), (130, 0), (64, 1)):
            jobs, ref, qer = kswv_saturated_jobs(n, n_live=n_live)
            padded, is8 = _padded(jobs)
            assert is8.all() and (padded == 256).all() and (jobs["len2"] == 249).all()       # one launch, full wavefronts of equal jobs
            for b in (9, 6):
                assert 249 + b >= 255
                want = _want(jobs, ref, qer, b=b)
                assert int((want[:, 0] == 255).sum()) == n - n_live and (want[:n - n_live, 1:3] >= 0).all() and (want[:n - n_live, 3:] == -1).all()
                assert (want[n - n_live:, 0] + b < 255).all()
                _same(_run(ctx, jobs, ref, qer, b=b), want, jobs, ("equal jobs", n, n_live, b))
    finally:
        ctx.close()


def test_kswv_size_class_edges_equal_the_oracle():
    """Query lengths on both sides of every LDS size class (one launch each), as int16 and as int8 jobs, under the default penalties and mismatch 9."""
    jobs, ref, qer = kswv_class_edge_jobs()
    assert jobs.shape[0] == 2 * len(KSWV_CLASS_EDGE_BOTH) + len(KSWV_CLASS_EDGE_I16) == 70
    padded, is8 = _padded(jobs)
    cls = _cls(padded)
    assert int(jobs["len2"].max()) == 512 == KSWV_CLS[-1] - 16                # the last accepted length
    for c, size in enumerate(KSWV_CLS):
        # a job that fills the class: padded length == class size.  (The last class keeps 16 columns of slack behind the longest query the driver
        # accepts, 512 bases: there the fullest job is the one padded to 512.)
        top = size if c < len(KSWV_CLS) - 1 else size - 16
        assert ((padded == top) & (cls == c) & ~is8).any(), ("no int16 job fills class", size)
        assert top > 256 or ((padded == top) & (cls == c) & is8).any(), ("no int8 job fills class", size)
        if c > 0:
            # the first padded length past the previous class: one stripe more (8 columns for int16 jobs, 16 for int8 jobs)
            prev = KSWV_CLS[c - 1]
            assert ((padded == prev + 8) & (cls == c) & ~is8).any(), ("no int16 job just past class", prev)
            assert prev + 16 > 256 or ((padded == prev + 16) & (cls == c) & is8).any(), ("no int8 job just past class", prev)
    first = cls == 0
    assert 2 <= int(first.sum()) <= 64 and is8[first].any() and (~is8[first]).any()       # the first launch: one wavefront, both kinds of lane
    same_q = [p for p in np.unique(padded[first]) if is8[first & (padded == p)].any() and (~is8[first & (padded == p)]).any()]
    assert len(same_q) >= 2                                                               # ... also at equal padded lengths (16 and 64 columns)
    ctx = hipapi.Context(0)
    try:
        for pen in ({}, dict(b=9)):
            _same(_run(ctx, jobs, ref, qer, **pen), _want(jobs, ref, qer, **pen), jobs, ("class edges", pen))
    finally:
        ctx.close()


def test_kswv_partly_filled_wavefronts_equal_the_oracle():
    """One class that holds 1, 64, 65 and 129 jobs: the idle lanes of the last wavefront re-read the launch's first job with an empty window."""
    jobs, ref, qer = kswv_workload(n=129, seed=60, read_len=(150, 151), a=2)
    padded, is8 = _padded(jobs)
    assert (jobs["len2"] == 150).all() and not is8.any() and (padded == 152).all() and (_cls(padded) == 2).all()
    pen = dict(a=2, b=4)
    want = _want(jobs, ref, qer, **pen)
    assert int((want[:, 5] >= 0).sum()) > 60                                    # (most jobs run the second pass too)
    ctx = hipapi.Context(0)
    try:
        for n in (1, 64, 65, 129):
            assert (n + 63) // 64 == {1: 1, 64: 1, 65: 2, 129: 3}[n]
            _same(_run(ctx, jobs[:n], ref, qer, **pen), want[:n], jobs[:n], ("jobs", n))
    finally:
        ctx.close()


def test_kswv_field_and_size_limits():
    """The top of the 12-bit H / F fields (4 088 = 511 x 8), thresholds an int8 lane cannot hold, empty jobs, a long window beside a one-base one;
    what lies beyond the kernel's limits is refused, the last values inside them are served."""
    rng = np.random.default_rng(11)
    g = rng.integers(0, 4, size=40000, dtype=np.uint8)
    X16, X8 = XSUBO | XSTART | 19, XSUBO | XSTART | XBYTE | 19
    ctx = hipapi.Context(0)
    try:
        jobs, ref, qer = kswv_limit_jobs()
        want = _want(jobs, ref, qer, **KSWV_LIMIT_PEN)
        assert int(want[:, 0].max()) == 4088 == 511 * KSWV_LIMIT_PEN["a"] and 4088 < 1 << 12 <= 512 * KSWV_LIMIT_PEN["a"]
        is8 = (jobs["xtra"] & XBYTE) != 0
        assert int((is8 & ((jobs["xtra"] & 0xffff) > 255)).sum()) >= 3 and (jobs["len1"] == 0).any() and (jobs["len2"] == 0).any()
        _same(_run(ctx, jobs, ref, qer, **KSWV_LIMIT_PEN), want, jobs, "limits")
        _same(_run(ctx, jobs[3:], ref, qer), _want(jobs[3:], ref, qer), jobs[3:], "thresholds and empty jobs, default penalties")
        # a window of 8 000 bases and one of 1 base in the same wavefront (equal queries: the driver sorts them next to each other)
        q = g[3000:3100].copy()
        two = np.zeros(2, O.KSWV_JOB_DTYPE)
        two[0] = (0, 0, 8000, 100, X8, 0)
        two[1] = (8000, 0, 1, 100, X8, 0)
        ref2, qer2 = np.concatenate([g[:8000], g[3050:3051], np.zeros(8, np.uint8)]), np.concatenate([q, np.zeros(8, np.uint8)])
        assert np.unique(_padded(two)[0]).size == 1
        want = _want(two, ref2, qer2)
        assert want[0, 0] == 100 and want[0, 1] == 3099 and want[1, 0] <= 1
        _same(_run(ctx, two, ref2, qer2), want, two, "8 000-base window beside a 1-base window")
        # refused
        long_q, win = g[10000:10600], g[9900:10700]
        for what, (jb, r, qq), pen in (("len2 = 513", _job(win, long_q[:513], X16), {}), ("len2 = 512, a = 8", _job(win, long_q[:512], X16), dict(a=8)),
                                       ("int8 job of 256 bases", _job(win, long_q[:256], X8), {}), ("len1 = 32768", _job(g[:32768], long_q[:100], X16), {}),
                                       ("a = 128", _job(win, long_q[:30], X16), dict(a=128)), ("b = 128", _job(win, long_q[:30], X16), dict(b=128))):
            with pytest.raises(RuntimeError):
                _run(ctx, jb, r, qq, **pen)
                pytest.fail("served: " + what)
        # served: the last values inside the limits
        for what, (jb, r, qq), pen in (("len2 = 512", _job(win, long_q[:512], X16), dict(a=1)), ("int8 job of 255 bases", _job(win, long_q[:255], X8), dict(a=1)),
                                       ("len1 = 32767", _job(g[:32767], g[20000:20100], X16), {}),
                                       ("a = b = 127", _job(win, long_q[100:130], XSUBO | XSTART | 19 * 127), dict(a=127, b=127)),
                                       ("a = b = 127, int8", _job(win, long_q[100:130], XSUBO | XSTART | XBYTE | 100), dict(a=127, b=127))):
            want = _want(jb, r, qq, **pen)
            _same(_run(ctx, jb, r, qq, **pen), want, jb, what)
            if what == "len2 = 512":
                assert want[0].tolist() == [512, 611, 511, -1, -1, 100, 0]
            if what == "a = b = 127":
                assert want[0, [0, 1, 2, 5, 6]].tolist() == [30 * 127, 229, 29, 200, 0]
            if what == "a = b = 127, int8":
                assert want[0, 0] == 255
    finally:
        ctx.close()
