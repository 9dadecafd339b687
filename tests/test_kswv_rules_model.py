"""The rules of mate rescue -- the kswv kernels (reference src/kswv.cpp:372-712, :934-1199), their driver mem_sam_pe_batch (src/bwamem_pair.cpp:719-818) and the posing
step mem_sam_pe_batch_pre / mem_matesw_batch_pre (:660-716, :1060-1223) -- that k_kswv, k_mate_plan and k_mate_seq share, written once in
bwa-meme_amd/csrc/meme_kswv_rules.h: flags and job kind, the constants of a pass, the row rules (Block I, Block II, the stop, the last row, the saturated score), the
score2 scan, the second pass, the limits' class table, the launch plan, mem_infer_dir, the skip mask, the orientation windows, the job test, the query's bases; and the
seed filter's window swizzle of meme_ext_rules.h.  The headers are compiled here with g++ into a scalar kswv pair (plain row and column loops; the cell arithmetic is the
driver's own plain C, the GPU tests hold the device cell), a lane-less posing step and the plan.  They have to give what the compiled reference recorded
(tests/golden/kswv_golden.npz, matesw_golden.npz) and what the oracle gives on the edge, limit, class-edge and saturating job sets, exactly and for every job; the plan has
to keep every wavefront's rowMax slice apart and every launch inside its LDS class.  (The kernels themselves are checked in tests/test_gpu_kswv.py, test_gpu_mate.py and
test_gpu_ext.py.)"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
from common import (GOLDEN, KSWV_GOLDEN_SETS, KSWV_LIMIT_PEN, KSWV_SAT_SETS, kswv_class_edge_jobs, kswv_edge_jobs, kswv_limit_jobs, kswv_saturated_jobs, kswv_workload,
                    matesw_pose_workload)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''#include <vector>
#include "meme_ext_rules.h"
#include "meme_kswv_rules.h"
struct Pen { int a, b, o_del, e_del, o_ins, e_ins; };
struct PassOut { int raw, score, te, qe, score2, te2; };

// one pass of one job: rows over the target, columns over the padded query; H(i-1, .) and F in arrays, E and the diagonal along the row
static PassOut pass(bool is8, const uint8_t* t, const uint8_t* q, const KswvView& V, bool want2, const Pen& o) {
    const KswvPass P = kswv_pass_of(is8, V.xtra, o.a, o.b);
    const int quanta = kswv_padded(V.qlen, is8);
    std::vector<int> H((size_t)quanta + 1, 0), F((size_t)quanta + 1, 0);
    std::vector<unsigned short> rowmax((size_t)V.tlen + 1, (unsigned short)0x7000);      // (a row the scan must not read would win it)
    KswvLane L = kswv_lane0();
    int keep;
    for (int i = 0; i < V.tlen && !L.exited; ++i) {
        const int tb = t[V.target(i)];
        int e = 0, diag = 0, imax = 0, iqe = 0;
        for (int j = 0; j < quanta; ++j) {
            int sc = 0;
            if (j < V.qlen) { const int qc = q[V.query(j)]; sc = (tb > 3 || qc > 3) ? -1 : (tb == qc ? o.a : -o.b); }
            int m = diag + sc;
            m = m < P.cap ? m : P.cap;
            int h = m > e ? m : e;
            h = h > F[j] ? h : F[j];
            h = h > 0 ? h : 0;
            if (h > imax) { imax = h; iqe = j; }
            diag = H[j]; H[j] = h;
            const int e1 = h - (o.o_ins + o.e_ins), e2 = e - o.e_ins, f1 = h - (o.o_del + o.e_del), f2 = F[j] - o.e_del;
            e = e1 > e2 ? e1 : e2; e = e > 0 ? e : 0;
            F[j] = f1 > f2 ? f1 : f2; F[j] = F[j] > 0 ? F[j] : 0;
        }
        if (kswv_block1(P, L, i, imax, keep)) rowmax[(size_t)i - 1] = (unsigned short)keep;
        kswv_block2(P, L, i, imax, iqe);
        kswv_stop(P, L, i);
    }
    if (kswv_last_row(P, L, V.tlen, keep)) rowmax[(size_t)V.tlen - 1] = (unsigned short)keep;
    PassOut R{L.gmax, kswv_score(P, L.gmax), L.te, L.qe, -1, -1};
    if (want2) {
        const KswvScan S = kswv_scan_of(P, L, V.tlen);
        int mx = P.none, t2 = -1;
        for (int i = 0; i <= S.last; ++i) if (kswv_scan_row(S, i)) kswv_scan_take(kswv_rowmax_value(P, rowmax[(size_t)i]), i, mx, t2);
        R.score2 = kswv_score2(P, mx); R.te2 = t2;
    }
    return R;
}

extern "C" void t_kswv_batch(const meme_kswv_job* jobs, int64_t n, const uint8_t* ref, const uint8_t* qer, const Pen* o, meme_kswr* out) {
    for (int64_t k = 0; k < n; ++k) {
        const meme_kswv_job& J = jobs[k];
        const bool is8 = kswv_is8(J.xtra);
        const PassOut F = pass(is8, ref + J.idr, qer + J.idq, kswv_first_view(J.len1, J.len2, J.xtra), true, *o);
        meme_kswr R{F.score, F.te, F.qe, F.score2, F.te2, -1, -1};
        const bool again = kswv_second_runs(J.xtra, R.score);
        const PassOut B = pass(is8, ref + J.idr, qer + J.idq, kswv_second_view(again, J.len1, R), false, *o);
        kswv_start(R, again, B.raw, B.te, B.qe);
        out[k] = R;
    }
}

// mem_sam_pe_batch_pre over the worker batch of reads [first, first + count) (first even): gar, four entries per (end, record) looked at, and the jobs in its order
struct MJob { int64_t rb; int32_t read, len1, len2, xtra, is_rev, pad; };
struct MOpt { int32_t a, pen_unpaired, max_matesw, min_seed_len; };
extern "C" int64_t t_mate_pose(const meme_mate_reg* regs, const int64_t* reg_off, int64_t first, int64_t count, const int32_t* read_len, const meme_pestat* pes, int64_t l_pac,
                               const int64_t* contig_off, const int* contig_len, int n_contigs, const MOpt* opt, int32_t* gar, int64_t* n_gar, MJob* jobs) {
    int64_t nq = 0, nj = 0;
    for (int64_t r = first; r < first + count; ++r) {
        const int64_t m = r ^ 1;
        const meme_mate_reg* a = regs + reg_off[r];
        const int na = (int)(reg_off[r + 1] - reg_off[r]), nm = (int)(reg_off[m + 1] - reg_off[m]), l_ms = read_len[m];
        int taken = 0;
        for (int j = 0; j < na && taken < opt->max_matesw; ++j) {
            if (!(a[j].score >= a[0].score - opt->pen_unpaired)) continue;
            const int skip = mate_skip_mask(pes, l_pac, a[j].rb, regs + reg_off[m], nm);
            int rid = -1;
            for (int o = 0; o < 4; ++o) {
                int idx = -1;
                if (mate_tries(skip, o)) {
                    const MateWindow W = mate_window(o, pes[o], a[j].rb, l_ms, l_pac);
                    int64_t rb = W.rb, re = W.re;
                    if (rb < re) rid = bns_clamp_to_mid(l_pac, contig_off, contig_len, n_contigs, (rb + re) >> 1, rb, re);
                    if (mate_is_job(a[j].rid, rid, rb, re, opt->min_seed_len)) {
                        jobs[nj] = MJob{rb, (int32_t)m, (int32_t)(re - rb), l_ms, mate_xtra(l_ms, opt->a, opt->min_seed_len), W.is_rev, 0};
                        idx = (int)nj++;
                    }
                }
                gar[4 * nq + o] = idx;
            }
            ++nq; ++taken;
        }
    }
    *n_gar = 4 * nq;
    return nj;
}
// the jobs' sequences back to back
extern "C" void t_mate_seqs(const MJob* jobs, int64_t n, const uint8_t* text, const uint8_t* reads, const int64_t* read_off, uint8_t* ref, uint8_t* qer) {
    for (int64_t k = 0; k < n; ++k) {
        for (int l = 0; l < jobs[k].len1; ++l) *ref++ = text[jobs[k].rb + l];
        for (int l = 0; l < jobs[k].len2; ++l) *qer++ = mate_query_base(reads + read_off[jobs[k].read], jobs[k].len2, l, jobs[k].is_rev != 0);
    }
}

// the plan flat: launches as (first, count, columns, w0) rows; returns the number of launches
extern "C" int t_kswv_plan(const meme_kswv_job* jobs, int n, int32_t* order, int64_t* launches, int64_t* rm_off, int64_t* n_waves, int64_t* rows_total, int32_t* padded, int32_t* cls) {
    const KswvPlan P = kswv_plan(jobs, n);
    for (size_t k = 0; k < P.order.size(); ++k) order[k] = P.order[k];
    for (size_t k = 0; k < P.launches.size(); ++k) {
        launches[4 * k] = P.launches[k].first; launches[4 * k + 1] = P.launches[k].count; launches[4 * k + 2] = P.launches[k].columns; launches[4 * k + 3] = (int64_t)P.launches[k].w0;
    }
    for (size_t k = 0; k < P.rm_off.size(); ++k) rm_off[k] = P.rm_off[k];
    *n_waves = (int64_t)P.rm_off.size(); *rows_total = P.rows_total;
    for (int k = 0; k < n; ++k) { padded[k] = kswv_padded(jobs[k].len2, kswv_is8(jobs[k].xtra)); cls[k] = kswv_cls_of(padded[k]); }
    return (int)P.launches.size();
}

// the bases mem_seed_sw's window holds at positions p[0..n) of the fwd + rc text
extern "C" void t_flt_bases(const uint8_t* text, int64_t l_pac, int64_t n, const int64_t* p, uint8_t* out) {
    for (int64_t k = 0; k < n; ++k) {
        const FltBase B = flt_base_index(l_pac, p[k]);
        const int c = B.pos < l_pac << 1 ? text[B.pos] & 3 : 0;
        out[k] = (uint8_t)(B.complement ? 3 - c : c);
    }
}
'''

_p = lambda a: C.c_void_p(a.ctypes.data)
MJOB = np.dtype([("rb", "<i8"), ("read", "<i4"), ("len1", "<i4"), ("len2", "<i4"), ("xtra", "<i4"), ("is_rev", "<i4"), ("pad", "<i4")])
assert MJOB == O.MATE_JOB_DTYPE

# the driver's arithmetic restated independently (the same few lines tests/test_gpu_kswv.py holds the device against)
KSWV_CLS = (64, 128, 160, 256, 384, 528)


def _padded(jobs):
    is8 = (jobs["xtra"] & O.KSW_XBYTE) != 0
    L = jobs["len2"].astype(np.int64)
    return np.where(is8, (L + 15) // 16 * 16, (L + 7) // 8 * 8), is8


def _cls(padded):
    return np.searchsorted(np.array(KSWV_CLS), padded, side="left")         # the first class that holds the padded query


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("kswv_rules")
    src = d / "t_kswv_rules.cpp"
    src.write_text(DRIVER)
    so = str(d / "libt_kswv_rules.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"),
                    str(src), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.t_mate_pose.restype = C.c_int64
    return lib


def test_header_compiles_alone(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "meme_kswv_rules.h"\n')
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-c", "-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"), str(src),
                    "-o", str(tmp_path / "alone.o")], check=True)


# ---- the job sets (generated once) ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden_jobs(name):
    kw = {n: k for n, k, _ in KSWV_GOLDEN_SETS}[name]
    return kswv_workload(**kw)


@functools.lru_cache(maxsize=None)
def _partly_filled():
    return kswv_workload(n=129, seed=60, read_len=(150, 151), a=2)


ORACLE_SETS = {
    "edges": (kswv_edge_jobs, [{}]),
    "limits": (kswv_limit_jobs, [KSWV_LIMIT_PEN]),
    "class_edges": (kswv_class_edge_jobs, [{}, dict(b=9)]),
    "saturated_64": (lambda: kswv_saturated_jobs(64), [dict(b=9), dict(b=6)]),
    "saturated_130": (lambda: kswv_saturated_jobs(130), [dict(b=9), dict(b=6)]),
    "saturated_64_one_live": (lambda: kswv_saturated_jobs(64, n_live=1), [dict(b=9), dict(b=6)]),
}


def _pen(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1):
    return np.array([a, b, o_del, e_del, o_ins, e_ins], np.int32)


def _pairs(lib, jobs, ref, qer, **pen):
    jobs = np.ascontiguousarray(jobs, O.KSWV_JOB_DTYPE)
    ref = np.concatenate([np.ascontiguousarray(ref, np.uint8), np.zeros(8, np.uint8)])
    qer = np.concatenate([np.ascontiguousarray(qer, np.uint8), np.zeros(8, np.uint8)])
    out = np.zeros(jobs.shape[0], O.KSWR_DTYPE)
    pn = _pen(**pen)
    lib.t_kswv_batch(_p(jobs), C.c_int64(jobs.shape[0]), _p(ref), _p(qer), _p(pn), _p(out))
    return out.view(np.int32).reshape(-1, 7)


def _same(got, want, jobs, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), jobs[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


# ---- a scalar kswv pair ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [name for name, _, _ in KSWV_GOLDEN_SETS])
def test_scalar_pair_equals_the_reference_golden(driver, name):
    """All seven kswr fields of every job of the set == the compiled reference's AVX-512 kernels (11 500 jobs over the six sets, the three saturating ones among them)."""
    G = np.load(os.path.join(GOLDEN, "kswv_golden.npz"))
    pen = {n: p for n, _, p in KSWV_GOLDEN_SETS}[name]
    jobs, ref, qer = _golden_jobs(name)
    assert jobs.shape[0] == G[name].shape[0] and sum(G[n].shape[0] for n, _, _ in KSWV_GOLDEN_SETS) == 11500
    if name in KSWV_SAT_SETS:
        assert int((G[name][:, 0] == 255).sum()) > 100
    _same(_pairs(driver, jobs, ref, qer, **pen), G[name], jobs, name)


@pytest.mark.parametrize("name", sorted(ORACLE_SETS))
def test_scalar_pair_equals_the_oracle_on_edge_limit_class_edge_and_saturated_jobs(driver, name):
    make, pens = ORACLE_SETS[name]
    jobs, ref, qer = make()
    for pen in pens:
        want = O.kswv_batch(jobs, ref, qer, threads=4, **pen)[0].view(np.int32).reshape(-1, 7)
        if name.startswith("saturated"):
            assert int((want[:, 0] == 255).sum()) >= jobs.shape[0] - 1
        _same(_pairs(driver, jobs, ref, qer, **pen), want, jobs, (name, pen))


# ---- a scalar posing step --------------------------------------------------------------------------------------------------------------------
def _pose(lib, W, first, count, a=1, pen_unpaired=17, max_matesw=50, min_seed_len=19):
    regs = np.ascontiguousarray(W["regs"], O.MATE_REG_DTYPE)
    reg_off = np.ascontiguousarray(W["reg_off"], np.int64)
    read_len = np.ascontiguousarray(W["read_len"], np.int32)
    pes4 = np.zeros((4, 4), np.int32)
    pes4[:, :3] = np.asarray(W["pes"], np.int32).reshape(4, 3)
    contig_off = np.ascontiguousarray(W["contig_off"], np.int64)
    contig_len = np.ascontiguousarray(W["contig_len"], np.int32)
    opt = np.array([a, pen_unpaired, max_matesw, min_seed_len], np.int32)
    nrec = int(reg_off[first + count] - reg_off[first])
    gar = np.full(4 * nrec + 8, -7, np.int32)
    jobs = np.zeros(4 * nrec + 8, MJOB)
    n_gar = C.c_int64(0)
    n = lib.t_mate_pose(_p(regs), _p(reg_off), C.c_int64(first), C.c_int64(count), _p(read_len), _p(pes4), C.c_int64(int(W["l_pac"])), _p(contig_off), _p(contig_len),
                        C.c_int(contig_off.shape[0]), _p(opt), _p(gar), C.byref(n_gar), _p(jobs))
    return gar[:n_gar.value].copy(), jobs[:n].copy()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_scalar_posing_equals_the_reference_golden(driver, tag):
    """gar, len1, len2 and xtra of every worker batch == what the compiled reference's mem_sam_pe_batch_pre posed."""
    z = np.load(os.path.join(GOLDEN, "matesw_golden.npz"))
    W = {k: z[tag + "_" + k] for k in ("contig_off", "contig_len", "read_len", "regs", "reg_off", "pes")}
    W["l_pac"] = int(z[tag + "_l_pac"])
    n = W["read_len"].shape[0]
    assert z[tag + "_len1"].shape[0] > 500
    for b, first in enumerate(range(0, n, 512)):
        gar, jobs = _pose(driver, W, first, min(512, n - first))
        assert np.array_equal(gar, z[tag + "_gar"][z[tag + "_gar_off"][b]:z[tag + "_gar_off"][b + 1]]), ("gar of batch", b)
        j0, j1 = z[tag + "_job_off"][b], z[tag + "_job_off"][b + 1]
        for f in ("len1", "len2", "xtra"):
            assert np.array_equal(jobs[f], z[tag + "_" + f][j0:j1]), (f, "batch", b)


# the six parameter sets of tests/test_gpu_mate.py::test_mate_rescue_on_the_device_equals_the_oracle
POSE_SETS = [(321, [(10, 2000, 0)] * 4, {}), (322, [(0, 0, 1)] * 4, {}), (323, [(50, 500, 0), (120, 680, 0), (100, 900, 0), (0, 0, 1)], dict(max_matesw=2, pen_unpaired=40)),
             (324, None, dict(min_seed_len=40, a=2, b=5)), (325, [(0, 0, 1), (200, 260, 0), (0, 0, 1), (150, 151, 0)], dict(batch_reads=64)),
             (326, [(10, 2000, 0)] * 4, dict(b=70, read_len=(236, 250)))]


@pytest.mark.parametrize("seed,pes,kw", POSE_SETS)
def test_scalar_posing_equals_the_oracle(driver, seed, pes, kw):
    kw = dict(kw)
    read_len = kw.pop("read_len", None)
    br = kw.pop("batch_reads", 512)
    W = matesw_pose_workload(seed=seed, pes=pes, n_pairs=700, **({} if read_len is None else dict(read_len=read_len)))
    okw = {k: v for k, v in kw.items() if k in ("a", "pen_unpaired", "max_matesw", "min_seed_len")}
    n = W["read_len"].shape[0]
    n_jobs = 0
    for b, first in enumerate(range(0, n, br)):
        count = min(br, n - first)
        want_gar, want_jobs = O.matesw_pose(W["regs"], W["reg_off"], first, count, W["read_len"], W["pes"], int(W["l_pac"]), W["contig_off"], W["contig_len"], **okw)
        gar, jobs = _pose(driver, W, first, count, **okw)
        assert np.array_equal(gar, want_gar), ("gar of batch", b)
        assert np.array_equal(jobs, want_jobs), ("jobs of batch", b)
        n_jobs += jobs.shape[0]
        if seed == 321 and jobs.shape[0]:                                     # the sequences of every posed job of this set
            kj, ref, qer = O.matesw_job_seqs(want_jobs, W["text"], W["reads"], W["read_off"])
            got_ref, got_qer = np.zeros(ref.shape[0] + 8, np.uint8), np.zeros(qer.shape[0] + 8, np.uint8)
            text, reads, read_off = np.ascontiguousarray(W["text"], np.uint8), np.ascontiguousarray(W["reads"], np.uint8), np.ascontiguousarray(W["read_off"], np.int64)
            driver.t_mate_seqs(_p(jobs), C.c_int64(jobs.shape[0]), _p(text), _p(reads), _p(read_off), _p(got_ref), _p(got_qer))
            assert np.array_equal(got_ref[:-8], ref) and np.array_equal(got_qer[:-8], qer), ("sequences of batch", b)
            assert jobs["is_rev"].any() and (~(jobs["is_rev"] != 0)).any() and (qer == 4).any()
    assert (n_jobs > 0) == (seed != 322)                                      # (322: the statistics rule every orientation out)


# ---- the launch plan ---------------------------------------------------------------------------------------------------------------------------
def _plan_sets():
    sets = [("golden " + name, functools.partial(_golden_jobs, name)) for name, _, _ in KSWV_GOLDEN_SETS]
    sets += [(name, make) for name, (make, _) in sorted(ORACLE_SETS.items())]
    sets += [("one class, %d jobs" % n, functools.partial(lambda n: tuple(x[:n] if i == 0 else x for i, x in enumerate(_partly_filled())), n)) for n in (1, 64, 65, 129)]
    return sets


@pytest.mark.parametrize("what,make", _plan_sets(), ids=[w for w, _ in _plan_sets()])
def test_plan_keeps_wavefronts_apart_and_launches_inside_their_class(driver, what, make):
    jobs = np.ascontiguousarray(make()[0], O.KSWV_JOB_DTYPE)
    n = jobs.shape[0]
    order = np.zeros(n, np.int32); padded = np.zeros(n, np.int32); cls = np.zeros(n, np.int32)
    launches = np.zeros((8, 4), np.int64); rm_off = np.zeros(n + 8, np.int64)
    n_waves, rows_total = C.c_int64(0), C.c_int64(0)
    nl = driver.t_kswv_plan(_p(jobs), C.c_int(n), _p(order), _p(launches), _p(rm_off), C.byref(n_waves), C.byref(rows_total), _p(padded), _p(cls))
    want_padded, _ = _padded(jobs)
    assert np.array_equal(padded, want_padded) and np.array_equal(cls, _cls(want_padded))
    assert np.array_equal(np.sort(order), np.arange(n))                                   # a permutation
    launches = launches[:nl]
    bounds = np.concatenate([rm_off[:n_waves.value], [rows_total.value]])
    assert (np.diff(bounds) > 0).all() and bounds[0] == 0                                 # slices in order, none empty: they do not overlap
    assert launches[0, 0] == 0 and np.array_equal(launches[1:, 0], np.cumsum(launches[:, 1])[:-1]) and int(launches[:, 1].sum()) == n
    assert np.unique(cls).size == nl
    w = 0
    for first, count, columns, w0 in launches.tolist():
        ids = order[first:first + count]
        c = np.unique(cls[ids])
        assert c.size == 1 and KSWV_CLS[int(c[0])] == columns and int((cls == c[0]).sum()) == count       # exactly the jobs of one class
        assert (padded[ids] <= columns).all() and (columns + 2) * 256 <= 160 * 1024
        key = np.stack([padded[ids].astype(np.int64), -jobs["len1"][ids].astype(np.int64)], axis=1)
        assert (np.diff(padded[ids]) >= 0).all()
        assert all(tuple(key[k]) <= tuple(key[k + 1]) for k in range(count - 1))          # len1 descending inside equal padded length
        assert w0 == w
        for k in range(0, count, 64):
            rows = int(jobs["len1"][ids[k:k + 64]].max())
            assert bounds[w + 1] - bounds[w] >= rows + 1, (what, w)
            w += 1
    assert w == n_waves.value
    if what.startswith("one class"):
        assert nl == 1 and w == (n + 63) // 64 and (padded == 152).all() and (cls == 2).all()


# ---- the seed filter's window swizzle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l_pac", [37, 40, 203])
def test_seed_filter_window_bases_are_the_ones_the_oracle_reads(driver, l_pac):
    """flt_base_index against orc_seed_sw_window (what tests/test_ext_rules_model.py aligns with): a one-base query against the one-base window at p scores the
    match score exactly when the query is the window's base -- at every position of the fwd + rc text, l_pac and both ends of the text among them."""
    rng = np.random.default_rng(l_pac)
    g = rng.integers(0, 4, size=l_pac, dtype=np.uint8)
    text = np.concatenate([g, (3 - g[::-1]).astype(np.uint8)])
    pos = np.arange(2 * l_pac, dtype=np.int64)
    assert {0, l_pac - 1, l_pac, 2 * l_pac - 1} <= set(pos.tolist())
    got = np.zeros(pos.shape[0], np.uint8)
    driver.t_flt_bases(_p(text), C.c_int64(l_pac), C.c_int64(pos.shape[0]), _p(pos), _p(got))
    oo = O.default_ext_opt()
    sw = O.lib().orc_seed_sw_window
    sw.restype = C.c_int
    want = np.full(pos.shape[0], 255, np.uint8)
    for p in pos.tolist():
        hit = [c for c in range(4) if sw(C.c_int(1), _p(np.array([c], np.uint8)), _p(text), C.c_int64(l_pac), C.c_int64(p), C.c_int(1), C.byref(oo)) == oo.a]
        assert len(hit) == 1, (p, hit)
        want[p] = hit[0]
    assert np.array_equal(got, want)
    assert (got != text).any()                                                            # (the swizzle is not the identity)
