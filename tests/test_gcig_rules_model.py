"""The rules of ksw_global2 under bwa_gen_cigar2 (reference src/ksw.cpp:560-670, src/bwa.cpp:262-316) that the CIGAR kernels of meme_gcig.hip share, written
once in bwa-meme_amd/csrc/meme_gcig_rules.h: the scoring entry, the band preamble, n_col and a row's band, the borders of the matrix, the cell, the walk back and
the writer of its operations.  The header is compiled here with g++ into a scalar driver -- a plain row and column loop, H and E as int arrays, F carried along
the row, every rule taken from the header -- which has to give score and operations the compiled reference recorded (tests/golden/gcig_golden.npz,
gencig_golden.npz) and the oracle's on generated jobs, exactly.  In every cell the driver also holds the forms only the kernels use against that loop: F read
off a scan of 64-column chunks (gcig_scan_key / gcig_scan_f), H(i-1, -1) and the end of the row above as the group kernel computes them (gcig_corner,
gcig_end_above), and the walk with its index as int.  (The kernels themselves are checked in tests/test_gpu_gcig.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
from common import GOLDEN, cjob_band, gcig_workload, gencig_workload
from pymeme import hipapi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''#include <stddef.h>
#include <climits>
#include <vector>
#include "meme_gcig_rules.h"
// score (INT_MIN: one of the kernels' forms disagrees with the plain loop); the operations in CIGAR order to cig, their number to *n_cigar
static int global2(int qlen, const uint8_t* query, int tlen, const uint8_t* target, int w, const meme_bsw_opt& o, uint32_t* cig, int* n_cigar) {
    const int oe_del = o.o_del + o.e_del, oe_ins = o.o_ins + o.e_ins, n_col = gcig_n_col(qlen, w);
    std::vector<int> H(qlen + 2), E(qlen + 2);
    std::vector<uint8_t> z((size_t)n_col * tlen);
    bool forms = true;
    for (int j = 0; j <= qlen; ++j) { H[j] = gcig_row0(j, w, o.o_ins, o.e_ins); E[j] = GCIG_MINUS_INF; }
    for (int i = 0; i < tlen; ++i) {
        const int beg = gcig_beg(i, w), end = gcig_end(i, w, qlen);
        int h1 = gcig_left(i, beg, o.o_del, o.e_del), f = GCIG_MINUS_INF, carry = 0, below = 0;
        for (int j = beg; j < end; ++j) {
            const int m = H[j] + gcig_score(target[i], query[j], o.a, o.b), e = E[j], c = (j - beg) & 63;
            if (c == 0) { carry = f; below = GCIG_SCAN_FLOOR; }
            forms = forms && gcig_scan_f(below, carry, o.e_ins, c) == f && (j != 0 || H[0] == gcig_corner(i, o.o_del, o.e_del)) &&
                    (j < gcig_end_above(i, w, qlen) || e == GCIG_MINUS_INF);
            const int key = gcig_scan_key(true, m, oe_ins, o.e_ins, c);
            below = below > key ? below : key;
            const GcigCell x = gcig_cell(m, e, f, oe_del, o.e_del, oe_ins, o.e_ins);
            H[j] = h1; h1 = x.h; E[j] = x.e; f = x.f;
            z[(size_t)i * n_col + (j - beg)] = (uint8_t)x.d;
        }
        H[end] = h1; E[end] = GCIG_MINUS_INF;
    }
    const int cap = qlen + tlen + 2;
    std::vector<uint32_t> scratch(cap);
    GcigOps ops{scratch.data(), cap, true}, dry{nullptr, cap, false};
    gcig_walk<int64_t>(tlen, qlen, w, n_col, [&](int64_t x) { return (int)z[x]; }, ops);
    gcig_walk<int>(tlen, qlen, w, n_col, [&](int x) { return (int)z[x]; }, dry);
    forms = forms && dry.n == ops.n && gcig_scan_key(false, 0, oe_ins, o.e_ins, 0) == GCIG_SCAN_FLOOR;
    for (int k = 0; k < ops.n; ++k) cig[k] = scratch[ops.cigar_off() + k];
    *n_cigar = ops.n;
    return forms ? H[qlen] : INT_MIN;
}
extern "C" int t_global2(int qlen, const uint8_t* query, int tlen, const uint8_t* target, int w, const meme_bsw_opt* o, uint32_t* cig, int* n_cigar) {
    return global2(qlen, query, tlen, target, w, *o, cig, n_cigar);
}
extern "C" void t_band(int n, const int* qlen, const int* tlen, const int* w_, const meme_bsw_opt* o, int* w) {
    for (int k = 0; k < n; ++k) w[k] = gcig_band(qlen[k], tlen[k], w_[k], *o);
}
// a call of bwa_gen_cigar2 on the (already reversed) sequences: the band from the preamble, the shortcut's one M and summed score or the alignment
extern "C" int t_gen_cigar(int qlen, const uint8_t* query, int tlen, const uint8_t* target, int w_, const meme_bsw_opt* o, uint32_t* cig, int* n_cigar) {
    const int w = gcig_band(qlen, tlen, w_, *o);
    if (w >= 0) return global2(qlen, query, tlen, target, w, *o, cig, n_cigar);
    int score = 0;
    for (int j = 0; j < qlen; ++j) score += gcig_score(target[j], query[j], o->a, o->b);
    GcigOps ops{cig, 1, true};
    ops.push(0, qlen);
    ops.flush();
    *n_cigar = ops.n;
    return score;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("gcig_rules")
    src = d / "t_gcig_rules.cpp"
    src.write_text(DRIVER)
    so = str(d / "libt_gcig_rules.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"),
                    str(src), "-o", so], check=True)
    lib = C.CDLL(so)

    def align(fn, q, t, w, pen=(1, 4, 6, 1, 6, 1)):
        """(score, operations) of the driver's t_global2 (w: the band) or t_gen_cigar (w: the band argument w_); pen: a, b, o_del, e_del, o_ins, e_ins"""
        a, b, od, ed, oi, ei = pen
        q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
        cig = np.zeros(q.shape[0] + t.shape[0] + 2, np.uint32)
        n = C.c_int(0)
        sc = getattr(lib, fn)(C.c_int(q.shape[0]), C.c_void_p(q.ctypes.data), C.c_int(t.shape[0]), C.c_void_p(t.ctypes.data), C.c_int(int(w)),
                              C.byref(hipapi.BswOpt(od, ed, oi, ei, 100, 5, a, b)), C.c_void_p(cig.ctypes.data), C.byref(n))
        return sc, cig[:n.value]

    def band(qlen, tlen, w_, pen):
        """gcig_band of the three int arrays"""
        a, b, od, ed, oi, ei = pen
        arg = [np.ascontiguousarray(x, np.int32) for x in (qlen, tlen, w_)]
        w = np.zeros(arg[0].shape[0], np.int32)
        lib.t_band(C.c_int(w.shape[0]), *(C.c_void_p(x.ctypes.data) for x in arg), C.byref(hipapi.BswOpt(od, ed, oi, ei, 100, 5, a, b)), C.c_void_p(w.ctypes.data))
        return w
    align.band = band
    return align


def test_shared_rules_equal_the_reference_golden(driver):
    _, _, jobs, seqs = gcig_workload()
    G = np.load(os.path.join(GOLDEN, "gcig_golden.npz"))
    off = np.concatenate([[0], np.cumsum(G["n_cigar"])])
    assert jobs.shape[0] == G["score"].shape[0]
    for k, (J, (q, t)) in enumerate(zip(jobs, seqs)):
        sc, cg = driver("t_global2", q, t, int(J["w"]))
        assert sc == int(G["score"][k]) and cg.shape[0] == int(G["n_cigar"][k]) and np.array_equal(cg, G["cigars"][off[k]:off[k + 1]]), k


def test_shared_rules_and_preamble_equal_the_reference_golden_of_gen_cigar(driver):
    g, reads, calls = gencig_workload()
    G = np.load(os.path.join(GOLDEN, "gencig_golden.npz"))
    off = np.concatenate([[0], np.cumsum(G["n_cigar"])])
    text = hipapi.fwd_rc_text(g)
    shortcuts = 0
    assert calls.shape[0] == G["score"].shape[0]
    for k, J in enumerate(calls):
        q = reads[int(J["read"])][int(J["qb"]):int(J["qb"]) + int(J["qlen"])]
        t = text[int(J["rb"]):int(J["rb"]) + int(J["tlen"])]
        if int(J["rb"]) >= g.shape[0]:
            q, t = q[::-1], t[::-1]
        sc, cg = driver("t_gen_cigar", q, t, int(J["w_"]))
        assert sc == int(G["score"][k]) and np.array_equal(cg, G["cigars"][off[k]:off[k + 1]]), k
        if int(J["qlen"]) == int(J["tlen"]) and int(J["w_"]) == 0:
            shortcuts += 1
            assert cg.shape[0] == 1 and int(cg[0]) == int(J["qlen"]) << 4, k
    assert shortcuts > calls.shape[0] // 4


@pytest.mark.parametrize("pen", [(2, 3, 4, 2, 7, 1), (1, 9, 1, 1, 1, 1)])
def test_shared_rules_equal_the_oracle_with_other_penalties(driver, pen):
    _, _, jobs, seqs = gcig_workload(n=800, seed=91)
    for k, (J, (q, t)) in enumerate(zip(jobs, seqs)):
        sc, cg = O.ksw_global2(q, t, int(J["w"]), *pen)
        got = driver("t_global2", q, t, int(J["w"]), pen)
        assert got[0] == sc and np.array_equal(got[1], cg), (k, pen)


def test_band_preamble_around_the_rounding_of_its_division(driver):
    """gcig_band against the host model of the preamble (common.cjob_band: what tests/test_gpu_gcig.py predicts every call's class from), for every query length
    1 .. 259 -- so every length at which ((qlen + 1) >> 1) * a - o crosses a multiple of e and (int)(double / e + 1.) steps --, tlen - qlen in -3 .. 3 and ten
    band arguments, with extension penalties of 1, 2, 3 and 7 and with gap-open penalties above the numerator (negative quotients: (int) rounds towards zero)."""
    for pen in ((1, 4, 6, 1, 6, 1), (2, 3, 4, 2, 7, 3), (3, 1, 5, 3, 2, 2), (1, 4, 40, 7, 90, 3), (5, 4, 1, 7, 0, 2)):
        a, _, od, ed, oi, ei = pen
        qlen, dl, w_ = (x.reshape(-1) for x in np.meshgrid(np.arange(1, 260), np.arange(-3, 4), np.array([0, 1, 2, 3, 5, 10, 30, 100, 200, 400]), indexing="ij"))
        tlen = qlen + dl
        keep = tlen >= 1
        qlen, tlen, w_ = qlen[keep], tlen[keep], w_[keep]
        want = cjob_band(qlen, tlen, w_, a, od, ed, oi, ei)
        got = driver.band(qlen, tlen, w_, pen)
        assert np.array_equal(got, want), (pen, np.flatnonzero(got != want)[:5])
        # the shortcut, and calls whose band is neither the argument nor the floor |tlen - qlen| + 3: the division decides it
        assert int((want == -1).sum()) > 0 and int(((want > np.abs(tlen - qlen) + 3) & (want < w_)).sum()) > 100, pen
