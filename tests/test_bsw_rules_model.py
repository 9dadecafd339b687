"""The row rules of scalarBandedSWA == ksw_extend2 (reference src/bandedSWA.cpp:116-237) that the three banded-SW kernels of meme_bsw.hip share,
written once in bwa-meme_amd/csrc/meme_bsw_rules.h: the band cap, the first row, the head of a row, the end of a row (gscore, the m == 0 exit, the
maximum, z-drop), the next row's end and the store of the six outputs.  The header is compiled here with g++ into a scalar driver -- a plain
column loop over H and E as int arrays, the cell and the band trimming written out, every row rule taken from the header -- which has to give
the six outputs the compiled reference recorded (tests/golden/bsw_golden.npz) and the oracle's on generated batches, exactly.
(The kernels themselves are checked in tests/test_gpu_bsw.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bsw_gen
import oracle_py as O
from common import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''#include <vector>
#include "meme_bsw_rules.h"
extern "C" void t_bsw_batch(meme_seqpair* pairs, const uint8_t* ref, const uint8_t* qer, int n, int w_arg, const meme_bsw_opt* opt) {
    const meme_bsw_opt o = *opt;
    const int oe_del = o.o_del + o.e_del, oe_ins = o.o_ins + o.e_ins;
    std::vector<int> H, E;
    for (int k = 0; k < n; ++k) {
        meme_seqpair* P = &pairs[k];
        const int qlen = P->len2, tlen = P->len1, h0 = P->h0;
        const uint8_t *query = qer + P->idq, *target = ref + P->idr;
        H.assign(qlen + 2, 0); E.assign(qlen + 2, 0);
        for (int j = 0; j <= qlen; ++j) H[j] = bsw_row0(h0, oe_ins, o.e_ins, j);
        const int w = bsw_band_cap(o, qlen, w_arg);
        BswBest best(h0);
        int beg = 0, end = qlen;
        for (int i = 0; i < tlen; ++i) {
            int f = 0, m = 0, mj = -1;
            const int beg_v = bsw_band_beg(beg, i, w), end_v = bsw_band_end(end, i, w, qlen);       // the row head's two forms must agree
            int h1 = bsw_row_head(i, w, qlen, h0, o.o_del, o.e_del, beg, end);
            if (beg_v != beg || end_v != end || bsw_first_h1(beg, i, h0, o.o_del, o.e_del) != h1) { best.max = INT32_MIN; break; }
            for (int j = beg; j < end; ++j) {
                int M = H[j], e = E[j];
                H[j] = h1;
                const int sc = target[i] > 3 || query[j] > 3 ? -1 : (target[i] == query[j] ? o.a : -o.b);
                M = M ? M + sc : 0;
                int h = M > e ? M : e;
                h = h > f ? h : f;
                h1 = h;
                mj = m > h ? mj : j;
                m = m > h ? m : h;
                int t = M - oe_del;
                t = t > 0 ? t : 0;
                e -= o.e_del;
                E[j] = e > t ? e : t;
                t = M - oe_ins;
                t = t > 0 ? t : 0;
                f -= o.e_ins;
                f = f > t ? f : t;
            }
            H[end] = h1; E[end] = 0;
            if (bsw_row_end(best, i, m, mj, h1, beg, end, qlen, o.e_del, o.e_ins, o.zdrop)) break;
            int j = beg;
            while (j < end && H[j] == 0 && E[j] == 0) ++j;
            beg = j;
            for (j = end; j >= beg && H[j] == 0 && E[j] == 0; --j) {}
            end = bsw_next_end(j, qlen);
        }
        best.store(P);
    }
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("bsw_rules")
    src = d / "t_bsw_rules.cpp"
    src.write_text(DRIVER)
    so = str(d / "libt_bsw_rules.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"),
                    str(src), "-o", so], check=True)
    lib = C.CDLL(so)

    def run(pairs, ref, qer, w, p):
        """the six outputs of the driver for a batch; p: the oracle's parameters (same eight fields, same order as meme_bsw_opt)"""
        got = pairs.copy()
        ref = np.ascontiguousarray(ref, np.uint8); qer = np.ascontiguousarray(qer, np.uint8)
        lib.t_bsw_batch(C.c_void_p(got.ctypes.data), C.c_void_p(ref.ctypes.data), C.c_void_p(qer.ctypes.data), C.c_int(got.shape[0]), C.c_int(w), C.byref(p))
        return bsw_gen.outputs(got)
    return run


@pytest.mark.parametrize("w,eb", [(100, 5), (100, 0), (200, 5), (200, 0)])
def test_shared_row_rules_equal_the_reference_golden(driver, w, eb):
    z = np.load(os.path.join(GOLDEN, "bsw_golden.npz"))
    pairs = z["pairs"].astype(O.SEQPAIR_DTYPE).copy()
    assert np.array_equal(driver(pairs, z["ref"], z["qer"], w, O.default_bsw_params(eb)), z["scalar_w%d_eb%d" % (w, eb)])


@pytest.mark.parametrize("kw", [dict(), dict(max_q=300, sub=0.06, indel=0.02), dict(h0_max=900)], ids=["default", "long_noisy", "large_h0"])
def test_shared_row_rules_equal_the_oracle(driver, kw):
    pairs, ref, qer = bsw_gen.make_pairs(2000, seed=41, **kw)
    for w in (100, 7):
        want = pairs.copy()
        O.bsw_batch(want, ref, qer, w, O.default_bsw_params(5), threads=2)      # (2 000 pairs: not worth a pool of every core)
        assert np.array_equal(driver(pairs, ref, qer, w, O.default_bsw_params(5)), bsw_gen.outputs(want)), (kw, w)
