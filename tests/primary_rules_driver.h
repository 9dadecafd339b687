// A scalar host driver of bwa-meme_amd/csrc/meme_primary_rules.h: mem_mark_primary_se, mem_reorder_primary5 and mem_approx_mapq_se for the reads of a batch,
// one after the other.  tests/test_primary_rules_model.py compiles it with g++ into a shared object; scripts/primary_rules_main.cpp wraps it in a program of
// its own (for a sanitizer build).  Nothing here decides a result: the two orders are klib's introsort (meme_ksort.h) over a column of indices with the
// header's less-than functions, the walk is a scan for the lowest index that is not secondary and overlaps, the logarithms are a table the host's libm
// fills, and every decision is a call into the header.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

#include "meme_primary_rules.h"

namespace pri_driver {

struct Stack {                               // ks_introsort's stack
    std::vector<int> v;
    void push(int l, int r, int d) { v.push_back(l); v.push_back(r); v.push_back(d); }
    bool pop(int& l, int& r, int& d) { if (v.empty()) return false; d = v.back(); v.pop_back(); r = v.back(); v.pop_back(); l = v.back(); v.pop_back(); return true; }
};
struct Before {                              // alnreg_hlt (second == false) or alnreg_hlt2 over indices into a
    const meme_alnreg* a; bool second;
    bool operator()(int x, int y) const {
        const meme_alnreg &p = a[x], &q = a[y];
        return second ? pri_hlt2(p.score, pri_is_alt(p.n_comp_is_alt), p.hash, q.score, pri_is_alt(q.n_comp_is_alt), q.hash)
                      : pri_hlt(p.score, pri_is_alt(p.n_comp_is_alt), p.hash, q.score, pri_is_alt(q.n_comp_is_alt), q.hash);
    }
};
// ord = the indices of a[0, n) in the order
inline void order(const meme_alnreg* a, int n, bool second, std::vector<int>& ord) {
    ord.resize((size_t)n);
    for (int k = 0; k < n; ++k) ord[(size_t)k] = k;
    Stack st;
    ks_introsort(KsPtr<int>{ord.data()}, n, Before{a, second}, st);
}
// mem_mark_primary_se_core over a[0, n)
inline void core(meme_alnreg* a, int n, float mask_level, int tmp) {
    for (int i = 1; i < n; ++i) {
        int found = -1;
        for (int j = 0; j < i && found < 0; ++j)
            if (a[j].secondary < 0 && pri_overlap(a[j].qb, a[j].qe, a[i].qb, a[i].qe, mask_level)) found = j;
        if (found < 0) continue;
        meme_alnreg& q = a[found];
        const PriHit h = pri_hit(q.sub, q.sub_n, q.score, pri_is_alt(q.n_comp_is_alt), a[i].score, pri_is_alt(a[i].n_comp_is_alt), tmp);
        q.sub = h.sub; q.sub_n = h.sub_n;
        a[i].secondary = found;
    }
}
inline const double* logtab() {
    static const std::vector<double> tab = [] { std::vector<double> t((size_t)PRI_LOG); for (int k = 0; k < PRI_LOG; ++k) t[(size_t)k] = log((double)k); return t; }();
    return tab.data();
}
inline int mapq(const meme_alnreg& R, const meme_primary_opt& o, bool* beyond) {
    const PriQual Q = {R.score, R.sub, R.csub, R.sub_n, R.qb, R.qe, R.rb, R.re, R.frac_rep};
    const double* tab = logtab();
    return pri_mapq(Q, o, [&](int k) -> double { return tab[k]; }, beyond);
}
static int64_t orders_taken = 0;             // sorts of the last t_primary call (a read takes one, or two where ALT and primary-assembly records mix)

}  // namespace pri_driver

// out: the records of every read in the final order (offsets = reg_off); n_pri, status per read; mapq per record
extern "C" void t_primary(const meme_alnreg* regs, const int64_t* reg_off, int64_t nreads, int64_t id_base, const meme_primary_opt* opt, meme_alnreg* out, int32_t* n_pri_out,
                          uint8_t* mapq, uint8_t* status) {
    using namespace pri_driver;
    const meme_primary_opt& o = *opt;
    const int tmp = pri_score_distance(o);
    std::vector<meme_alnreg> in, t;
    std::vector<int> ord, rk;
    orders_taken = 0;
    for (int64_t r = 0; r < nreads; ++r) {
        const int64_t base = reg_off[r];
        const int n = (int)(reg_off[r + 1] - base);
        meme_alnreg* a = out + base;
        n_pri_out[r] = 0; status[r] = 0;
        if (n == 0) continue;
        int n_pri = 0;
        in.assign(regs + base, regs + base + n);
        for (int k = 0; k < n; ++k) {                                                // :2008-2012
            meme_alnreg& R = in[(size_t)k];
            R.sub = R.alt_sc = 0; R.secondary = R.secondary_all = -1;
            R.hash = pri_hash64((uint64_t)id_base + (uint64_t)r + (uint64_t)k);
            n_pri += pri_is_alt(R.n_comp_is_alt) == 0;
        }
        order(in.data(), n, false, ord); ++orders_taken;
        t.resize((size_t)n);
        for (int k = 0; k < n; ++k) t[(size_t)k] = in[(size_t)ord[(size_t)k]];
        core(t.data(), n, o.mask_level, tmp);
        for (int k = 0; k < n; ++k) {                                                // :2015-2021
            meme_alnreg& R = t[(size_t)k];
            const meme_alnreg& parent = t[(size_t)(R.secondary < 0 ? 0 : R.secondary)];
            R.secondary_all = k;
            R.alt_sc = pri_alt_sc(R.alt_sc, pri_is_alt(R.n_comp_is_alt), R.secondary, pri_is_alt(parent.n_comp_is_alt), parent.score);
        }
        if (n_pri < n) {                                                             // :2022-2039
            rk.resize((size_t)n);
            if (n_pri > 0) {
                order(t.data(), n, true, ord); ++orders_taken;
                for (int k = 0; k < n; ++k) rk[(size_t)ord[(size_t)k]] = k;
            } else
                for (int k = 0; k < n; ++k) rk[(size_t)k] = k;
            for (int k = 0; k < n; ++k) {
                meme_alnreg R = t[(size_t)k];
                const PriMarks m = pri_remap(R.sub, R.secondary, pri_is_alt(R.n_comp_is_alt), rk[(size_t)k], n_pri, rk[(size_t)(R.secondary < 0 ? 0 : R.secondary)]);
                R.sub = m.sub; R.secondary = m.secondary; R.secondary_all = m.secondary_all;
                a[rk[(size_t)k]] = R;
            }
            if (n_pri > 0) core(a, n_pri, o.mask_level, tmp);
        } else
            for (int k = 0; k < n; ++k) { a[k] = t[(size_t)k]; a[k].secondary_all = a[k].secondary; }      // :2041-2042
        if (o.primary5) {                                                            // mem_reorder_primary5
            int cnt = 0;
            PriLeft left = pri_left_none();
            for (int k = 0; k < n; ++k)
                if (pri_candidate(a[k].secondary, pri_is_alt(a[k].n_comp_is_alt), a[k].score, o.T)) { ++cnt; const PriLeft c = {a[k].qb, k}; left = pri_leftmost(left, c); }
            if (cnt > 1 && left.k != 0 && left.k < n) {
                const meme_alnreg x = a[0]; a[0] = a[left.k]; a[left.k] = x;
                for (int k = 1; k < n; ++k) { a[k].secondary = pri_swapped(a[k].secondary, left.k); a[k].secondary_all = pri_swapped(a[k].secondary_all, left.k); }
            }
        }
        bool beyond = false;
        for (int k = 0; k < n; ++k) mapq[base + k] = pri_byte(pri_driver::mapq(a[k], o, &beyond));
        status[r] = beyond ? 1 : 0;
        n_pri_out[r] = n_pri;
    }
}
extern "C" int64_t t_primary_orders(void) { return pri_driver::orders_taken; }

// the quality of one record; *beyond = 1: a logarithm outside the table was asked for
extern "C" int t_primary_mapq(const meme_alnreg* reg, const meme_primary_opt* opt, int* beyond) {
    bool b = false;
    const int q = pri_driver::mapq(*reg, *opt, &b);
    *beyond = b ? 1 : 0;
    return q;
}
