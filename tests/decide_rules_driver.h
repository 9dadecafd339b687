// A scalar host driver of bwa-meme_amd/csrc/meme_decide_rules.h: the pairing decision for the pairs of a batch, one after the other, on post-primary records and
// mem_pair's outputs.  tests/test_decide_rules_model.py compiles it with g++ into a shared object; scripts/decide_rules_main.cpp wraps it in a program of its own
// (for a sanitizer build).  Nothing here decides a result: the loops over the records are sequential where the kernel's are strided over lanes, the logarithms are
// a table the host's libm fills as the stage's is, and everything else is the header's (and pri_mapq of meme_primary_rules.h).  The status follows the stage's
// host form: 1 for a pair-stage status or a logarithm beyond the table, the pair then left at its defaults and its records untouched.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

#include "meme_decide_rules.h"

namespace decide_driver {

inline const std::vector<double>& logtab() {
    static std::vector<double> tab;
    if (tab.empty()) { tab.resize((size_t)PRI_LOG); for (int k = 0; k < PRI_LOG; ++k) tab[(size_t)k] = log((double)k); }
    return tab;
}
inline PriQual qual(const meme_alnreg& R, int sub) { const PriQual Q = {R.score, sub, R.csub, R.sub_n, R.qb, R.qe, R.rb, R.re, R.frac_rep}; return Q; }

}  // namespace decide_driver

// per pair (reads 2p, 2p + 1): path, q_pe, flag, status; sel, q_se, alt two per pair; regs changes in place.  -> 0, or -1 for what the stage's host form refuses
extern "C" int t_decide(meme_alnreg* regs, const int64_t* reg_off, const int32_t* n_pri, int64_t nreads, const int32_t* score, const int32_t* sub, const int32_t* n_sub, const int32_t* z,
                        const uint8_t* pair_status, int64_t l_pac, const meme_pair_pes* pes, const meme_decide_opt* opt, int32_t* path, int32_t* sel, int32_t* q_se, int32_t* q_pe, int32_t* flag,
                        int32_t* alt, uint8_t* status) {
    using namespace decide_driver;
    if ((nreads & 1) || opt->a < 1 || (int64_t)opt->a + opt->b <= 0 || !(opt->mapQ_coef_len > 0)) return -1;
    const std::vector<double>& tab = logtab();
    const auto lg = [&](int k) -> double { return tab[(size_t)k]; };
    const meme_decide_opt& o = *opt;
    const meme_primary_opt po = dec_pri_opt(o);
    for (int64_t p = 0; p < nreads / 2; ++p) {
        path[p] = DEC_PATH_NONE; q_pe[p] = 0; flag[p] = 1; status[p] = 0;
        for (int i = 0; i < 2; ++i) { sel[2 * p + i] = -1; q_se[2 * p + i] = 0; alt[2 * p + i] = -1; }
        if (pair_status[p]) { status[p] = 1; continue; }
        meme_alnreg* a[2] = {regs + reg_off[2 * p], regs + reg_off[2 * p + 1]};
        const int n[2] = {(int)(reg_off[2 * p + 1] - reg_off[2 * p]), (int)(reg_off[2 * p + 2] - reg_off[2 * p + 1])}, np[2] = {n_pri[2 * p], n_pri[2 * p + 1]};
        if (np[0] < 0 || np[0] > n[0] || np[1] < 0 || np[1] > n[1]) return -1;
        const bool entered = dec_entered(np[0], np[1], score[p], o.no_pairing);
        bool multi = false;
        if (entered)
            for (int i = 0; i < 2; ++i)
                for (int j = 1; j < np[i]; ++j) multi = multi || dec_multi(j, a[i][j].secondary, a[i][j].score, o.T);
        if (!entered || multi) {
            int which[2], rid[2];
            for (int i = 0; i < 2; ++i) {
                which[i] = dec_which(n[i], np[i], n[i] > 0 ? a[i][0].score : 0, np[i] < n[i] ? a[i][np[i]].score : 0, o.T);
                rid[i] = which[i] >= 0 ? a[i][which[i]].rid : -1;
                sel[2 * p + i] = which[i];
            }
            if (which[0] >= 0 && which[1] >= 0) flag[p] = dec_flag_unpaired(o.no_pairing, rid[0], rid[1], l_pac, a[0][0].rb, a[1][0].rb, pes);
            path[p] = multi ? DEC_PATH_MULTI : DEC_PATH_NONE;
            continue;
        }
        const int score_un = dec_score_un(a[0][0].score, a[1][0].score, o.pen_unpaired);
        bool beyond = false;
        const int qpe = dec_q_pe(score[p], sub[p], score_un, n_sub[p], o.a, a[0][0].frac_rep, a[1][0].frac_rep, lg, &beyond);
        const bool paired = dec_paired_preferred(score[p], score_un);
        int zz[2], qse[2], k[2];
        DecMarks marks[2];
        for (int i = 0; i < 2; ++i) {
            zz[i] = paired ? z[2 * p + i] : 0;
            if (zz[i] < 0 || zz[i] >= np[i]) return -1;
            const meme_alnreg& c = a[i][zz[i]];
            if (c.secondary >= n[i]) return -1;
            marks[i].sub = c.sub; marks[i].secondary = c.secondary;
            if (paired) marks[i] = dec_c_marks(c.sub, c.secondary, c.secondary >= 0 ? a[i][c.secondary].score : 0);
            qse[i] = pri_mapq(qual(c, marks[i].sub), po, lg, &beyond);
            if (paired) qse[i] = dec_q_se_paired(qse[i], qpe, c.score, c.csub, o.a);
            k[i] = c.secondary_all;
        }
        if (beyond) { status[p] = 1; continue; }
        path[p] = paired ? DEC_PATH_PAIRED : DEC_PATH_UNPAIRED; q_pe[p] = qpe; flag[p] = paired ? 3 : 1;
        for (int i = 0; i < 2; ++i) {
            sel[2 * p + i] = zz[i]; q_se[2 * p + i] = qse[i];
            alt[2 * p + i] = np[i] < n[i] ? dec_alt(np[i], n[i], a[i][np[i]].score, a[i][np[i]].secondary, pri_is_alt(a[i][np[i]].n_comp_is_alt), o.T) : -1;
            if (paired) { a[i][zz[i]].sub = marks[i].sub; a[i][zz[i]].secondary = marks[i].secondary; }
            if (dec_swap_taken(k[i], np[i]))
                for (int j = 0; j < n[i]; ++j) a[i][j].secondary_all = dec_swapped(j, a[i][j].secondary_all, k[i], zz[i]);
        }
    }
    return 0;
}
