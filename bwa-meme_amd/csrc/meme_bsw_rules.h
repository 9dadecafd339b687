// The row-granular rules of scalarBandedSWA == ksw_extend2 (reference src/bandedSWA.cpp:116-237) that every banded-SW kernel of meme_bsw.hip
// applies, written ONCE on plain values: the kernels differ in who computes a row's cells and where the H/E columns live (one lane and an LDS
// word per column, a ring of them, 16-64 lanes and two LDS / HBM arrays), not in these.  Band trimming (:217-221) stays with the kernels: it
// is a walk over the columns' storage.
#pragma once
#include <stdint.h>

#include "meme_hip.h"
#include "meme_ksort.h"      // KS_HD

// the band cap (:148-156): no gap can be longer than the best score of the whole query pays for.  (max of bwa_fill_scmat(a, b) = max(a, 0))
KS_HD int bsw_band_cap(const meme_bsw_opt& o, int qlen, int w) {
    const int mx = o.a > 0 ? o.a : 0;
    int max_ins = (int)((double)(qlen * mx + o.end_bonus - o.o_ins) / o.e_ins + 1.);
    if (max_ins < 1) max_ins = 1;
    if (w > max_ins) w = max_ins;
    int max_del = (int)((double)(qlen * mx + o.end_bonus - o.o_del) / o.e_del + 1.);
    if (max_del < 1) max_del = 1;
    if (w > max_del) w = max_del;
    return w;
}

// H(-1, j) of the first row (:143-145): eh[0] = h0, eh[1] = max(h0 - oe_ins, 0), eh[j] = eh[j-1] - e_ins while eh[j-1] > e_ins, 0 behind that
// (E = 0 throughout).  These are the "stale cells" the function reads when its band grows into columns no row has computed yet.
KS_HD int bsw_row0(int h0, int oe_ins, int e_ins, int j) {
    const int first = h0 > oe_ins ? h0 - oe_ins : 0;
    if (j == 0) return h0;
    if (j == 1) return first;
    const int prev = first - (j - 2) * e_ins;
    return prev > e_ins ? prev - e_ins : 0;
}

// head of row i (:167-174): the band [beg, end) clamped to i -+ w and the query; returns h1 = H(i, beg - 1).
KS_HD int bsw_row_head(int i, int w, int qlen, int h0, int o_del, int e_del, int& beg, int& end) {
    if (beg < i - w) beg = i - w;
    if (end > i + w + 1) end = i + w + 1;
    if (end > qlen) end = qlen;
    int h1;
    if (beg == 0) { h1 = h0 - (o_del + e_del * (i + 1)); if (h1 < 0) h1 = 0; }
    else h1 = 0;
    return h1;
}
// The same three statements on values, for k_bsw_lane alone: the compiler turns this form into selects and that one into branches, and each kernel is at the
// parent's speed with one of them only (profiles/bsw_rules_once.md, "Three things to know"; tests/test_bsw_rules_model.py holds the two forms against each other)
KS_HD int bsw_band_beg(int beg, int i, int w) { if (beg < i - w) beg = i - w; return beg; }
KS_HD int bsw_band_end(int end, int i, int w, int qlen) { if (end > i + w + 1) end = i + w + 1; if (end > qlen) end = qlen; return end; }
KS_HD int bsw_first_h1(int beg, int i, int h0, int o_del, int e_del) {
    int h1;
    if (beg == 0) { h1 = h0 - (o_del + e_del * (i + 1)); if (h1 < 0) h1 = 0; }
    else h1 = 0;
    return h1;
}

// what a pair's rows accumulate (:159-161) and what is stored of it (:225-229, 236)
struct BswBest {
    int max, max_i, max_j, max_ie, gscore, max_off;
    KS_HD explicit BswBest(int h0) : max(h0), max_i(-1), max_j(-1), max_ie(-1), gscore(-1), max_off(0) {}
    KS_HD void store(meme_seqpair* P) const {
        P->score = max;
        P->qle = max_j + 1;
        P->tle = max_i + 1;
        P->gtle = max_ie + 1;
        P->gscore = gscore;
        P->max_off = max_off;
    }
};

// end of row i (:202-216), after the cells of [beg, end): m = the row's maximum (0: none), mj = its rightmost column, h1 = H(i, end - 1).
// True: the pair is finished (nothing scores, or z-drop).
KS_HD bool bsw_row_end(BswBest& b, int i, int m, int mj, int h1, int beg, int end, int qlen, int e_del, int e_ins, int zdrop) {
    if ((beg < end ? end : beg) == qlen) {             // "if (j == qlen)" after the column loop: the row reached the query's end
        b.max_ie = b.gscore > h1 ? b.max_ie : i;
        b.gscore = b.gscore > h1 ? b.gscore : h1;
    }
    if (m == 0) return true;                           // :206
    if (m > b.max) {
        b.max = m; b.max_i = i; b.max_j = mj;
        int off = mj - i;
        if (off < 0) off = -off;
        b.max_off = b.max_off > off ? b.max_off : off;
    } else if (zdrop > 0) {
        if (i - b.max_i > mj - b.max_j) {
            if (b.max - m - ((i - b.max_i) - (mj - b.max_j)) * e_del > zdrop) return true;
        } else {
            if (b.max - m - ((mj - b.max_j) - (i - b.max_i)) * e_ins > zdrop) return true;
        }
    }
    return false;
}

// the next row's `end` from the last column jt whose H or E is not zero (:221)
KS_HD int bsw_next_end(int jt, int qlen) { return jt + 2 < qlen ? jt + 2 : qlen; }
