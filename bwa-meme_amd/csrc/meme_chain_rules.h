// The rules of mem_chain_Learned and mem_chain_flt (reference src/bwamem.cpp) that every chaining tier of meme_chain.hip applies, written ONCE
// on plain values: the tiers differ in where a chain's fields live (HBM rows, LDS arrays, records) and in who walks them, not in these.
#pragma once
#include <stdint.h>

#include "meme_hip.h"
#include "meme_ksort.h"      // KS_HD

// the (start, end, index) order the SMEMs are walked in (ks_introsort at :1397; equal (start, end) describe the same substring, hence the same hits)
KS_HD bool smem_before(int s1, int e1, int i1, int s2, int e2, int i2) { return s1 < s2 || (s1 == s2 && (e1 < e2 || (e1 == e2 && i1 < i2))); }

// frac_rep (:1140-1147): the query span [b, e) covered by SMEMs with more than max_occ hits, finished spans summed in l_rep
KS_HD void rep_span_step(int& b, int& e, int& l_rep, int start, int end) {
    if (start > e) { l_rep += e - b; b = start; e = end; }
    else if (end > e) e = end;
}

// the hits of an SMEM that are walked (:1154-1155): every step-th, at most max_occ of them
KS_HD int occ_step(int hitcount, int max_occ) { return hitcount > max_occ ? hitcount / max_occ : 1; }
KS_HD int occ_count(int hitcount, int step, int max_occ) { const int cnt = (hitcount + step - 1) / step; return cnt < max_occ ? cnt : max_occ; }

// test_and_merge (:450-492): what the hit (rbeg, qbeg, len, rid) does to the chain below it, given the chain's first (f_) and last (l_) seed:
// 0 nothing (contained), 1 appended, 2 a new chain
KS_HD int merge_outcome(int c_rid, int64_t f_rbeg, int f_qbeg, int64_t l_rbeg, int l_qbeg, int l_len, int64_t rbeg, int qbeg, int len, int rid,
                        const meme_chain_opt& o) {
    if (rid != c_rid) return 2;
    const int64_t qend = l_qbeg + l_len, rend = l_rbeg + l_len;
    if (qbeg >= f_qbeg && qbeg + len <= qend && rbeg >= f_rbeg && rbeg + len <= rend) return 0;
    if ((l_rbeg < o.l_pac || f_rbeg < o.l_pac) && rbeg >= o.l_pac) return 2;          // the chain on the forward strand, the hit on the reverse
    const int64_t x = qbeg - l_qbeg, y = rbeg - l_rbeg;
    return y >= 0 && x - y <= o.w && y - x <= o.w && x - l_len < o.max_chain_gap && y - l_len < o.max_chain_gap ? 1 : 2;
}

// mem_chain_weight (:522-541): one seed [beg, beg + len) added to a coverage sum w whose seeds so far end at `end` ("the part of it behind end");
// the weight is the smaller of the query and the reference coverage, capped
template <class T> KS_HD void cover_step(int& w, T& end, T beg, int len) {
    if (beg >= end) w += len;
    else if (beg + len > end) w += (int)(beg + len - end);
    end = end > beg + len ? end : beg + len;
}
KS_HD int chain_weight_of(int wq, int wr) { const int w = wq < wr ? wq : wr; return w < 1 << 30 ? w : (1 << 30) - 1; }

// mem_chain_flt's test of chain i against a kept, heavier chain j (:655-668) on their query spans, weights and ALT flags: bit 0 = they overlap
// largely (large_ovlp; j's `first` becomes i if it has none), bit 1 = and i is dropped (the loop over the kept chains ends)
KS_HD int flt_overlap(int beg_i, int end_i, int w_i, int alt_i, int beg_j, int end_j, int w_j, int alt_j, const meme_chain_opt& o) {
    const int b_max = beg_j > beg_i ? beg_j : beg_i, e_min = end_j < end_i ? end_j : end_i;
    if (!(e_min > b_max && (!alt_j || alt_i))) return 0;
    const int li = end_i - beg_i, lj = end_j - beg_j;
    const int min_l = li < lj ? li : lj;
    if (!((float)(e_min - b_max) >= (float)min_l * o.mask_level && min_l < o.max_chain_gap)) return 0;
    return (float)w_i < (float)w_j * o.drop_ratio && w_j - w_i >= o.min_seed_len << 1 ? 3 : 1;
}

// at most max_chain_extend chains of kind 1 / 2 go on (:690-695): behind the one that reaches the cap only kind 3 stays.  kept(i): reference to chain i's mark
template <class K> KS_HD void cap_chain_extend(const K& kept, int n, int max_chain_extend) {
    int i = 0, k = 0;
    for (; i < n; ++i) {
        const int kp = kept(i);
        if (kp == 0 || kp == 3) continue;
        if (++k >= max_chain_extend) break;
    }
    for (; i < n; ++i) if (kept(i) < 3) kept(i) = 0;
}
