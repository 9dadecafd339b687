// The rules of primary marking and mapping quality -- mem_mark_primary_se with mem_mark_primary_se_core (reference src/bwamem.cpp:1974-2046),
// mem_reorder_primary5 (:2078-2100) and mem_approx_mapq_se (:2052-2076) -- written ONCE on plain values: the hash and the two orders, the float overlap
// test, the score distance, what a hit does to the list member it hits, alt_sc, the remap behind the second order, the primary5 candidate and the choice
// of the leftmost, the index swap, and the quality.  meme_primary.hip's two tiers call them (where the state lives -- registers and shuffles, LDS
// columns, HBM -- the ballots, the ranks by counting and the barriers stay there); tests/test_primary_rules_model.py compiles this file with g++ into
// a sequential driver (tests/primary_rules_driver.h) and holds it against the compiled reference's fixture.
//
// Arithmetic: the overlap test in float as in the reference (int times float is a float multiply: one operation, nothing to contract); the quality in
// IEEE double, no contraction (the pragma below for clang; -ffp-contract=off for g++), its logarithms from a callable the caller supplies -- the
// kernels and the driver look them up in a table the host's libm filled (the device's log is not glibc's; the arguments are small integers).
#pragma once
#include <limits.h>
#include <stdint.h>

#include "meme_hip.h"
#include "meme_ksort.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr int PRI_LOG = 65536;               // entries of the table of logarithms: log((double)k), k < PRI_LOG

KS_HD uint64_t pri_hash64(uint64_t key) {    // hash_64, reference src/utils.h:117
    key += ~(key << 32); key ^= (key >> 22); key += ~(key << 13); key ^= (key >> 8); key += (key << 3); key ^= (key >> 15); key += ~(key << 27); key ^= (key >> 31);
    return key;
}
KS_HD int pri_is_alt(int n_comp_is_alt) { return n_comp_is_alt >> 30; }     // int n_comp:30, is_alt:2
// alnreg_hlt / alnreg_hlt2 (:174, :177): x before y.  Strict total orders (the hash is a bijection of distinct ids), so a record's place in the reference's
// introsort is the number of records before it
KS_HD bool pri_hlt(int sx, int ax, uint64_t hx, int sy, int ay, uint64_t hy) { return sx > sy || (sx == sy && (ax < ay || (ax == ay && hx < hy))); }
KS_HD bool pri_hlt2(int sx, int ax, uint64_t hx, int sy, int ay, uint64_t hy) { return ax < ay || (ax == ay && (sx > sy || (sx == sy && hx < hy))); }
// significant overlap of two query spans (:1985-1989), the comparison in float
KS_HD bool pri_overlap(int qbj, int qej, int qbi, int qei, float mask_level) {
    const int b_max = qbj > qbi ? qbj : qbi, e_min = qej < qei ? qej : qei;
    if (e_min <= b_max) return false;
    const int min_l = qei - qbi < qej - qbj ? qei - qbi : qej - qbj;
    return (float)(e_min - b_max) >= (float)min_l * mask_level;
}
// tmp: the score distance up to which a secondary hit counts in sub_n (:1977-1979)
KS_HD int pri_score_distance(const meme_primary_opt& o) {
    int tmp = o.a + o.b;
    tmp = o.o_del + o.e_del > tmp ? o.o_del + o.e_del : tmp;
    return o.o_ins + o.e_ins > tmp ? o.o_ins + o.e_ins : tmp;
}
// what a hit does to the list member it hits (:1990-1992): sub while it is 0, sub_n under the tmp / is_alt rule.  (sub, sub_n, score, alt) are the member's
struct PriHit { int sub, sub_n; };
KS_HD PriHit pri_hit(int sub, int sub_n, int score, int alt, int hit_score, int hit_alt, int tmp) {
    const PriHit h = {sub == 0 ? hit_score : sub, sub_n + (score - hit_score <= tmp && (alt || !hit_alt) ? 1 : 0)};
    return h;
}
// alt_sc behind the first walk (:2019-2020): a primary-assembly record whose parent is an ALT record takes the parent's score (parent_*: of record
// `secondary`; anything where secondary < 0)
KS_HD int pri_alt_sc(int alt_sc, int alt, int secondary, int parent_alt, int parent_score) { return !alt && secondary >= 0 && parent_alt ? parent_score : alt_sc; }
// a record behind the second order (:2027-2036): secondary_all through the ranks, INT_MAX for an ALT secondary, -1 for none, and the reset of the first
// n_pri.  rank: the record's own new position; parent_rank: that of record `secondary` (anything where secondary < 0).  With n_pri == 0 nothing is reset
struct PriMarks { int sub, secondary, secondary_all; };
KS_HD PriMarks pri_remap(int sub, int secondary, int alt, int rank, int n_pri, int parent_rank) {
    PriMarks m = {sub, secondary, -1};
    if (secondary >= 0) { m.secondary_all = parent_rank; if (alt) m.secondary = INT_MAX; }
    if (rank < n_pri) { m.sub = 0; m.secondary = -1; }
    return m;
}
// mem_reorder_primary5: who is a candidate (:2083, :2087), and the leftmost of two (:2088 over ascending k: the smaller qb, the earlier record among equals)
KS_HD bool pri_candidate(int secondary, int alt, int score, int T) { return secondary < 0 && !alt && score >= T; }
struct PriLeft { int qb, k; };
KS_HD PriLeft pri_left_none() { const PriLeft x = {INT_MAX, INT_MAX}; return x; }
KS_HD PriLeft pri_leftmost(PriLeft x, PriLeft y) { return y.qb < x.qb || (y.qb == x.qb && y.k < x.k) ? y : x; }
// ... and its index update (:2093-2099) for the records behind the first
KS_HD int pri_swapped(int s, int left_k) { return s == 0 ? left_k : s == left_k ? 0 : s; }

// mem_approx_mapq_se, the mapQ_coef_len > 0 branch.  lg(k) = log((double)k) for 0 <= k < PRI_LOG; *beyond: a logarithm outside that range was asked for (lg
// is not called, the value returned means nothing)
struct PriQual { int score, sub, csub, sub_n, qb, qe; int64_t rb, re; float frac_rep; };
template <class LG> KS_HD int pri_mapq(const PriQual& R, const meme_primary_opt& o, LG&& lg, bool* beyond) {
    int sub = R.sub ? R.sub : o.min_seed_len * o.a;
    sub = R.csub > sub ? R.csub : sub;
    if (sub >= R.score) return 0;
    const int l = (int)(R.qe - R.qb > R.re - R.rb ? R.qe - R.qb : R.re - R.rb);
    const double identity = 1. - (double)(l * o.a - R.score) / (o.a + o.b) / l;
    int mapq;
    if (R.score == 0) mapq = 0;
    else {
        double t = 1.;
        if (!((float)l < o.mapQ_coef_len)) {
            if (l < 0 || l >= PRI_LOG) { *beyond = true; return 0; }
            t = o.mapQ_coef_fac / lg(l);
        }
        t *= identity * identity;
        mapq = (int)(6.02 * (R.score - sub) / o.a * t * t + .499);
    }
    if (R.sub_n > 0) {
        if (R.sub_n >= PRI_LOG - 1) { *beyond = true; return 0; }
        mapq -= (int)(4.343 * lg(R.sub_n + 1) + .499);
    }
    if (mapq > 60) mapq = 60;
    if (mapq < 0) mapq = 0;
    return (int)(mapq * (1. - R.frac_rep) + .499);
}
KS_HD uint8_t pri_byte(int q) { return (uint8_t)(q < 0 ? 0 : q > 255 ? 255 : q); }
