// The rules of pair scoring -- mem_pair (reference src/bwamem_pair.cpp:372-433), the second step of mem_sam_pe -- written ONCE on plain values: the key of a
// record and the order of the keys, the candidate test, the score of a candidate and its key, the top two of the candidates and what counts in n_sub.
// meme_pair.hip's two tiers call them (where the keys live -- registers and shuffles, LDS, HBM -- the ranks by counting and the reductions stay there);
// tests/test_pair_rules_model.py compiles this file with g++ into a sequential driver (tests/pair_rules_driver.h) and holds it against the compiled
// reference's fixture.
//
// The candidate test is a predicate.  The reference walks, for key i of the sorted keys and each of the two directions r, backwards from y[which] -- the last
// key before i whose low two bits are `which` -- skips keys of another `which`, breaks at dist > high and skips dist < low.  dist = x_i - x_k does not fall as
// k falls (the keys are sorted by x), so behind the break no key is in range: the loop visits exactly the k < i with (y_k & 3) == which and
// low <= dist <= high, and y[which] >= 0 is "some k < i has that which".  A key's low two bits are one value, so a pair (i, k) is a candidate of at most one r.
// tests/test_pair_rules_model.py holds the predicate against a literal restatement of the loop.
//
// Arithmetic: the score is IEEE double, no contraction (the pragma below for clang; -ffp-contract=off for g++); its penalty term
// .721 * log(2 * erfc(|ns| / sqrt 2)) * a comes from a table the host's libm filled (pair_penalty below, host only): no erfc and no log on the device.
#pragma once
#include <math.h>
#include <stdint.h>

#include "meme_hip.h"
#include "meme_ksort.h"
#include "meme_primary_rules.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr int64_t PAIR_TABLE_MAX = (int64_t)1 << 20;     // entries of the penalty table of one orientation: high - low + 1 beyond it is refused
constexpr int PAIR_MAX_PRI = 1 << 28;                     // records of an end that take part: the key holds the index as i << 2 in an int

struct PairKey { uint64_t x, y; };
// pair64_lt: x, then y.  All y of a pair's keys are distinct (index and end), so the order is strict and total: a key's place in the reference's introsort
// is the number of keys before it
KS_HD bool pair_lt(PairKey a, PairKey b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }
KS_HD bool pair_same(PairKey a, PairKey b) { return a.x == b.x && a.y == b.y; }
// who takes part (the convention of the stage, not the reference's: it would index anns[] out of bounds, or shift a negative score into the key)
KS_HD bool pair_record_ok(int rid, int score, int n_contigs) { return rid >= 0 && rid < n_contigs && score >= 0; }
// the key of record i of end r (:382-384); contig_offset: bns->anns[rid].offset
KS_HD PairKey pair_key(int64_t rb, int rid, int score, int i, int r, int64_t l_pac, int64_t contig_offset) {
    const uint64_t fwd = (uint64_t)(rb < l_pac ? rb : (l_pac << 1) - 1 - rb);
    const PairKey k = {(uint64_t)(int64_t)rid << 32 | (fwd - (uint64_t)contig_offset),
                       (uint64_t)(int64_t)score << 32 | (uint64_t)(int64_t)(i << 2 | (rb >= l_pac ? 1 : 0) << 1 | r)};
    return k;
}
KS_HD int pair_key_score(PairKey k) { return (int)(k.y >> 32); }
KS_HD int pair_key_end(PairKey k) { return (int)(k.y & 1); }
KS_HD int pair_key_index(PairKey k) { return (int)(k.y << 32 >> 34); }         // :423
// the orientations that are alive, as the kernels carry them: low, high, failed of pes[4] and where an orientation's penalties start in the table
struct PairDirs { int32_t low[4], high[4], failed[4]; int64_t tab_off[4]; };
// member d of four by selects (constant indices: a copy of PairDirs in registers stays there)
KS_HD int32_t pair_pick(const int32_t (&v)[4], int d) { return d == 0 ? v[0] : d == 1 ? v[1] : d == 2 ? v[2] : v[3]; }
KS_HD int64_t pair_pick64(const int64_t (&v)[4], int d) { return d == 0 ? v[0] : d == 1 ? v[1] : d == 2 ? v[2] : v[3]; }
// the candidate test of key i against key k in front of it (:393-406): -1, or the orientation; *dist = x_i - x_k
KS_HD int pair_candidate(PairKey ki, PairKey kk, const PairDirs& D, int64_t* dist) {
    if (((ki.y ^ kk.y) & 1) == 0) return -1;                                   // which = r << 1 | (end of i ^ 1): the other end's keys only, and then r = (y_k >> 1 & 1)
    const int dir = (int)(kk.y >> 1 & 1) << 1 | (int)(ki.y >> 1 & 1);
    if (pair_pick(D.failed, dir)) return -1;
    const int64_t d = (int64_t)(ki.x - kk.x);
    *dist = d;
    return d >= pair_pick(D.low, dir) && d <= pair_pick(D.high, dir) ? dir : -1;
}
// the largest `high` of the live orientations: a walk towards smaller k ends where dist exceeds it (below every dist where none is alive: dist is never negative)
KS_HD int64_t pair_reach(const PairDirs& D) {
    int64_t h = -((int64_t)1 << 32);
#if defined(__clang__)
#pragma unroll
#endif
    for (int d = 0; d < 4; ++d) if (!D.failed[d] && D.high[d] > h) h = D.high[d];
    return h;
}
// key k, in front of key i, is beyond the reach: so is every key in front of it (the keys are sorted by x)
KS_HD bool pair_beyond(PairKey ki, PairKey kk, int64_t reach) { return (int64_t)(ki.x - kk.x) > reach; }
// the score of a candidate (:408-409): T = .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * a.  (int) of a double outside the int range, of an infinity or of a
// NaN is INT_MIN on x86 (cvttsd2si), which :409 turns into 0 with every other negative value; values in (-1, 1) truncate to 0
KS_HD int pair_q(int s_i, int s_k, double T) {
    const double v = ((double)((uint64_t)s_i + (uint64_t)s_k) + T) + .499;
    return v >= 1. && v < 2147483648. ? (int)v : 0;
}
// `id << 8` on the int the prototype truncates the 64-bit id to, as the `^` with a 64-bit value sees it (:412)
KS_HD uint64_t pair_idx(uint64_t id) { return (uint64_t)(int64_t)(int32_t)((uint32_t)id << 8); }
// the key of the candidate (k, i), k < i positions of the sorted keys (:411-412)
KS_HD PairKey pair_cand_key(int q, int k, int i, uint64_t idx) {
    const uint64_t y = (uint64_t)k << 32 | (uint64_t)i;
    const PairKey c = {(uint64_t)q << 32 | (pri_hash64(y ^ idx) & 0xffffffffu), y};
    return c;
}
KS_HD int pair_cand_q(PairKey c) { return (int)(c.x >> 32); }
// the two largest candidates under (x, y) and how many there are -- all the reference reads of its sorted u besides one count (:421-428)
struct PairTop { PairKey best, second; int n; };
KS_HD PairTop pair_top_none() { const PairTop t = {{0, 0}, {0, 0}, 0}; return t; }
KS_HD PairTop pair_top_push(PairTop t, PairKey c) {
    if (t.n == 0 || pair_lt(t.best, c)) { t.second = t.best; t.best = c; }      // (second is read only where n > 1)
    else if (t.n == 1 || pair_lt(t.second, c)) t.second = c;
    ++t.n;
    return t;
}
KS_HD PairTop pair_top_merge(PairTop a, PairTop b) {                            // of two disjoint sets of candidates
    if (b.n == 0) return a;
    if (a.n == 0) return b;
    PairTop t;
    t.n = a.n + b.n;
    const bool a_first = pair_lt(b.best, a.best);
    const PairKey hi_second = a_first ? a.second : b.second, lo_best = a_first ? b.best : a.best;      // (values, not references: the two sets stay in registers)
    t.best = a_first ? a.best : b.best;
    t.second = (a_first ? a.n : b.n) > 1 && pair_lt(lo_best, hi_second) ? hi_second : lo_best;
    return t;
}
KS_HD int pair_top_score(const PairTop& t) { return t.n ? pair_cand_q(t.best) : 0; }
KS_HD int pair_top_sub(const PairTop& t) { return t.n > 1 ? pair_cand_q(t.second) : 0; }
// tmp (:418-420) and what n_sub counts (:427-428): every candidate but the best within tmp of sub
KS_HD int pair_score_distance(const meme_pair_opt& o) {
    int tmp = o.a + o.b;
    tmp = tmp > o.o_del + o.e_del ? tmp : o.o_del + o.e_del;
    return tmp > o.o_ins + o.e_ins ? tmp : o.o_ins + o.e_ins;
}
KS_HD bool pair_in_n_sub(PairKey c, const PairTop& t, int tmp) { return !pair_same(c, t.best) && pair_top_sub(t) - pair_cand_q(c) <= tmp; }

// one entry of the penalty table (:407-408), by the host's libm (host code only)
inline double pair_penalty(int64_t dist, double avg, double std, int a) {
    const double ns = ((double)dist - avg) / std;
    return .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * a;
}
