// The rules of the pairing decision -- what mem_sam_pe does behind mem_pair (reference src/bwamem_pair.cpp:536-590, the same text at :936-992 in the batch
// form) and where it leaves for no_pairing (:632-648, :1032-1048 in the batch form) -- written ONCE on plain values: whether the paired branch is entered,
// is_multi, score_un, subo, q_pe, the two branches of q_se with the cap, the secondary_all swap as a function of one record, the ALT record of an end,
// `which` and the proper-pair flag of the no-pairing paths.  meme_decide.hip's kernel calls them (who reads which record, the ballot and the order of the
// stores stay there); tests/test_decide_rules_model.py compiles this file with g++ into a sequential driver (tests/decide_rules_driver.h) and holds it
// against the model of tests/decide_gen.py and the compiled reference's fixture.  Nothing here depends on the kernel.
//
// Arithmetic: IEEE double, no contraction (the pragma below for clang; -ffp-contract=off for g++).  Logarithms come from a callable the caller supplies,
// lg(k) = log((double)k) for k < PRI_LOG by the host's libm (the table of the primary stage): no log runs on the device.  The one float operation is the
// sum of the two frac_rep (:556), which x86-64 evaluates in float before it widens to double.
#pragma once
#include <stdint.h>

#include "meme_hip.h"
#include "meme_ksort.h"
#include "meme_kswv_rules.h"       // mem_infer_dir
#include "meme_primary_rules.h"    // pri_mapq, PRI_LOG

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// the four ways through the block
constexpr int DEC_PATH_NONE = 0;       // pairing not entered: an end without primaries, mem_pair's score <= 0, or MEM_F_NOPAIRING (:533, :536)
constexpr int DEC_PATH_MULTI = 1;      // left through is_multi (:546)
constexpr int DEC_PATH_UNPAIRED = 2;   // the paired branch, the unpaired alignment preferred (:576-580)
constexpr int DEC_PATH_PAIRED = 3;     // the paired alignment preferred (:559-575)

// mem_approx_mapq_se's options out of the stage's (pri_mapq reads a, b, min_seed_len, mapQ_coef_len and mapQ_coef_fac only)
KS_HD meme_primary_opt dec_pri_opt(const meme_decide_opt& o) {
    const meme_primary_opt p = {o.a, o.b, 0, 0, 0, 0, o.min_seed_len, o.T, 0.f, o.mapQ_coef_len, o.mapQ_coef_fac, 0};
    return p;
}
// :533, :536: the paired branch is entered (o: what mem_pair returned)
KS_HD bool dec_entered(int n_pri0, int n_pri1, int o, int no_pairing) { return !no_pairing && n_pri0 && n_pri1 && o > 0; }
// :542-543: record j of an end's first n_pri makes the end multi
KS_HD bool dec_multi(int j, int secondary, int score, int T) { return j >= 1 && secondary < 0 && score >= T; }
// raw_mapq (:438): truncation towards zero, diff may be negative
KS_HD int dec_raw_mapq(int diff, int a) { return (int)(6.02 * diff / a + .499); }
// :548
KS_HD int dec_score_un(int score0, int score1, int pen_unpaired) { return score0 + score1 - pen_unpaired; }
// :550-556.  subo: mem_pair's sub; f0, f1: frac_rep of record 0 of either end.  *beyond: n_sub + 1 is outside the table (lg is not called, the value means nothing)
template <class LG> KS_HD int dec_q_pe(int o, int subo, int score_un, int n_sub, int a, float f0, float f1, LG&& lg, bool* beyond) {
    subo = subo > score_un ? subo : score_un;
    int q_pe = dec_raw_mapq(o - subo, a);
    if (n_sub > 0) {
        if (n_sub >= PRI_LOG - 1) { *beyond = true; return 0; }
        q_pe -= (int)(4.343 * lg(n_sub + 1) + .499);
    }
    if (q_pe < 0) q_pe = 0;
    if (q_pe > 60) q_pe = 60;
    const float f = f0 + f1;                                                      // (float + float is a float add; the product with .5 widens it)
    return (int)(q_pe * (1. - .5 * f) + .499);
}
// :559
KS_HD bool dec_paired_preferred(int o, int score_un) { return o > score_un; }
// :563-564: c[i] with a parent takes the parent's score as sub and is marked -2
struct DecMarks { int sub, secondary; };
KS_HD DecMarks dec_c_marks(int sub, int secondary, int parent_score) {
    const DecMarks m = {secondary >= 0 ? parent_score : sub, secondary >= 0 ? -2 : secondary};
    return m;
}
// :568-569 and :573-574: q_se of c[i] against q_pe, capped at the tandem-repeat score
KS_HD int dec_q_se_paired(int q_se, int q_pe, int score, int csub, int a) {
    q_se = q_se > q_pe ? q_se : q_pe < q_se + 40 ? q_pe : q_se + 40;
    const int cap = dec_raw_mapq(score - csub, a);
    return q_se < cap ? q_se : cap;
}
// :582-583: the swap is taken (k: secondary_all of record z as it is before the swap)
KS_HD bool dec_swap_taken(int k, int n_pri) { return k >= 0 && k < n_pri; }
// :585-588 for record j of all the end's records: its secondary_all behind the swap.  A function of the record alone, so a sequential loop and a lane per
// record agree: z itself ends with -1 whatever the loop gave it (:588), every other record is judged by its old value and its index (:586-587)
KS_HD int dec_swapped(int j, int secondary_all, int k, int z) { return j == z ? -1 : secondary_all == k || j == k ? z : secondary_all; }
// :603-605: the ALT record the paired branch reports behind the end's own, or -1 (the fields are those of record n_pri; anything where n_pri == n)
KS_HD int dec_alt(int n_pri, int n, int score, int secondary, int is_alt, int T) { return n_pri < n && score >= T && secondary < 0 && is_alt ? n_pri : -1; }
// :634-639: the record an end reports on the no-pairing paths (score0: of record 0; score_alt: of record n_pri; anything where they do not exist)
KS_HD int dec_which(int n, int n_pri, int score0, int score_alt, int T) { return n > 0 && score0 >= T ? 0 : n > 0 && n_pri < n && score_alt >= T ? n_pri : -1; }
// :643-647: the proper-pair bit of the no-pairing paths.  rid0, rid1: of the records `which` names (-1 where which < 0, as mem_reg2aln gives for no record);
// rb0, rb1: of record 0 of either end, whatever `which` is (read only where both ends report a record, so both have one)
KS_HD int dec_flag_unpaired(int no_pairing, int rid0, int rid1, int64_t l_pac, int64_t rb0, int64_t rb1, const meme_pair_pes* pes) {
    if (no_pairing || rid0 != rid1 || rid0 < 0) return 1;
    int64_t dist;
    const int d = mem_infer_dir(l_pac, rb0, rb1, &dist);
    const int32_t low = d == 0 ? pes[0].low : d == 1 ? pes[1].low : d == 2 ? pes[2].low : pes[3].low;
    const int32_t high = d == 0 ? pes[0].high : d == 1 ? pes[1].high : d == 2 ? pes[2].high : pes[3].high;
    const int32_t failed = d == 0 ? pes[0].failed : d == 1 ? pes[1].failed : d == 2 ? pes[2].failed : pes[3].failed;
    return !failed && dist >= low && dist <= high ? 3 : 1;
}
