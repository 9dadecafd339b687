// The rules of mate rescue's record updates -- what mem_sam_pe_batch_post does with the kswr_t results before it marks primaries (reference src/bwamem_pair.cpp:851-921),
// with mem_matesw_batch_post (:1225-1334), mem_matesw_batch_post_mate_sort (:1337-1485), mem_sort_dedup_patch (src/bwamem.cpp:385-446) and mem_dedup_patch (:258-308)
// as they run with bns == 0 -- written ONCE on plain values: which records of an end are looked at, where their four gar entries stand, the record a result becomes,
// the two insertions, the two clean-ups and the driver of one end (rescue_end).  meme_rescue.hip runs the driver on every lane of a wavefront (the same loads, the same
// stores) and gives it the lanes for the skip mask; tests/test_rescue_rules_model.py compiles this file with g++ and runs it sequentially.
//
// Not restated here: mem_infer_dir, mate_skip_mask, mate_tries, mate_window and mate_is_job (meme_kswv_rules.h: the posing step asks the same questions), the two
// orders, the redundancy walk, the identical-hit pass and the column idiom (meme_finish_rules.h), klib's introsort (meme_ksort.h: mem_ars2 is no total order, so
// where records of equal end land decides what the walk compares).  The records never move: the sorts, the insertions and the compactions permute the column FIN_ORD.
#pragma once
#include <stdint.h>

#include "meme_hip.h"
#include "meme_ksort.h"
#include "meme_kswv_rules.h"
#include "meme_finish_rules.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// a new record's is_alt bits travel in a column the walk with bns == 0 never reads (sub of a new record is 0, :1302)
constexpr int RES_ISALT = FIN_SUB;

// ---- the records of an end that are looked at, and their gar entries ------------------------------------------------------------------------
// b[i] holds the records within pen_unpaired of the end's first (:854-857) ...
KS_HD bool res_is_anchor(int score, int score0, int pen_unpaired) { return score >= score0 - pen_unpaired; }
// ... and the loops take the first max_matesw of them (:877, :898).  score(k) = the score of record k of the end AS IT WAS HANDED OVER (b[] is a snapshot)
template <class SC>
KS_HD int res_anchor_count(int n, SC&& score, int pen_unpaired, int max_matesw) {
    int na = 0;
    for (int k = 0; k < n && na < max_matesw; ++k) na += res_is_anchor(score(k), score(0), pen_unpaired) ? 1 : 0;
    return na;
}
// gcnt advances by 4 per record looked at, end 0's before end 1's, pair after pair, from 0 at the first read of a worker batch (:884, :904; worker_sam resets it
// per batch): with off[r] = the records looked at of the reads before r, the first gar entry of read r's records, relative to its batch's gar
KS_HD int64_t res_batch_first(int64_t r, int batch_reads) { return r / batch_reads * batch_reads; }
KS_HD int64_t res_cursor(int64_t off_r, int64_t off_batch_first) { return 4 * (off_r - off_batch_first); }
// the path of a pair: the mate-sort functions only where both lists came out of mem_sort_dedup_patch_mate_sort without equal ends (:865-872)
KS_HD bool res_mate_sort(int ums0, int ums1) { return ums0 && ums1; }
// a list the driver has to walk: a result may be pushed into it, or -- on the mate-sort path -- its order may change as soon as the other end has a record (:874-875,
// :891: sorted by end, then by score; a list of at most one record has one order)
KS_HD bool res_listed(int n_posed, bool mate_sort, int n_other, int n_in) { return n_posed > 0 || (mate_sort && n_other > 0 && n_in > 1); }

// ---- the record a result becomes (:1302-1313, :1419-1430) -------------------------------------------------------------------------------------
KS_HD bool res_taken(const meme_kswr& aln, int min_seed_len) { return aln.score >= min_seed_len && aln.qb >= 0; }      // "something goes wrong if aln.qb < 0"
struct ResAnchor { int64_t rb; int rid, score, is_alt; };
struct ResRec { int64_t rb, re; int qb, qe, rid, is_alt, score, csub, seedcov; };      // every other byte of the record is 0, secondary = -1
KS_HD ResRec res_record(const meme_kswr& aln, const ResAnchor& a, bool is_rev, int64_t rb, int l_ms, int64_t l_pac) {
    ResRec b;
    b.rid = a.rid; b.is_alt = a.is_alt;
    b.qb = is_rev ? l_ms - (aln.qe + 1) : aln.qb;
    b.qe = is_rev ? l_ms - aln.qb : aln.qe + 1;
    b.rb = is_rev ? (l_pac << 1) - (rb + aln.te + 1) : rb + aln.tb;
    b.re = is_rev ? (l_pac << 1) - (rb + aln.tb) : rb + aln.te + 1;
    b.score = aln.score; b.csub = aln.score2;
    b.seedcov = (int)((b.re - b.rb < b.qe - b.qb ? b.re - b.rb : b.qe - b.qb) >> 1);
    return b;
}
template <class S> KS_HD void res_put(const S& s, int x, const ResRec& b) {
    s.setl(FIN_RB, x, b.rb); s.setl(FIN_RE, x, b.re);
    s.seti(FIN_QB, x, b.qb); s.seti(FIN_QE, x, b.qe); s.seti(FIN_RID, x, b.rid); s.seti(FIN_SCORE, x, b.score); s.seti(FIN_CSUB, x, b.csub); s.seti(FIN_SEEDCOV, x, b.seedcov);
    s.seti(FIN_NCOMP, x, 0); s.seti(RES_ISALT, x, b.is_alt);
}
// n_comp:30, is_alt:2 of a record that leaves the stage: an old record keeps its is_alt bits, a new one has its anchor's
KS_HD int res_word_old(int word_in, int n_comp) { return (int)(((uint32_t)word_in & 0xc0000000u) | ((uint32_t)n_comp & 0x3fffffffu)); }
KS_HD int res_word_new(int is_alt, int n_comp) { return (int)(((uint32_t)is_alt << 30) | ((uint32_t)n_comp & 0x3fffffffu)); }
KS_HD int res_is_alt_of(int word) { return (int)((uint32_t)word >> 30); }

// ---- the list: n records in the order FIN_ORD ---------------------------------------------------------------------------------------------------
template <class S> KS_HD void res_sort_re(const S& s, int n, FinStack& st) { st.n = 0; ks_introsort(FinOrd<S>{s}, n, FinLtEnd<S>{s}, st); }          // sort_alnreg_re (src/bwamem.cpp:181)
template <class S> KS_HD void res_sort_score(const S& s, int n, FinStack& st) { st.n = 0; ks_introsort(FinOrd<S>{s}, n, FinLtScore<S>{s}, st); }     // sort_alnreg_score (:185)
// record x in front of position `at` (:1321-1322, :1464-1465, :1472-1473)
template <class S> KS_HD void res_insert(const S& s, int n, int at, int x) {
    for (int i = n; i > at; --i) s.seti(FIN_ORD, i, s.geti(FIN_ORD, i - 1));
    s.seti(FIN_ORD, at, x);
}
// mem_dedup_patch with bns == 0 (:258-308): the list as it stands, nothing sorted
template <class S> KS_HD int res_dedup_patch(const S& s, int n, const meme_rescue_opt& o) {
    if (n <= 1) return n;                                                          // :263 (n_comp stays)
    const FinOrd<S> ord = {s};
    for (int i = 0; i < n; ++i) s.seti(FIN_NCOMP, ord.get(i), 1);
    fin_walk(s, ord, n, (int64_t)o.max_chain_gap, o.mask_level_redun, [](int, int, const FinSpan&, const FinSpan&) {});       // mem_patch_reg returns 0 (:200)
    return fin_compact(s, ord, n, 0);
}
// mem_sort_dedup_patch with bns == 0 (:385-446)
template <class S> KS_HD int res_sort_dedup_patch(const S& s, int n, const meme_rescue_opt& o, FinStack& st) {
    if (n <= 1) return n;                                                          // :390
    res_sort_re(s, n, st);
    n = res_dedup_patch(s, n, o);                                                  // (:393-434: the same text; n > 1 here)
    res_sort_score(s, n, st);
    return fin_identical(s, FinOrd<S>{s}, n);
}
// the plain insertion (:1315-1322): in front of the first record with a smaller score
template <class S> KS_HD int res_insert_plain(const S& s, int n, int x) {
    const int score = s.geti(FIN_SCORE, x);
    int at = 0;
    while (at < n && !(s.geti(FIN_SCORE, s.geti(FIN_ORD, at)) < score)) ++at;
    res_insert(s, n, at, x);
    return n + 1;
}
// the mate-sort insertion (:1431-1474): by end; where an equal end is met nobody knows the place, and the scores decide
template <class S> KS_HD int res_insert_mate_sort(const S& s, int n, int x, FinStack& st, int* n_resort) {
    const int64_t re = s.getl(FIN_RE, x);
    bool resort = false;
    int at = 0;
    for (; at < n; ++at) {
        const int64_t e = s.getl(FIN_RE, s.geti(FIN_ORD, at));
        if (e == re) { resort = true; break; }
        if (e > re) break;
    }
    if (!resort) { res_insert(s, n, at, x); return n + 1; }
    ++*n_resort;
    res_sort_score(s, n, st);
    n = fin_identical(s, FinOrd<S>{s}, n);
    n = res_insert_plain(s, n, x);                                                 // (:1457-1465: over all n records)
    res_sort_re(s, n, st);
    return n;
}

// ---- the driver of one end (:864-907 for i, with the post function of the pair's path) ----------------------------------------------------------
// s holds the n_in records of the list that is written (the mate's, a[!i]) in positions [0, n_in), FIN_NCOMP = the n_comp they carry, and has room for `cap`; the
// other end's n_other records are read as they were handed over:
//   anchor(k)            ResAnchor of its record k
//   skip(rb, n)          mate_skip_mask of a record at rb over the n records the list holds NOW (:1244-1249: a record pushed for an earlier anchor can switch an
//                        orientation off, a removed one on again)
//   clamp(mid, rb, re)   bns_fetch_seq's clamp of the window to the sequence of its midpoint -> rid
//   job(q, o, &aln)      the result of orientation o of the q-th record looked at; false: gar holds -1 or an index outside the jobs -- the reference would call
//                        ksw_align2 (:1290-1296)
// -> the records left (their order: the first entries of FIN_ORD), or -1 with out->status = 1: the caller hands the list back as it came.
struct ResRead { int status, n_tested, n_pushed, n_resort; };
template <class S, class AN, class SK, class CL, class JB>
KS_HD int rescue_end(const S& s, int n_in, int cap, int n_other, AN&& anchor, bool mate_sort, int l_ms, int64_t l_pac, const meme_pestat* pes, SK&& skip, CL&& clamp, JB&& job,
                     const meme_rescue_opt& o, FinStack& st, ResRead* out) {
    out->status = 0; out->n_tested = 0; out->n_pushed = 0; out->n_resort = 0;
    int n = n_in, n_tot = n_in;
    for (int i = 0; i < n_in; ++i) s.seti(FIN_ORD, i, i);
    if (n_other <= 0) return n;                                                    // b[i].n == 0 (:874; the plain loops do not turn)
    if (mate_sort) res_sort_re(s, n, st);                                          // :875
    const int score0 = anchor(0).score;
    int swcount = 0;
    for (int k = 0, q = 0; k < n_other && q < o.max_matesw; ++k) {
        const ResAnchor a = anchor(k);
        if (!res_is_anchor(a.score, score0, o.pen_unpaired)) continue;
        const int mask = skip(a.rb, n);
        int nj = 0, rid = -1;                                                      // (rid is carried from one orientation to the next, :1238)
        for (int r = 0; r < 4; ++r) {
            if (!mate_tries(mask, r)) continue;                                    // :1252-1254, :1260
            const MateWindow W = mate_window(r, pes[r], a.rb, l_ms, l_pac);
            int64_t rb = W.rb, re = W.re;
            if (rb < re) rid = clamp((rb + re) >> 1, rb, re);
            if (mate_is_job(a.rid, rid, rb, re, o.min_seed_len)) {
                meme_kswr aln;
                if (!job(q, r, &aln) || n_tot >= cap) { out->status = 1; return -1; }
                if (res_taken(aln, o.min_seed_len)) {
                    res_put(s, n_tot, res_record(aln, a, W.is_rev != 0, rb, l_ms, l_pac));
                    n = mate_sort ? res_insert_mate_sort(s, n, n_tot, st, &out->n_resort) : res_insert_plain(s, n, n_tot);
                    ++n_tot; ++out->n_pushed;
                }
                ++nj;
            }
            if (nj) n = mate_sort ? res_dedup_patch(s, n, o) : res_sort_dedup_patch(s, n, o, st);      // :1479, :1328: inside the loop, once n > 0
        }
        out->n_tested += nj; swcount += nj;
        ++q;
    }
    if (mate_sort) {                                                               // :886-892
        if (swcount > 0) n = res_sort_dedup_patch(s, n, o, st);
        else res_sort_score(s, n, st);
    }
    return n;
}
