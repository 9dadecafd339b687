// The rules of record finishing -- the tail of mem_kernel2_core (reference src/bwamem.cpp:1681-1719): the compaction of a read's alignment records to
// the live ones, mem_sort_dedup_patch_mate_sort (:312-383) with mem_patch_reg (:194-244) and the is_alt flag -- written ONCE on plain values: the two
// orders, the redundancy test, the bars of mem_patch_reg, what a patch alignment is (bwa_gen_cigar2 asked for its score only, src/bwa.cpp:274-322), the
// merge, the useMateSort scan, the identical-hit pass, the is_alt bit, and the sequential driver that performs the whole function for one read
// (finish_read).  meme_finish.hip runs the driver on every lane of a wavefront (the same loads, the same stores) and gives it the lanes only for
// the patch score; tests/test_finish_rules_model.py compiles this file with g++ and gives it the scalar score routine below (fin_patch_score).
//
// Arithmetic: the redundancy test in float, mem_patch_reg in IEEE double with the constants as floats, no contraction (the pragma below for clang;
// -ffp-contract=off for g++).  Both sorts are klib's ks_introsort (meme_ksort.h): mem_ars2 is no total order and the walk depends on where equal
// ends land, so ranks by counting would not do.  The records themselves never move: the sorts and the compactions permute the column FIN_ORD.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "meme_hip.h"
#include "meme_ksort.h"
#include "meme_gcig_rules.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr int FIN_MAX_QLEN = 500;            // a patch's query is a span of a read: LEARNED_MAX_READ_LEN
constexpr int FIN_MAX_TLEN = 1 << 16;        // the longest target span a patch is aligned over (a record of a 500-base read spans hundreds of bases; the stage's bound on a row loop)
constexpr int FIN_STACK = 64;                // entries of the introsort's stack (at most log2(n / 16) + 1 are live)
constexpr float FIN_PATCH_MAX_R_BW = 0.05f;  // PATCH_MAX_R_BW, PATCH_MIN_SC_RATIO (:191-192)
constexpr float FIN_PATCH_MIN_SC_RATIO = 0.90f;

// What the function reads and writes of a record, as columns: `int geti(f, i)`, `void seti(f, i, v)` for the int fields, `int64_t getl(f, i)`,
// `void setl(f, i, v)` for rb and re.  FIN_ORD is the permutation: position k of the current order holds record geti(FIN_ORD, k).
enum { FIN_QB, FIN_QE, FIN_RID, FIN_SCORE, FIN_TRUESC, FIN_SUB, FIN_CSUB, FIN_SEEDCOV, FIN_W, FIN_NCOMP, FIN_ORD, FIN_INTS };
enum { FIN_RB, FIN_RE, FIN_LONGS };
struct FinCols {                             // plain arrays, `cap` entries per column
    int* c; long long* l; int cap;
    KS_HD int geti(int f, int i) const { return c[(size_t)f * cap + i]; }
    KS_HD void seti(int f, int i, int v) const { c[(size_t)f * cap + i] = v; }
    KS_HD int64_t getl(int f, int i) const { return l[(size_t)f * cap + i]; }
    KS_HD void setl(int f, int i, int64_t v) const { l[(size_t)f * cap + i] = v; }
};
struct FinStack {                            // ks_introsort's stack in memory the caller owns (3 * FIN_STACK ints)
    int* v; int n;
    KS_HD void push(int l, int r, int d) { if (n < FIN_STACK) { v[3 * n] = l; v[3 * n + 1] = r; v[3 * n + 2] = d; ++n; } }
    KS_HD bool pop(int& l, int& r, int& d) { if (!n) return false; --n; l = v[3 * n]; r = v[3 * n + 1]; d = v[3 * n + 2]; return true; }
};
template <class S> struct FinOrd {           // the order as ks_introsort's array
    S s;
    KS_HD int get(int i) const { return s.geti(FIN_ORD, i); }
    KS_HD void set(int i, int v) const { s.seti(FIN_ORD, i, v); }
};
// mem_ars2 (alnreg_slt2, src/bwamem.cpp:170): by the end on the reference only
template <class S> struct FinLtEnd {
    S s;
    KS_HD bool operator()(int x, int y) const { return s.getl(FIN_RE, x) < s.getl(FIN_RE, y); }
};
// mem_ars (alnreg_slt, :173): score descending, then rb, then qb
template <class S> struct FinLtScore {
    S s;
    KS_HD bool operator()(int x, int y) const {
        const int sx = s.geti(FIN_SCORE, x), sy = s.geti(FIN_SCORE, y);
        if (sx != sy) return sx > sy;
        const int64_t bx = s.getl(FIN_RB, x), by = s.getl(FIN_RB, y);
        return bx < by || (bx == by && s.geti(FIN_QB, x) < s.geti(FIN_QB, y));
    }
};

// one of two hits is redundant (:332-336): both overlaps exceed mask_level_redun of the shorter span, compared in float
KS_HD bool fin_redundant(int64_t or_, int64_t oq, int64_t mr, int64_t mq, float mask_level_redun) {
    return (float)or_ > mask_level_redun * (float)mr && (float)oq > mask_level_redun * (float)mq;
}

// mem_patch_reg up to its alignment (:203-223): false = no merge; else *w = the band bwa_gen_cigar2 is asked with
struct FinSpan { int64_t rb, re; int qb, qe, score, w; };
KS_HD bool fin_patch_bars(const FinSpan& a, const FinSpan& b, int64_t l_pac, int opt_w, int* w_out) {
    if (a.rb < l_pac && b.rb >= l_pac) return false;                              // on different strands
    if (a.qb >= b.qb || a.qe >= b.qe || a.re >= b.re) return false;               // not colinear
    int w = (int)((a.re - b.rb) - (a.qe - b.qb));
    w = w > 0 ? w : -w;
    double r = (double)(a.re - b.rb) / (double)(b.re - a.rb) - (double)(a.qe - b.qb) / (double)(b.qe - a.qb);
    r = r > 0. ? r : -r;
    if (a.re < b.rb || a.qe < b.qb) {                                              // no overlap on the query or on the reference
        if (w > opt_w << 1 || r >= FIN_PATCH_MAX_R_BW) return false;
    } else if (w > opt_w << 2 || r >= FIN_PATCH_MAX_R_BW * 2) return false;
    w += a.w + b.w;
    *w_out = w < opt_w << 2 ? w : opt_w << 2;
    return true;
}
// ... and behind it (:232-241): whether the alignment's score stands against the score predicted from the two records (a zero denominator divides as IEEE does)
KS_HD bool fin_patch_ratio(const FinSpan& a, const FinSpan& b, int score) {
    const int q_s = (int)((double)(b.qe - a.qb) / ((b.qe - b.qb) + (a.qe - a.qb)) * (b.score + a.score) + .499);
    const int r_s = (int)((double)(b.re - a.rb) / (double)((b.re - b.rb) + (a.re - a.rb)) * (b.score + a.score) + .499);
    return !((double)score / (double)(q_s > r_s ? q_s : r_s) < FIN_PATCH_MIN_SC_RATIO);
}

// The alignment mem_patch_reg asks bwa_gen_cigar2 for: query span [qb, qe) of the read against [rb, re) of the fwd + rc text.  ok == false: the call the
// reference's function returns from without writing the score (an empty span, a target bridging the strands or outside the text), or one beyond this
// stage's bounds (FIN_MAX_QLEN, FIN_MAX_TLEN, a query span outside the read).  rev: both sequences reversed (rb >= l_pac, src/bwa.cpp:288-293); w: the band
// ksw_global2 gets, -1 for the gap-free shortcut.
struct FinPose { bool ok, rev; int qlen, tlen, w; };
KS_HD FinPose fin_pose(int64_t l_pac, int qb, int qe, int read_len, int64_t rb, int64_t re, int w_, const meme_finish_opt& o) {
    FinPose P = {false, false, 0, 0, 0};
    if (qb < 0 || qe <= qb || qe > read_len || qe - qb > FIN_MAX_QLEN) return P;
    if (rb < 0 || rb >= re || re > 2 * l_pac || (rb < l_pac && re > l_pac) || re - rb > FIN_MAX_TLEN) return P;
    P.ok = true;
    P.rev = rb >= l_pac;
    P.qlen = qe - qb;
    P.tlen = (int)(re - rb);
    const meme_bsw_opt bo = {o.o_del, o.e_del, o.o_ins, o.e_ins, 0, 0, o.a, o.b};
    P.w = gcig_band(P.qlen, P.tlen, w_, bo);
    return P;
}

// ksw_global2 for its score alone (src/ksw.cpp:631-651), scalar: q(j), t(i) = the codes of the (possibly reversed) sequences; h, e: qlen + 1 ints each
template <class Q, class T>
KS_HD int fin_global_score(int qlen, Q&& q, int tlen, T&& t, int w, const meme_finish_opt& o, int* h, int* e) {
    const int oe_del = o.o_del + o.e_del, oe_ins = o.o_ins + o.e_ins;
    for (int j = 0; j <= qlen; ++j) { h[j] = gcig_row0(j, w, o.o_ins, o.e_ins); e[j] = GCIG_MINUS_INF; }
    for (int i = 0; i < tlen; ++i) {
        const int beg = gcig_beg(i, w), end = gcig_end(i, w, qlen), tb = t(i);
        int f = GCIG_MINUS_INF, h1 = gcig_left(i, beg, o.o_del, o.e_del);
        for (int j = beg; j < end; ++j) {
            const int m = h[j] + gcig_score(tb, q(j), o.a, o.b);
            const GcigCell c = gcig_cell(m, e[j], f, oe_del, o.e_del, oe_ins, o.e_ins);
            h[j] = h1;
            h1 = c.h; e[j] = c.e; f = c.f;
        }
        if (end >= 0 && end <= qlen) { h[end] = h1; e[end] = GCIG_MINUS_INF; }
    }
    return h[qlen];
}
// the score of a posed alignment, scalar: text(p) = the base at position p of the fwd + rc text, read(j) = base j of the read
template <class TX, class RD>
KS_HD int fin_patch_score(const FinPose& P, int64_t rb, int qb, TX&& text, RD&& read, const meme_finish_opt& o, int* h, int* e) {
    const auto q = [&](int j) -> int { return read(qb + (P.rev ? P.qlen - 1 - j : j)); };
    const auto t = [&](int i) -> int { return text(rb + (P.rev ? P.tlen - 1 - i : i)); };
    if (P.w < 0) {
        int score = 0;
        for (int j = 0; j < P.qlen; ++j) score += gcig_score(t(j), q(j), o.a, o.b);
        return score;
    }
    return fin_global_score(P.qlen, q, P.tlen, t, P.w, o, h, e);
}

// n_comp:30, is_alt:2 of a record that leaves the function (:1713-1718): the count the function left, is_alt = 1 where the record's sequence is an ALT contig
KS_HD int fin_word(int word_in, int n_comp, int rid, const unsigned char* alt, int n_contigs) {
    const uint32_t w = ((uint32_t)word_in & 0xc0000000u) | ((uint32_t)n_comp & 0x3fffffffu);
    return (int)(rid >= 0 && rid < n_contigs && alt[rid] ? (w & 0x3fffffffu) | (1u << 30) : w);
}

// what the driver reports besides the records
struct FinRead { int use_mate_sort, status, n_jobs, n_merged; };

// The redundancy walk over n records in the order by end (:321-355; the same text in mem_sort_dedup_patch :394-428 and mem_dedup_patch :266-300): a record whose
// overlaps with an earlier one exceed mask_level_redun loses against the higher score (qe = qb); for the others patch(p, q, a, b) stands where the reference calls
// mem_patch_reg and merges.  With bns == 0 that function returns 0 (:200): mate rescue's callers hand a patch that does nothing (meme_rescue_rules.h).
template <class S, class P>
KS_HD void fin_walk(const S& s, const FinOrd<S>& ord, int n, int64_t gap, float mask_level_redun, P&& patch) {
    for (int i = 1; i < n; ++i) {
        const int p = ord.get(i), prev = ord.get(i - 1);
        const int p_rid = s.geti(FIN_RID, p);
        if (p_rid != s.geti(FIN_RID, prev) || s.getl(FIN_RB, p) >= s.getl(FIN_RE, prev) + gap) continue;
        for (int j = i - 1; j >= 0; --j) {
            const int q = ord.get(j);
            if (!(p_rid == s.geti(FIN_RID, q) && s.getl(FIN_RB, p) < s.getl(FIN_RE, q) + gap)) break;
            FinSpan a = {s.getl(FIN_RB, q), s.getl(FIN_RE, q), s.geti(FIN_QB, q), s.geti(FIN_QE, q), s.geti(FIN_SCORE, q), s.geti(FIN_W, q)};
            FinSpan b = {s.getl(FIN_RB, p), s.getl(FIN_RE, p), s.geti(FIN_QB, p), s.geti(FIN_QE, p), s.geti(FIN_SCORE, p), s.geti(FIN_W, p)};
            if (a.qe == a.qb) continue;                                            // a[j] has been excluded
            const int64_t or_ = a.re - b.rb, oq = a.qb < b.qb ? a.qe - b.qb : b.qe - a.qb;
            const int64_t mr = a.re - a.rb < b.re - b.rb ? a.re - a.rb : b.re - b.rb, mq = a.qe - a.qb < b.qe - b.qb ? a.qe - a.qb : b.qe - b.qb;
            if (fin_redundant(or_, oq, mr, mq, mask_level_redun)) {
                if (b.score < a.score) { s.seti(FIN_QE, p, b.qb); break; }
                s.seti(FIN_QE, q, a.qb);
            } else if (a.rb < b.rb) patch(p, q, a, b);
        }
    }
}
// the records of the order that are left (qe > qb), from position `from` on, closed up (:356-362, :376-380); -> their number
template <class S>
KS_HD int fin_compact(const S& s, const FinOrd<S>& ord, int n, int from) {
    int m = n < from ? n : from;
    for (int i = from; i < n; ++i) {
        const int x = ord.get(i);
        if (s.geti(FIN_QE, x) > s.geti(FIN_QB, x)) ord.set(m++, x);
    }
    return m;
}
// the identical-hit pass over n records in the order by score (:372-381): a record equal to its predecessor in score, rb and qb leaves; element 0 stays whatever it holds (:376)
template <class S>
KS_HD int fin_identical(const S& s, const FinOrd<S>& ord, int n) {
    for (int i = 1; i < n; ++i) {
        const int x = ord.get(i), y = ord.get(i - 1);
        if (s.geti(FIN_SCORE, x) == s.geti(FIN_SCORE, y) && s.getl(FIN_RB, x) == s.getl(FIN_RB, y) && s.geti(FIN_QB, x) == s.geti(FIN_QB, y)) s.seti(FIN_QE, x, s.geti(FIN_QB, x));
    }
    return fin_compact(s, ord, n, 1);
}

// The whole function for one read.  s holds the read's n_in records as they are handed over (live and purged) in positions [0, n_in) with FIN_NCOMP = the
// n_comp they carry; on return the first m entries of FIN_ORD name the records that are left, in their final order, and their fields are as the function
// leaves them (m is returned).  score_fn(P, rb, qb) = the score of the posed alignment P whose target starts at rb and whose query starts at base qb of the read.
// Every loop is bounded by n_in; the comparators read inside [0, n).
template <class S, class SC>
KS_HD int finish_read(const S& s, int n_in, int read_len, int64_t l_pac, const meme_finish_opt& o, SC&& score_fn, FinStack& st, FinRead* out) {
    out->use_mate_sort = 1; out->status = 0; out->n_jobs = 0; out->n_merged = 0;
    int n = 0;
    for (int i = 0; i < n_in; ++i)                                                 // :1689-1693
        if (s.geti(FIN_QE, i) > s.geti(FIN_QB, i)) s.seti(FIN_ORD, n++, i);
    if (n <= 1) return n;                                                          // :317 (a lone record keeps its n_comp)
    const FinOrd<S> ord = {s};
    st.n = 0;
    ks_introsort(ord, n, FinLtEnd<S>{s}, st);
    for (int i = 0; i < n; ++i) s.seti(FIN_NCOMP, ord.get(i), 1);
    fin_walk(s, ord, n, (int64_t)o.max_chain_gap, o.mask_level_redun, [&](int p, int q, const FinSpan& a, const FinSpan& b) {
        int w = 0;
        if (!fin_patch_bars(a, b, l_pac, o.w, &w)) return;
        ++out->n_jobs;
        const FinPose P = fin_pose(l_pac, a.qb, b.qe, read_len, a.rb, b.re, w, o);
        if (!P.ok) { out->status = 1; return; }                                    // (the reference reads a score nobody wrote)
        const int score = score_fn(P, a.rb, a.qb);
        if (!fin_patch_ratio(a, b, score) || score <= 0) return;
        ++out->n_merged;                                                           // merge q into p (:345-352)
        s.seti(FIN_NCOMP, p, s.geti(FIN_NCOMP, p) + s.geti(FIN_NCOMP, q) + 1);
        const int cq = s.geti(FIN_SEEDCOV, q), sq = s.geti(FIN_SUB, q), csq = s.geti(FIN_CSUB, q);
        if (cq > s.geti(FIN_SEEDCOV, p)) s.seti(FIN_SEEDCOV, p, cq);
        if (sq > s.geti(FIN_SUB, p)) s.seti(FIN_SUB, p, sq);
        if (csq > s.geti(FIN_CSUB, p)) s.seti(FIN_CSUB, p, csq);
        s.seti(FIN_QB, p, a.qb); s.setl(FIN_RB, p, a.rb);
        s.seti(FIN_SCORE, p, score); s.seti(FIN_TRUESC, p, score);
        s.seti(FIN_W, p, w);
        s.seti(FIN_QB, q, a.qe);
    });
    n = fin_compact(s, ord, n, 0);                                                 // :356-362
    for (int i = 0; i + 1 < n; ++i)                                                // :363-370
        if (s.getl(FIN_RE, ord.get(i)) == s.getl(FIN_RE, ord.get(i + 1))) { out->use_mate_sort = 0; break; }
    st.n = 0;
    ks_introsort(ord, n, FinLtScore<S>{s}, st);
    return fin_identical(s, ord, n);
}
