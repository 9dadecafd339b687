// The rules of mem_chain2aln_across_reads_V2 (reference src/bwamem.cpp:2573-3497), of mem_seed_sw / mem_flt_chained_seeds (:494-598) and of bns_fetch_seq
// (src/bntseq.cpp:479-570) that the extension kernels of meme_ext.hip and the posing kernel of meme_mate.hip apply, written ONCE on plain values: the kernels
// differ in who walks a read's seeds (a lane, eight lanes, a wavefront) and in where the records live, not in these.  tests/test_ext_rules_model.py compiles
// this header with g++ into a scalar mem_chain2aln and holds it against the compiled reference's records.
#pragma once
#include <stdint.h>
#include <string.h>

#include "meme_hip.h"
#include "meme_ksort.h"      // KS_HD

constexpr int H0 = -99;                    // H0_, src/macro.h:44
constexpr int EXT_BAND_TRIES = 2;          // MAX_BAND_TRY, src/bwamem.cpp:62
constexpr int SEEDSW_EXT = 50;             // MEM_SHORT_EXT, src/bwamem.cpp:249
constexpr int FLT_OFF = INT32_MIN;         // score of a chained seed of a read the seed filter does not run for (:583)

KS_HD int ext_max_gap(const meme_ext_opt& o, int qlen) {       // cal_max_gap, src/bwamem.cpp:85-95
    const int l_del = (int)((double)(qlen * o.a - o.o_del) / o.e_del + 1.);
    const int l_ins = (int)((double)(qlen * o.a - o.o_ins) / o.e_ins + 1.);
    int l = l_del > l_ins ? l_del : l_ins;
    l = l > 1 ? l : 1;
    return l < o.w << 1 ? l : o.w << 1;
}

// ---- spans of the reference --------------------------------------------------------------------------------------------------------------
struct ExtSpan { int64_t b, e; };
// the widest [b, e) the extensions of one seed may reach (:2648-2690)
KS_HD ExtSpan ext_seed_reach(const meme_chain_seed& t, int l_query, const meme_ext_opt& o) {
    const int tail = l_query - t.qbeg - t.len;
    return ExtSpan{t.rbeg - (t.qbeg + ext_max_gap(o, t.qbeg)), t.rbeg + t.len + (tail + ext_max_gap(o, tail))};
}
// a span finished: inside the fwd + rc text, and on the strand of `mid` where it bridges the two
KS_HD void ext_span_finish(int64_t& rb, int64_t& re, int64_t mid, int64_t l_pac) {
    rb = rb > 0 ? rb : 0;
    re = re < l_pac << 1 ? re : l_pac << 1;
    if (rb < l_pac && l_pac < re) { if (mid < l_pac) re = l_pac; else rb = l_pac; }
}
// bns_fetch_seq: the span stays inside one reference sequence (offset, len on the forward strand), seen from the strand it lies on
KS_HD void bns_clamp(int64_t l_pac, int64_t offset, int len, bool rev, int64_t& rb, int64_t& re) {
    int64_t far_beg = offset, far_end = offset + len;
    if (rev) { const int64_t t = far_beg; far_beg = (l_pac << 1) - far_end; far_end = (l_pac << 1) - t; }
    rb = rb > far_beg ? rb : far_beg;
    re = re < far_end ? re : far_end;
}
// the last reference sequence whose offset is <= fpos (bns_pos2rid)
KS_HD int bns_contig_of(const int64_t* contig_off, int n_contigs, int64_t fpos) {
    int lo = 0, hi = n_contigs - 1;
    while (lo < hi) { const int m = (lo + hi + 1) >> 1; if (contig_off[m] <= fpos) lo = m; else hi = m - 1; }
    return lo;
}
// the two together for a span that knows its midpoint only: clamped to the midpoint's sequence on the midpoint's strand; returns that sequence
KS_HD int bns_clamp_to_mid(int64_t l_pac, const int64_t* contig_off, const int* contig_len, int n_contigs, int64_t mid, int64_t& rb, int64_t& re) {
    const bool rev = mid >= l_pac;
    const int rid = bns_contig_of(contig_off, n_contigs, rev ? (l_pac << 1) - 1 - mid : mid);
    bns_clamp(l_pac, contig_off[rid], contig_len[rid], rev, rb, re);
    return rid;
}

// ---- mem_flt_chained_seeds ---------------------------------------------------------------------------------------------------------------
// the alignment mem_seed_sw runs for a chained seed (:494-520): SEEDSW_EXT bases around it on the read and on the reference; no job for a seed or a
// window of short_len (MEM_SHORT_LEN) and more
struct FltWindow { bool job; int64_t rb, re; int qb, qe; };
KS_HD FltWindow flt_window(const meme_chain_seed& t, int l_query, int64_t l_pac, const int64_t* contig_off, const int* contig_len, int n_contigs, int short_len) {
    FltWindow W{false, t.rbeg - SEEDSW_EXT, t.rbeg + t.len + SEEDSW_EXT, t.qbeg - SEEDSW_EXT, t.qbeg + t.len + SEEDSW_EXT};
    if (t.len >= short_len) return W;
    const int64_t mid = (t.rbeg + t.rbeg + t.len) >> 1;
    W.qb = W.qb > 0 ? W.qb : 0; W.qe = W.qe < l_query ? W.qe : l_query;
    ext_span_finish(W.rb, W.re, mid, l_pac);
    if (W.qe - W.qb >= short_len || W.re - W.rb >= short_len) return W;
    bns_clamp_to_mid(l_pac, contig_off, contig_len, n_contigs, mid, W.rb, W.re);
    W.job = true;
    return W;
}
// The base at position p of the window is the one the REFERENCE's call reads, which is not the genome's: mem_kernel1_core_Learned is handed worker_t::rc_pac
// as `pac` (src/bwamem.cpp:1770) -- the 2-bit fwd + rc text with the four bases of every BYTE in reverse order, as the learned index's key extraction wants
// them (src/fastmap.cpp:440-457; "BitReverseTable256", src/LearnedIndex_seeding.h:129-137, reverses 2-bit groups) -- and bns_get_seq (src/bntseq.cpp:515-539)
// reads it with the plain _get_pac: within every aligned group of four bases the order is reversed; windows on the reverse strand are fetched from the forward
// half and complemented (:526-531).  SAM output depends on it (under -W), so it is reproduced, not corrected.  pos: the position whose 2-bit code is read.
struct FltBase { int64_t pos; bool complement; };
KS_HD FltBase flt_base_index(int64_t l_pac, int64_t p) {
    const int64_t k = p < l_pac ? p : (l_pac << 1) - 1 - p;
    return FltBase{(k & ~(int64_t)3) + 3 - (k & 3), p >= l_pac};
}
// v: FLT_OFF, -1 (no alignment: kept, :502 / :515) or the alignment's score; the seed stays (:589) with the score (:591)
KS_HD bool flt_keeps(int v, int hsp) { return v == FLT_OFF || v < 0 || v >= hsp; }
KS_HD int flt_kept_score(int v, int len, int a) { return v == FLT_OFF ? len : (v < 0 ? len * a : v); }

// ---- the extension jobs of a chained seed ------------------------------------------------------------------------------------------------
KS_HD int pad4(int x) { return (x + 3) & ~3; }
KS_HD int ext_job_bytes(int l1, int l2) { return pad4(l1) + pad4(l2); }       // target, then query, each padded to whole words
KS_HD int ext_query_off(int l1) { return pad4(l1); }                          // ... so the query starts here behind the target
// which flanks the seed has (:2722, :2783), their target (1) and query (2) lengths within the chain's span [rmax0, rmax1), their sequence bytes
struct ExtGeom { bool sideL, sideR; int l1L, l2L, l1R, l2R, bytesL, bytesR; KS_HD int jobs() const { return (int)sideL + (int)sideR; } };
KS_HD ExtGeom ext_geom(const meme_chain_seed& t, int64_t rmax0, int64_t rmax1, int l_query) {
    ExtGeom g;
    const int qe = t.qbeg + t.len;
    g.sideL = t.qbeg > 0; g.sideR = qe != l_query;
    g.l2L = t.qbeg; g.l1L = (int)(t.rbeg - rmax0);
    g.l2R = l_query - qe; g.l1R = (int)(rmax1 - (t.rbeg + t.len));
    g.bytesL = g.sideL ? ext_job_bytes(g.l1L, g.l2L) : 0;
    g.bytesR = g.sideR ? ext_job_bytes(g.l1R, g.l2R) : 0;
    return g;
}
// the SeqPair of one side: sequences at idr (target) and behind it (query)
KS_HD meme_seqpair ext_pose(int h0, int seqid, int regid, int len1, int len2, int idr) {
    meme_seqpair sp;
    memset(&sp, 0, sizeof(sp));
    sp.h0 = h0; sp.seqid = seqid; sp.regid = regid; sp.len1 = len1; sp.len2 = len2; sp.idr = idr; sp.idq = idr + ext_query_off(len1);
    return sp;
}

// ---- alignment records -------------------------------------------------------------------------------------------------------------------
// the order a chain's seeds are extended in, worst first: ks_introsort_64 on score << 32 | index (:2692-2699; keys unique)
KS_HD bool ext_seed_before(int score1, int i1, int score2, int i2) { return score1 < score2 || (score1 == score2 && i1 < i2); }
// seeds of the chain fully inside the alignment (:2907-2917 and after every fold)
KS_HD void seedcov(meme_alnreg& a, const meme_chain_seed* sd, int n) {
    if (a.rb == H0 || a.qb == H0 || a.qe == H0 || a.re == H0) return;
    int cov = 0;
    for (int i = 0; i < n; ++i) {
        const meme_chain_seed t = sd[i];
        if (t.qbeg >= a.qb && t.qbeg + t.len <= a.qe && t.rbeg >= a.rb && t.rbeg + t.len <= a.re) cov += t.len;
    }
    a.seedcov = cov;
}
// the record a chained seed starts as (:2722-2850): H0 where an extension has yet to say, the seed's own ends where there is no flank to extend
KS_HD meme_alnreg ext_record0(const meme_chain_seed& t, bool sideL, bool sideR, int l_query, const meme_ext_opt& o, int rid, float frac_rep, uint64_t c,
                              const meme_chain_seed* sd, int n_seeds) {
    meme_alnreg a;
    memset(&a, 0, sizeof(a));
    a.w = o.w; a.score = a.truesc = -1; a.rid = rid; a.frac_rep = frac_rep; a.seedlen0 = t.len; a.c = c;
    a.rb = a.re = H0; a.qb = a.qe = H0;
    if (sideL) { a.qb = t.qbeg; a.rb = t.rbeg; } else { a.score = a.truesc = t.len * o.a; a.qb = 0; a.rb = t.rbeg; }
    if (sideR) { a.qe = t.qbeg + t.len; a.re = t.rbeg + t.len; } else { a.qe = l_query; a.re = t.rbeg + t.len; seedcov(a, sd, n_seeds); }
    return a;
}
// one banded-SW result into its record (:2985-3018 left, :3253-3290 right): false = the band (w) was too narrow and this was not the last try -- the job
// runs again (the record keeps the score it got); true = folded, the caller recounts seedcov
template <bool LEFT> KS_HD bool ext_fold(meme_alnreg& a, const meme_seqpair& sp, int w, int last, const meme_ext_opt& o, int l_query) {
    const int prev = a.score;
    a.score = sp.score;
    if (!(a.score == prev || sp.max_off < (w >> 1) + (w >> 2) || last)) return false;
    if (LEFT) {
        if (sp.gscore <= 0 || sp.gscore <= a.score - o.pen_clip5) { a.qb -= sp.qle; a.rb -= sp.tle; a.truesc = a.score; }
        else { a.qb = 0; a.rb -= sp.gtle; a.truesc = sp.gscore; }
    } else {
        if (sp.gscore <= 0 || sp.gscore <= a.score - o.pen_clip3) { a.qe += sp.qle; a.re += sp.tle; a.truesc += a.score - sp.h0; }
        else { a.qe = l_query; a.re += sp.gtle; a.truesc += sp.gscore - sp.h0; }
    }
    a.w = a.w > w ? a.w : w;
    return true;
}

// ---- the purge (:3389-3485) --------------------------------------------------------------------------------------------------------------
// is a point qd query bases and rd reference bases from an end of an alignment of band p_w within that band?
KS_HD bool ext_in_band(int qd, int64_t rd, int p_w, const meme_ext_opt& o) {
    const int max_gap = ext_max_gap(o, qd < rd ? qd : (int)rd), band = max_gap < p_w ? max_gap : p_w;
    return qd - rd < band && rd - qd < band;
}
// does the surviving alignment p contain the seed s, with s within p's band of either of p's ends?
KS_HD bool ext_covers(int64_t p_rb, int64_t p_re, int p_qb, int p_qe, int p_w, int p_seedlen0, const meme_chain_seed& s, int l_query, const meme_ext_opt& o) {
    if (p_qb == -1 && p_qe == -1) return false;                   // purged itself
    if (s.rbeg < p_rb || s.rbeg + s.len > p_re || s.qbeg < p_qb || s.qbeg + s.len > p_qe) return false;
    if (s.len - p_seedlen0 > .1 * l_query) return false;
    return ext_in_band(s.qbeg - p_qb, s.rbeg - p_rb, p_w, o) || ext_in_band(p_qe - (s.qbeg + s.len), p_re - (s.rbeg + s.len), p_w, o);
}
// ... unless t, a seed of s's chain extended before it, is about as long, overlaps s and lies on another diagonal
KS_HD bool ext_other_diagonal(const meme_chain_seed& s, const meme_chain_seed& t) {
    if (t.len < s.len * .95) return false;
    if (s.qbeg <= t.qbeg && s.qbeg + s.len - t.qbeg >= s.len >> 2 && t.qbeg - s.qbeg != t.rbeg - s.rbeg) return true;
    return t.qbeg <= s.qbeg && t.qbeg + t.len - s.qbeg >= s.len >> 2 && s.qbeg - t.qbeg != s.rbeg - t.rbeg;
}
