// The rules of mate rescue -- the kswv kernels (reference src/kswv.cpp:372-712 int8 lanes, :934-1199 int16 lanes), their driver mem_sam_pe_batch
// (src/bwamem_pair.cpp:719-818) and the posing step mem_sam_pe_batch_pre / mem_matesw_batch_pre (:660-716, :1060-1223) -- that k_kswv / k_seedsw of
// meme_kswv.hip and k_mate_plan / k_mate_seq of meme_mate.hip apply, written ONCE on plain values: the kernels keep what needs lanes, LDS and HBM.
// tests/test_kswv_rules_model.py compiles this header with g++ into a scalar kswv pair, a lane-less posing step and the launch plan and holds them
// against the compiled reference's records and the oracle.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "meme_hip.h"
#include "meme_ksort.h"      // KS_HD

// ---- flags and the kind of a job ---------------------------------------------------------------------------------------------------------
constexpr int KSW_XBYTE = 0x10000, KSW_XSTOP = 0x20000, KSW_XSUBO = 0x40000, KSW_XSTART = 0x80000;      // src/ksw.h:31-34
// what mem_matesw_batch_pre asks of a job (:1135): second-best score, start, the threshold; int8 lanes while mate length x match score stays below 250
KS_HD int mate_xtra(int l_ms, int a, int min_seed_len) { return KSW_XSUBO | KSW_XSTART | (l_ms * a < 250 ? KSW_XBYTE : 0) | (min_seed_len * a); }
KS_HD bool kswv_is8(int xtra) { return (xtra & KSW_XBYTE) != 0; }       // sort_classify, src/bwamem.cpp:1798-1825
// the query padded (with a base that scores 0) to the stripe of bwa's SSE2 ksw_u8 / ksw_i16: 16 columns for int8 jobs, 8 for int16 jobs
KS_HD int kswv_padded(int len2, bool is8) { return is8 ? (len2 + 15) / 16 * 16 : (len2 + 7) / 8 * 8; }

// ---- the constants of a pass (:398-405, :131-132) ----------------------------------------------------------------------------------------
// int8 lanes: unsigned bytes biased by `shift`, i.e. H + S capped at 255 - shift, "no row maximum" is 0; thresholds a lane's number format cannot hold do not apply
struct KswvPass { bool is8, has_minsc, has_endsc; int shift, cap, none, qmax, minsc, endsc; };
KS_HD KswvPass kswv_pass_of(bool is8, int xtra, int a, int b) {
    const int w_match = a, w_mismatch = -b, w_ambig = -1;
    int mn = w_match < w_mismatch ? w_match : w_mismatch, mx = w_match > w_mismatch ? w_match : w_mismatch;
    mn = mn < w_ambig ? mn : w_ambig; mx = mx > w_ambig ? mx : w_ambig;
    KswvPass P;
    P.is8 = is8; P.shift = is8 ? (256 - (mn & 0xff)) & 0xff : 0; P.cap = is8 ? 255 - P.shift : 0x3fffffff; P.none = is8 ? 0 : -1; P.qmax = mx;
    P.minsc = (xtra & KSW_XSUBO) ? (xtra & 0xffff) : 0x10000; P.has_minsc = P.minsc <= (is8 ? 255 : 32767);
    P.endsc = (xtra & KSW_XSTOP) ? (xtra & 0xffff) : 0x10000; P.has_endsc = P.endsc <= (is8 ? 255 : 32767);
    return P;
}

// ---- the row rules, on what a lane carries from row to row -------------------------------------------------------------------------------
struct KswvLane { int gmax, te, qe, pimax, exit_row; bool mask, minsc_ok, exited; };
KS_HD KswvLane kswv_lane0() { return KswvLane{0, -1, 0, 0, -1, false, false, false}; }
// Block I (:505-518, :1063-1078), behind row i whose maximum is imax: true = rowMax[i - 1] gets `keep` -- the previous row's maximum if that row is a
// local peak in the reference's sense (a two-state mask) and reached the KSW_XSUBO threshold, else `none`
KS_HD bool kswv_block1(const KswvPass& P, KswvLane& L, int i, int imax, int& keep) {
    if (i > 0) {
        const bool msk = imax > L.pimax || L.mask;
        keep = (!msk && L.minsc_ok) ? L.pimax : P.none;
        L.mask = !msk;
    }
    L.pimax = imax;
    L.minsc_ok = P.has_minsc && imax >= P.minsc;
    return i > 0;
}
// Block II: the global maximum moves only on a strictly larger row maximum (the first row wins ties); iqe = that maximum's first column
KS_HD void kswv_block2(const KswvPass& P, KswvLane& L, int i, int imax, int iqe) {
    if (imax > L.gmax) { L.gmax = imax; L.te = i; L.qe = P.is8 ? (iqe & 0xff) : iqe; }
}
// the stop: KSW_XSTOP reached, or an int8 lane saturates; row i and all later ones keep nothing
KS_HD bool kswv_stop(const KswvPass& P, KswvLane& L, int i) {
    if ((P.has_endsc && L.gmax >= P.endsc) || (P.is8 && L.gmax + P.shift >= 255)) { L.exited = true; L.exit_row = i; }
    return L.exited;
}
// behind the last row: true = rowMax[tlen - 1] gets `keep`
KS_HD bool kswv_last_row(const KswvPass& P, const KswvLane& L, int tlen, int& keep) {
    keep = (!L.mask && L.minsc_ok) ? L.pimax : P.none;
    return !L.exited && tlen > 0;
}
// the finished pass: a saturated int8 lane reports 255
KS_HD int kswv_score(const KswvPass& P, int raw) { return P.is8 ? (raw + P.shift < 255 ? raw : 255) : raw; }

// score2 / te2 (:594-646, :1141-1183): the largest kept row maximum of rows [0, last] outside te +- ceil(score / qmax), the first row on ties.  Rows at and
// after a stop keep nothing (and were not written); a saturated lane has none (last = -1, which leaves score2 = te2 = -1 as an empty window does)
struct KswvScan { int low, high, last; };
KS_HD KswvScan kswv_scan_of(const KswvPass& P, const KswvLane& L, int tlen) {
    const int val = (L.gmax + P.qmax - 1) / P.qmax;
    const bool on = !(P.is8 && kswv_score(P, L.gmax) == 255);
    return KswvScan{L.te - val, L.te + val, !on ? -1 : (L.exited ? L.exit_row - 1 : tlen - 1)};
}
KS_HD bool kswv_scan_row(const KswvScan& S, int i) { return i <= S.last && (i < S.low || i > S.high); }
KS_HD int kswv_rowmax_value(const KswvPass& P, unsigned short raw) { return P.is8 ? (int)raw : (int)(short)raw; }
KS_HD void kswv_scan_take(int rv, int i, int& mx, int& t2) { if (rv > mx) { mx = rv; t2 = i; } }
KS_HD int kswv_score2(const KswvPass& P, int mx) { return P.is8 ? (mx == 0 ? -1 : mx) : mx; }      // int8: 0 means none

// ---- a pass's view of its job; the second pass (src/bwamem_pair.cpp:768-808) ---------------------------------------------------------------
// target(i) = t[i <= t_rev ? t_rev - i : i], query(j) = q[q_rev >= 0 ? q_rev - j : j]: the first pass reads both as they are (t_rev = q_rev = -1); the second
// reads query[0..qe] and target[0..te] reversed, the target's length unchanged, and stops at the first pass's score.  Lanes without one run an empty job.
struct KswvView {
    int tlen, qlen, t_rev, q_rev, xtra;
    KS_HD int target(int i) const { return i <= t_rev ? t_rev - i : i; }
    KS_HD int query(int j) const { return q_rev >= 0 ? q_rev - j : j; }
};
KS_HD KswvView kswv_first_view(int len1, int len2, int xtra) { return KswvView{len1, len2, -1, -1, xtra}; }
KS_HD bool kswv_second_runs(int xtra, int score) { return (xtra & KSW_XSTART) != 0 && !((xtra & KSW_XSUBO) && score < (xtra & 0xffff)); }
KS_HD KswvView kswv_second_view(bool runs, int len1, const meme_kswr& R) { return KswvView{runs ? len1 : 0, runs ? R.qe + 1 : 0, R.te, R.qe, KSW_XSTOP | R.score}; }
// tb / qb only if the second pass reaches exactly the first one's score (raw2, te2, qe2: its maximum and where)
KS_HD void kswv_start(meme_kswr& R, bool runs, int raw2, int te2, int qe2) { if (runs && R.score == raw2) { R.tb = R.te - te2; R.qb = R.qe - qe2; } }

// ---- posing (mem_matesw_batch_pre) -------------------------------------------------------------------------------------------------------
KS_HD int mem_infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t* dist) {          // src/bwamem_pair.cpp:58-65
    const int r1 = b1 >= l_pac, r2 = b2 >= l_pac;
    const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
    *dist = p2 > b1 ? p2 - b1 : b1 - p2;
    return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}
// bit o: orientation o is not tried for the record at rb -- the statistics rule it out (:1081-1083) or one of the mate's nm records explains it (:1085-1091)
KS_HD int mate_skip_mask(const meme_pestat* pes, int64_t l_pac, int64_t rb, const meme_mate_reg* ma, int nm) {
    int skip = 0;
    for (int o = 0; o < 4; ++o) skip |= (pes[o].failed ? 1 : 0) << o;
    for (int k = 0; k < nm; ++k) {
        int64_t dist;
        const int o = mem_infer_dir(l_pac, rb, ma[k].rb, &dist);
        if (dist >= pes[o].low && dist <= pes[o].high) skip |= 1 << o;
    }
    return skip;
}
KS_HD bool mate_tries(int skip, int o) { return !(skip >> o & 1) && skip != 15; }
// the window of the text a mate of l_ms bases in orientation o is looked for in (:1108-1125), inside the fwd + rc text; bns_fetch_seq's clamp (bns_clamp_to_mid
// of meme_ext_rules.h, for rb < re) comes behind it
struct MateWindow { int is_rev, is_larger; int64_t rb, re; };
KS_HD MateWindow mate_window(int o, const meme_pestat& pe, int64_t rec_rb, int l_ms, int64_t l_pac) {
    MateWindow W;
    W.is_rev = (o >> 1) != (o & 1); W.is_larger = !(o >> 1);
    W.rb = (W.is_larger ? rec_rb + pe.low : rec_rb - pe.high) - (W.is_rev ? l_ms : 0);
    W.re = (W.is_larger ? rec_rb + pe.high : rec_rb - pe.low) + (W.is_rev ? 0 : l_ms);
    if (W.rb < 0) W.rb = 0;
    if (W.re > l_pac << 1) W.re = l_pac << 1;
    return W;
}
// a job if the window lies on the record's sequence (rid: the one the last clamp found, carried across orientations as in the reference) and holds a seed (:1131)
KS_HD bool mate_is_job(int rec_rid, int rid, int64_t rb, int64_t re, int min_seed_len) { return rec_rid == rid && re - rb >= min_seed_len; }
// base l of the job's query: the mate as it is, or reversed and complemented with N staying N (:1111-1116)
KS_HD uint8_t mate_query_base(const uint8_t* ms, int l_ms, int l, bool is_rev) {
    if (!is_rev) return ms[l];
    const uint8_t b = ms[l_ms - 1 - l];
    return b < 4 ? (uint8_t)(3 - b) : (uint8_t)4;
}

// ---- host: the limits and the launch plan ---- -------------------------------------------------------------------------------------------
constexpr int KSWV_SCORE_LIMIT = 1 << 12;            // H and F fields of the column word
constexpr int N_KSWV_CLS = 6;
constexpr int KSWV_CLS_Q[N_KSWV_CLS] = {64, 128, 160, 256, 384, 528};     // padded query columns per LDS size class: (q + 2) * 256 B per wavefront
constexpr int KSWV_MAX_QUERY = KSWV_CLS_Q[N_KSWV_CLS - 1] - 16;
inline int kswv_cls_of(int padded) { int c = 0; while (KSWV_CLS_Q[c] < padded) ++c; return c; }
// the row's scores are a table of signed bytes
inline bool kswv_opt_ok(int a, int b) { return a <= 127 && b <= 127; }
// a job the kernels serve: sequences inside their buffers, scores inside the 12-bit fields, the query inside the last class, the window's rows inside rowMax's 16 bits
inline bool kswv_job_ok(const meme_kswv_job& J, int a, int64_t ref_bytes, int64_t qer_bytes) {
    return !(J.len1 < 0 || J.len2 < 0 || J.len1 > 32767 || J.idr < 0 || J.idq < 0 || J.idr + J.len1 > ref_bytes || J.idq + J.len2 > qer_bytes ||
             (int64_t)J.len2 * a >= KSWV_SCORE_LIMIT || J.len2 > KSWV_MAX_QUERY || (kswv_is8(J.xtra) && J.len2 > 255));
}

// Jobs in the order the launches read them -- LDS size class, then padded query length, then window length descending (so a wavefront's lanes run about the
// same number of rows) -- one launch per class; wavefront w (over all launches; a launch's first is w0) keeps its row maxima, [row][lane], in rows
// [rm_off[w], rm_off[w + 1]) of the scratch: one more than its longest window
struct KswvLaunch { int first, count, columns; size_t w0; };
struct KswvPlan { std::vector<int> order; std::vector<KswvLaunch> launches; std::vector<int64_t> rm_off; int64_t rows_total; };
inline KswvPlan kswv_plan(const meme_kswv_job* jobs, int n) {
    KswvPlan P;
    P.rows_total = 0;
    std::vector<int> padded((size_t)n);
    P.order.resize((size_t)n);
    for (int k = 0; k < n; ++k) { padded[(size_t)k] = kswv_padded(jobs[k].len2, kswv_is8(jobs[k].xtra)); P.order[(size_t)k] = k; }
    std::sort(P.order.begin(), P.order.end(), [&](int x, int y) {
        const int cx = kswv_cls_of(padded[(size_t)x]), cy = kswv_cls_of(padded[(size_t)y]);
        if (cx != cy) return cx < cy;
        if (padded[(size_t)x] != padded[(size_t)y]) return padded[(size_t)x] < padded[(size_t)y];
        if (jobs[x].len1 != jobs[y].len1) return jobs[x].len1 > jobs[y].len1;
        return x < y;
    });
    for (int p = 0; p < n;) {
        const int c = kswv_cls_of(padded[(size_t)P.order[(size_t)p]]);
        int e = p;
        while (e < n && kswv_cls_of(padded[(size_t)P.order[(size_t)e]]) == c) ++e;
        P.launches.push_back(KswvLaunch{p, e - p, KSWV_CLS_Q[c], P.rm_off.size()});
        for (int w = p; w < e; w += 64) {
            int mr = 1;
            for (int k = w; k < e && k < w + 64; ++k) mr = std::max(mr, jobs[P.order[(size_t)k]].len1);
            P.rm_off.push_back(P.rows_total);
            P.rows_total += mr + 1;
        }
        p = e;
    }
    return P;
}
