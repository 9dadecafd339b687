// Mate-rescue Smith-Waterman of the SAM phase on the device: what mem_sam_pe_batch (reference src/bwamem_pair.cpp:719-818)
// computes with the AVX-512 kswv kernels (src/kswv.cpp:372-712 int8 lanes, :934-1199 int16 lanes) for the jobs mem_matesw_batch_pre
// (src/bwamem_pair.cpp:1060-1223) has posed -- a mate (or its reverse complement) against the window of the reference its partner's
// alignment and the insert-size distribution point at: forward pass (score, end positions, second-best score outside the best hit),
// then, for hits above the threshold, the pass over the reversed prefixes that finds the start.
//
// The reference puts one job in each SIMD lane; so does this kernel, at wavefront width: one job per lane, 64 jobs per wavefront, jobs
// sorted so that a wavefront's jobs have the same padded query length and similar windows.  Per lane the column state {H(i-1,j), F(i,j),
// query code} is one 32-bit LDS word, laid out [column][lane] (conflict-free whatever column a lane is at); E and the diagonal travel
// in registers along the row.  What one SIMD lane of the reference computes does not depend on its neighbours (oracle/meme_oracle.c,
// kswv_pass, spells out why), so every quirk is per-lane arithmetic here too:
//   * int8 jobs (KSW_XBYTE: a short read under a small match score, mate_xtra): unsigned bytes biased by `shift`, i.e. H + S capped at 255 - shift; the
//     query padded with a base that scores 0 up to a multiple of 16 columns (8 for int16 jobs), the stripe of bwa's SSE2 ksw_u8 / ksw_i16;
//   * a row's maximum and its first column; the global maximum moves only on a strictly larger one (first row wins ties);
//   * rowMax: the row maximum is kept only for rows that are local peaks of that sequence in the reference's sense (Block I, a two-state
//     mask), reach the KSW_XSUBO threshold and precede the lane's stop (KSW_XSTOP reached; int8: score + shift saturates);
//   * score2 / te2: the largest kept row maximum outside te +- ceil(score / match), first row on ties; int8: 0 means none;
//   * second pass when KSW_XSTART is set and the score reaches the threshold: query[0..qe] and target[0..te] reversed, the target's
//     length unchanged, stop at the first pass's score; tb / qb only if it reaches exactly that score.
// rowMax lives in HBM ([row][lane] per wavefront: one 128-byte line per row), the only global traffic of the row loop besides one
// target base per lane and row.
#include <string.h>

#include "meme_colword.h"
#include "meme_ext_rules.h"      // flt_base_index
#include "meme_kswv_rules.h"

namespace {

struct KswvArgs {
    const meme_kswv_job* jobs;
    const int* order;            // job indices, sorted; this launch: [first, first + count)
    int first, count;
    const uint8_t* ref;
    const uint8_t* qer;
    meme_kswr* out;
    unsigned short* rowmax;      // scratch: per wavefront [row][lane]
    const i64* rm_off;           // first row of each wavefront of this launch in the scratch
    int a, b, o_del, e_del, o_ins, e_ins;
};

struct PassOut { int raw, score, te, qe, score2, te2; };

// one pass of one job per lane: the rules are meme_kswv_rules.h's; here are the column words, the row loop and rowMax's traffic
__device__ __forceinline__ PassOut kswv_pass(lds_u32 W, bool is8, const uint8_t* t, const uint8_t* q, const KswvView& V, bool want2, const KswvArgs& A, unsigned short* rm) {
    const KswvPass P = kswv_pass_of(is8, V.xtra, A.a, A.b);
    const int w_match = A.a, w_mismatch = -A.b, w_ambig = -1;
    const int tlen = V.tlen, qlen = V.qlen, quanta = kswv_padded(qlen, is8), cap = P.cap;
    const int oe_del = A.o_del + A.e_del, oe_ins = A.o_ins + A.e_ins, e_del = A.e_del, e_ins = A.e_ins;
    // column words: word j + 1 = {query code of column j in the low byte (0..3, 4 = N, 5 = padding), H(i-1, j) = 0 in bits 8..19, F = 0 in 20..31}
    for (int j = 0; j < quanta; ++j) {
        unsigned c = 5u;
        if (j < qlen) { c = q[V.query(j)]; c = c > 4u ? 4u : c; }
        W[(j + 1) * 64] = c;
    }
    KswvLane L = kswv_lane0();
    int keep;
    int tb_next = tlen > 0 ? (int)t[V.target(0)] : 4;
    const int wave_rows = wave_max(tlen);
    const unsigned tab_hi = (unsigned)(w_ambig & 0xff);                        // code 4 (N): ambiguous; code 5 (padding): 0
    for (int i = 0; i < wave_rows; ++i) {
        const bool live = i < tlen && !L.exited;
        if (!__any(live)) break;
        if (live) {
            const int tb = tb_next;
            if (i + 1 < tlen) tb_next = t[V.target(i + 1)];
            const unsigned tab_lo = cw_score_tab(tb, w_match, w_mismatch, w_ambig);
            int e = 0, diag = 0;
            // Four columns per trip with rotating registers (the next word is requested a cell ahead); the row maximum and its FIRST column as
            // one key (h << 10 | 1023 - column), one accumulator per unrolled position (cw_join_keys).  E travels along the row, F down the column.
#define KSWV_CELL(cur_, nxt_, j_, mk_, jr_)                                                                   \
            {                                                                                                  \
                nxt_ = W[((j_) + 2) * 64];                     /* (one word of slack behind the last column) */  \
                cw_gotoh_cell<true>(W + ((j_) + 1) * 64, cur_, tab_hi, tab_lo, cap, diag, e, oe_del, e_del, oe_ins, e_ins,                    \
                                    [&](int h) { const int key = (h << 10) + (jr_); mk_ = mk_ > key ? mk_ : key; });                            \
            }
            unsigned wa = W[64], wb = 0u, wc = 0u, wd = 0u;
            int mk0 = -8, mk1 = -8, mk2 = -8, mk3 = -8;
            for (int j = 0; j < quanta; j += 4) {
                const int jr = 1023 - j;
                KSWV_CELL(wa, wb, j, mk0, jr)
                KSWV_CELL(wb, wc, j + 1, mk1, jr)
                KSWV_CELL(wc, wd, j + 2, mk2, jr)
                KSWV_CELL(wd, wa, j + 3, mk3, jr)
            }
#undef KSWV_CELL
            const int key = cw_join_keys(mk0, mk1, mk2, mk3, -1);
            const int imax = key < 0 ? 0 : key >> 10;
            if (kswv_block1(P, L, i, imax, keep)) rm[(i64)(i - 1) * 64] = (unsigned short)keep;
            kswv_block2(P, L, i, imax, 1023 - (key & 1023));
            kswv_stop(P, L, i);
        }
    }
    if (kswv_last_row(P, L, tlen, keep)) rm[(i64)(tlen - 1) * 64] = (unsigned short)keep;
    PassOut R;
    R.raw = L.gmax; R.score = kswv_score(P, L.gmax);
    R.te = L.te; R.qe = L.qe; R.score2 = -1; R.te2 = -1;
    if (want2) {                                                           // (wave-uniform: first passes only)
        const KswvScan S = kswv_scan_of(P, L, tlen);
        const int wave_last = wave_max(S.last);
        int mx = P.none, t2 = -1;
        __threadfence_block();
        for (int i = 0; i <= wave_last; ++i)
            if (kswv_scan_row(S, i)) kswv_scan_take(kswv_rowmax_value(P, rm[(i64)i * 64]), i, mx, t2);
        R.score2 = kswv_score2(P, mx); R.te2 = t2;
    }
    return R;
}

__global__ void __launch_bounds__(64) k_kswv(KswvArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned int w_raw[];
    const int lane = threadIdx.x;
    const lds_u32 W = (lds_u32)w_raw + lane;
    const int slot = (int)blockIdx.x * 64 + lane;
    const bool active = slot < A.count;
    const int jid = A.order[A.first + (active ? slot : 0)];
    const meme_kswv_job J = A.jobs[jid];
    const bool is8 = kswv_is8(J.xtra);
    const uint8_t* t = A.ref + J.idr;
    const uint8_t* q = A.qer + J.idq;
    unsigned short* rm = A.rowmax + A.rm_off[blockIdx.x] * 64 + lane;
    const PassOut F = kswv_pass(W, is8, t, q, kswv_first_view(active ? J.len1 : 0, active ? J.len2 : 0, J.xtra), true, A, rm);
    meme_kswr R;
    R.score = F.score; R.te = F.te; R.qe = F.qe; R.score2 = F.score2; R.te2 = F.te2; R.tb = -1; R.qb = -1;
    const bool again = active && kswv_second_runs(J.xtra, R.score);
    __builtin_amdgcn_wave_barrier();
    const PassOut B = kswv_pass(W, is8, t, q, kswv_second_view(again, J.len1, R), false, A, rm);
    kswv_start(R, again, B.raw, B.te, B.qe);
    if (active) A.out[jid] = R;
}

// ---- mem_seed_sw (reference src/bwamem.cpp:494-520): the local alignment score of a chained seed's neighbourhood, at most 199 x 199 bases,
// as ksw_align2 without KSW_XBYTE computes it -- ksw_i16 (src/ksw.cpp:236-320; only .score is used).  One job per lane, the window straight
// from the 2-bit text, the query from the resident read; column word = {query code, H(i-1, j), E(i, j)} as above.
//
// ksw_i16 is Farrar's striped recurrence; its "lazy F" loop raises H where an insertion crosses a lane boundary of the striping but not
// the E the main loop has already stored for the next row (:280-283 vs :289-299), i.e. it loses some insertion -> deletion transitions.
// That is not observable: the same two gaps in the other order (deletion, then insertion: E feeds h, h feeds F, both exact) reach the same
// cell with the same score, so every H equals the plain Gotoh value and the kernel computes that (the oracle restates the striping lane
// by lane and agrees; tests/test_ref_live.py pins it on the compiled reference).  Columns past qlen score 0 in the reference's profile and
// can only repeat values already counted; they are not computed.
// The window's bases are the ones the reference's call reads (flt_base_index of meme_ext_rules.h), not the genome's.
__device__ __forceinline__ int flt_window_base(const u64* __restrict__ pac, i64 l_pac, i64 p) {
    const FltBase B = flt_base_index(l_pac, p);
    const int c = B.pos < l_pac << 1 ? text_base(pac, B.pos) : 0;
    return B.complement ? 3 - c : c;
}

__device__ __forceinline__ int seedsw_score(lds_u32 W, const u64* __restrict__ pac, i64 l_pac, i64 rb, int tlen, const uint8_t* __restrict__ q, int qlen, const KswvArgs& A) {
    const int w_match = A.a, w_mismatch = -A.b, w_ambig = -1;
    const int oe_del = A.o_del + A.e_del, oe_ins = A.o_ins + A.e_ins, e_del = A.e_del, e_ins = A.e_ins;
    const int wave_q = wave_max(qlen), wave_rows = wave_max(tlen);
    for (int j = 0; j <= wave_q; ++j) {                      // (one word of slack behind the last column)
        unsigned c = 5u;
        if (j < qlen) { c = q[j]; c = c > 4u ? 4u : c; }
        W[(j + 1) * 64] = c;
    }
    const unsigned tab_hi = (unsigned)(w_ambig & 0xff);     // code 4 (N): ambiguous; code 5 (past the query): 0
    int gmax = 0;
    for (int i = 0; i < wave_rows; ++i) {
        if (i < tlen) {
            const int tb = flt_window_base(pac, l_pac, rb + i);
            const unsigned tab_lo = cw_score_tab(tb, w_match, w_mismatch, w_ambig);
            int f = 0, diag = 0, rmax = 0;
            unsigned cur = W[64];
            for (int j = 0; j < qlen; ++j) {
                const unsigned nxt = W[(j + 2) * 64];
                // (:274-277; e, f >= 0: _mm_subs_epu16.)  Here E travels down the column and F along the row
                cw_gotoh_cell<false>(W + (j + 1) * 64, cur, tab_hi, tab_lo, 0, diag, f, oe_del, e_del, oe_ins, e_ins, [&](int h) { rmax = rmax > h ? rmax : h; });
                cur = nxt;
            }
            gmax = gmax > rmax ? gmax : rmax;
        }
    }
    return gmax;
}

__global__ void __launch_bounds__(64) k_seedsw(const meme_seedsw_job* __restrict__ jobs, const unsigned long long* __restrict__ n_jobs, const u64* __restrict__ pac,
                                               i64 l_pac, const uint8_t* __restrict__ reads, int* __restrict__ sc, KswvArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned int w_raw[];
    const int lane = threadIdx.x;
    const lds_u32 W = (lds_u32)w_raw + lane;
    const i64 n = (i64)*n_jobs;
    if ((i64)blockIdx.x * 64 >= n) return;
    const i64 slot = (i64)blockIdx.x * 64 + lane;
    const bool active = slot < n;
    const meme_seedsw_job J = jobs[active ? slot : 0];
    const int score = seedsw_score(W, pac, l_pac, J.rb, active ? (int)J.tlen : 0, reads + J.qoff, active ? (int)J.qlen : 0, A);
    if (active) sc[J.seed] = score;
}

}  // namespace

int meme_seedsw_launch(meme_ctx* ctx, const meme_seedsw_job* d_jobs, const unsigned long long* d_njobs, i64 max_jobs, int* d_sc, const meme_ext_opt* o) {
    if (max_jobs <= 0) return MEME_OK;
    const meme_kswv_job longest = {0, 0, MEME_SEEDSW_MAX - 1, MEME_SEEDSW_MAX - 1, 0, 0};       // (the filter's windows and queries are shorter than MEM_SHORT_LEN)
    if (!kswv_opt_ok(o->a, o->b) || !kswv_job_ok(longest, o->a, longest.len1, longest.len2)) {
        meme_set_error("seed filter (mem_flt_chained_seeds): match score %d / mismatch penalty %d beyond the kernel's limits (199 x match < %d)", o->a, o->b, KSWV_SCORE_LIMIT);
        return MEME_E_ARG;
    }
    KswvArgs A;
    memset(&A, 0, sizeof(A));
    A.a = o->a; A.b = o->b; A.o_del = o->o_del; A.e_del = o->e_del; A.o_ins = o->o_ins; A.e_ins = o->e_ins;
    const size_t lds = (size_t)(MEME_SEEDSW_MAX + 2) * 256;
    hipLaunchKernelGGL(k_seedsw, dim3((unsigned)((max_jobs + 63) / 64)), dim3(64), lds, ctx->stream, d_jobs, d_njobs, ctx->idx.pac, ctx->idx.n >> 1, (const uint8_t*)ctx->batch.reads.p, d_sc, A);
    HIP_TRY(hipGetLastError());
    return MEME_OK;
}

extern "C" int meme_kswv_batch_host(meme_ctx* ctx, const meme_kswv_job* jobs, int64_t njobs, const uint8_t* ref, int64_t ref_bytes, const uint8_t* qer,
                                    int64_t qer_bytes, const meme_bsw_opt* opt, meme_kswv_host_result* out) {
    return meme_kswv_run(ctx, jobs, njobs, ref, ref_bytes, qer, qer_bytes, opt, false, out);
}

int meme_kswv_run(meme_ctx* ctx, const meme_kswv_job* jobs, int64_t njobs, const uint8_t* ref, int64_t ref_bytes, const uint8_t* qer, int64_t qer_bytes, const meme_bsw_opt* opt,
                  bool staged, meme_kswv_host_result* out) {
    if (!ctx || !opt || !out || njobs < 0 || (njobs > 0 && (!jobs || (!staged && (!ref || !qer))))) { meme_set_error("meme_kswv_batch_host: null argument"); return MEME_E_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    if (!staged) ctx->mate.last_nb = -1;                        // (KswvWs::res is about to hold another call's results: meme_matesw_last_device)
    if (njobs == 0) return MEME_OK;
    if (njobs > 0x7fffffff / 2) { meme_set_error("meme_kswv_batch_host: too many jobs in one call"); return MEME_E_ARG; }
    if (opt->a < 1 || opt->b < 0 || opt->e_del < 0 || opt->e_ins < 0 || opt->o_del < 0 || opt->o_ins < 0) { meme_set_error("meme_kswv_batch_host: bad scoring parameters"); return MEME_E_ARG; }
    if (!kswv_opt_ok(opt->a, opt->b)) {
        meme_set_error("meme_kswv_batch_host: match score %d / mismatch penalty %d beyond the kernel's limits (both <= 127)", opt->a, opt->b);
        return MEME_E_ARG;
    }
    const int n = (int)njobs;
    for (int k = 0; k < n; ++k) {
        const meme_kswv_job& J = jobs[k];
        if (!kswv_job_ok(J, opt->a, ref_bytes, qer_bytes)) {
            meme_set_error("meme_kswv_batch_host: job %d is malformed or beyond the kernel's limits (window %d at %lld, query %d at %lld, match score %d: "
                           "query x match < %d, query <= %d, window <= 32767)", k, J.len1, (long long)J.idr, J.len2, (long long)J.idq, opt->a, KSWV_SCORE_LIMIT,
                           KSWV_MAX_QUERY);
            return MEME_E_ARG;
        }
    }
    const KswvPlan plan = kswv_plan(jobs, n);
    int rc;
    KswvWs& K = ctx->kswv;
    if ((rc = meme_buf_reserve(ctx, K.jobs, (size_t)n * sizeof(meme_kswv_job))) || (rc = meme_buf_reserve(ctx, K.order, (size_t)n * 4)) ||
        (rc = meme_buf_reserve(ctx, K.ref, (size_t)ref_bytes + 64)) || (rc = meme_buf_reserve(ctx, K.qer, (size_t)qer_bytes + 64)) ||
        (rc = meme_buf_reserve(ctx, K.res, (size_t)n * sizeof(meme_kswr))) || (rc = meme_buf_reserve(ctx, K.rowmax, (size_t)plan.rows_total * 128 + 256)) ||
        (rc = meme_buf_reserve(ctx, K.rm_off, plan.rm_off.size() * 8 + 8))) return rc;
    Events<2>& ev = K.ev;
    HIP_TRY(ev.ensure());
    if (!staged) HIP_TRY(hipMemcpyAsync(K.jobs.p, jobs, (size_t)n * sizeof(meme_kswv_job), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(K.order.p, plan.order.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (!staged) {                                     // (staged: the caller's kernels have written the jobs and both sequence buffers where they are read)
        HIP_TRY(hipMemcpyAsync(K.ref.p, ref, (size_t)ref_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(K.qer.p, qer, (size_t)qer_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(hipMemcpyAsync(K.rm_off.p, plan.rm_off.data(), plan.rm_off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ev[0], ctx->stream));
    for (const KswvLaunch& L : plan.launches) {
        KswvArgs A;
        A.jobs = (const meme_kswv_job*)K.jobs.p; A.order = (const int*)K.order.p; A.first = L.first; A.count = L.count;
        A.ref = (const uint8_t*)K.ref.p; A.qer = (const uint8_t*)K.qer.p; A.out = (meme_kswr*)K.res.p;
        A.rowmax = (unsigned short*)K.rowmax.p; A.rm_off = (const i64*)K.rm_off.p + L.w0;
        A.a = opt->a; A.b = opt->b; A.o_del = opt->o_del; A.e_del = opt->e_del; A.o_ins = opt->o_ins; A.e_ins = opt->e_ins;
        const size_t lds = (size_t)(L.columns + 2) * 256;
        if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)k_kswv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_kswv, dim3((unsigned)((L.count + 63) / 64)), dim3(64), lds, ctx->stream, A);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], ctx->stream));
    if ((rc = meme_hostbuf_reserve(ctx, K.h_res, (size_t)n * sizeof(meme_kswr)))) return rc;
    HIP_TRY(hipMemcpyAsync(K.h_res.p, K.res.p, (size_t)n * sizeof(meme_kswr), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    out->njobs = njobs; out->res = (const meme_kswr*)K.h_res.p; out->kernel_ms = ms;
    return MEME_OK;
}
