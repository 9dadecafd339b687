// The pairing decision on the device: what mem_sam_pe does behind mem_pair (reference src/bwamem_pair.cpp:536-590; the no_pairing block's choice of records
// and flag, :632-648) for every pair of a batch -- the fourth step of mem_sam_pe behind mate rescue, after record finishing (meme_finish.hip), primary marking
// (meme_primary.hip) and pair scoring (meme_pair.hip), on the arrays those stages leave.  Reads 2p and 2p + 1 of the call are pair p.
//
// Per pair: is_multi over the first n_pri records of either end; the handful of scalars (score_un, q_pe, the two q_se, the flag, the ALT records, `which`);
// sub and secondary of the two records the paired alignment names; and the secondary_all swap over ALL records of either end.  The records change in
// place, in those three fields and in nothing else.
//
// One body, k_decide<G>, G lanes per pair, in two tiers by the records of both ends together (tuning key decide_split):
//   k_decide<8>   eight lanes per pair, 32 pairs to a workgroup, for pairs of at most decide_split records
//   k_decide<64>  a wavefront (one workgroup) per pair for the rest, any count
// k_decide_route checks every pair, writes its defaults and lists the heavy pairs.  Inside a group the lanes stride over the records for is_multi (a
// ballot), every lane computes the scalars redundantly (control stays uniform over the group), lane 0 writes the outputs and the two fields of c[i], and
// the lanes stride over all records for the swap.  The swap reads and writes secondary_all alone, a dword per record, and what it needs of the record at z
// (its secondary_all, k) every lane has read before lane 0 stores anything: no store of the group lands on a word another of its lanes still reads, so
// the group needs no barrier.  Every loop is bounded by a record count; no kernel waits for another workgroup.
//
// Everything that decides a result is meme_decide_rules.h (and pri_mapq of meme_primary_rules.h); this file holds who reads which record and who writes.
//
// Arithmetic: IEEE double with contraction off; logarithms from the ctx's table of the host libm's log((double)k) (the primary stage's).
#include <string.h>

#include "meme_common.h"
#include "meme_alnreg_words.h"
#include "meme_decide_rules.h"

#pragma clang fp contract(off)

constexpr int DEC_G = 8;                     // lanes per pair in the light tier
constexpr i64 DEC_SPLIT_MAX = 1 << 20;       // decide_split is clamped to [0, this]: at it every pair a test can build is light
constexpr int DEC_RES = 9;                   // ints of a pair in the host form's result: path, q_pe, flag, sel[2], q_se[2], alt[2]

struct DecArgs {
    meme_alnreg* regs; const i64* reg_off; const int* n_pri; i64 npairs, total_regs;
    const int *score, *sub, *n_sub, *z; const uint8_t* pair_status;
    i64 l_pac; meme_pair_pes pes[4]; meme_decide_opt o; int split;
    int *path, *sel, *q_se, *q_pe, *flag, *alt; uint8_t* status;
    i64* list; unsigned long long* n_heavy;
    const double* logtab;
};

struct DecEnds { i64 base[2]; int n[2], n_pri[2]; };
// the two ends of pair p: where their records start, how many there are and how many take part.  false (status 2): offsets that are no span, or a count that is no part of it
__device__ __forceinline__ bool dec_ends(const DecArgs& A, i64 p, DecEnds* E) {
    bool ok = reg_span(A.reg_off, 2 * p, A.total_regs, &E->base[0], &E->n[0]);
    ok = reg_span(A.reg_off, 2 * p + 1, A.total_regs, &E->base[1], &E->n[1]) && ok;
    const int c0 = A.n_pri[2 * p], c1 = A.n_pri[2 * p + 1];
    ok = ok && c0 >= 0 && c0 <= E->n[0] && c1 >= 0 && c1 <= E->n[1];
    if (!ok) E->n[0] = E->n[1] = 0;
    E->n_pri[0] = ok ? c0 : 0; E->n_pri[1] = ok ? c1 : 0;
    return ok;
}
__device__ __forceinline__ void dec_write(const DecArgs& A, i64 p, int path, int sel0, int sel1, int q_se0, int q_se1, int q_pe, int flag, int alt0, int alt1) {
    A.path[p] = path; A.sel[2 * p] = sel0; A.sel[2 * p + 1] = sel1; A.q_se[2 * p] = q_se0; A.q_se[2 * p + 1] = q_se1; A.q_pe[p] = q_pe; A.flag[p] = flag;
    A.alt[2 * p] = alt0; A.alt[2 * p + 1] = alt1;
}
__device__ __forceinline__ void dec_write_defaults(const DecArgs& A, i64 p) { dec_write(A, p, DEC_PATH_NONE, -1, -1, 0, 0, 0, 1, -1, -1); }

// ---- routing: the status of every pair, its defaults, the list of the heavy pairs ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_decide_route(DecArgs A) {
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < A.npairs; p += (i64)gridDim.x * blockDim.x) {
        DecEnds E;
        bool ok = dec_ends(A, p, &E);
        if (ok && A.score[p] > 0) {                                                   // z names the records the paired branch reads; c[i]'s parent is read too
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int z = A.z[2 * p + i];
                ok = ok && z >= 0 && z < E.n_pri[i];
                if (ok) { const int s = A.regs[E.base[i] + z].secondary; ok = s < E.n[i]; }
            }
        }
        A.status[p] = !ok ? 2 : A.pair_status[p] ? 1 : 0;
        dec_write_defaults(A, p);
        if (E.n[0] + E.n[1] > A.split) A.list[atomicAdd(A.n_heavy, 1ull)] = p;        // (at most npairs entries; their order does not matter)
    }
}

// ---- the body -------------------------------------------------------------------------------------------------------------------------------------
template <int G> __device__ __forceinline__ bool dec_group_any(bool x) {
    if (G == 64) return __any(x) != 0;
    return ((unsigned)(__ballot(x) >> (threadIdx.x & (64 - G))) & ((1u << G) - 1u)) != 0;
}
// what mem_approx_mapq_se reads of a record, with sub as given
__device__ __forceinline__ PriQual dec_qual(const meme_alnreg& R, int sub) {
    const PriQual Q = {R.score, sub, R.csub, R.sub_n, R.qb, R.qe, R.rb, R.re, R.frac_rep};
    return Q;
}

// pair p by the G lanes of a group (lane: 0 .. G - 1).  Control flow is uniform over the group: every condition around the ballot is computed from values all its lanes hold
template <int G> __device__ __forceinline__ void dec_pair(const DecArgs& A, i64 p, const DecEnds& E, int lane) {
    const meme_decide_opt& o = A.o;
    const double* __restrict__ logtab = A.logtab;
    const auto lg = [&](int k) -> double { return logtab[k]; };
    const int score = A.score[p];
    const bool entered = dec_entered(E.n_pri[0], E.n_pri[1], score, o.no_pairing);
    bool multi = false;
    if (entered) {                                                                    // :541-546
        bool mine = false;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            for (int j = 1 + lane; j < E.n_pri[i]; j += G) { const meme_alnreg& R = A.regs[E.base[i] + j]; mine = mine || dec_multi(j, R.secondary, R.score, o.T); }
        multi = dec_group_any<G>(mine);
    }
    if (!entered || multi) {                                                          // no_pairing (:632-648): which record an end reports, and the proper-pair bit
        int which[2], rid[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = E.n[i], np = E.n_pri[i];
            const int s0 = n > 0 ? A.regs[E.base[i]].score : 0, sa = np < n ? A.regs[E.base[i] + np].score : 0;
            which[i] = dec_which(n, np, s0, sa, o.T);
            rid[i] = which[i] >= 0 ? A.regs[E.base[i] + which[i]].rid : -1;
        }
        int flag = 1;
        if (which[0] >= 0 && which[1] >= 0) flag = dec_flag_unpaired(o.no_pairing, rid[0], rid[1], A.l_pac, A.regs[E.base[0]].rb, A.regs[E.base[1]].rb, A.pes);
        if (lane == 0) dec_write(A, p, multi ? DEC_PATH_MULTI : DEC_PATH_NONE, which[0], which[1], 0, 0, 0, flag, -1, -1);
        return;
    }
    // the paired branch (:548-590)
    const meme_alnreg &a0 = A.regs[E.base[0]], &a1 = A.regs[E.base[1]];
    const int score_un = dec_score_un(a0.score, a1.score, o.pen_unpaired);
    bool beyond = false;
    const int q_pe = dec_q_pe(score, A.sub[p], score_un, A.n_sub[p], o.a, a0.frac_rep, a1.frac_rep, lg, &beyond);
    const meme_primary_opt po = dec_pri_opt(o);
    const bool paired = dec_paired_preferred(score, score_un);
    int z[2], q_se[2], k[2], alt[2];
    DecMarks marks[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        z[i] = paired ? A.z[2 * p + i] : 0;
        const meme_alnreg& c = A.regs[E.base[i] + z[i]];
        const int sec = c.secondary;
        marks[i].sub = c.sub; marks[i].secondary = sec;
        if (paired) marks[i] = dec_c_marks(c.sub, sec, sec >= 0 ? A.regs[E.base[i] + sec].score : 0);      // (sec < n: the route kernel has checked it)
        q_se[i] = pri_mapq(dec_qual(c, marks[i].sub), po, lg, &beyond);
        if (paired) q_se[i] = dec_q_se_paired(q_se[i], q_pe, c.score, c.csub, o.a);
        k[i] = c.secondary_all;
        const int np = E.n_pri[i], n = E.n[i];
        alt[i] = -1;
        if (np < n) { const meme_alnreg& g = A.regs[E.base[i] + np]; alt[i] = dec_alt(np, n, g.score, g.secondary, pri_is_alt(g.n_comp_is_alt), o.T); }
    }
    if (beyond) {                                                                     // a logarithm beyond the table: defaults, the records untouched
        if (lane == 0) A.status[p] = 1;
        return;
    }
    if (lane == 0) {
        dec_write(A, p, paired ? DEC_PATH_PAIRED : DEC_PATH_UNPAIRED, z[0], z[1], q_se[0], q_se[1], q_pe, paired ? 3 : 1, alt[0], alt[1]);
        if (paired) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                meme_alnreg& c = A.regs[E.base[i] + z[i]];
                if (marks[i].secondary == -2) { c.sub = marks[i].sub; c.secondary = -2; }
            }
        }
    }
    // the swap (:581-590) over all records of either end
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (!dec_swap_taken(k[i], E.n_pri[i])) continue;
        for (int j = lane; j < E.n[i]; j += G) {
            meme_alnreg& R = A.regs[E.base[i] + j];
            const int old = R.secondary_all, now = dec_swapped(j, old, k[i], z[i]);
            if (now != old) R.secondary_all = now;
        }
    }
}

template <int G> __global__ void __launch_bounds__(G == 64 ? 64 : 256) k_decide(DecArgs A) {
    const int lane = threadIdx.x & (G - 1);
    if (G == 64) {
        const i64 n_heavy = (i64)*A.n_heavy;
        for (i64 hi = blockIdx.x; hi < n_heavy; hi += gridDim.x) {                    // (uniform over the workgroup)
            const i64 p = A.list[hi];
            DecEnds E;
            dec_ends(A, p, &E);
            if (A.status[p] == 0) dec_pair<G>(A, p, E, lane);
        }
    } else {
        const i64 groups = (i64)gridDim.x * (256 / G);
        for (i64 p = (i64)blockIdx.x * (256 / G) + threadIdx.x / G; p < A.npairs; p += groups) {      // (uniform within a group: its lanes stay together)
            DecEnds E;
            dec_ends(A, p, &E);
            if (E.n[0] + E.n[1] > A.split || A.status[p] != 0) continue;
            dec_pair<G>(A, p, E, lane);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
namespace {

int decide_check(const char* who, i64 nreads, const meme_decide_opt* o) {
    if (nreads & 1) { meme_set_error("%s: %lld reads are no pairs", who, (long long)nreads); return MEME_E_ARG; }
    if (!(o->mapQ_coef_len > 0)) { meme_set_error("%s: mapQ_coef_len must be positive (the stage has the reference's mapQ_coef_len > 0 branch only)", who); return MEME_E_ARG; }
    if (o->a < 1 || (i64)o->a + o->b <= 0) { meme_set_error("%s: a must be at least 1 and a + b positive", who); return MEME_E_ARG; }
    return MEME_OK;
}

// the stage's kernels on device arrays, asynchronous on ctx->stream; ev: recorded around them
int decide_launch(meme_ctx* ctx, meme_alnreg* d_regs, const i64* d_reg_off, const int32_t* d_n_pri, i64 npairs, i64 total_regs, const meme_decide_pair_in* in, i64 l_pac,
                  const meme_pair_pes* pes, const meme_decide_opt* opt, const meme_decide_device_out* o) {
    DecideWs& D = ctx->decide;
    int rc;
    const double* logtab;
    if ((rc = meme_buf_reserve(ctx, D.list, (size_t)(npairs + 1) * 8)) || (rc = meme_logtab(ctx, &logtab))) return rc;
    HIP_TRY(D.ev.ensure());
    DecArgs A;
    A.regs = d_regs; A.reg_off = d_reg_off; A.n_pri = d_n_pri; A.npairs = npairs; A.total_regs = total_regs;
    A.score = in->score; A.sub = in->sub; A.n_sub = in->n_sub; A.z = in->z; A.pair_status = in->status;
    A.l_pac = l_pac; memcpy(A.pes, pes, sizeof(A.pes)); A.o = *opt; A.o.no_pairing = opt->no_pairing ? 1 : 0;
    A.split = tune_split(ctx->decide_split, (int)DEC_SPLIT_MAX);
    A.path = o->d_path; A.sel = o->d_sel; A.q_se = o->d_q_se; A.q_pe = o->d_q_pe; A.flag = o->d_flag; A.alt = o->d_alt; A.status = o->d_status;
    A.list = (i64*)D.list.p; A.n_heavy = (unsigned long long*)o->d_n_heavy; A.logtab = logtab;
    const i64 cap = tune_grid_cap(ctx->decide_blocks);
    HIP_TRY(hipEventRecord(D.ev[0], ctx->stream));
    HIP_TRY(hipMemsetAsync(o->d_n_heavy, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_decide_route, dim3(grid_blocks(npairs, 256, cap)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_decide<DEC_G>, dim3(grid_blocks(npairs, 256 / DEC_G, cap)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_decide<64>, dim3(grid_blocks(npairs, 1, cap)), dim3(64), 0, ctx->stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(D.ev[1], ctx->stream));
    return MEME_OK;
}

}  // namespace

extern "C" int meme_pair_decide_batch_device(meme_ctx* ctx, meme_alnreg* d_regs, const int64_t* d_reg_off, const int32_t* d_n_pri, int64_t nreads, int64_t total_regs,
                                             const meme_decide_pair_in* d_pair, int64_t l_pac, const meme_pair_pes* pes, const meme_decide_opt* opt,
                                             const meme_decide_device_out* out) {
    static const char* const who = "meme_pair_decide_batch_device";
    const bool outs = out && out->d_n_heavy && (nreads <= 0 || (out->d_path && out->d_sel && out->d_q_se && out->d_q_pe && out->d_flag && out->d_alt && out->d_status));
    const bool ins = d_pair && (nreads <= 0 || (d_pair->score && d_pair->sub && d_pair->n_sub && d_pair->z && d_pair->status));
    if (!ctx || !opt || !pes || !outs || !ins || nreads < 0 || total_regs < 0 || l_pac < 0 || (nreads > 0 && (!d_reg_off || !d_n_pri)) || (total_regs > 0 && !d_regs)) {
        meme_set_error("%s: null argument (or a negative count)", who);
        return MEME_E_ARG;
    }
    if ((uintptr_t)d_regs & 15) { meme_set_error("%s: the record array must be 16-byte aligned", who); return MEME_E_ARG; }
    int rc;
    if ((rc = decide_check(who, nreads, opt))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (nreads == 0) { HIP_TRY(hipMemsetAsync(out->d_n_heavy, 0, 8, ctx->stream)); return MEME_OK; }
    return decide_launch(ctx, d_regs, (const i64*)d_reg_off, d_n_pri, nreads / 2, total_regs, d_pair, l_pac, pes, opt, out);
}

extern "C" int meme_pair_decide_batch_host(meme_ctx* ctx, const meme_alnreg* regs, const int64_t* reg_off, const int32_t* n_pri, int64_t nreads, const meme_decide_pair_in* pair,
                                           int64_t l_pac, const meme_pair_pes* pes, const meme_decide_opt* opt, meme_decide_host_result* out) {
    static const char* const who = "meme_pair_decide_batch_host";
    const bool ins = pair && (nreads <= 0 || (pair->score && pair->sub && pair->n_sub && pair->z && pair->status));
    if (!ctx || !opt || !pes || !out || !ins || nreads < 0 || l_pac < 0 || (nreads > 0 && (!reg_off || !n_pri))) { meme_set_error("%s: null argument (or a negative count)", who); return MEME_E_ARG; }
    if ((uintptr_t)regs & 15) { meme_set_error("%s: the record array must be 16-byte aligned", who); return MEME_E_ARG; }
    int rc;
    if ((rc = decide_check(who, nreads, opt))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    if (nreads == 0) return MEME_OK;
    if ((rc = reg_check_host(who, regs, reg_off, nreads))) return rc;
    // what the device form answers with status 2 the host form refuses
    for (i64 r = 0; r < nreads; ++r)
        if (n_pri[r] < 0 || n_pri[r] > reg_off[r + 1] - reg_off[r]) {
            meme_set_error("%s: n_pri of read %lld is %d, the read has %lld records", who, (long long)r, n_pri[r], (long long)(reg_off[r + 1] - reg_off[r]));
            return MEME_E_ARG;
        }
    const i64 npairs = nreads / 2;
    for (i64 p = 0; p < npairs; ++p) {
        if (pair->score[p] <= 0) continue;
        for (int i = 0; i < 2; ++i) {
            const i64 r = 2 * p + i;
            const int z = pair->z[r];
            if (z < 0 || z >= n_pri[r] || regs[reg_off[r] + z].secondary >= reg_off[r + 1] - reg_off[r]) {
                meme_set_error("%s: z of read %lld is %d (n_pri %d), or that record's parent is no record of the read", who, (long long)r, z, n_pri[r]);
                return MEME_E_ARG;
            }
        }
    }
    DecideWs& D = ctx->decide;
    i64 total;
    if ((rc = reg_upload(ctx, regs, reg_off, nreads, D.regs, D.reg_off, &total))) return rc;
    const Download recs = {D.h_regs, D.regs, (size_t)total * sizeof(meme_alnreg)}, res = {D.h_res, D.res, (size_t)npairs * DEC_RES * 4}, status = {D.h_status, D.status, (size_t)npairs},
                   ctrs = {ctx->h_ctr, D.counter, 8};
    if ((rc = reg_reserve(ctx, {{D.n_pri, (size_t)nreads * 4}, {D.in, (size_t)npairs * 5 * 4}, {D.in_status, (size_t)npairs}, {D.res, res.bytes}, {D.status, status.bytes}, {D.counter, ctrs.bytes}})) ||
        (rc = reg_download_reserve(ctx, {recs, res, status, ctrs}))) return rc;
    int32_t* in = (int32_t*)D.in.p;                            // columns: score, sub, n_sub, then z (two a pair)
    HIP_TRY(hipMemcpyAsync(D.n_pri.p, n_pri, (size_t)nreads * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(in, pair->score, (size_t)npairs * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(in + npairs, pair->sub, (size_t)npairs * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(in + 2 * npairs, pair->n_sub, (size_t)npairs * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(in + 3 * npairs, pair->z, (size_t)npairs * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(D.in_status.p, pair->status, (size_t)npairs, hipMemcpyHostToDevice, ctx->stream));
    const meme_decide_pair_in d_in = {in, in + npairs, in + 2 * npairs, in + 3 * npairs, (const uint8_t*)D.in_status.p};
    int32_t* r = (int32_t*)D.res.p;                            // columns: path, q_pe, flag, then sel, q_se, alt (two a pair each)
    const meme_decide_device_out d = {r, r + 3 * npairs, r + 5 * npairs, r + npairs, r + 2 * npairs, r + 7 * npairs, (uint8_t*)D.status.p, (uint64_t*)D.counter.p};
    if ((rc = decide_launch(ctx, (meme_alnreg*)D.regs.p, (const i64*)D.reg_off.p, (const int32_t*)D.n_pri.p, npairs, total, &d_in, l_pac, pes, opt, &d))) return rc;
    float ms = 0.f;
    if ((rc = reg_download(ctx, {recs, res, status, ctrs})) || (rc = reg_sync_ms(ctx, D.ev, &ms))) return rc;
    const int32_t* h = (const int32_t*)D.h_res.p;
    out->npairs = npairs; out->total_regs = total; out->regs = (const meme_alnreg*)D.h_regs.p;
    out->path = h; out->q_pe = h + npairs; out->flag = h + 2 * npairs; out->sel = h + 3 * npairs; out->q_se = h + 5 * npairs; out->alt = h + 7 * npairs;
    out->status = (const uint8_t*)D.h_status.p; out->n_heavy = (i64)*(const unsigned long long*)ctx->h_ctr.p; out->kernel_ms = ms;
    return MEME_OK;
}
