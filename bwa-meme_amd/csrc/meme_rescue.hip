// Mate rescue's record updates on the device: what mem_sam_pe_batch_post does with the kswr_t results before it marks primaries (reference src/bwamem_pair.cpp:851-921,
// with mem_matesw_batch_post :1225-1334 and mem_matesw_batch_post_mate_sort :1337-1485) -- between the Smith-Waterman launches of mate rescue (meme_kswv.hip) and the
// primary marking (meme_primary.hip), behind record finishing.  Everything that decides a result is meme_rescue_rules.h; this file holds where the records live and who
// runs what.  The two ends of a pair are independent: end i's loop reads the records of end i as they were handed over and writes only the list of end !i, so the
// work item is a LIST (a read), and its anchors are its mate's input records.
//
//   k_rescue_route<0>  a lane per read: the spans are checked and the read's own records that are looked at counted (their scan gives every read its gar cursor)
//   k_rescue_route<1>  a lane per read, the list that is written: its mate's cursor inside the worker batch's gar, the gar entries >= 0 among the mate's records looked at
//                      (n_in + that many records is all the list can come to hold), and lists that need the driver appended to the wavefront tier's list (one atomic each)
//   k_rescue_light     eight lanes per read that is not listed: its records copied to where the pack expects them, flg = 0
//   k_rescue_wave      a wavefront (one 64-thread workgroup) per listed read: every lane executes rescue_end of the rules on the list's columns -- in LDS up to
//                      rescue_lds_recs records, else in a workspace in HBM --, what it reads comes back through readfirstlane, so the walk lives in scalar registers and
//                      branches as one.  The lanes stride over the loads, the skip mask (an OR across the wavefront) and the final stores: a new record is put together at
//                      the store, an old one is the input's with flg, n_comp and qe set
//   k_rescue_pack      eight lanes per read behind the scan of the per-read counts: the lists from the stage to the compact output
//
// Nothing waits for another wavefront: no kernel reads what another workgroup of the same launch writes (the list is complete when the launch behind it starts), every
// loop is bounded by a record count, the records looked at or the four orientations, and every barrier, shuffle and readlane stands in control flow that is the same on
// all lanes of its workgroup.
#include <limits.h>
#include <string.h>
#include <string>

#include "meme_common.h"
#include "meme_alnreg_words.h"
#include "meme_ext_rules.h"      // bns_clamp_to_mid
#include "meme_rescue_rules.h"

#pragma clang fp contract(off)

namespace {

constexpr int RES_LDS_RECS = 128;            // records a list can come to hold whose columns stay in LDS (60 bytes each: 7.5 KB a workgroup; profiles/rescue_stage.md)
enum { RES_CTR_WAVE = 0, RES_CTR_TESTED = 1, RES_CTR_PUSHED = 2, RES_CTR_REMOVED = 3, RES_CTRS = 8 };

struct ResArgs {
    const meme_alnreg* in; const i64* reg_off; const uint8_t* ums; const int* rlen; i64 nreads, total_regs, out_cap;
    const int32_t* gar; const i64 *gar_off, *job_off; i64 nbatches; const meme_kswr* res; i64 njobs;
    meme_pestat pes[4];
    i64 l_pac; const i64* contig_off; const int* contig_len; int n_contigs;
    meme_rescue_opt o; int lds_recs;
    i64 *cnt_a, *cap, *cnt; const i64 *off_a, *off_c;
    meme_alnreg* stage; uint8_t* status; i64* list; unsigned long long* ctr;
    long long* cols_l; int* cols_c;          // FIN_LONGS / FIN_INTS values per record a list can hold, a list's columns at off_c
    meme_alnreg* out; const i64* off_out;
};

// the gar entries and the results of read r's worker batch, and the first entry of the records looked at of read m (r's mate: the same batch, batch_reads is even)
struct ResBatch { i64 g, j0; int nj, na; bool ok; };
__device__ __forceinline__ ResBatch res_batch(const ResArgs& A, i64 r, i64 m) {
    ResBatch B = {0, 0, 0, 0, false};
    const i64 b = r / A.o.batch_reads;
    if (b >= A.nbatches) return B;
    const i64 g0 = A.gar_off[b], g1 = A.gar_off[b + 1], j0 = A.job_off[b], j1 = A.job_off[b + 1], g_end = A.gar_off[A.nbatches];
    const i64 cur = res_cursor(A.off_a[m], A.off_a[res_batch_first(m, A.o.batch_reads)]);
    const i64 na = A.cnt_a[m];
    B.ok = g0 >= 0 && g1 >= g0 && g1 <= g_end && j0 >= 0 && j1 >= j0 && j1 <= A.njobs && j1 - j0 <= INT_MAX && cur >= 0 && na >= 0 && g0 + cur + 4 * na <= g1 &&
           (A.gar || na == 0) && (A.res || j1 == j0);      // (a null array is legitimate where the offsets say it is empty -- max_matesw 0, no jobs --, and status 2 where they do not)
    if (B.ok) { B.g = g0 + cur; B.j0 = j0; B.nj = (int)(j1 - j0); B.na = (int)na; }
    return B;
}

template <int PASS>
__global__ void __launch_bounds__(256) k_rescue_route(ResArgs A) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < A.nreads; r += (i64)gridDim.x * blockDim.x) {
        i64 base; int n;
        const bool ok = reg_span(A.reg_off, r, A.total_regs, &base, &n);
        if (PASS == 0) {
            A.cnt_a[r] = res_anchor_count(n, [&](int k) -> int { return A.in[base + k].score; }, A.o.pen_unpaired, A.o.max_matesw);
            continue;
        }
        const i64 m = r ^ 1;
        i64 mbase; int nm;
        const bool mok = reg_span(A.reg_off, m, A.total_regs, &mbase, &nm);
        const ResBatch B = res_batch(A, r, m);
        int posed = 0;
        if (ok && mok && B.ok)
            for (int e = 0; e < 4 * B.na; ++e) posed += A.gar[B.g + e] >= 0 ? 1 : 0;
        const bool fine = ok && mok && B.ok;
        A.status[r] = fine ? 0 : 2;
        A.cap[r] = fine ? (i64)n + posed : n;
        A.cnt[r] = 0;
        if (fine && res_listed(posed, res_mate_sort(A.ums[r], A.ums[m]), nm, n)) A.list[atomicAdd(A.ctr + RES_CTR_WAVE, 1ull)] = r;      // (at most nreads entries; their order does not matter)
        else A.cnt[r] = -1 - (i64)n;                                                // (the light tier's: n records to copy)
    }
}

__global__ void __launch_bounds__(256) k_rescue_light(ResArgs A) {
    const int p = threadIdx.x & 7;
    const i64 groups = (i64)gridDim.x * 32;
    for (i64 r = (i64)blockIdx.x * 32 + threadIdx.x / 8; r < A.nreads; r += groups) {
        const i64 c = A.cnt[r];
        if (c >= 0) continue;                                                       // (listed)
        const i64 n = -1 - c, at = A.off_c[r];
        i64 base; int n_in;
        reg_span(A.reg_off, r, A.total_regs, &base, &n_in);
        const bool fits = at >= 0 && at + n <= A.out_cap;
        const bool clear = A.status[r] == 0;
        if (fits && p < 7) {
            const uint4* src = reinterpret_cast<const uint4*>(A.in + base);
            uint4* dst = reinterpret_cast<uint4*>(A.stage + at);
            for (i64 k = 0; k < n; ++k) {
                uint4 w = src[k * 7 + p];
                if (p == 6 && clear) w.z = 0;                                       // flg (:859-862)
                dst[k * 7 + p] = w;
            }
        }
        if (p == 7) { A.cnt[r] = fits ? n : 0; if (!fits) A.status[r] = 2; }
    }
}
static_assert(sizeof(meme_alnreg) == 112 && offsetof(meme_alnreg, flg) == 104, "the record kernels copy a record as seven 16-byte words; flg is the third int of the last");

// the columns of the list a wavefront walks: every lane loads the same word, and the walk gets it as a wave-uniform value
struct ResColsWave {
    int* c; long long* l; int cap;
    __device__ __forceinline__ int geti(int f, int i) const { return __builtin_amdgcn_readfirstlane(c[(size_t)f * cap + i]); }
    __device__ __forceinline__ void seti(int f, int i, int v) const { c[(size_t)f * cap + i] = v; }
    __device__ __forceinline__ int64_t getl(int f, int i) const { return uniform(l[(size_t)f * cap + i]); }
    __device__ __forceinline__ void setl(int f, int i, int64_t v) const { l[(size_t)f * cap + i] = v; }
    static __device__ __forceinline__ int64_t uniform(long long v) {
        return (int64_t)((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) | ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((u64)v >> 32)) << 32));
    }
};

__global__ void __launch_bounds__(64) k_rescue_wave(ResArgs A) {
    __shared__ long long lds_l[FIN_LONGS * RES_LDS_RECS];
    __shared__ int lds_c[FIN_INTS * RES_LDS_RECS];
    __shared__ int stack[3 * FIN_STACK];
    __shared__ meme_pestat pes[4];                                                 // (the rules take the statistics by address)
    const int lane = threadIdx.x;
    const i64 n_wave = (i64)*(A.ctr + RES_CTR_WAVE);                               // (complete: k_rescue_route ran before this launch)
    if ((i64)blockIdx.x >= n_wave) return;                                          // (the grid is sized by the reads, the host does not know the list's length: the
                                                                                    // workgroups beyond it leave on their first load, the whole workgroup as one)
    if (lane < 4) pes[lane] = A.pes[lane];
    __syncthreads();
    for (i64 hi = blockIdx.x; hi < n_wave; hi += gridDim.x) {                       // (uniform over the workgroup, and so is everything below)
        const i64 r = A.list[hi], m = r ^ 1;
        i64 base, mbase; int n_in, nm;
        reg_span(A.reg_off, r, A.total_regs, &base, &n_in);
        reg_span(A.reg_off, m, A.total_regs, &mbase, &nm);
        n_in = __builtin_amdgcn_readfirstlane(n_in); nm = __builtin_amdgcn_readfirstlane(nm);
        const ResBatch B = res_batch(A, r, m);                                      // (ok: the route kernel listed the read)
        const i64 at = A.off_c[r];
        const i64 cap64 = A.cap[r];
        const bool room = at >= 0 && cap64 >= n_in && cap64 <= INT_MAX && at + cap64 <= A.out_cap && B.ok;
        const int cap = __builtin_amdgcn_readfirstlane(room ? (int)cap64 : 0);
        const meme_alnreg* in = A.in + base;
        const meme_alnreg* min_ = A.in + mbase;
        int m_out = -1;
        ResRead res = {0, 0, 0, 0};
        const bool in_lds = cap <= A.lds_recs;
        const ResColsWave s = {in_lds ? lds_c : A.cols_c + at * FIN_INTS, in_lds ? lds_l : A.cols_l + at * FIN_LONGS, in_lds ? RES_LDS_RECS : (cap > 0 ? cap : 1)};
        if (room) {
            for (int k = lane; k < n_in; k += 64) {
                const meme_alnreg& R = in[k];
                s.setl(FIN_RB, k, R.rb); s.setl(FIN_RE, k, R.re);
                s.seti(FIN_QB, k, R.qb); s.seti(FIN_QE, k, R.qe); s.seti(FIN_RID, k, R.rid); s.seti(FIN_SCORE, k, R.score); s.seti(FIN_W, k, R.w); s.seti(FIN_NCOMP, k, R.n_comp_is_alt & 0x3fffffff);
            }
            __threadfence_block();
            __syncthreads();
            FinStack st = {stack, 0};
            const int l_ms = __builtin_amdgcn_readfirstlane(A.rlen[r]);
            const bool mate_sort = res_mate_sort(A.ums[r], A.ums[m]);
            m_out = rescue_end(
                s, n_in, cap, nm,
                [&](int k) -> ResAnchor {
                    const meme_alnreg& R = min_[k];
                    return ResAnchor{ResColsWave::uniform(R.rb), __builtin_amdgcn_readfirstlane(R.rid), __builtin_amdgcn_readfirstlane(R.score), __builtin_amdgcn_readfirstlane(res_is_alt_of(R.n_comp_is_alt))};
                },
                mate_sort, l_ms, A.l_pac, pes,
                [&](i64 rb, int n) -> int {                                         // the lanes stride over the list as it stands; the statistics' own bits come with nm = 0
                    int part = mate_skip_mask(pes, A.l_pac, rb, nullptr, 0);
                    for (int k = lane; k < n; k += 64) {
                        const int x = s.c[(size_t)FIN_ORD * s.cap + k];
                        const meme_mate_reg one = {s.l[(size_t)FIN_RB * s.cap + x], 0, 0};
                        part |= mate_skip_mask(pes, A.l_pac, rb, &one, 1);
                    }
                    for (int d = 32; d; d >>= 1) part |= __shfl_xor(part, d);
                    return __builtin_amdgcn_readfirstlane(part);
                },
                [&](i64 mid, i64& rb, i64& re) -> int { return bns_clamp_to_mid(A.l_pac, A.contig_off, A.contig_len, A.n_contigs, mid, rb, re); },
                [&](int q, int o, meme_kswr* aln) -> bool {
                    if (q >= B.na) return false;
                    const int idx = __builtin_amdgcn_readfirstlane(A.gar[B.g + 4 * q + o]);
                    if (idx < 0 || idx >= B.nj) return false;
                    const meme_kswr& K = A.res[B.j0 + idx];
                    aln->score = __builtin_amdgcn_readfirstlane(K.score); aln->te = __builtin_amdgcn_readfirstlane(K.te); aln->qe = __builtin_amdgcn_readfirstlane(K.qe);
                    aln->score2 = __builtin_amdgcn_readfirstlane(K.score2); aln->te2 = __builtin_amdgcn_readfirstlane(K.te2); aln->tb = __builtin_amdgcn_readfirstlane(K.tb);
                    aln->qb = __builtin_amdgcn_readfirstlane(K.qb);
                    return true;
                },
                A.o, st, &res);
            __threadfence_block();
            __syncthreads();
        }
        const bool keep_input = m_out < 0;                                          // status 1, or no room: the list as it came, flg included
        const bool fits = at >= 0 && at + n_in <= A.out_cap;
        const int m_fin = keep_input ? (fits ? n_in : 0) : m_out;
        for (int k = lane; k < m_fin; k += 64) {
            RegWords R;
            if (keep_input) R = reg_load(in + k);
            else {
                const int x = s.c[(size_t)FIN_ORD * s.cap + k];
                const auto ci = [&](int f) -> int { return s.c[(size_t)f * s.cap + x]; };
                if (x < n_in) {
                    R = reg_load(in + x);
                    R.q1.y = (uint32_t)ci(FIN_QE);
                    R.set_word(res_word_old(R.word(), ci(FIN_NCOMP)));
                } else {
                    const uint4 z = {0u, 0u, 0u, 0u};
                    R.q0 = z; R.q1 = z; R.q2 = z; R.q3 = z; R.q4 = z; R.q5 = z; R.q6 = z;
                    R.set_span(s.l[(size_t)FIN_RB * s.cap + x], s.l[(size_t)FIN_RE * s.cap + x], ci(FIN_QB), ci(FIN_QE));
                    R.q1.z = (uint32_t)ci(FIN_RID);
                    R.set_scores(ci(FIN_SCORE), 0, 0, ci(FIN_CSUB), 0, ci(FIN_SEEDCOV));
                    R.q4.z = (uint32_t)-1;                                          // secondary
                    R.set_word(res_word_new(ci(RES_ISALT), ci(FIN_NCOMP)));
                }
                R.q6.z = 0;                                                         // flg (:859-862)
            }
            reg_store(A.stage + at + k, R);
        }
        if (lane == 0) {
            A.cnt[r] = m_fin;
            if (!room) A.status[r] = 2;
            else if (res.status) A.status[r] = 1;
            else {
                if (res.n_tested) atomicAdd(A.ctr + RES_CTR_TESTED, (unsigned long long)res.n_tested);
                if (res.n_pushed) atomicAdd(A.ctr + RES_CTR_PUSHED, (unsigned long long)res.n_pushed);
                if (n_in + res.n_pushed - m_out) atomicAdd(A.ctr + RES_CTR_REMOVED, (unsigned long long)(n_in + res.n_pushed - m_out));
            }
        }
        __syncthreads();                                                            // (the columns in LDS are the next list's)
    }
}

__global__ void __launch_bounds__(256) k_rescue_pack(ResArgs A) {
    const int p = threadIdx.x & 7;
    const i64 groups = (i64)gridDim.x * 32;
    for (i64 r = (i64)blockIdx.x * 32 + threadIdx.x / 8; r < A.nreads; r += groups) {
        const i64 m = A.cnt[r], at = A.off_c[r];
        if (m <= 0 || p >= 7) continue;
        if (A.off_out[r] < 0 || A.off_out[r] + m > A.out_cap || at < 0 || at + m > A.out_cap) continue;
        const uint4* src = reinterpret_cast<const uint4*>(A.stage + at);
        uint4* dst = reinterpret_cast<uint4*>(A.out + A.off_out[r]);
        for (i64 k = 0; k < m; ++k) dst[k * 7 + p] = src[k * 7 + p];
    }
}

int rescue_check(const char* who, i64 nreads, const meme_rescue_jobs_in* jobs, const meme_pestat* pes, const meme_contig* contigs, int32_t n_contigs, const meme_rescue_opt* o) {
    if (!jobs || !pes || !contigs || n_contigs < 1 || !o) { meme_set_error("%s: null argument", who); return MEME_E_ARG; }
    if (nreads & 1) { meme_set_error("%s: an odd number of reads is not a set of pairs", who); return MEME_E_ARG; }
    if (o->max_matesw < 0 || o->batch_reads < 2 || (o->batch_reads & 1)) { meme_set_error("%s: max_matesw must not be negative, batch_reads even and at least 2", who); return MEME_E_ARG; }
    if (jobs->njobs < 0 || jobs->nbatches != (nreads + o->batch_reads - 1) / o->batch_reads || (jobs->nbatches > 0 && (!jobs->gar_off || !jobs->job_off)) || (jobs->njobs > 0 && !jobs->res)) {
        meme_set_error("%s: jobs: %lld worker batches for %lld reads in batches of %d, or a null array", who, (long long)jobs->nbatches, (long long)nreads, o->batch_reads);
        return MEME_E_ARG;
    }
    return MEME_OK;
}

// the stage's kernels on device arrays, asynchronous on ctx->stream
int rescue_launch(meme_ctx* ctx, const meme_alnreg* d_regs, const i64* d_reg_off, const uint8_t* d_ums, const int32_t* d_rlen, i64 nreads, i64 total_regs, const meme_rescue_jobs_in* J,
                  const meme_pestat* pes, const ContigTab& ct, int32_t n_contigs, i64 l_pac, const meme_rescue_opt* opt, const meme_rescue_device_out* o) {
    RescueWs& W = ctx->rescue;
    const i64 out_cap = total_regs + J->njobs;
    int rc;
    if ((rc = meme_buf_reserve(ctx, W.stage, (size_t)(out_cap + 1) * sizeof(meme_alnreg))) || (rc = meme_buf_reserve(ctx, W.cnt_a, (size_t)(nreads + 1) * 8)) ||
        (rc = meme_buf_reserve(ctx, W.off_a, (size_t)(nreads + 1) * 8)) || (rc = meme_buf_reserve(ctx, W.cap, (size_t)(nreads + 1) * 8)) || (rc = meme_buf_reserve(ctx, W.off_c, (size_t)(nreads + 1) * 8)) ||
        (rc = meme_buf_reserve(ctx, W.cnt, (size_t)(nreads + 1) * 8)) || (rc = meme_buf_reserve(ctx, W.list, (size_t)(nreads + 1) * 8)) ||
        (rc = meme_buf_reserve(ctx, W.cols_l, (size_t)(out_cap + 1) * FIN_LONGS * 8)) || (rc = meme_buf_reserve(ctx, W.cols_c, (size_t)(out_cap + 1) * FIN_INTS * 4))) return rc;
    HIP_TRY(W.ev.ensure());
    ResArgs A;
    memset(&A, 0, sizeof(A));
    A.in = d_regs; A.reg_off = d_reg_off; A.ums = d_ums; A.rlen = d_rlen; A.nreads = nreads; A.total_regs = total_regs; A.out_cap = out_cap;
    A.gar = J->gar; A.gar_off = (const i64*)J->gar_off; A.job_off = (const i64*)J->job_off; A.nbatches = J->nbatches; A.res = J->res; A.njobs = J->njobs;
    for (int k = 0; k < 4; ++k) A.pes[k] = pes[k];
    A.l_pac = l_pac; A.contig_off = ct.off; A.contig_len = ct.len; A.n_contigs = n_contigs;
    A.o = *opt; A.lds_recs = tune_at_most(ctx->rescue_lds_recs, RES_LDS_RECS);
    A.cnt_a = (i64*)W.cnt_a.p; A.off_a = (const i64*)W.off_a.p; A.cap = (i64*)W.cap.p; A.off_c = (const i64*)W.off_c.p; A.cnt = (i64*)W.cnt.p;
    A.stage = (meme_alnreg*)W.stage.p; A.status = o->d_status; A.list = (i64*)W.list.p; A.ctr = (unsigned long long*)o->d_counters;
    A.cols_l = (long long*)W.cols_l.p; A.cols_c = (int*)W.cols_c.p; A.out = o->d_regs_out; A.off_out = o->d_reg_off_out;
    const i64 cap = tune_grid_cap(ctx->rescue_blocks);
    HIP_TRY(hipEventRecord(W.ev[0], ctx->stream));
    HIP_TRY(hipMemsetAsync(o->d_counters, 0, RES_CTRS * 8, ctx->stream));
    hipLaunchKernelGGL(k_rescue_route<0>, dim3(grid_blocks(nreads, 256, cap)), dim3(256), 0, ctx->stream, A);
    HIP_TRY(hipGetLastError());
    if ((rc = meme_scan_exclusive(ctx, A.cnt_a, (i64*)W.off_a.p, nreads))) return rc;
    hipLaunchKernelGGL(k_rescue_route<1>, dim3(grid_blocks(nreads, 256, cap)), dim3(256), 0, ctx->stream, A);
    HIP_TRY(hipGetLastError());
    if ((rc = meme_scan_exclusive(ctx, A.cap, (i64*)W.off_c.p, nreads))) return rc;
    hipLaunchKernelGGL(k_rescue_light, dim3(grid_blocks(nreads, 32, cap)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_rescue_wave, dim3(grid_blocks(nreads, 1, cap)), dim3(64), 0, ctx->stream, A);
    HIP_TRY(hipGetLastError());
    if ((rc = meme_scan_exclusive(ctx, A.cnt, o->d_reg_off_out, nreads))) return rc;
    hipLaunchKernelGGL(k_rescue_pack, dim3(grid_blocks(nreads, 32, cap)), dim3(256), 0, ctx->stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(W.ev[1], ctx->stream));
    return MEME_OK;
}

}  // namespace

extern "C" int meme_rescue_batch_device(meme_ctx* ctx, const meme_alnreg* d_regs, const int64_t* d_reg_off, const uint8_t* d_use_mate_sort, const int32_t* d_read_len, int64_t nreads,
                                        int64_t total_regs, const meme_rescue_jobs_in* d_jobs, const meme_pestat* pes, const meme_contig* contigs, int32_t n_contigs, int64_t l_pac,
                                        const meme_rescue_opt* opt, const meme_rescue_device_out* out) {
    static const char* const who = "meme_rescue_batch_device";
    const bool rest = ctx && out && out->d_counters && out->d_reg_off_out && (nreads <= 0 || (out->d_status && d_use_mate_sort && d_read_len));
    int rc;
    if ((rc = reg_check_device(who, rest, d_regs, out ? out->d_regs_out : nullptr, d_reg_off, nreads, total_regs)) || (rc = rescue_check(who, nreads, d_jobs, pes, contigs, n_contigs, opt))) return rc;
    if (d_jobs->njobs > 0 && (!out->d_regs_out || ((uintptr_t)out->d_regs_out & 15))) { meme_set_error("%s: null argument (or the output records are not 16-byte aligned)", who); return MEME_E_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    if (nreads == 0) {
        HIP_TRY(hipMemsetAsync(out->d_counters, 0, RES_CTRS * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(out->d_reg_off_out, 0, 8, ctx->stream));
        return MEME_OK;
    }
    ContigTab ct(nullptr, 0);
    if ((rc = meme_contigs(ctx, (std::string(who) + ": ").c_str(), contigs, n_contigs, l_pac, &ct))) return rc;
    return rescue_launch(ctx, d_regs, (const i64*)d_reg_off, d_use_mate_sort, d_read_len, nreads, total_regs, d_jobs, pes, ct, n_contigs, l_pac, opt, out);
}

extern "C" int meme_rescue_batch_host(meme_ctx* ctx, const meme_alnreg* regs, const int64_t* reg_off, const uint8_t* use_mate_sort, const int32_t* read_len, int64_t nreads,
                                      const meme_rescue_jobs_in* jobs, const meme_pestat* pes, const meme_contig* contigs, int32_t n_contigs, int64_t l_pac, const meme_rescue_opt* opt,
                                      meme_rescue_host_result* out) {
    static const char* const who = "meme_rescue_batch_host";
    if (!ctx || !out || nreads < 0 || (nreads > 0 && (!reg_off || !use_mate_sort || !read_len))) { meme_set_error("%s: null argument", who); return MEME_E_ARG; }
    int rc = rescue_check(who, nreads, jobs, pes, contigs, n_contigs, opt);
    if (rc) return rc;
    const i64 nb = jobs->nbatches, nj = jobs->njobs;
    const i64 n_gar = nb > 0 ? jobs->gar_off[nb] : 0;
    if (n_gar < 0 || (n_gar > 0 && !jobs->gar)) { meme_set_error("%s: jobs: gar_off ends at %lld, or gar is null", who, (long long)n_gar); return MEME_E_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    RescueWs& W = ctx->rescue;
    if ((rc = meme_hostbuf_reserve(ctx, W.h_reg_off, (size_t)(nreads + 1) * 8 + 64))) return rc;      // (an empty call has offsets too: one 0)
    out->reg_off = (const int64_t*)W.h_reg_off.p;
    ((i64*)W.h_reg_off.p)[0] = 0;
    if (nreads == 0) return MEME_OK;
    ContigTab ct(nullptr, 0);
    if ((rc = meme_contigs(ctx, (std::string(who) + ": ").c_str(), contigs, n_contigs, l_pac, &ct))) return rc;
    i64 total;
    if ((rc = reg_upload_host(ctx, who, regs, reg_off, nreads, W.regs, W.reg_off, &total))) return rc;
    const size_t obytes = (size_t)(total + nj) * sizeof(meme_alnreg);
    const Download offs = {W.h_reg_off, W.reg_off_out, (size_t)(nreads + 1) * 8}, status = {W.h_status, W.status, (size_t)nreads}, ctrs = {ctx->h_ctr, W.counters, RES_CTRS * 8},
                   recs = {W.h_regs, W.out, obytes};
    if ((rc = reg_reserve(ctx, {{W.out, obytes}, {W.reg_off_out, offs.bytes}, {W.status, status.bytes}, {W.counters, ctrs.bytes}, {W.ums, (size_t)nreads}, {W.rlen, (size_t)nreads * 4},
                                {W.gar, (size_t)n_gar * 4}, {W.gar_off, (size_t)(nb + 1) * 8}, {W.job_off, (size_t)(nb + 1) * 8}, {W.res, (size_t)nj * sizeof(meme_kswr)}})) ||
        (rc = reg_download_reserve(ctx, {offs, status, ctrs, recs}))) return rc;
    HIP_TRY(hipMemcpyAsync(W.ums.p, use_mate_sort, (size_t)nreads, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(W.rlen.p, read_len, (size_t)nreads * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_gar) HIP_TRY(hipMemcpyAsync(W.gar.p, jobs->gar, (size_t)n_gar * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(W.gar_off.p, jobs->gar_off, (size_t)(nb + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(W.job_off.p, jobs->job_off, (size_t)(nb + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (nj) HIP_TRY(hipMemcpyAsync(W.res.p, jobs->res, (size_t)nj * sizeof(meme_kswr), hipMemcpyHostToDevice, ctx->stream));
    const meme_rescue_jobs_in dj = {(const int32_t*)W.gar.p, (const int64_t*)W.gar_off.p, (const int64_t*)W.job_off.p, nb, (const meme_kswr*)W.res.p, nj};
    const meme_rescue_device_out d = {(meme_alnreg*)W.out.p, (int64_t*)W.reg_off_out.p, (uint8_t*)W.status.p, (uint64_t*)W.counters.p};
    if ((rc = rescue_launch(ctx, (const meme_alnreg*)W.regs.p, (const i64*)W.reg_off.p, (const uint8_t*)W.ums.p, (const int32_t*)W.rlen.p, nreads, total, &dj, pes, ct, n_contigs, l_pac, opt, &d))) return rc;
    float ms = 0.f;
    if ((rc = reg_download(ctx, {offs, status, ctrs})) || (rc = reg_sync_ms(ctx, W.ev, &ms))) return rc;
    const i64 left = ((const i64*)W.h_reg_off.p)[nreads];
    if (left < 0 || left > total + nj) { meme_set_error("%s: the stage left %lld records of %lld and %lld jobs", who, (long long)left, (long long)total, (long long)nj); return MEME_E_HIP; }
    if (left) {                                                // (what the stage left: known only now)
        if ((rc = reg_download(ctx, {{W.h_regs, W.out, (size_t)left * sizeof(meme_alnreg)}}))) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    const unsigned long long* ctr = (const unsigned long long*)ctx->h_ctr.p;
    out->nreads = nreads; out->total_regs = left; out->regs = (const meme_alnreg*)W.h_regs.p; out->status = (const uint8_t*)W.h_status.p;
    out->n_wave = (i64)ctr[RES_CTR_WAVE]; out->n_tested = (i64)ctr[RES_CTR_TESTED]; out->n_pushed = (i64)ctr[RES_CTR_PUSHED]; out->n_removed = (i64)ctr[RES_CTR_REMOVED]; out->kernel_ms = ms;
    return MEME_OK;
}
