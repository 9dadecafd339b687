// Record finishing on the device: the tail of mem_kernel2_core (reference src/bwamem.cpp:1681-1719) -- the compaction of a read's alignment records to the
// live ones, mem_sort_dedup_patch_mate_sort (:312-383) with mem_patch_reg (:194-244) and the is_alt flag -- for every read of a batch, between the seed
// extension and the primary marking.  Everything that decides a result is meme_finish_rules.h; this file holds where the records live and who runs what.
//
//   k_finish_route  a lane per read: the live records (qe > qb) are counted, the first of them noted, and reads with two or more appended to the wavefront tier's
//                   list (one atomic append per read, nothing else)
//   k_finish_light  a lane per read with at most one live record: the record is copied with its is_alt bit (the function's early return: n_comp stays)
//   k_finish_wave   a wavefront (one 64-thread workgroup) per listed read, from its first instruction to its last store: every lane executes finish_read of the
//                   rules on the read's records -- the same loads and the same stores, in columns in LDS (up to FIN_LDS_RECS records) or in a workspace in HBM --,
//                   what it reads comes back through readfirstlane, so the walk lives in scalar registers and branches as one.  Only the patch score uses the
//                   lanes: a score-only banded global alignment, 64 columns at a time as k_gcig_t runs them, two H rows and one E row in LDS, F by the scan
//                   the CIGAR rules describe, the target streamed from the 2-bit text FIN_TS rows at a time (no matrix, no row count to fit anything).
//   k_finish_pack   eight lanes per read behind the scan of the per-read counts: the kept records from their input offsets to the compact output
//
// Nothing waits for another wavefront: no kernel reads what another workgroup of the same launch writes (the list is complete when the launch behind it starts),
// every loop is bounded by a record count, a sequence length or a band known when it starts, list lengths are read once, and every barrier, DPP and readlane
// stands in control flow that is the same on all lanes of its workgroup.
#include <limits.h>
#include <string.h>
#include <string>

#include "meme_common.h"
#include "meme_alnreg_words.h"
#include "meme_finish_rules.h"

#pragma clang fp contract(off)

namespace {

constexpr int FIN_LDS_RECS = 128;            // records handed over for a read whose columns stay in LDS (60 bytes each).  With 320 -- the fixture's largest read -- a workgroup held
                                             // 26.8 KB and the stage took 8.0 ms per 2 M reads; with 128, 15.3 KB and 5.9 ms (profiles/finish_stage.md): more workgroups per CU
constexpr int FIN_ROW = FIN_MAX_QLEN + 4;    // ints of an H or E row
constexpr int FIN_TS = 256;                  // target bases fetched at a time
enum { FIN_CTR_WAVE = 0, FIN_CTR_JOBS = 1, FIN_CTR_MERGED = 2, FIN_CTRS = 8 };

struct FinArgs {
    const meme_alnreg* in; const i64* reg_off; i64 nreads, total_regs;
    const uint8_t* reads; const i64* read_off; const u64* pac; i64 l_pac;
    const unsigned char* alt; int n_contigs;
    meme_finish_opt o; int lds_recs;
    meme_alnreg* stage; i64* cnt; int *live, *first; uint8_t *ums, *status;
    i64* list; unsigned long long* ctr;
    long long* cols_l; int* cols_c;          // FIN_LONGS / FIN_INTS values per input record, a read's columns at its input offset
    meme_alnreg* out; const i64* off_out;
};

__global__ void __launch_bounds__(256) k_finish_route(FinArgs A) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < A.nreads; r += (i64)gridDim.x * blockDim.x) {
        i64 base; int n;
        A.status[r] = reg_span(A.reg_off, r, A.total_regs, &base, &n) ? 0 : 2;
        int live = 0, first = 0;
        for (int k = 0; k < n; ++k) {
            const meme_alnreg& R = A.in[base + k];
            if (R.qe > R.qb) { if (!live) first = k; ++live; }
        }
        A.live[r] = live; A.first[r] = first;
        A.cnt[r] = 0; A.ums[r] = 1;
        if (live > 1) A.list[atomicAdd(A.ctr + FIN_CTR_WAVE, 1ull)] = r;         // (at most nreads entries; their order does not matter)
    }
}

__global__ void __launch_bounds__(256) k_finish_light(FinArgs A) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < A.nreads; r += (i64)gridDim.x * blockDim.x) {
        if (A.live[r] != 1) continue;
        i64 base; int n;
        reg_span(A.reg_off, r, A.total_regs, &base, &n);
        RegWords R = reg_load(A.in + base + A.first[r]);
        R.set_word(fin_word(R.word(), R.word(), R.rid(), A.alt, A.n_contigs));
        reg_store(A.stage + base, R);
        A.cnt[r] = 1;
    }
}

// the columns of the read a wavefront walks: every lane loads the same word, and the walk gets it as a wave-uniform value
struct FinColsWave {
    int* c; long long* l; int cap;
    __device__ __forceinline__ int geti(int f, int i) const { return __builtin_amdgcn_readfirstlane(c[(size_t)f * cap + i]); }
    __device__ __forceinline__ void seti(int f, int i, int v) const { c[(size_t)f * cap + i] = v; }
    __device__ __forceinline__ int64_t getl(int f, int i) const {
        const long long v = l[(size_t)f * cap + i];
        return (int64_t)((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) | ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((u64)v >> 32)) << 32));
    }
    __device__ __forceinline__ void setl(int f, int i, int64_t v) const { l[(size_t)f * cap + i] = v; }
};

// F's scan over the 64 lanes (gcig_scan_key / gcig_scan_f of the CIGAR rules): the maximum of the keys of the lanes below each lane, in the register file
// (row_shr 1/2/4/8, row_bcast15 into rows 1 and 3, row_bcast31 into rows 2 and 3, then wave_shr 1), as the CIGAR kernels scan it
#define FIN_DPP(src_, ctrl_, rowmask_) __builtin_amdgcn_update_dpp(GCIG_SCAN_FLOOR, (src_), (ctrl_), (rowmask_), 0xF, false)
__device__ __forceinline__ int fin_fscan(int key) {
    int sg = key, y;
    y = FIN_DPP(sg, 0x111, 0xF); sg = sg > y ? sg : y;
    y = FIN_DPP(sg, 0x112, 0xF); sg = sg > y ? sg : y;
    y = FIN_DPP(sg, 0x114, 0xF); sg = sg > y ? sg : y;
    y = FIN_DPP(sg, 0x118, 0xF); sg = sg > y ? sg : y;
    y = FIN_DPP(sg, 0x142, 0xA); sg = sg > y ? sg : y;
    y = FIN_DPP(sg, 0x143, 0xC); sg = sg > y ? sg : y;
    return FIN_DPP(sg, 0x138, 0xF);
}

// the patch score by the wavefront: P, rb and qb are the same on every lane (the caller's walk is); rd = the read's bases, rows = 3 * FIN_ROW ints, qs = FIN_MAX_QLEN
// + 12 bytes, ts = FIN_TS bytes of LDS
__device__ __forceinline__ int fin_wave_score(const FinArgs& A, const FinPose& P, i64 rb, int qb, const uint8_t* rd, int* rows, uint8_t* qs, uint8_t* ts) {
    const int lane = threadIdx.x;
    const int qlen = P.qlen, tlen = P.tlen, w = P.w;
    const bool rev = P.rev;
    const auto text_at = [&](int p) -> int { return text_base(A.pac, rev ? rb + tlen - 1 - p : rb + p); };
    __syncthreads();
    for (int j = lane; j < qlen; j += 64) qs[j] = rd[qb + (rev ? qlen - 1 - j : j)];
    __syncthreads();
    if (w < 0) {                                                                   // the gap-free shortcut (src/bwa.cpp:294-304)
        int part = 0;
        for (int j = lane; j < qlen; j += 64) part += gcig_score(text_at(j), qs[j], A.o.a, A.o.b);
        for (int d = 32; d; d >>= 1) part += __shfl_xor(part, d);
        return __builtin_amdgcn_readfirstlane(part);
    }
    const int oe_del = A.o.o_del + A.o.e_del, oe_ins = A.o.o_ins + A.o.e_ins, e_del = A.o.e_del, e_ins = A.o.e_ins;
    int* hp = rows;                              // H(i-1, j-1) at [j]
    int* hn = rows + FIN_ROW;
    int* eE = rows + 2 * FIN_ROW;
    for (int j = lane; j <= qlen; j += 64) { hp[j] = gcig_row0(j, w, A.o.o_ins, e_ins); eE[j] = GCIG_MINUS_INF; }
    __syncthreads();
    for (int i = 0; i < tlen; ++i) {
        if ((i & (FIN_TS - 1)) == 0) {                                             // the next FIN_TS target bases, in row order (the barrier above the loop, or the row's, has passed)
            for (int k = lane; k < FIN_TS && i + k < tlen; k += 64) ts[k] = (uint8_t)text_at(i + k);
            __syncthreads();
        }
        const int tb = ts[i & (FIN_TS - 1)];
        const int beg = gcig_beg(i, w), end = gcig_end(i, w, qlen);
        int f_in = GCIG_MINUS_INF;                                                 // F(i, first column of the chunk)
        if (lane == 0 && beg <= qlen) hn[beg] = gcig_left(i, beg, A.o.o_del, e_del);
        for (int cb = beg; cb < end; cb += 64) {
            const int j = cb + lane;
            const bool in = j < end;
            int m = GCIG_MINUS_INF, e = GCIG_MINUS_INF;
            if (in) { m = hp[j] + gcig_score(tb, qs[j], A.o.a, A.o.b); e = eE[j]; }
            const int f = gcig_scan_f(fin_fscan(gcig_scan_key(in, m, oe_ins, e_ins, lane)), f_in, e_ins, lane);
            const GcigCell c = gcig_cell(m, e, f, oe_del, e_del, oe_ins, e_ins);
            if (in) { eE[j] = c.e; hn[j + 1] = c.h; }
            f_in = __builtin_amdgcn_readlane(c.f, 63);                             // carry to the next chunk: F(i, cb + 64)
        }
        if (lane == 0 && end >= 0 && end <= qlen) eE[end] = GCIG_MINUS_INF;
        __syncthreads();
        int* t = hp; hp = hn; hn = t;
    }
    return __builtin_amdgcn_readfirstlane(hp[qlen]);
}

__global__ void __launch_bounds__(64) k_finish_wave(FinArgs A) {
    __shared__ long long lds_l[FIN_LONGS * FIN_LDS_RECS];
    __shared__ int lds_c[FIN_INTS * FIN_LDS_RECS];
    __shared__ int rows[3 * FIN_ROW];
    __shared__ int stack[3 * FIN_STACK];
    __shared__ __attribute__((aligned(4))) uint8_t qs[FIN_MAX_QLEN + 12];
    __shared__ __attribute__((aligned(4))) uint8_t ts[FIN_TS];
    const int lane = threadIdx.x;
    const i64 n_wave = (i64)*(A.ctr + FIN_CTR_WAVE);                               // (complete: k_finish_route ran before this launch)
    for (i64 hi = blockIdx.x; hi < n_wave; hi += gridDim.x) {                       // (uniform over the workgroup, and so is everything below)
        const i64 r = A.list[hi];
        i64 base; int n_in;
        reg_span(A.reg_off, r, A.total_regs, &base, &n_in);
        n_in = __builtin_amdgcn_readfirstlane(n_in);
        const bool in_lds = n_in <= A.lds_recs;
        const FinColsWave s = {in_lds ? lds_c : A.cols_c + base * FIN_INTS, in_lds ? lds_l : A.cols_l + base * FIN_LONGS, in_lds ? FIN_LDS_RECS : n_in};
        const meme_alnreg* in = A.in + base;
        for (int k = lane; k < n_in; k += 64) {
            const meme_alnreg& R = in[k];
            s.setl(FIN_RB, k, R.rb); s.setl(FIN_RE, k, R.re);
            s.seti(FIN_QB, k, R.qb); s.seti(FIN_QE, k, R.qe); s.seti(FIN_RID, k, R.rid); s.seti(FIN_SCORE, k, R.score); s.seti(FIN_TRUESC, k, R.truesc); s.seti(FIN_SUB, k, R.sub);
            s.seti(FIN_CSUB, k, R.csub); s.seti(FIN_SEEDCOV, k, R.seedcov); s.seti(FIN_W, k, R.w); s.seti(FIN_NCOMP, k, R.n_comp_is_alt & 0x3fffffff);
        }
        __threadfence_block();
        __syncthreads();
        const i64 ro = A.read_off[r];
        const int read_len = __builtin_amdgcn_readfirstlane((int)(A.read_off[r + 1] - ro));
        const uint8_t* rd = A.reads + ro;
        FinStack st = {stack, 0};
        FinRead res;
        const int m = finish_read(s, n_in, read_len, A.l_pac, A.o,
                                  [&](const FinPose& P, i64 rb, int qb) -> int { return fin_wave_score(A, P, rb, qb, rd, rows, qs, ts); }, st, &res);
        __threadfence_block();
        __syncthreads();
        for (int k = lane; k < m; k += 64) {
            const int x = s.c[(size_t)FIN_ORD * s.cap + k];
            const auto ci = [&](int f) -> int { return s.c[(size_t)f * s.cap + x]; };
            RegWords R = reg_load(in + x);
            R.set_span(s.l[(size_t)FIN_RB * s.cap + x], s.l[(size_t)FIN_RE * s.cap + x], ci(FIN_QB), ci(FIN_QE));
            R.set_scores(ci(FIN_SCORE), ci(FIN_TRUESC), ci(FIN_SUB), ci(FIN_CSUB), ci(FIN_W), ci(FIN_SEEDCOV));
            R.set_word(fin_word(R.word(), ci(FIN_NCOMP), R.rid(), A.alt, A.n_contigs));
            reg_store(A.stage + base + k, R);
        }
        if (lane == 0) {
            A.cnt[r] = m; A.ums[r] = (uint8_t)res.use_mate_sort;
            if (res.status) A.status[r] = 1;
            if (res.n_jobs) atomicAdd(A.ctr + FIN_CTR_JOBS, (unsigned long long)res.n_jobs);
            if (res.n_merged) atomicAdd(A.ctr + FIN_CTR_MERGED, (unsigned long long)res.n_merged);
        }
        __syncthreads();                                                            // (the columns in LDS are the next read's)
    }
}

__global__ void __launch_bounds__(256) k_finish_pack(FinArgs A) {
    const int p = threadIdx.x & 7;
    const i64 groups = (i64)gridDim.x * 32;
    for (i64 r = (i64)blockIdx.x * 32 + threadIdx.x / 8; r < A.nreads; r += groups) {
        const i64 m = A.cnt[r];
        if (m <= 0 || p >= 7) continue;
        i64 base; int n;
        reg_span(A.reg_off, r, A.total_regs, &base, &n);
        if (A.off_out[r] < 0 || A.off_out[r] + m > A.total_regs) continue;       // (spans of the device form that overlap: more records kept than the output holds)
        const uint4* src = reinterpret_cast<const uint4*>(A.stage + base);
        uint4* dst = reinterpret_cast<uint4*>(A.out + A.off_out[r]);
        for (i64 k = 0; k < m; ++k) dst[k * 7 + p] = src[k * 7 + p];
    }
}
static_assert(sizeof(meme_alnreg) == 112, "k_finish_pack copies a record as seven 16-byte words");

int finish_check_opt(const char* who, const meme_finish_opt* o) {
    if (o->w < 0 || o->e_del < 1 || o->e_ins < 1) { meme_set_error("%s: w must not be negative, e_del and e_ins at least 1 (the band of a patch alignment divides by them)", who); return MEME_E_ARG; }
    if (o->w > (INT_MAX >> 3)) { meme_set_error("%s: w is too large", who); return MEME_E_ARG; }
    return MEME_OK;
}

// what both forms check of the ctx and stage for the kernels: the resident batch, the index, the contigs
int finish_prepare(meme_ctx* ctx, const char* who, i64 nreads, const meme_contig* contigs, int32_t n_contigs, i64 l_pac, ContigTab* ct) {
    if (ctx->batch.last_seed_reads <= 0 || !ctx->batch.reads_resident || !ctx->batch.reads.p || !ctx->batch.read_off.p || !ctx->idx.pac) {
        meme_set_error("%s: no seeded batch (or no index) on this ctx: a patch aligns a read of the batch against the index's text", who);
        return MEME_E_STATE;
    }
    if (nreads > ctx->batch.last_seed_reads) { meme_set_error("%s: %lld reads, the batch on the ctx has %lld", who, (long long)nreads, (long long)ctx->batch.last_seed_reads); return MEME_E_ARG; }
    if (n_contigs < 0 || (n_contigs > 0 && !contigs) || 2 * l_pac != ctx->idx.n) { meme_set_error("%s: null contigs, or l_pac is not the index's (%lld)", who, (long long)(ctx->idx.n >> 1)); return MEME_E_ARG; }
    return meme_contigs(ctx, (std::string(who) + ": ").c_str(), contigs, n_contigs, l_pac, ct);
}

// the stage's kernels on device arrays, asynchronous on ctx->stream; ev: recorded around them
int finish_launch(meme_ctx* ctx, const meme_alnreg* d_regs, const i64* d_reg_off, i64 nreads, i64 total_regs, const ContigTab& ct, int32_t n_contigs, i64 l_pac,
                  const meme_finish_opt* opt, const meme_finish_device_out* o) {
    FinishWs& F = ctx->finish;
    int rc;
    if ((rc = meme_buf_reserve(ctx, F.stage, (size_t)(total_regs + 1) * sizeof(meme_alnreg))) || (rc = meme_buf_reserve(ctx, F.cnt, (size_t)(nreads + 1) * 8)) ||
        (rc = meme_buf_reserve(ctx, F.live, (size_t)(nreads + 1) * 4)) || (rc = meme_buf_reserve(ctx, F.first, (size_t)(nreads + 1) * 4)) ||
        (rc = meme_buf_reserve(ctx, F.list, (size_t)(nreads + 1) * 8)) || (rc = meme_buf_reserve(ctx, F.cols_l, (size_t)(total_regs + 1) * FIN_LONGS * 8)) ||
        (rc = meme_buf_reserve(ctx, F.cols_c, (size_t)(total_regs + 1) * FIN_INTS * 4))) return rc;
    HIP_TRY(F.ev.ensure());
    FinArgs A;
    A.in = d_regs; A.reg_off = d_reg_off; A.nreads = nreads; A.total_regs = total_regs;
    A.reads = (const uint8_t*)ctx->batch.reads.p; A.read_off = (const i64*)ctx->batch.read_off.p; A.pac = ctx->idx.pac; A.l_pac = l_pac;
    A.alt = ct.alt; A.n_contigs = n_contigs; A.o = *opt;
    A.lds_recs = tune_at_most(ctx->finish_lds_recs, FIN_LDS_RECS);
    A.stage = (meme_alnreg*)F.stage.p; A.cnt = (i64*)F.cnt.p; A.live = (int*)F.live.p; A.first = (int*)F.first.p; A.ums = o->d_use_mate_sort; A.status = o->d_status;
    A.list = (i64*)F.list.p; A.ctr = (unsigned long long*)o->d_counters; A.cols_l = (long long*)F.cols_l.p; A.cols_c = (int*)F.cols_c.p;
    A.out = o->d_regs_out; A.off_out = o->d_reg_off_out;
    const i64 cap = tune_grid_cap(ctx->finish_blocks);
    HIP_TRY(hipEventRecord(F.ev[0], ctx->stream));
    HIP_TRY(hipMemsetAsync(o->d_counters, 0, FIN_CTRS * 8, ctx->stream));
    hipLaunchKernelGGL(k_finish_route, dim3(grid_blocks(nreads, 256, cap)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_finish_light, dim3(grid_blocks(nreads, 256, cap)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_finish_wave, dim3(grid_blocks(nreads, 1, cap)), dim3(64), 0, ctx->stream, A);
    HIP_TRY(hipGetLastError());
    if ((rc = meme_scan_exclusive(ctx, A.cnt, o->d_reg_off_out, nreads))) return rc;
    hipLaunchKernelGGL(k_finish_pack, dim3(grid_blocks(nreads, 32, cap)), dim3(256), 0, ctx->stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(F.ev[1], ctx->stream));
    return MEME_OK;
}

}  // namespace

extern "C" int meme_finish_batch_device(meme_ctx* ctx, const meme_alnreg* d_regs, const int64_t* d_reg_off, int64_t nreads, int64_t total_regs, const meme_contig* contigs,
                                        int32_t n_contigs, int64_t l_pac, const meme_finish_opt* opt, const meme_finish_device_out* out) {
    static const char* const who = "meme_finish_batch_device";
    const bool rest = ctx && opt && out && out->d_counters && out->d_reg_off_out && (nreads <= 0 || (out->d_use_mate_sort && out->d_status));
    int rc;
    if ((rc = reg_check_device(who, rest, d_regs, out ? out->d_regs_out : nullptr, d_reg_off, nreads, total_regs)) || (rc = finish_check_opt(who, opt))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ContigTab ct(nullptr, 0);
    if ((rc = finish_prepare(ctx, who, nreads, contigs, n_contigs, l_pac, &ct))) return rc;
    if (nreads == 0) {
        HIP_TRY(hipMemsetAsync(out->d_counters, 0, FIN_CTRS * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(out->d_reg_off_out, 0, 8, ctx->stream));
        return MEME_OK;
    }
    return finish_launch(ctx, d_regs, (const i64*)d_reg_off, nreads, total_regs, ct, n_contigs, l_pac, opt, out);
}

extern "C" int meme_finish_batch_host(meme_ctx* ctx, const meme_alnreg* regs, const int64_t* reg_off, int64_t nreads, const meme_contig* contigs, int32_t n_contigs, int64_t l_pac,
                                      const meme_finish_opt* opt, meme_finish_host_result* out) {
    static const char* const who = "meme_finish_batch_host";
    if (!ctx || !opt || !out || nreads < 0 || (nreads > 0 && !reg_off)) { meme_set_error("%s: null argument", who); return MEME_E_ARG; }
    int rc = finish_check_opt(who, opt);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    ContigTab ct(nullptr, 0);
    if ((rc = finish_prepare(ctx, who, nreads, contigs, n_contigs, l_pac, &ct))) return rc;
    FinishWs& F = ctx->finish;
    if ((rc = meme_hostbuf_reserve(ctx, F.h_reg_off, (size_t)(nreads + 1) * 8 + 64))) return rc;      // (an empty call has offsets too: one 0)
    out->reg_off = (const int64_t*)F.h_reg_off.p;
    ((i64*)F.h_reg_off.p)[0] = 0;
    if (nreads == 0) return MEME_OK;
    i64 total;
    if ((rc = reg_upload_host(ctx, who, regs, reg_off, nreads, F.regs, F.reg_off, &total))) return rc;
    const size_t rbytes = (size_t)total * sizeof(meme_alnreg);
    const Download offs = {F.h_reg_off, F.reg_off_out, (size_t)(nreads + 1) * 8}, ums = {F.h_ums, F.ums, (size_t)nreads}, status = {F.h_status, F.status, (size_t)nreads},
                   ctrs = {ctx->h_ctr, F.counters, FIN_CTRS * 8}, recs = {F.h_regs, F.out, rbytes};
    if ((rc = reg_reserve(ctx, {{F.out, rbytes}, {F.reg_off_out, offs.bytes}, {F.ums, ums.bytes}, {F.status, status.bytes}, {F.counters, ctrs.bytes}})) ||
        (rc = reg_download_reserve(ctx, {offs, ums, status, ctrs, recs}))) return rc;
    const meme_finish_device_out d = {(meme_alnreg*)F.out.p, (int64_t*)F.reg_off_out.p, (uint8_t*)F.ums.p, (uint8_t*)F.status.p, (uint64_t*)F.counters.p};
    if ((rc = finish_launch(ctx, (const meme_alnreg*)F.regs.p, (const i64*)F.reg_off.p, nreads, total, ct, n_contigs, l_pac, opt, &d))) return rc;
    float ms = 0.f;
    if ((rc = reg_download(ctx, {offs, ums, status, ctrs})) || (rc = reg_sync_ms(ctx, F.ev, &ms))) return rc;
    const i64 left = ((const i64*)F.h_reg_off.p)[nreads];
    if (left < 0 || left > total) { meme_set_error("%s: the stage left %lld records of %lld", who, (long long)left, (long long)total); return MEME_E_HIP; }
    if (left) {                                                // (what the stage kept: known only now)
        if ((rc = reg_download(ctx, {{F.h_regs, F.out, (size_t)left * sizeof(meme_alnreg)}}))) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    const unsigned long long* ctr = (const unsigned long long*)ctx->h_ctr.p;
    out->nreads = nreads; out->total_regs = left; out->regs = (const meme_alnreg*)F.h_regs.p; out->use_mate_sort = (const uint8_t*)F.h_ums.p; out->status = (const uint8_t*)F.h_status.p;
    out->n_wave = (i64)ctr[FIN_CTR_WAVE]; out->n_patch_jobs = (i64)ctr[FIN_CTR_JOBS]; out->n_patched = (i64)ctr[FIN_CTR_MERGED]; out->kernel_ms = ms;
    return MEME_OK;
}
