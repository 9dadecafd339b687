// Primary marking and mapping quality on the device: mem_mark_primary_se with mem_mark_primary_se_core (reference src/bwamem.cpp:1974-2046),
// mem_reorder_primary5 (:2078-2100) and mem_approx_mapq_se (:2052-2076) for every read of a batch -- the first and the third step of mem_sam_pe.
//
// Per read: hash every record (hash_64 of id + input index), order the records by alnreg_hlt (score descending, is_alt, hash: a strict total order, so
// ranks by counting give the order of the reference's introsort), walk them against the list z of non-secondary records, set secondary_all and alt_sc,
// and where ALT and primary-assembly records mix, order again by alnreg_hlt2, map the indices through the ranks and walk the primary-assembly records
// a second time (sub_n is not reset in between: the reference counts twice, so does this).  z is pushed in ascending index order, so "the first member
// of z, in list order, that overlaps significantly" is the lowest index that is not secondary and overlaps: a ballot and its lowest set bit.
//
// Two tiers in one call, by record count (tuning key primary_split, at most PRI_G):
//   k_primary_light  eight lanes per read, one record per lane, everything in registers and shuffles within the group
//   k_primary_heavy  a wavefront (one workgroup) per read for the rest, any count: records ordered into a workspace in HBM, z scanned 64 indices at a time
//                    (what the walk touches of a read's first 256 records is kept in LDS meanwhile)
// k_primary_route lists the heavy reads.  Every loop is bounded by the read's record count; no kernel waits for another workgroup.
//
// Everything that decides a result is meme_primary_rules.h (the orders, the overlap test, the score distance, what a hit does, alt_sc, the remap, the
// primary5 choice, the quality); this file holds where the records live and who runs what.  The record in registers and a read's span of the record
// array are meme_alnreg_words.h, shared with the record-finishing stage.
//
// Arithmetic: the overlap test is float as in the reference (one multiply, nothing to contract); the quality is IEEE double with contraction off, its
// logarithms looked up in a table the host's libm filled (the device's log is not glibc's; the arguments are small integers).
#include <math.h>
#include <string.h>

#include "meme_common.h"
#include "meme_alnreg_words.h"
#include "meme_primary_rules.h"

#pragma clang fp contract(off)

constexpr int PRI_G = 8;             // lanes per read in the light tier = the most records it takes

struct PriArgs {
    const meme_alnreg* in; const i64* reg_off; i64 nreads, total_regs; u64 id_base;
    meme_primary_opt o; int tmp, split;                       // tmp: pri_score_distance(o)
    meme_alnreg *out, *sorted; int* rank;
    int* n_pri; uint8_t *mapq, *status;
    i64* list; unsigned long long* n_heavy;
    const double* logtab;
};

// the quality of a record in registers, its logarithms from the table
__device__ __forceinline__ int pri_mapq_of(const PriArgs& A, const RegWords& R, bool* beyond) {
    const PriQual Q = {R.score(), R.sub(), R.csub(), R.sub_n(), R.qb(), R.qe(), R.rb(), R.re(), R.frac_rep()};
    const double* __restrict__ logtab = A.logtab;
    return pri_mapq(Q, A.o, [&](int k) -> double { return logtab[k]; }, beyond);
}

// ---- routing --------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_primary_route(PriArgs A) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < A.nreads; r += (i64)gridDim.x * blockDim.x) {
        i64 base; int n;
        A.status[r] = reg_span(A.reg_off, r, A.total_regs, &base, &n) ? 0 : 2;
        A.n_pri[r] = 0;
        if (n > A.split) A.list[atomicAdd(A.n_heavy, 1ull)] = r;      // (at most nreads entries; their order does not matter)
    }
}

// ---- light tier: eight lanes per read ----------------------------------------------------------------------------------------------------------
// The state of one record, held by the lane whose index in the group is the record's position in the current order.
struct PriLane { int qb, qe, score, alt, sub, sub_n, alt_sc, secondary, secondary_all, src; u64 hash; };
__device__ __forceinline__ PriLane pri_take(const PriLane& x, int from) {      // every lane takes the state of lane `from` of its group
    PriLane y;
    y.qb = __shfl(x.qb, from, PRI_G); y.qe = __shfl(x.qe, from, PRI_G); y.score = __shfl(x.score, from, PRI_G); y.alt = __shfl(x.alt, from, PRI_G);
    y.sub = __shfl(x.sub, from, PRI_G); y.sub_n = __shfl(x.sub_n, from, PRI_G); y.alt_sc = __shfl(x.alt_sc, from, PRI_G); y.secondary = __shfl(x.secondary, from, PRI_G);
    y.secondary_all = __shfl(x.secondary_all, from, PRI_G); y.src = __shfl(x.src, from, PRI_G);
    y.hash = (u64)__shfl((unsigned long long)x.hash, from, PRI_G);
    return y;
}
__device__ __forceinline__ unsigned pri_group_ballot(bool x) { return (unsigned)(__ballot(x) >> (threadIdx.x & 56)) & 0xffu; }
// the lane that holds position p after ranking: the lane whose rank is p (ranks of a group are a permutation of 0..7)
__device__ __forceinline__ int pri_inverse(int rank, int p) {
    int inv = p;
#pragma unroll
    for (int j = 0; j < PRI_G; ++j) if (__shfl(rank, j, PRI_G) == p) inv = j;
    return inv;
}
// mem_mark_primary_se_core over positions [0, n) of the group
__device__ __forceinline__ void pri_core_group(PriLane& x, int p, int n, float mask_level, int tmp) {
    for (int i = 1; i < n; ++i) {
        const int qbi = __shfl(x.qb, i, PRI_G), qei = __shfl(x.qe, i, PRI_G), sci = __shfl(x.score, i, PRI_G), alti = __shfl(x.alt, i, PRI_G);
        const unsigned m = pri_group_ballot(p < i && x.secondary < 0 && pri_overlap(x.qb, x.qe, qbi, qei, mask_level));
        if (m) {
            const int j = __ffs(m) - 1;
            if (p == j) { const PriHit h = pri_hit(x.sub, x.sub_n, x.score, x.alt, sci, alti, tmp); x.sub = h.sub; x.sub_n = h.sub_n; }
            if (p == i) x.secondary = j;
        }
    }
}

__global__ void __launch_bounds__(256) k_primary_light(PriArgs A) {
    const int p = threadIdx.x & (PRI_G - 1);
    const i64 groups = (i64)gridDim.x * (256 / PRI_G);
    for (i64 r = (i64)blockIdx.x * (256 / PRI_G) + threadIdx.x / PRI_G; r < A.nreads; r += groups) {     // (control flow below is uniform within a group: its lanes stay together)
        i64 base; int n;
        reg_span(A.reg_off, r, A.total_regs, &base, &n);
        if (n == 0 || n > A.split) continue;
        const bool live = p < n;
        PriLane x;
        x.qb = x.qe = x.score = x.alt = x.sub_n = 0; x.hash = 0;
        if (live) {
            const meme_alnreg& R = A.in[base + p];
            x.qb = R.qb; x.qe = R.qe; x.score = R.score; x.alt = pri_is_alt(R.n_comp_is_alt); x.sub_n = R.sub_n;
            x.hash = pri_hash64(A.id_base + (u64)r + (u64)p);
        }
        x.sub = x.alt_sc = 0; x.secondary = x.secondary_all = -1; x.src = p;
        // order by alnreg_hlt
        int rank = 0;
#pragma unroll
        for (int j = 0; j < PRI_G; ++j) {
            const int sj = __shfl(x.score, j, PRI_G), aj = __shfl(x.alt, j, PRI_G);
            const u64 hj = (u64)__shfl((unsigned long long)x.hash, j, PRI_G);
            rank += j < n && pri_hlt(sj, aj, hj, x.score, x.alt, x.hash);
        }
        if (!live) rank = p;
        x = pri_take(x, pri_inverse(rank, p));
        pri_core_group(x, p, n, A.o.mask_level, A.tmp);
        x.secondary_all = p;
        {
            const int s = x.secondary < 0 ? 0 : x.secondary;
            const int s_alt = __shfl(x.alt, s, PRI_G), s_score = __shfl(x.score, s, PRI_G);
            if (live) x.alt_sc = pri_alt_sc(x.alt_sc, x.alt, x.secondary, s_alt, s_score);
        }
        const int n_pri = __popc(pri_group_ballot(live && !x.alt));
        if (n_pri < n) {
            int rank2 = p;
            if (n_pri > 0) {
                rank2 = 0;
#pragma unroll
                for (int j = 0; j < PRI_G; ++j) {
                    const int sj = __shfl(x.score, j, PRI_G), aj = __shfl(x.alt, j, PRI_G);
                    const u64 hj = (u64)__shfl((unsigned long long)x.hash, j, PRI_G);
                    rank2 += j < n && pri_hlt2(sj, aj, hj, x.score, x.alt, x.hash);
                }
                if (!live) rank2 = p;
            }
            const int mapped = __shfl(rank2, x.secondary < 0 || x.secondary >= PRI_G ? 0 : x.secondary, PRI_G);
            if (live) {                                                  // (rank2 is the position the record is about to take)
                const PriMarks m = pri_remap(x.sub, x.secondary, x.alt, rank2, n_pri, mapped);
                x.sub = m.sub; x.secondary = m.secondary; x.secondary_all = m.secondary_all;
            }
            if (n_pri > 0) {
                x = pri_take(x, pri_inverse(rank2, p));
                pri_core_group(x, p, n_pri, A.o.mask_level, A.tmp);
            }
        } else x.secondary_all = x.secondary;
        if (A.o.primary5) {
            const unsigned cand = pri_group_ballot(p < n && pri_candidate(x.secondary, x.alt, x.score, A.o.T));
            if (__popc(cand) > 1) {
                PriLeft left = pri_left_none();
#pragma unroll
                for (int j = 0; j < PRI_G; ++j) {
                    const PriLeft c = {__shfl(x.qb, j, PRI_G), j};
                    if ((cand >> j) & 1u) left = pri_leftmost(left, c);
                }
                if (left.k != 0) {
                    x = pri_take(x, pri_swapped(p, left.k));
                    if (p >= 1) { x.secondary = pri_swapped(x.secondary, left.k); x.secondary_all = pri_swapped(x.secondary_all, left.k); }
                }
            }
        }
        if (live) {
            RegWords R = reg_load(A.in + base + x.src);
            R.set_marks(x.sub, x.alt_sc, x.sub_n, x.secondary, x.secondary_all);
            R.set_hash(x.hash);
            bool beyond = false;
            const int q = pri_mapq_of(A, R, &beyond);
            reg_store(A.out + base + p, R);
            A.mapq[base + p] = pri_byte(q);
            if (beyond) A.status[r] = 1;
            if (p == 0) A.n_pri[r] = n_pri;
        }
    }
}

// ---- heavy tier: a wavefront per read ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pri_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// What the walk reads and writes of a record.  The first PRI_LDS records of a read are walked in LDS (loaded before the walk, written back after it), the records behind
// them, if any, where they lie in HBM: a read of any size is walked, the usual ones without a trip to memory per step.
constexpr int PRI_LDS = 256;
struct PriWalk {
    meme_alnreg* a; int nc;                                   // records [0, nc) are in LDS
    int *qb, *qe, *score, *alt, *sub, *sub_n, *secondary;     // LDS, PRI_LDS entries each
    __device__ __forceinline__ int get_qb(int k) const { return k < nc ? qb[k] : a[k].qb; }
    __device__ __forceinline__ int get_qe(int k) const { return k < nc ? qe[k] : a[k].qe; }
    __device__ __forceinline__ int get_score(int k) const { return k < nc ? score[k] : a[k].score; }
    __device__ __forceinline__ int get_alt(int k) const { return k < nc ? alt[k] : pri_is_alt(a[k].n_comp_is_alt); }
    __device__ __forceinline__ int get_secondary(int k) const { return k < nc ? secondary[k] : a[k].secondary; }
    __device__ __forceinline__ int* at_sub(int k) const { return k < nc ? sub + k : &a[k].sub; }
    __device__ __forceinline__ int* at_sub_n(int k) const { return k < nc ? sub_n + k : &a[k].sub_n; }
    __device__ __forceinline__ int* at_secondary(int k) const { return k < nc ? secondary + k : &a[k].secondary; }
};
// mem_mark_primary_se_core over a[0, n): record i against the non-secondary records in front of it, 64 at a time; the earliest chunk with a hit has the first
// member of z that overlaps, its lowest lane.  One workgroup = one wavefront: the barrier orders lane 0's stores (LDS or HBM) before the next record's loads.
__device__ __forceinline__ void pri_core_wave(PriWalk w, int n, float mask_level, int tmp) {
    const int lane = threadIdx.x;
    w.nc = n < PRI_LDS ? n : PRI_LDS;
    for (int k = lane; k < w.nc; k += 64) {
        const meme_alnreg& r = w.a[k];
        w.qb[k] = r.qb; w.qe[k] = r.qe; w.score[k] = r.score; w.alt[k] = pri_is_alt(r.n_comp_is_alt); w.sub[k] = r.sub; w.sub_n[k] = r.sub_n; w.secondary[k] = r.secondary;
    }
    __syncthreads();
    for (int i = 1; i < n; ++i) {
        const int qbi = w.get_qb(i), qei = w.get_qe(i);
        int found = -1;
        for (int c = 0; c < i; c += 64) {
            const int k = c + lane;
            const unsigned long long m = __ballot(k < i && w.get_secondary(k) < 0 && pri_overlap(w.get_qb(k), w.get_qe(k), qbi, qei, mask_level));
            if (m) { found = c + __ffsll(m) - 1; break; }
        }
        if (found >= 0 && lane == 0) {
            int *sub = w.at_sub(found), *sub_n = w.at_sub_n(found);
            const PriHit h = pri_hit(*sub, *sub_n, w.get_score(found), w.get_alt(found), w.get_score(i), w.get_alt(i), tmp);
            *sub = h.sub; *sub_n = h.sub_n;
            *w.at_secondary(i) = found;
        }
        __syncthreads();
    }
    for (int k = lane; k < w.nc; k += 64) { meme_alnreg& r = w.a[k]; r.sub = w.sub[k]; r.sub_n = w.sub_n[k]; r.secondary = w.secondary[k]; }
    __syncthreads();
}

// Ranks by counting: rk[k] = how many of a[0, n) come before a[k] -- by alnreg_hlt with the hash of record j taken from id + j (second == false: a is the input, its hash field
// not yet written), by alnreg_hlt2 with the hash the record carries (second == true).  64 records at a time count against all, which pass through LDS PRI_LDS at a time as
// {score, is_alt, hash} -- one 16-byte LDS read, the same for every lane, per comparison.
__device__ __forceinline__ void pri_ranks_wave(const meme_alnreg* a, int n, bool second, u64 id, int4* keys, int* rk) {
    const int lane = threadIdx.x;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool valid = k < n;
        int sk = 0, ak = 0, rank = 0;
        u64 hk = 0;
        if (valid) { sk = a[k].score; ak = pri_is_alt(a[k].n_comp_is_alt); hk = second ? a[k].hash : pri_hash64(id + (u64)k); }
        for (int c = 0; c < n; c += PRI_LDS) {
            const int cn = n - c < PRI_LDS ? n - c : PRI_LDS;
            __syncthreads();                                                       // (the chunk before this one has been counted)
            for (int j = lane; j < cn; j += 64) {
                const u64 h = second ? a[c + j].hash : pri_hash64(id + (u64)(c + j));
                keys[j] = make_int4(a[c + j].score, pri_is_alt(a[c + j].n_comp_is_alt), (int)(uint32_t)h, (int)(uint32_t)(h >> 32));
            }
            __syncthreads();
            if (valid)
                for (int j = 0; j < cn; ++j) {
                    const int4 q = keys[j];
                    const u64 hj = (u64)(uint32_t)q.z | ((u64)(uint32_t)q.w << 32);
                    rank += second ? pri_hlt2(q.x, q.y, hj, sk, ak, hk) : pri_hlt(q.x, q.y, hj, sk, ak, hk);
                }
        }
        if (valid) rk[k] = rank;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(64) k_primary_heavy(PriArgs A) {
    __shared__ __attribute__((aligned(16))) int lds[7][PRI_LDS];                     // the walk's seven columns; the ranking's keys in the first four
    PriWalk walk = {nullptr, 0, lds[0], lds[1], lds[2], lds[3], lds[4], lds[5], lds[6]};
    int4* keys = reinterpret_cast<int4*>(&lds[0][0]);
    const int lane = threadIdx.x;
    const i64 n_heavy = (i64)*A.n_heavy;
    for (i64 hi = blockIdx.x; hi < n_heavy; hi += gridDim.x) {                       // (uniform over the workgroup, and so is every branch around a barrier below)
        const i64 r = A.list[hi];
        i64 base; int n;
        reg_span(A.reg_off, r, A.total_regs, &base, &n);
        const meme_alnreg* in = A.in + base;
        meme_alnreg *t = A.sorted + base, *out = A.out + base;
        int* rk = A.rank + base;
        const u64 id = A.id_base + (u64)r;
        // order by alnreg_hlt into t
        pri_ranks_wave(in, n, false, id, keys, rk);
        int pri = 0;
        for (int k = lane; k < n; k += 64) {
            RegWords R = reg_load(in + k);
            R.set_marks(0, 0, R.sub_n(), -1, -1);
            R.set_hash(pri_hash64(id + (u64)k));
            reg_store(t + rk[k], R);
            pri += R.is_alt() == 0;
        }
        const int n_pri = pri_wave_sum(pri);
        __syncthreads();
        walk.a = t;
        pri_core_wave(walk, n, A.o.mask_level, A.tmp);
        for (int k = lane; k < n; k += 64) {
            const int s = t[k].secondary;
            const meme_alnreg& parent = t[s < 0 ? 0 : s];
            t[k].secondary_all = k;
            t[k].alt_sc = pri_alt_sc(t[k].alt_sc, pri_is_alt(t[k].n_comp_is_alt), s, pri_is_alt(parent.n_comp_is_alt), parent.score);
        }
        __syncthreads();
        if (n_pri < n) {
            if (n_pri > 0) pri_ranks_wave(t, n, true, id, keys, rk);
            else {
                for (int k = lane; k < n; k += 64) rk[k] = k;
                __syncthreads();
            }
            for (int k = lane; k < n; k += 64) {
                RegWords R = reg_load(t + k);
                const int d = rk[k];
                const PriMarks m = pri_remap(R.sub(), R.secondary(), R.is_alt(), d, n_pri, rk[R.secondary() < 0 ? 0 : R.secondary()]);
                R.set_marks(m.sub, R.alt_sc(), R.sub_n(), m.secondary, m.secondary_all);
                reg_store(out + d, R);
            }
            __syncthreads();
            walk.a = out;
            if (n_pri > 0) pri_core_wave(walk, n_pri, A.o.mask_level, A.tmp);
        } else {
            for (int k = lane; k < n; k += 64) { RegWords R = reg_load(t + k); R.set_secondary_all(R.secondary()); reg_store(out + k, R); }
            __syncthreads();
        }
        if (A.o.primary5) {
            int cnt = 0;
            PriLeft left = pri_left_none();
            for (int k = lane; k < n; k += 64)
                if (pri_candidate(out[k].secondary, pri_is_alt(out[k].n_comp_is_alt), out[k].score, A.o.T)) { ++cnt; const PriLeft c = {out[k].qb, k}; left = pri_leftmost(left, c); }
            cnt = pri_wave_sum(cnt);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {                                       // the leftmost over the lanes
                const PriLeft other = {__shfl_xor(left.qb, d), __shfl_xor(left.k, d)};
                left = pri_leftmost(left, other);
            }
            const int left_k = left.k;
            if (cnt > 1 && left_k != 0 && left_k < n) {
                if (lane < (int)(sizeof(meme_alnreg) / 4)) {                          // swap the two records a 32-bit word per lane
                    uint32_t *x = (uint32_t*)&out[0] + lane, *y = (uint32_t*)&out[left_k] + lane;
                    const uint32_t v = *x; *x = *y; *y = v;
                }
                __syncthreads();
                for (int k = lane < 1 ? 64 : lane; k < n; k += 64) { out[k].secondary = pri_swapped(out[k].secondary, left_k); out[k].secondary_all = pri_swapped(out[k].secondary_all, left_k); }
                __syncthreads();
            }
        }
        bool beyond = false;
        for (int k = lane; k < n; k += 64) A.mapq[base + k] = pri_byte(pri_mapq_of(A, reg_load(out + k), &beyond));
        if (beyond) A.status[r] = 1;
        if (lane == 0) A.n_pri[r] = n_pri;
        __syncthreads();
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------
static int primary_check_opt(const char* who, const meme_primary_opt* o) {
    if (!(o->mapQ_coef_len > 0)) { meme_set_error("%s: mapQ_coef_len must be positive (the stage has the reference's mapQ_coef_len > 0 branch only)", who); return MEME_E_ARG; }
    if (o->a < 1 || (i64)o->a + o->b <= 0) { meme_set_error("%s: a must be at least 1 and a + b positive", who); return MEME_E_ARG; }
    return MEME_OK;
}

// the table of logarithms of the ctx (the pairing decision looks its own up in it too)
int meme_logtab(meme_ctx* ctx, const double** d_tab) {
    PrimaryWs& P = ctx->primary;
    if (int rc = meme_buf_reserve(ctx, P.logtab, (size_t)PRI_LOG * 8)) return rc;
    if (!P.log_ready) {
        std::vector<double> tab((size_t)PRI_LOG);
        for (int k = 0; k < PRI_LOG; ++k) tab[(size_t)k] = log((double)k);
        HIP_TRY(hipMemcpyAsync(P.logtab.p, tab.data(), (size_t)PRI_LOG * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));          // (tab goes out of scope)
        P.log_ready = true;
    }
    *d_tab = (const double*)P.logtab.p;
    return MEME_OK;
}

// the stage's kernels on device arrays, asynchronous on ctx->stream; ev: recorded around them
static int primary_launch(meme_ctx* ctx, const meme_alnreg* d_regs, const i64* d_reg_off, i64 nreads, i64 total_regs, i64 id_base, const meme_primary_opt* opt,
                          const meme_primary_device_out* o) {
    PrimaryWs& P = ctx->primary;
    int rc;
    const double* logtab;
    if ((rc = meme_buf_reserve(ctx, P.sorted, (size_t)(total_regs + 1) * sizeof(meme_alnreg))) || (rc = meme_buf_reserve(ctx, P.rank, (size_t)(total_regs + 1) * 4)) ||
        (rc = meme_buf_reserve(ctx, P.list, (size_t)(nreads + 1) * 8)) || (rc = meme_logtab(ctx, &logtab))) return rc;
    HIP_TRY(P.ev.ensure());
    PriArgs A;
    A.in = d_regs; A.reg_off = d_reg_off; A.nreads = nreads; A.total_regs = total_regs; A.id_base = (u64)id_base; A.o = *opt;
    A.tmp = pri_score_distance(*opt);
    A.split = tune_split(ctx->primary_split, PRI_G);
    A.out = o->d_regs_out; A.sorted = (meme_alnreg*)P.sorted.p; A.rank = (int*)P.rank.p; A.n_pri = o->d_n_pri; A.mapq = o->d_mapq; A.status = o->d_status;
    A.list = (i64*)P.list.p; A.n_heavy = (unsigned long long*)o->d_n_heavy; A.logtab = logtab;
    const i64 cap = tune_grid_cap(ctx->primary_blocks);
    HIP_TRY(hipEventRecord(P.ev[0], ctx->stream));
    HIP_TRY(hipMemsetAsync(o->d_n_heavy, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_primary_route, dim3(grid_blocks(nreads, 256, cap)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_primary_light, dim3(grid_blocks(nreads, 256 / PRI_G, cap)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_primary_heavy, dim3(grid_blocks(nreads, 1, cap)), dim3(64), 0, ctx->stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(P.ev[1], ctx->stream));
    return MEME_OK;
}

extern "C" int meme_primary_batch_device(meme_ctx* ctx, const meme_alnreg* d_regs, const int64_t* d_reg_off, int64_t nreads, int64_t total_regs, int64_t id_base,
                                         const meme_primary_opt* opt, const meme_primary_device_out* out) {
    static const char* const who = "meme_primary_batch_device";
    const bool rest = ctx && opt && out && out->d_n_heavy && (nreads <= 0 || (out->d_n_pri && out->d_status)) && (total_regs <= 0 || out->d_mapq);
    int rc;
    if ((rc = reg_check_device(who, rest, d_regs, out ? out->d_regs_out : nullptr, d_reg_off, nreads, total_regs)) || (rc = primary_check_opt(who, opt))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (nreads == 0) { HIP_TRY(hipMemsetAsync(out->d_n_heavy, 0, 8, ctx->stream)); return MEME_OK; }
    return primary_launch(ctx, d_regs, (const i64*)d_reg_off, nreads, total_regs, id_base, opt, out);
}

extern "C" int meme_primary_batch_host(meme_ctx* ctx, const meme_alnreg* regs, const int64_t* reg_off, int64_t nreads, int64_t id_base, const meme_primary_opt* opt,
                                       meme_primary_host_result* out) {
    static const char* const who = "meme_primary_batch_host";
    if (!ctx || !opt || !out || nreads < 0 || (nreads > 0 && !reg_off)) { meme_set_error("%s: null argument", who); return MEME_E_ARG; }
    int rc = primary_check_opt(who, opt);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    if (nreads == 0) return MEME_OK;
    PrimaryWs& P = ctx->primary;
    i64 total;
    if ((rc = reg_upload_host(ctx, who, regs, reg_off, nreads, P.regs, P.reg_off, &total))) return rc;
    const Download recs = {P.h_regs, P.out, (size_t)total * sizeof(meme_alnreg)}, mapq = {P.h_mapq, P.mapq, (size_t)total}, n_pri = {P.h_n_pri, P.n_pri, (size_t)nreads * 4},
                   status = {P.h_status, P.status, (size_t)nreads}, ctrs = {ctx->h_ctr, P.counter, 8};
    if ((rc = reg_reserve(ctx, {{P.out, recs.bytes}, {P.n_pri, n_pri.bytes}, {P.mapq, mapq.bytes}, {P.status, status.bytes}, {P.counter, ctrs.bytes}})) ||
        (rc = reg_download_reserve(ctx, {recs, mapq, n_pri, status, ctrs}))) return rc;
    const meme_primary_device_out d = {(meme_alnreg*)P.out.p, (int32_t*)P.n_pri.p, (uint8_t*)P.mapq.p, (uint8_t*)P.status.p, (uint64_t*)P.counter.p};
    if ((rc = primary_launch(ctx, (const meme_alnreg*)P.regs.p, (const i64*)P.reg_off.p, nreads, total, id_base, opt, &d))) return rc;
    float ms = 0.f;
    if ((rc = reg_download(ctx, {recs, mapq, n_pri, status, ctrs})) || (rc = reg_sync_ms(ctx, P.ev, &ms))) return rc;
    out->nreads = nreads; out->total_regs = total; out->regs = (const meme_alnreg*)P.h_regs.p; out->n_pri = (const int32_t*)P.h_n_pri.p; out->mapq = (const uint8_t*)P.h_mapq.p;
    out->status = (const uint8_t*)P.h_status.p; out->n_heavy = (i64)*(const unsigned long long*)ctx->h_ctr.p; out->kernel_ms = ms;
    return MEME_OK;
}
