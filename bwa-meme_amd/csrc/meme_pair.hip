// Pair scoring on the device: mem_pair (reference src/bwamem_pair.cpp:372-433) for every pair of a batch -- the second step of mem_sam_pe, between the two
// the primary stage (meme_primary.hip) runs.  Reads 2p and 2p + 1 of the call are pair p; the first n_pri records of either end take part.
//
// Per pair: a key per record (reference id and forward position within it; score, index, strand, end), the keys ordered by pair64_lt (a strict total order,
// so ranks by counting give the order of the reference's introsort), every key i against the keys k in front of it under the candidate test, a score q per
// candidate, and of the candidates -- never stored -- the two largest under (q, hash, k, i) and two counts: how many there are, and how many besides the best
// lie within tmp of the second's q.  That is all the reference reads of its sorted list u.
//
// Two tiers in one call, by key count (tuning key pair_split, at most PAIR_G):
//   k_pair_light  eight lanes per pair, one key per lane, everything in registers and shuffles within the group
//   k_pair_heavy  a wavefront (one workgroup) per pair for the rest, any count: keys ranked through LDS PAIR_CHUNK at a time, the sorted keys in LDS up to a cap
//                 (tuning key pair_lds_keys) and behind it in a workspace in HBM; lane i walks its k downwards and stops where the distance is beyond every
//                 orientation's reach; the candidates are enumerated twice, for the top two and then for n_sub, which needs sub
// k_pair_route writes every pair's defaults and lists the heavy pairs.  Every loop is bounded by a record count; no kernel waits for another workgroup.
//
// Everything that decides a result is meme_pair_rules.h; this file holds where the keys live and who runs what.
//
// Arithmetic: q is IEEE double with contraction off; its penalty term comes from a table the host's libm fills per call for every distance low .. high of the
// orientations that have not failed (the device's erfc and log are not glibc's): the device adds, compares and truncates.
#include <math.h>
#include <string.h>
#include <string>

#include "meme_common.h"
#include "meme_alnreg_words.h"
#include "meme_pair_rules.h"

#pragma clang fp contract(off)

constexpr int PAIR_G = 8;               // lanes per pair in the light tier = the most keys it takes
constexpr int PAIR_CHUNK = 256;         // keys that pass through LDS at a time while the heavy tier ranks
constexpr int PAIR_LDS_KEYS = 512;      // sorted keys of a pair the heavy tier keeps in LDS (the most; tuning key pair_lds_keys lowers it)
constexpr size_t PAIR_TAB_HEAD = 128;   // bytes in front of the table's doubles: PairDirs
static_assert(sizeof(PairDirs) <= PAIR_TAB_HEAD && sizeof(PairKey) == 16, "PairDirs heads the table; a key is one 16-byte word");

struct PairArgs {
    const meme_alnreg* regs; const i64* reg_off; const int* n_pri; i64 npairs, total_regs;
    const i64* contig_off; int n_contigs; i64 l_pac;
    const PairDirs* dirs; const double* tab; u64 id_base; int tmp, split, lds_keys;
    int *score, *sub, *n_sub, *n_cand, *z; uint8_t* status;
    PairKey* keys; i64* list; unsigned long long* n_heavy;
};

// the two ends of pair p: where their records start and how many take part.  false (status 2): offsets that are no span, or a count that is no part of it
__device__ __forceinline__ bool pair_ends(const PairArgs& A, i64 p, i64* base0, int* n0, i64* base1, int* n1) {
    int span0, span1;
    bool ok = reg_span(A.reg_off, 2 * p, A.total_regs, base0, &span0);
    ok = reg_span(A.reg_off, 2 * p + 1, A.total_regs, base1, &span1) && ok;
    const int c0 = A.n_pri[2 * p], c1 = A.n_pri[2 * p + 1];
    ok = ok && c0 >= 0 && c0 <= span0 && c0 <= PAIR_MAX_PRI && c1 >= 0 && c1 <= span1 && c1 <= PAIR_MAX_PRI;
    *n0 = ok ? c0 : 0; *n1 = ok ? c1 : 0;
    return ok;
}
// keys of the pair: none where an end has no record that takes part (the reference does not call mem_pair there)
__device__ __forceinline__ int pair_keys(int n0, int n1) { return n0 > 0 && n1 > 0 ? n0 + n1 : 0; }
// key j of the pair's unsorted keys: end 0's records, then end 1's.  *ok: the record may take part (the key means nothing otherwise)
__device__ __forceinline__ PairKey pair_key_at(const PairArgs& A, i64 base0, int n0, i64 base1, int j, bool* ok) {
    const int r = j >= n0, i = r ? j - n0 : j;
    const meme_alnreg& R = A.regs[(r ? base1 : base0) + i];
    const i64 rb = R.rb; const int rid = R.rid, score = R.score;
    *ok = pair_record_ok(rid, score, A.n_contigs);
    return pair_key(rb, rid, score, i, r, A.l_pac, *ok ? A.contig_off[rid] : 0);
}
// the candidate (k, i) of two sorted keys, if it is one: its key, the penalty from the table
__device__ __forceinline__ bool pair_cand(const PairArgs& A, const PairDirs& D, PairKey ki, PairKey kk, int k, int i, u64 idx, PairKey* c) {
    i64 dist;
    const int dir = pair_candidate(ki, kk, D, &dist);
    if (dir < 0) return false;
    const double* __restrict__ tab = A.tab;
    const double T = tab[pair_pick64(D.tab_off, dir) + (dist - pair_pick(D.low, dir))];
    *c = pair_cand_key(pair_q(pair_key_score(ki), pair_key_score(kk), T), k, i, idx);
    return true;
}
__device__ __forceinline__ void pair_write(const PairArgs& A, i64 p, int score, int sub, int n_sub, int n_cand, int z0, int z1) {
    A.score[p] = score; A.sub[p] = sub; A.n_sub[p] = n_sub; A.n_cand[p] = n_cand; A.z[2 * p] = z0; A.z[2 * p + 1] = z1;
}
// the result of a pair from the top two, the count and the keys of the best candidate's members (:417-430)
__device__ __forceinline__ void pair_write_top(const PairArgs& A, i64 p, const PairTop& t, int n_sub, PairKey first, PairKey second) {
    int z0 = -1, z1 = -1;                                      // (the two members are of different ends)
    if (t.n) { const bool swap = pair_key_end(first) != 0; z0 = pair_key_index(swap ? second : first); z1 = pair_key_index(swap ? first : second); }
    pair_write(A, p, pair_top_score(t), pair_top_sub(t), n_sub, t.n, z0, z1);
}

// ---- routing --------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pair_route(PairArgs A) {
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < A.npairs; p += (i64)gridDim.x * blockDim.x) {
        i64 base0, base1; int n0, n1;
        A.status[p] = pair_ends(A, p, &base0, &n0, &base1, &n1) ? 0 : 2;
        pair_write(A, p, 0, 0, 0, 0, -1, -1);
        if (pair_keys(n0, n1) > A.split) A.list[atomicAdd(A.n_heavy, 1ull)] = p;      // (at most npairs entries; their order does not matter)
    }
}

// ---- light tier: eight lanes per pair --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pair_group_ballot(bool x) { return (unsigned)(__ballot(x) >> (threadIdx.x & 56)) & 0xffu; }
__device__ __forceinline__ PairKey pair_take(PairKey k, int from) {                 // every lane takes the key of lane `from` of its group
    const PairKey y = {(u64)__shfl((unsigned long long)k.x, from, PAIR_G), (u64)__shfl((unsigned long long)k.y, from, PAIR_G)};
    return y;
}
__device__ __forceinline__ PairTop pair_top_xor(const PairTop& t, int d, int width) {
    PairTop o;
    o.best.x = (u64)__shfl_xor((unsigned long long)t.best.x, d, width); o.best.y = (u64)__shfl_xor((unsigned long long)t.best.y, d, width);
    o.second.x = (u64)__shfl_xor((unsigned long long)t.second.x, d, width); o.second.y = (u64)__shfl_xor((unsigned long long)t.second.y, d, width);
    o.n = __shfl_xor(t.n, d, width);
    return o;
}

__global__ void __launch_bounds__(256) k_pair_light(PairArgs A) {
    const int q = threadIdx.x & (PAIR_G - 1);
    const i64 groups = (i64)gridDim.x * (256 / PAIR_G);
    const PairDirs& D = *A.dirs;                                                    // (the same address for every lane: scalar loads; read through pair_pick only)
    for (i64 p = (i64)blockIdx.x * (256 / PAIR_G) + threadIdx.x / PAIR_G; p < A.npairs; p += groups) {     // (control flow below is uniform within a group: its lanes stay together)
        i64 base0, base1; int n0, n1;
        pair_ends(A, p, &base0, &n0, &base1, &n1);
        const int m = pair_keys(n0, n1);
        if (m == 0 || m > A.split) continue;
        const bool live = q < m;
        PairKey key = {0, 0};
        bool ok = true;
        if (live) key = pair_key_at(A, base0, n0, base1, q, &ok);
        if (pair_group_ballot(live && !ok)) {
            if (q == 0) A.status[p] = 1;
            continue;
        }
        // order by pair64_lt
        int rank = 0;
#pragma unroll
        for (int j = 0; j < PAIR_G; ++j) rank += j < m && pair_lt(pair_take(key, j), key);
        if (!live) rank = q;
        int inv = q;                                                                // the lane whose rank is q (ranks of a group are a permutation of 0..7)
#pragma unroll
        for (int j = 0; j < PAIR_G; ++j) if (__shfl(rank, j, PAIR_G) == q) inv = j;
        key = pair_take(key, inv);
        // key q against the keys in front of it
        const u64 idx = pair_idx(A.id_base + (u64)p);
        PairTop top = pair_top_none();
        PairKey cand[PAIR_G - 1];                                                   // (constant indices below: registers)
        bool is_cand[PAIR_G - 1];
#pragma unroll
        for (int k = 0; k < PAIR_G - 1; ++k) {
            const PairKey kk = pair_take(key, k);
            cand[k].x = cand[k].y = 0;
            is_cand[k] = live && k < q && pair_cand(A, D, key, kk, k, q, idx, &cand[k]);
            if (is_cand[k]) top = pair_top_push(top, cand[k]);
        }
#pragma unroll
        for (int d = PAIR_G / 2; d >= 1; d >>= 1) top = pair_top_merge(top, pair_top_xor(top, d, PAIR_G));
        int n_sub = 0;
#pragma unroll
        for (int k = 0; k < PAIR_G - 1; ++k) n_sub += is_cand[k] && pair_in_n_sub(cand[k], top, A.tmp);
#pragma unroll
        for (int d = PAIR_G / 2; d >= 1; d >>= 1) n_sub += __shfl_xor(n_sub, d, PAIR_G);
        const PairKey first = pair_take(key, top.n ? (int)(top.best.y >> 32) : 0), second = pair_take(key, top.n ? (int)(top.best.y & 0xffffffffu) : 0);
        if (q == 0) pair_write_top(A, p, top, n_sub, first, second);
    }
}

// ---- heavy tier: a wavefront per pair ----------------------------------------------------------------------------------------------------------
// Where sorted key j of a pair lies: the first nc in LDS, the others in the workspace at the place of the record the unsorted key j comes from (end 0's, then end 1's:
// inside the record array's bounds whatever the offsets are)
struct PairSorted {
    PairKey* lds; PairKey* ws; int nc, n0; i64 base0, base1;
    __device__ __forceinline__ PairKey* at(int j) const { return j < nc ? lds + j : ws + (j < n0 ? base0 + j : base1 + (j - n0)); }
    __device__ __forceinline__ PairKey get(int j) const { return *at(j); }
};
// every candidate (k, i), i = lane, lane + 64, ... and k from i - 1 downwards until the distance is beyond every orientation's reach, handed to f
template <class F> __device__ __forceinline__ void pair_walk(const PairArgs& A, const PairDirs& D, const PairSorted& S, int m, i64 reach, u64 idx, F&& f) {
    for (int i = threadIdx.x; i < m; i += 64) {
        const PairKey ki = S.get(i);
        for (int k = i - 1; k >= 0; --k) {
            const PairKey kk = S.get(k);
            if (pair_beyond(ki, kk, reach)) break;
            PairKey c;
            if (pair_cand(A, D, ki, kk, k, i, idx, &c)) f(c);
        }
    }
}

__global__ void __launch_bounds__(64) k_pair_heavy(PairArgs A) {
    __shared__ __attribute__((aligned(16))) PairKey chunk[PAIR_CHUNK];
    __shared__ __attribute__((aligned(16))) PairKey sorted[PAIR_LDS_KEYS];
    const int lane = threadIdx.x;
    const i64 n_heavy = (i64)*A.n_heavy;
    const PairDirs& D = *A.dirs;
    const i64 reach = pair_reach(D);
    for (i64 hi = blockIdx.x; hi < n_heavy; hi += gridDim.x) {                       // (uniform over the workgroup, and so is every branch around a barrier below)
        const i64 p = A.list[hi];
        i64 base0, base1; int n0, n1;
        pair_ends(A, p, &base0, &n0, &base1, &n1);
        const int m = pair_keys(n0, n1);
        int bad = 0;
        for (int j = lane; j < m; j += 64) { bool ok; pair_key_at(A, base0, n0, base1, j, &ok); bad |= !ok; }
        if (__any(bad)) {
            if (lane == 0) A.status[p] = 1;
            continue;
        }
        const PairSorted S = {sorted, A.keys, m < A.lds_keys ? m : A.lds_keys, n0, base0, base1};
        // ranks by counting: 64 keys at a time count against all, which pass through LDS PAIR_CHUNK at a time
        for (int k0 = 0; k0 < m; k0 += 64) {
            const int k = k0 + lane;
            const bool valid = k < m;
            bool ok;
            PairKey key = {0, 0};
            if (valid) key = pair_key_at(A, base0, n0, base1, k, &ok);
            int rank = 0;
            for (int c = 0; c < m; c += PAIR_CHUNK) {
                const int cn = m - c < PAIR_CHUNK ? m - c : PAIR_CHUNK;
                __syncthreads();                                                       // (the chunk before this one has been counted)
                for (int j = lane; j < cn; j += 64) chunk[j] = pair_key_at(A, base0, n0, base1, c + j, &ok);
                __syncthreads();
                if (valid)
                    for (int j = 0; j < cn; ++j) rank += pair_lt(chunk[j], key);
            }
            if (valid) *S.at(rank) = key;
        }
        __syncthreads();
        const u64 idx = pair_idx(A.id_base + (u64)p);
        PairTop top = pair_top_none();
        pair_walk(A, D, S, m, reach, idx, [&](PairKey c) { top = pair_top_push(top, c); });
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) top = pair_top_merge(top, pair_top_xor(top, d, 64));
        int n_sub = 0;
        if (top.n > 1) pair_walk(A, D, S, m, reach, idx, [&](PairKey c) { n_sub += pair_in_n_sub(c, top, A.tmp); });     // (top is the same in every lane)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n_sub += __shfl_xor(n_sub, d);
        if (lane == 0) pair_write_top(A, p, top, n_sub, S.get(top.n ? (int)(top.best.y >> 32) : 0), S.get(top.n ? (int)(top.best.y & 0xffffffffu) : 0));
        __syncthreads();                                                               // (the next pair's keys go where this one's were read)
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------
namespace {

// what both forms check and stage for the kernels: the options, the contigs, the orientations and their penalty table
int pair_prepare(meme_ctx* ctx, const char* who, i64 nreads, const meme_contig* contigs, int32_t n_contigs, i64 l_pac, const meme_pair_pes* pes, const meme_pair_opt* opt,
                 ContigTab* ct) {
    if (nreads & 1) { meme_set_error("%s: %lld reads are no pairs", who, (long long)nreads); return MEME_E_ARG; }
    if (opt->a < 1) { meme_set_error("%s: a must be at least 1", who); return MEME_E_ARG; }
    if (n_contigs < 0 || (n_contigs > 0 && !contigs) || l_pac < 0) { meme_set_error("%s: null contigs or a negative l_pac", who); return MEME_E_ARG; }
    PairDirs D;
    i64 entries = 0;
    for (int d = 0; d < 4; ++d) {
        D.low[d] = pes[d].low; D.high[d] = pes[d].high; D.failed[d] = pes[d].failed ? 1 : 0; D.tab_off[d] = entries;
        if (D.failed[d] || pes[d].high < pes[d].low) continue;
        const i64 n = (i64)pes[d].high - pes[d].low + 1;
        if (n > PAIR_TABLE_MAX) {
            meme_set_error("%s: orientation %d spans %lld distances (low %d, high %d): the penalty table holds at most %lld", who, d, (long long)n, pes[d].low, pes[d].high, (long long)PAIR_TABLE_MAX);
            return MEME_E_ARG;
        }
        entries += n;
    }
    PairWs& P = ctx->pair;
    int rc;
    if ((rc = meme_contigs(ctx, (std::string(who) + ": ").c_str(), contigs, n_contigs, l_pac, ct))) return rc;
    // the table: built per call by the host's libm, copied on the ctx's stream from pinned memory that the copy before it has left
    const size_t bytes = PAIR_TAB_HEAD + (size_t)(entries + 1) * 8;
    HIP_TRY(P.tab_ev.ensure());
    if (P.tab_in_flight) { HIP_TRY(hipEventSynchronize(P.tab_ev[0])); P.tab_in_flight = false; }
    if ((rc = meme_buf_reserve(ctx, P.tab, bytes)) || (rc = meme_hostbuf_reserve(ctx, P.h_tab, bytes))) return rc;
    memset(P.h_tab.p, 0, PAIR_TAB_HEAD);
    memcpy(P.h_tab.p, &D, sizeof(D));
    double* tab = (double*)((unsigned char*)P.h_tab.p + PAIR_TAB_HEAD);
    for (int d = 0; d < 4; ++d) {
        if (D.failed[d]) continue;
        for (i64 dist = pes[d].low; dist <= pes[d].high; ++dist) tab[D.tab_off[d] + (dist - pes[d].low)] = pair_penalty(dist, pes[d].avg, pes[d].std, opt->a);
    }
    tab[entries] = 0.;
    HIP_TRY(hipMemcpyAsync(P.tab.p, P.h_tab.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(P.tab_ev[0], ctx->stream));
    P.tab_in_flight = true;
    return MEME_OK;
}

// the stage's kernels on device arrays, asynchronous on ctx->stream; ev: recorded around them
int pair_launch(meme_ctx* ctx, const meme_alnreg* d_regs, const i64* d_reg_off, const int32_t* d_n_pri, i64 npairs, i64 total_regs, const ContigTab& ct, int32_t n_contigs, i64 l_pac,
                i64 id_base, const meme_pair_opt* opt, const meme_pair_device_out* o) {
    PairWs& P = ctx->pair;
    int rc;
    if ((rc = meme_buf_reserve(ctx, P.keys, (size_t)(total_regs + 1) * sizeof(PairKey))) || (rc = meme_buf_reserve(ctx, P.list, (size_t)(npairs + 1) * 8))) return rc;
    HIP_TRY(P.ev.ensure());
    PairArgs A;
    A.regs = d_regs; A.reg_off = d_reg_off; A.n_pri = d_n_pri; A.npairs = npairs; A.total_regs = total_regs;
    A.contig_off = ct.off; A.n_contigs = n_contigs; A.l_pac = l_pac;
    A.dirs = (const PairDirs*)P.tab.p; A.tab = (const double*)((const unsigned char*)P.tab.p + PAIR_TAB_HEAD); A.id_base = (u64)id_base;
    A.tmp = pair_score_distance(*opt);
    A.split = tune_split(ctx->pair_split, PAIR_G);
    A.lds_keys = tune_at_most(ctx->pair_lds_keys, PAIR_LDS_KEYS);
    A.score = o->d_score; A.sub = o->d_sub; A.n_sub = o->d_n_sub; A.n_cand = o->d_n_cand; A.z = o->d_z; A.status = o->d_status;
    A.keys = (PairKey*)P.keys.p; A.list = (i64*)P.list.p; A.n_heavy = (unsigned long long*)o->d_n_heavy;
    const i64 cap = tune_grid_cap(ctx->pair_blocks);
    HIP_TRY(hipEventRecord(P.ev[0], ctx->stream));
    HIP_TRY(hipMemsetAsync(o->d_n_heavy, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_pair_route, dim3(grid_blocks(npairs, 256, cap)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_pair_light, dim3(grid_blocks(npairs, 256 / PAIR_G, cap)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_pair_heavy, dim3(grid_blocks(npairs, 1, cap)), dim3(64), 0, ctx->stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(P.ev[1], ctx->stream));
    return MEME_OK;
}

}  // namespace

extern "C" int meme_pair_batch_device(meme_ctx* ctx, const meme_alnreg* d_regs, const int64_t* d_reg_off, const int32_t* d_n_pri, int64_t nreads, int64_t total_regs,
                                      const meme_contig* contigs, int32_t n_contigs, int64_t l_pac, const meme_pair_pes* pes, int64_t id_base, const meme_pair_opt* opt,
                                      const meme_pair_device_out* out) {
    static const char* const who = "meme_pair_batch_device";
    const bool outs = out && out->d_n_heavy && (nreads <= 0 || (out->d_score && out->d_sub && out->d_n_sub && out->d_n_cand && out->d_z && out->d_status));
    if (!ctx || !opt || !pes || !outs || nreads < 0 || total_regs < 0 || (nreads > 0 && (!d_reg_off || !d_n_pri)) || (total_regs > 0 && !d_regs)) {
        meme_set_error("%s: null argument", who);
        return MEME_E_ARG;
    }
    if ((uintptr_t)d_regs & 15) { meme_set_error("%s: the record array must be 16-byte aligned", who); return MEME_E_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    ContigTab ct(nullptr, 0);
    int rc;
    if ((rc = pair_prepare(ctx, who, nreads, contigs, n_contigs, l_pac, pes, opt, &ct))) return rc;
    if (nreads == 0) { HIP_TRY(hipMemsetAsync(out->d_n_heavy, 0, 8, ctx->stream)); return MEME_OK; }
    return pair_launch(ctx, d_regs, (const i64*)d_reg_off, d_n_pri, nreads / 2, total_regs, ct, n_contigs, l_pac, id_base, opt, out);
}

extern "C" int meme_pair_batch_host(meme_ctx* ctx, const meme_alnreg* regs, const int64_t* reg_off, const int32_t* n_pri, int64_t nreads, const meme_contig* contigs,
                                    int32_t n_contigs, int64_t l_pac, const meme_pair_pes* pes, int64_t id_base, const meme_pair_opt* opt, meme_pair_host_result* out) {
    static const char* const who = "meme_pair_batch_host";
    if (!ctx || !opt || !pes || !out || nreads < 0 || (nreads > 0 && (!reg_off || !n_pri))) { meme_set_error("%s: null argument", who); return MEME_E_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    ContigTab ct(nullptr, 0);
    int rc;
    if ((rc = pair_prepare(ctx, who, nreads, contigs, n_contigs, l_pac, pes, opt, &ct))) return rc;
    if (nreads == 0) return MEME_OK;
    if ((rc = reg_check_host(who, regs, reg_off, nreads))) return rc;
    for (i64 r = 0; r < nreads; ++r)
        if (n_pri[r] < 0 || n_pri[r] > reg_off[r + 1] - reg_off[r] || n_pri[r] > PAIR_MAX_PRI) {
            meme_set_error("%s: n_pri of read %lld is %d, the read has %lld records", who, (long long)r, n_pri[r], (long long)(reg_off[r + 1] - reg_off[r]));
            return MEME_E_ARG;
        }
    PairWs& P = ctx->pair;
    i64 total;
    if ((rc = reg_upload(ctx, regs, reg_off, nreads, P.regs, P.reg_off, &total))) return rc;
    const i64 npairs = nreads / 2;
    const Download res = {P.h_res, P.res, (size_t)npairs * 6 * 4}, status = {P.h_status, P.status, (size_t)npairs}, ctrs = {ctx->h_ctr, P.counter, 8};
    if ((rc = reg_reserve(ctx, {{P.n_pri, (size_t)nreads * 4}, {P.res, res.bytes}, {P.status, status.bytes}, {P.counter, ctrs.bytes}})) ||
        (rc = reg_download_reserve(ctx, {res, status, ctrs}))) return rc;
    HIP_TRY(hipMemcpyAsync(P.n_pri.p, n_pri, (size_t)nreads * 4, hipMemcpyHostToDevice, ctx->stream));
    int32_t* r = (int32_t*)P.res.p;                            // columns: score, sub, n_sub, n_cand, then z (two a pair)
    const meme_pair_device_out d = {r, r + npairs, r + 2 * npairs, r + 3 * npairs, r + 4 * npairs, (uint8_t*)P.status.p, (uint64_t*)P.counter.p};
    if ((rc = pair_launch(ctx, (const meme_alnreg*)P.regs.p, (const i64*)P.reg_off.p, (const int32_t*)P.n_pri.p, npairs, total, ct, n_contigs, l_pac, id_base, opt, &d))) return rc;
    float ms = 0.f;
    if ((rc = reg_download(ctx, {res, status, ctrs})) || (rc = reg_sync_ms(ctx, P.ev, &ms))) return rc;
    const int32_t* h = (const int32_t*)P.h_res.p;
    out->npairs = npairs; out->score = h; out->sub = h + npairs; out->n_sub = h + 2 * npairs; out->n_cand = h + 3 * npairs; out->z = h + 4 * npairs;
    out->status = (const uint8_t*)P.h_status.p; out->n_heavy = (i64)*(const unsigned long long*)ctx->h_ctr.p; out->kernel_ms = ms;
    return MEME_OK;
}
