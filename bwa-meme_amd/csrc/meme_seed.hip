// Learned-index seeding on MI355X: host side of the C ABI (launch logic, offsets scan, hit gather).
// The search kernel itself lives in meme_seed_kernel.h.
//
// Replaces the per-read loop body of mem_kernel1_core_Learned() (reference src/bwamem.cpp:1249-1394); the
// outputs are the mem_tl records and hit positions its unchanged consumer mem_chain_Learned() reads
// (src/bwamem.cpp:1122-1204): hits of one SMEM in ascending suffix-array order.
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include <utility>

#include "meme_seed_kernel.h"

namespace {

using namespace seedk;

// ---- offsets: two-level exclusive scan over reads -------------------------------------------------------
constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;

__device__ __forceinline__ i64 block_scan_excl(i64 v, i64* total) {
    __shared__ i64 wsum[SCAN_BLOCK / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    i64 x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        i64 y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    i64 off = 0, tot = 0;
    for (int w = 0; w < SCAN_BLOCK / 64; ++w) {
        if (w < wid) off += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();
    *total = tot;
    return off + x - v;
}

// pass 1: per-tile sums of (smem count, hit count)
__global__ void __launch_bounds__(SCAN_BLOCK) k_tile_sums(const int* __restrict__ cnt, const i64* __restrict__ hits, i64 n,
                                                          i64 ntiles, i64* __restrict__ tile_sums) {
  for (i64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    i64 base = tile * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    i64 a = 0, b = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        i64 i = base + k;
        if (i < n) {
            int c = cnt[i];
            a += c < 0 ? 0 : c;
            b += hits[i];
        }
    }
    i64 ta, tb;
    block_scan_excl(a, &ta);
    block_scan_excl(b, &tb);
    if (threadIdx.x == 0) { tile_sums[2 * tile] = ta; tile_sums[2 * tile + 1] = tb; }
  }
}

// pass 2: one block scans the tile sums in place (exclusive); totals to out[0..1]
__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_tiles(i64* __restrict__ tile_sums, i64 ntiles, i64* __restrict__ totals) {
    i64 ca = 0, cb = 0;
    for (i64 base = 0; base < ntiles; base += SCAN_BLOCK) {
        i64 i = base + threadIdx.x;
        i64 a = i < ntiles ? tile_sums[2 * i] : 0, b = i < ntiles ? tile_sums[2 * i + 1] : 0;
        i64 ta, tb;
        i64 ea = block_scan_excl(a, &ta);
        i64 eb = block_scan_excl(b, &tb);
        if (i < ntiles) { tile_sums[2 * i] = ca + ea; tile_sums[2 * i + 1] = cb + eb; }
        ca += ta;
        cb += tb;
    }
    if (threadIdx.x == 0) { totals[0] = ca; totals[1] = cb; }
}

// pass 3: per-read offsets
__global__ void __launch_bounds__(SCAN_BLOCK) k_offsets(const int* __restrict__ cnt, const i64* __restrict__ hits, i64 n,
                                                        i64 ntiles, const i64* __restrict__ tile_sums, i64* __restrict__ smem_off,
                                                        i64* __restrict__ hit_off) {
  for (i64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    i64 base = tile * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    i64 va[SCAN_ITEMS], vb[SCAN_ITEMS], a = 0, b = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        i64 i = base + k;
        va[k] = vb[k] = 0;
        if (i < n) {
            int c = cnt[i];
            va[k] = c < 0 ? 0 : c;
            vb[k] = hits[i];
        }
        a += va[k];
        b += vb[k];
    }
    i64 ta, tb;
    i64 ea = block_scan_excl(a, &ta) + tile_sums[2 * tile];
    i64 eb = block_scan_excl(b, &tb) + tile_sums[2 * tile + 1];
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        i64 i = base + k;
        if (i < n) { smem_off[i] = ea; hit_off[i] = eb; }
        ea += va[k];
        eb += vb[k];
    }
    if (tile == ntiles - 1 && threadIdx.x == SCAN_BLOCK - 1) { smem_off[n] = ea; hit_off[n] = eb; }
  }
}

// ---- compaction + hit gather: one 16-lane group per read --------------------------------------------------
struct TierTable {
    const SlotRec* base[N_TIERS];
    int cap[N_TIERS];
};

__global__ void __launch_bounds__(BLOCK) k_gather(const SaEnt* __restrict__ sa, TierTable tiers, const i64* __restrict__ slot_loc,
                                                   const int* __restrict__ cnt, i64 n, int hits_per_smem,
                                                   const i64* __restrict__ smem_off, const i64* __restrict__ hit_off,
                                                   meme_mem_tl* __restrict__ smems, u64* __restrict__ hits) {
    // one 16-lane group per read, one lane per SMEM: the slot reads, the first-hit lookups and the mem_tl stores of up
    // to 16 SMEMs go out together; hit lists longer than a few entries are copied cooperatively afterwards
    constexpr int GL = 16;
    const int lane = threadIdx.x & 63;
    const int t = lane & (GL - 1);
    const int gbase = lane - t;
    i64 gid = ((i64)blockIdx.x * BLOCK + threadIdx.x) / GL;
    const i64 ngroups = (i64)gridDim.x * BLOCK / GL;
    for (i64 r = gid; r < n; r += ngroups) {
        const int c = cnt[r];
        if (c <= 0) continue;
        const i64 loc = slot_loc[r];
        const int tier = (int)(loc >> 40);
        const SlotRec* sl = tiers.base[tier] + (loc & ((1ll << 40) - 1)) * tiers.cap[tier];
        meme_mem_tl* out = smems + smem_off[r];
        u64* hout = hits + hit_off[r];
        i64 hb0 = 0;                                   // hits before this chunk of SMEMs
        for (int k0 = 0; k0 < c; k0 += GL) {
            const int k = k0 + t;
            const bool act = k < c;
            SlotRec s;
            s.start = s.end = 0; s.sa_start = 0; s.count = 0;
            if (act) s = sl[k];
            i64 h = s.count;
            if (hits_per_smem > 0 && h > hits_per_smem) h = hits_per_smem;
            // exclusive prefix of h over the group's lanes
            i64 incl = h;
#pragma unroll
            for (int d = 1; d < GL; d <<= 1) {
                i64 y = __shfl_up(incl, d, GL);
                if (t >= d) incl += y;
            }
            const i64 hb = hb0 + incl - h;
            u64 first = 0;
            if (act) {
                // an SMEM with one occurrence usually carries the position itself (the search had it in registers)
                first = (s.sa_start & SLOT_POS) ? (u64)(s.sa_start & SLOT_VAL) : sa[s.sa_start].pos;
                meme_mem_tl m;
                m.start = s.start;
                m.end = s.end;
                m.hitbeg = (int32_t)hb;
                m.hitcount = s.count > (i64)INT_MAX ? INT_MAX : (int32_t)s.count;
                m.cache_refpos = first;
                out[k] = m;
                if (h > 0) hout[hb] = first;
                for (i64 i = 1; i < h && i < 4; ++i) hout[hb + i] = sa[s.sa_start + i].pos;
            }
            // long hit lists: all lanes of the group copy them together
            u64 longmask = (__ballot(act && h > 4) >> gbase) & 0xffffull;
            while (longmask) {
                const int src = __ffsll((long long)longmask) - 1;
                longmask &= longmask - 1;
                const i64 lh = __shfl(h, src, GL), lhb = __shfl(hb, src, GL), lsa = __shfl(s.sa_start, src, GL);
                for (i64 i = 4 + t; i < lh; i += GL) hout[lhb + i] = sa[lsa + i].pos;
            }
            hb0 += __shfl(incl, GL - 1, GL);
        }
    }
}

template <int G, int RND>
int launch_k_seed_rounds(hipStream_t stream, const SeedArgs& A, size_t lds, i64 blocks) {
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void*)k_seed<G, RND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_seed<G, RND>), dim3((unsigned)blocks), dim3(BLOCK), lds, stream, A);
    HIP_TRY(hipGetLastError());
    return MEME_OK;
}
template <int G>
int launch_k_seed(hipStream_t stream, const SeedArgs& A, size_t lds, i64 blocks, int rnd) {
    switch (rnd) {
    case SEED_R12: return launch_k_seed_rounds<G, SEED_R12>(stream, A, lds, blocks);
    case SEED_R3: return launch_k_seed_rounds<G, SEED_R3>(stream, A, lds, blocks);
    default: return launch_k_seed_rounds<G, SEED_ALL>(stream, A, lds, blocks);
    }
}

// ---- one seeding call, in phases ----------------------------------------------------------------------------
// What the phases share.
struct SeedRun {
    meme_ctx* ctx;
    const i64* d_read_off; i64 nreads;
    const meme_seed_opt* opt;
    PackGeom geo;
    TierTable tiers = {};              // where every tier that ran keeps its slots (k_gather)
    bool defer = false;                // tier 0 leaves the re-seeding regions of unique SMEMs to k_reseed
    bool split = false;                // tier 0 runs its third round in a k_seed launch of its own (tuning seed_r3_split)
    i64 n_early = -1;                  // reads of the tier-1 launch that ran beside the re-seeding kernels (-1: none did)
    i64 n_todo = 0;                    // reads the last tier left to the next one
    float ms_total = 0.f, ms_reseed = 0.f;
    i64 launches = 0, searches = 0, windows = 0, lane_searches = 0;
    unsigned long long h_early[SEED_CTRS];   // the early tier-1 launch's counters (n_early >= 0), read back together with tier 0's
};

// grids of the helper kernels (packer, scan, gather): tuning key helper_blocks caps them, so that a small batch goes round their loops
i64 helper_grid(const meme_ctx* ctx, i64 blocks) {
    if (ctx->helper_blocks > 0 && blocks > ctx->helper_blocks) blocks = ctx->helper_blocks;
    return blocks < 1 ? 1 : blocks;
}
// workgroups of a kernel that are resident on the device together: the grid of a kernel whose workgroups share the work out evenly and go
// round (more would run as a second, thinner wave of workgroups)
template <typename K>
int resident_grid(const meme_ctx* ctx, K kernel, int threads, i64* blocks) {
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0));
    *blocks = (i64)ctx->n_cus * (per_cu < 1 ? 1 : per_cu);
    return MEME_OK;
}

// pack the reads: 2 bits/base, both strands, N masks (k_pack_reads)
int seed_pack(SeedRun& R, const uint8_t* d_reads, i64 max_len, i64 total_bytes) {
    meme_ctx* ctx = R.ctx;
    // the reference exits on reads longer than LEARNED_MAX_READ_LEN (src/bwamem.cpp:1259-1262): fail loudly, never seed part of a batch
    if (max_len > MAX_READ_LEN) {
        meme_set_error("read of %lld bases exceeds the learned-index limit of %d (LEARNED_MAX_READ_LEN)", (long long)max_len, MAX_READ_LEN);
        return MEME_E_ARG;
    }
    if (max_len < 1) max_len = 1;                                 // longest read as staged by the packing kernel
    PackGeom& geo = R.geo;
    geo.W = (int)((max_len + 31) / 32) + 2;
    geo.MW = (int)((max_len + 63) / 64);
    geo.stride = 2 * geo.W + 2 * geo.MW + 1;
    int rc;
    if ((rc = meme_buf_reserve(ctx, ctx->batch.packed, (size_t)R.nreads * geo.stride * 8))) return rc;
    HIP_TRY(hipEventRecord(ctx->seed.ev[SEED_EV_PACK0], ctx->stream));
    const int rw = pack_chunk_reads(max_len);                      // reads per wavefront and chunk
    const i64 nchunks = (R.nreads + rw - 1) / rw;
    i64 pblocks = (nchunks + 3) / 4, pmax = 0;                     // four wavefronts per workgroup, a chunk each; they go round beyond a full device
    if ((rc = resident_grid(ctx, k_pack_reads, 256, &pmax))) return rc;
    pblocks = helper_grid(ctx, pblocks > pmax ? pmax : pblocks);
    hipLaunchKernelGGL(k_pack_reads, dim3((unsigned)pblocks), dim3(256), 0, ctx->stream, d_reads,
                       R.d_read_off, R.nreads, total_bytes, geo, rw, (u64*)ctx->batch.packed.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->seed.ev[SEED_EV_PACK1], ctx->stream));
    ctx->batch.packed_reads = R.nreads;
    ctx->batch.packed_geom[0] = geo.W; ctx->batch.packed_geom[1] = geo.MW; ctx->batch.packed_geom[2] = geo.stride;
    return MEME_OK;
}

// One k_seed launch of a tier: `n_todo` reads (tier 0: the batch; overflow tiers: the reads named in `pending`), SMEM slots in
// ctx->seed.slots[tier], the reads that overflow THIS tier appended to ctx->seed.ovf[tier & 1], counters in set `cset`.
// `rnd` (SeedRounds): SEED_ALL, or tier 0 in two launches -- SEED_R12, then SEED_R3 over the same reads on the same stream: it appends to the slot rows, the
// overflow list and the counter set of the first (its own read cursor: SEED_CTR_SLOT3), so buffers and counters are set up by the first alone.
int launch_tier(SeedRun& R, int tier, i64 n_todo, const i64* pending, int cset, hipStream_t stream, bool defer, int rnd = SEED_ALL) {
    meme_ctx* ctx = R.ctx;
    // overflow tiers hold a 512-entry SMEM ring per read in LDS: run them 32 lanes per read (8 reads per block)
    int G = tier == 0 ? (int)ctx->group_lanes : 32;
    const int cap = tier == 0 ? (int)ctx->smem_cap : TIER_CAP[tier];
    const int lcap = cap < TIER_LCAP[tier] ? cap : TIER_LCAP[tier];
    DevBuf& sb = ctx->seed.slots[tier];
    DevBuf& ob = ctx->seed.ovf[tier & 1];
    const size_t need = (size_t)n_todo * cap * sizeof(SlotRec);
    if (tier > 0 && need > sb.cap) {
        // overflow tiers re-run the reads that emitted more SMEMs than their slots hold, with 32 x more slots each:
        // refuse instead of exhausting the HBM the index lives in
        size_t free_b = 0;
        if (!meme_fits_free_hbm(need, 0, &free_b)) {
            meme_set_error("%lld reads emitted more than %d SMEMs each: re-running them needs %.1f GB of slots, more than half of the "
                           "free HBM (%.1f GB); seed this batch in smaller pieces", (long long)n_todo, R.tiers.cap[tier - 1],
                           need / 1e9, free_b / 1e9);
            return MEME_E_CAPACITY;
        }
    }
    int rc;
    unsigned long long* counters = ctx->seed.counter_set(cset);
    if (rnd != SEED_R3) {
        if ((rc = meme_buf_reserve(ctx, sb, need))) return rc;
        if ((rc = meme_buf_reserve(ctx, ob, (size_t)n_todo * sizeof(i64)))) return rc;
        HIP_TRY(hipMemsetAsync(counters, 0, SEED_CTRS * sizeof(unsigned long long), stream));
    }
    SeedArgs A;
    A.I = ctx->idx;
    A.packed = (const u64*)ctx->batch.packed.p;
    A.read_off = R.d_read_off;
    A.nreads = n_todo;
    A.geo = R.geo;
    A.opt = *R.opt;
    A.slots = (SlotRec*)sb.p;
    A.slot_cnt = (int*)ctx->seed.slot_cnt.p;
    A.slot_hits = (i64*)ctx->seed.slot_hits.p;
    A.slot_loc = (i64*)ctx->seed.slot_loc.p;
    A.pending = pending;
    A.ovf_list = (i64*)ob.p;
    A.cap = cap;
    A.lcap = lcap;
    A.tier = tier;
    A.counters = counters;
    A.defer = defer ? 1 : 0;
    A.carry = rnd == SEED_ALL ? nullptr : (u64*)ctx->seed.carry.p;
    A.r3cap = (rnd == SEED_R3 && SEED_R3_CAP && R.opt->min_seed_len + 1 <= 32) ? 1 : 0;   // (msl of the third round; above 32 the keys decide no level)
    R.tiers.base[tier] = (const SlotRec*)sb.p;
    R.tiers.cap[tier] = cap;
    const bool r3 = rnd == SEED_R3;                                                      // (stages the forward words and mask only, keeps no ring)
    while (G < 32 && seed_lds_bytes(G, R.geo, lcap, r3) > (size_t)160 * 1024) G *= 2;   // long reads: fewer reads per workgroup
    const int groups = BLOCK / G;
    size_t lds = seed_lds_bytes(G, R.geo, lcap, r3);
    i64 want = (n_todo + groups - 1) / groups;
    i64 blocks = ctx->seed_blocks > 0 ? ctx->seed_blocks : (i64)ctx->n_cus * ctx->seed_blocks_per_cu;
    if (blocks > want) blocks = want;
    if (blocks < 1) blocks = 1;
    if (tier == 0 && rnd != SEED_R3) HIP_TRY(hipEventRecord(ctx->seed.ev[SEED_EV_SEARCH0], stream));   // (the stage's events span both launches)
    switch (G) {
    case 1: return launch_k_seed<1>(stream, A, lds, blocks, rnd);
    case 2: return launch_k_seed<2>(stream, A, lds, blocks, rnd);
    case 4: return launch_k_seed<4>(stream, A, lds, blocks, rnd);
    case 8: return launch_k_seed<8>(stream, A, lds, blocks, rnd);
    case 16: return launch_k_seed<16>(stream, A, lds, blocks, rnd);
    case 32: return launch_k_seed<32>(stream, A, lds, blocks, rnd);
    default: meme_set_error("group_lanes must be 1, 2, 4, 8, 16 or 32"); return MEME_E_ARG;
    }
}

// the counters a tier's launch left, on the host (waits for ctx->stream); then its share of the call's tallies.  `nsets` = 2: both sets (they
// are contiguous) in one copy and one wait, h[SEED_CTRS..] = set cset + 1
int fetch_counters(SeedRun& R, int cset, unsigned long long* h, int nsets = 1) {
    HIP_TRY(hipMemcpyAsync(h, R.ctx->seed.counter_set(cset), (size_t)nsets * SEED_CTRS * sizeof(unsigned long long), hipMemcpyDeviceToHost, R.ctx->stream));
    HIP_TRY(hipStreamSynchronize(R.ctx->stream));
    return MEME_OK;
}
void tally(SeedRun& R, const unsigned long long* h) {
    ++R.launches;
    R.searches += (i64)h[SEED_CTR_SEARCHES];
    R.windows += (i64)h[SEED_CTR_WINDOWS];
    R.n_todo = (i64)h[SEED_CTR_OVERFLOW];
#ifdef SEED_PROF
    {
        double tot = 0; for (int k = 0; k < 8; ++k) tot += (double)h[SEED_CTR_PROF + k];
        fprintf(stderr, "[seed prof]:");
        const char* nm[6] = {"control", "request+rmi", "window+compare", "resolve", "level", "apply"};
        for (int k = 0; k < 6; ++k) fprintf(stderr, " %s %.1f%%", nm[k], 100.0 * (double)h[SEED_CTR_PROF + k] / (tot > 0 ? tot : 1));
        fprintf(stderr, "\n");
    }
#endif
}

// The re-seeding kernels behind tier 0's k_seed: k_reseed (a walk on the plcp table, one lane per read), then the pending intervals on a stream of
// their own beside the rounds over the blocked regions.
// Batch searches before the last pass searches for itself, and whether k_reseed_emit runs beside the rounds or behind them: compile-time
// constants, re-measured whenever the searches change (profiles/reseed_early_stop.md §6; named configuration: with 4 rounds the last pass
// still does 0.23 M one-by-one searches, the fifth batch takes 0.13 ms off the series, a sixth gives it back in launches; behind the
// rounds k_reseed_emit adds 0.3 ms to the series).
#ifndef RESEED_ROUNDS
#define RESEED_ROUNDS 5
#endif
#ifndef RESEED_EMIT_BESIDE
#define RESEED_EMIT_BESIDE 1
#endif
int launch_reseed(SeedRun& R) {
    meme_ctx* ctx = R.ctx;
    SeedWs& S = ctx->seed;
    const i64 nreads = R.nreads;
    HIP_TRY(hipEventRecord(S.ev[SEED_EV_RESEED0], ctx->stream));
    ReseedArgs A;
    A.I = ctx->idx; A.packed = (const u64*)ctx->batch.packed.p; A.geo = R.geo; A.nreads = nreads; A.opt = *R.opt;
    A.slots = (SlotRec*)S.slots[0].p; A.cap = (int)ctx->smem_cap; A.slot_cnt = (int*)S.slot_cnt.p; A.slot_hits = (i64*)S.slot_hits.p;
    A.ovf_list = (i64*)S.ovf[0].p; A.counters = S.counter_set(0); A.pend_list = (i64*)S.pend.p;
    A.blk = (BlkRec*)S.blk.p; A.blk_out = A.blk + nreads * BLK_PER_READ; A.blk_cap = nreads * BLK_PER_READ;
    A.blk_ctr = SEED_CTR_BLK; A.blk_out_ctr = SEED_CTR_BLK_OUT;
    A.read_off = R.d_read_off; A.round = 0;
    i64 rblocks = (nreads + 255) / 256;
    if (rblocks > (i64)ctx->n_cus * 32) rblocks = (i64)ctx->n_cus * 32;
    hipLaunchKernelGGL(k_reseed, dim3((unsigned)rblocks), dim3(256), 0, ctx->stream, A);
    HIP_TRY(hipEventRecord(ctx->side.fork[0], ctx->stream));     // (the early overflow launch starts here)
    // the batch searches (list sizes stay on the device: fixed grids, grid-stride loops), then the blocked regions' passes
    const unsigned sblocks = (unsigned)(rblocks < (i64)ctx->n_cus * 4 ? rblocks : (i64)ctx->n_cus * 4);
    // the pending intervals on a stream of their own, beside the blocked regions' rounds (both are latency-bound lane-per-item
    // kernels; they touch different slots of the reads they share)
    if (!S.emit.s) HIP_TRY(hipStreamCreateWithFlags(&S.emit.s, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) if (!S.emit_ev[i]) HIP_TRY(hipEventCreateWithFlags(&S.emit_ev[i], hipEventDisableTiming));
    if (RESEED_EMIT_BESIDE) {
        HIP_TRY(hipEventRecord(S.emit_ev[0], ctx->stream));
        HIP_TRY(hipStreamWaitEvent(S.emit, S.emit_ev[0], 0));
        hipLaunchKernelGGL(k_reseed_emit, dim3(sblocks), dim3(256), 0, S.emit, A);
        HIP_TRY(hipEventRecord(S.emit_ev[1], S.emit));
    }
    constexpr int ROUNDS = RESEED_ROUNDS;
    static_assert(ROUNDS >= 1 && ROUNDS <= RESEED_MAX_ROUNDS, "one counter per round");
    S.reseed_rounds = ROUNDS;
    for (int round = 0; round < ROUNDS; ++round) {     // blocked regions ping-pong between two lists; the last pass searches for itself
        A.round = round;
        hipLaunchKernelGGL(k_reseed_search, dim3(sblocks), dim3(256), 0, ctx->stream, A);
        if (round < ROUNDS - 1) {
            hipLaunchKernelGGL(k_reseed_resume<false>, dim3(sblocks), dim3(256), 0, ctx->stream, A);
            HIP_TRY(hipMemsetAsync(S.counter_set(0) + A.blk_ctr, 0, sizeof(unsigned long long), ctx->stream));
            std::swap(A.blk, A.blk_out); std::swap(A.blk_ctr, A.blk_out_ctr);
        } else hipLaunchKernelGGL(k_reseed_resume<true>, dim3(sblocks), dim3(256), 0, ctx->stream, A);
    }
    if (!RESEED_EMIT_BESIDE) {
        hipLaunchKernelGGL(k_reseed_emit, dim3(sblocks), dim3(256), 0, ctx->stream, A);
        HIP_TRY(hipEventRecord(S.emit_ev[1], ctx->stream));
    }
    HIP_TRY(hipGetLastError());
    return MEME_OK;
}

// The reads that overflowed their slots in k_seed or in k_reseed's pass are known once k_reseed has finished -- the only re-seeding
// kernel that looks at every read; the ones behind it work from lists of reads that did NOT overflow.  Their tier-1 launch (a few
// homopolymer reads of thousands of SMEMs each: 2.5 ms at the named configuration however few they are) runs beside the batches
// of searches instead of behind them.  Reads that overflow later (appended by a resume pass: rare) get a second launch in seed_overflow_tiers.
int launch_early_overflow(SeedRun& R) {
    meme_ctx* ctx = R.ctx;
    Stream& side = ctx->side.st[0];
    unsigned long long h_ovf = 0;
    HIP_TRY(hipStreamWaitEvent(side, ctx->side.fork[0], 0));
    HIP_TRY(hipMemcpyAsync(&h_ovf, ctx->seed.counter_set(0) + SEED_CTR_OVERFLOW, 8, hipMemcpyDeviceToHost, side));
    HIP_TRY(hipStreamSynchronize(side));
    if (h_ovf == 0) return MEME_OK;
    R.n_early = (i64)h_ovf;
    int rc;
    if ((rc = launch_tier(R, 1, R.n_early, (const i64*)ctx->seed.ovf[0].p, 1, side, false))) return rc;
    HIP_TRY(hipEventRecord(ctx->side.done[0], side));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->side.done[0], 0));
    return MEME_OK;
}

// tier 0: the whole batch.  It leaves the re-seeding regions of unique SMEMs to k_reseed and the batches of searches behind it; the overflow
// tiers search everything themselves.
int seed_tier0(SeedRun& R) {
    meme_ctx* ctx = R.ctx;
    SeedWs& S = ctx->seed;
    int rc;
    R.defer = ctx->seed_defer != 0 && ctx->idx.plcp != nullptr && R.opt->rounds >= 2;
    S.reseed_rounds = 0;
    if (R.defer && (rc = meme_buf_reserve(ctx, S.pend, (size_t)R.nreads * sizeof(i64)))) return rc;
    if (R.defer && (rc = meme_buf_reserve(ctx, S.blk, (size_t)R.nreads * BLK_PER_READ * 2 * sizeof(BlkRec)))) return rc;
    // Three rounds: rounds 1-2, then the third round in a launch of its own over the same reads, then the re-seeding kernels -- a read's slots stay in today's
    // order (first round, third round, re-seeding).  The second launch leaves alone what the first sent to the overflow list and sends there what overflows now.
    R.split = ctx->seed_r3_split != 0 && R.opt->rounds >= 3 && R.opt->max_mem_intv > 0;
    if (R.split) {
        if ((rc = meme_buf_reserve(ctx, S.carry, (size_t)R.nreads * sizeof(u64)))) return rc;
        if ((rc = launch_tier(R, 0, R.nreads, nullptr, 0, ctx->stream, R.defer, SEED_R12))) return rc;
        if ((rc = launch_tier(R, 0, R.nreads, nullptr, 0, ctx->stream, R.defer, SEED_R3))) return rc;
    } else if ((rc = launch_tier(R, 0, R.nreads, nullptr, 0, ctx->stream, R.defer))) return rc;
    if (R.defer) {
        if ((rc = meme_side_stream(ctx, 0)) || (rc = launch_reseed(R)) || (rc = launch_early_overflow(R))) return rc;
        HIP_TRY(hipStreamWaitEvent(ctx->stream, S.emit_ev[1], 0));
    }
    HIP_TRY(hipEventRecord(S.ev[SEED_EV_SEARCH1], ctx->stream));
    // (ctx->stream waits for the early tier-1 launch above: its counter set is final too, and is read in the same copy)
    unsigned long long h[2 * SEED_CTRS];
    if ((rc = fetch_counters(R, 0, h, R.n_early >= 0 ? 2 : 1))) return rc;
    if (R.n_early >= 0) memcpy(R.h_early, h + SEED_CTRS, sizeof(R.h_early));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, S.ev[SEED_EV_SEARCH0], S.ev[SEED_EV_SEARCH1]));
    R.ms_total += ms;
    if (R.defer) {
        float a = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, S.ev[SEED_EV_RESEED0], S.ev[SEED_EV_SEARCH1]));
        R.ms_reseed += a;
        R.lane_searches += (i64)h[SEED_CTR_LANE];
        for (int k = SEED_CTR_RS_ROUND; k < SEED_CTRS; ++k) S.reseed_counts[k - SEED_CTR_RS_ROUND] = (long long)h[k];
#ifdef RESEED_PROF
        {
            // the census of the blocked regions' lane searches: single-entry probes by kind and the region's stage
            const unsigned long long* c = h + SEED_CTR_PROF;
            fprintf(stderr, "[reseed prof] lists per round:");
            for (int k = 0; k < S.reseed_rounds; ++k) fprintf(stderr, " %llu", h[SEED_CTR_RS_ROUND + k]);
            fprintf(stderr, "\n[reseed prof] stage searches partition_probes run_probes\n");
            for (int k = 0; k < 3; ++k) fprintf(stderr, "[reseed prof] %d %llu %llu %llu\n", k, h[SEED_CTR_RS_STAGE + k], c[k], c[3 + k]);
            fprintf(stderr, "[reseed prof] interval read %llu, without interval %llu, walked %llu, neighbour probes %llu, last-pass searches %llu\n", c[6],
                    h[SEED_CTR_RS_NOINTV], h[SEED_CTR_RS_WALKED], h[SEED_CTR_RS_NBPROBE], h[SEED_CTR_LANE]);
        }
#endif
        if (getenv("MEME_SEED_TRACE")) fprintf(stderr, "[meme] seed tier 0: search kernel + re-seeding kernels %.2f ms, of which behind k_seed %.2f ms (%lld lane searches; %lld reads of the "
                                               "overflow tier beside them)\n", ms, a, (long long)h[SEED_CTR_LANE], (long long)(R.n_early < 0 ? 0 : R.n_early));
    }
    S.r3_counts[0] = R.split ? 1 : 0;
    S.r3_counts[1] = (long long)h[SEED_CTR_R3_REPEAT];
    tally(R, h);
    return MEME_OK;
}

// overflow tiers: reads that produced more SMEMs than their slots hold (pathological repeats) are re-run alone
int seed_overflow_tiers(SeedRun& R) {
    meme_ctx* ctx = R.ctx;
    SeedWs& S = ctx->seed;
    int rc;
    unsigned long long h[SEED_CTRS];
    for (int tier = 1; R.n_todo > 0; ++tier) {
        if (tier >= N_TIERS) {
            meme_set_error("a read produced more than %d SMEMs", TIER_CAP[N_TIERS - 1]);
            return MEME_E_CAPACITY;
        }
        const int cset = tier & 1;
        if (tier == 1 && R.n_early == R.n_todo) {
            // the launch beside the re-seeding kernels took them all: its counters came with tier 0's
            memcpy(h, R.h_early, sizeof(h));
        } else {
            // (tier 1 after an early launch that did not see every overflowed read: all of them again -- rare, and simple)
            HIP_TRY(hipEventRecord(S.ev[SEED_EV_SEARCH0], ctx->stream));
            if ((rc = launch_tier(R, tier, R.n_todo, (const i64*)S.ovf[(tier - 1) & 1].p, cset, ctx->stream, false))) return rc;
            HIP_TRY(hipEventRecord(S.ev[SEED_EV_SEARCH1], ctx->stream));
            if ((rc = fetch_counters(R, cset, h))) return rc;
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, S.ev[SEED_EV_SEARCH0], S.ev[SEED_EV_SEARCH1]));
            R.ms_total += ms;
        }
        tally(R, h);
    }
    return MEME_OK;
}

// per-read offsets of the SMEMs and hits (a two-level scan), then the gather of every tier's slots into the batch's packed arrays
int seed_gather(SeedRun& R, meme_seed_result* out) {
    meme_ctx* ctx = R.ctx;
    SeedWs& S = ctx->seed;
    ResidentBatch& B = ctx->batch;
    const i64 nreads = R.nreads;
    int rc;
    i64 ntiles = (nreads + SCAN_TILE - 1) / SCAN_TILE;
    if ((rc = meme_buf_reserve(ctx, ctx->scan_tmp, (size_t)(2 * ntiles + 2) * sizeof(i64)))) return rc;
    if ((rc = meme_buf_reserve(ctx, B.smem_off, (size_t)(nreads + 1) * sizeof(i64)))) return rc;
    if ((rc = meme_buf_reserve(ctx, B.hit_off, (size_t)(nreads + 1) * sizeof(i64)))) return rc;
    i64* tiles = (i64*)ctx->scan_tmp.p;
    i64* totals = tiles + 2 * ntiles;
    HIP_TRY(hipEventRecord(S.ev[SEED_EV_GATHER0], ctx->stream));
    const i64 sblocks = helper_grid(ctx, ntiles);                  // a tile per workgroup unless helper_blocks says fewer
    hipLaunchKernelGGL(k_tile_sums, dim3((unsigned)sblocks), dim3(SCAN_BLOCK), 0, ctx->stream, (const int*)S.slot_cnt.p,
                       (const i64*)S.slot_hits.p, nreads, ntiles, tiles);
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(SCAN_BLOCK), 0, ctx->stream, tiles, ntiles, totals);
    hipLaunchKernelGGL(k_offsets, dim3((unsigned)sblocks), dim3(SCAN_BLOCK), 0, ctx->stream, (const int*)S.slot_cnt.p,
                       (const i64*)S.slot_hits.p, nreads, ntiles, (const i64*)tiles, (i64*)B.smem_off.p, (i64*)B.hit_off.p);
    HIP_TRY(hipGetLastError());
    i64 h_tot[2];
    HIP_TRY(hipMemcpyAsync(h_tot, totals, sizeof(h_tot), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if ((rc = meme_buf_reserve(ctx, B.smems, (size_t)(h_tot[0] + 1) * sizeof(meme_mem_tl)))) return rc;
    if ((rc = meme_buf_reserve(ctx, B.hits, (size_t)(h_tot[1] + 1) * sizeof(u64)))) return rc;
    i64 gblocks = (nreads + 15) / 16;
    if (gblocks > (i64)ctx->n_cus * 8) gblocks = (i64)ctx->n_cus * 8;
    gblocks = helper_grid(ctx, gblocks);
    hipLaunchKernelGGL(k_gather, dim3((unsigned)gblocks), dim3(BLOCK), 0, ctx->stream, ctx->idx.sa, R.tiers,
                       (const i64*)S.slot_loc.p, (const int*)S.slot_cnt.p, nreads, R.opt->hits_per_smem,
                       (const i64*)B.smem_off.p, (const i64*)B.hit_off.p, (meme_mem_tl*)B.smems.p, (u64*)B.hits.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S.ev[SEED_EV_GATHER1], ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipEventElapsedTime(&ctx->tm.seed_gather_ms, S.ev[SEED_EV_GATHER0], S.ev[SEED_EV_GATHER1]));
    out->d_smems = (const meme_mem_tl*)B.smems.p;
    out->d_smem_off = (const i64*)B.smem_off.p;
    out->d_hits = (const u64*)B.hits.p;
    out->d_hit_off = (const i64*)B.hit_off.p;
    out->total_smems = h_tot[0];
    out->total_hits = h_tot[1];
    out->searches = R.searches;
    return MEME_OK;
}

int launch_seed(meme_ctx* ctx, const uint8_t* d_reads, const i64* d_read_off, i64 nreads, i64 max_len, i64 total_bytes,
                const meme_seed_opt* opt, meme_seed_result* out) {
    int rc;
    SeedWs& S = ctx->seed;
    ctx->batch.last_seed_reads = 0;          // whatever batch meme_chain_last_batch_host could have chained is being overwritten
    ctx->sam_text_reads = 0;           // ... and the names / qualities staged for it belong to the previous batch
    if ((rc = meme_buf_reserve(ctx, S.slot_cnt, (size_t)nreads * sizeof(int)))) return rc;
    if ((rc = meme_buf_reserve(ctx, S.slot_hits, (size_t)nreads * sizeof(i64)))) return rc;
    if ((rc = meme_buf_reserve(ctx, S.slot_loc, (size_t)nreads * sizeof(i64)))) return rc;
    if ((rc = meme_buf_reserve(ctx, S.counters, 2 * SEED_CTRS * sizeof(unsigned long long)))) return rc;
    HIP_TRY(S.ev.ensure());
    SeedRun R;
    R.ctx = ctx; R.d_read_off = d_read_off; R.nreads = nreads; R.opt = opt;
    if ((rc = seed_pack(R, d_reads, max_len, total_bytes)) || (rc = seed_tier0(R)) || (rc = seed_overflow_tiers(R))) return rc;
    HIP_TRY(hipEventElapsedTime(&ctx->tm.seed_pack_ms, S.ev[SEED_EV_PACK0], S.ev[SEED_EV_PACK1]));
    ctx->tm.seed_kernel_ms = R.ms_total;
    ctx->tm.seed_launches = R.launches;
    ctx->tm.seed_windows = R.windows;
    ctx->tm.seed_reseed_ms = R.ms_reseed;
    ctx->tm.seed_lane_searches = R.lane_searches;
    S.r3_valid = true;
    return seed_gather(R, out);
}

// longest read of the batch (sizes the packed layout and the LDS tile)
__global__ void __launch_bounds__(256) k_max_len(const i64* __restrict__ off, i64 n, int* out) {
    __shared__ int wmax[4];
    int v = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        int l = (int)(off[i + 1] - off[i]);
        v = v > l ? v : l;
    }
    for (int d = 32; d >= 1; d >>= 1) { int y = __shfl_xor(v, d); v = v > y ? v : y; }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) v = v > wmax[k] ? v : wmax[k];
        atomicMax(out, v);
    }
}

int device_max_len(meme_ctx* ctx, const i64* d_read_off, i64 nreads, i64* max_len) {
    int rc;
    if ((rc = meme_buf_reserve(ctx, ctx->scan_tmp, 64))) return rc;
    HIP_TRY(hipMemsetAsync(ctx->scan_tmp.p, 0, 4, ctx->stream));
    i64 mblocks = (nreads + 255) / 256;
    if (mblocks > 1024) mblocks = 1024;
    hipLaunchKernelGGL(k_max_len, dim3((unsigned)mblocks), dim3(256), 0, ctx->stream, d_read_off, nreads,
                       (int*)ctx->scan_tmp.p);
    int v = 0;
    HIP_TRY(hipMemcpyAsync(&v, ctx->scan_tmp.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *max_len = v;
    return MEME_OK;
}

int check_opt(const meme_seed_opt* opt) {
    if (!opt || opt->min_seed_len < 1 || opt->rounds < 1 || opt->rounds > 3 || opt->hits_per_smem < 0) {
        meme_set_error("bad meme_seed_opt");
        return MEME_E_ARG;
    }
    return MEME_OK;
}

}  // namespace

extern "C" int meme_seed_batch_device(meme_ctx* ctx, const uint8_t* d_reads, const int64_t* d_read_off, int64_t nreads,
                                      int64_t total_bases, const meme_seed_opt* opt, meme_seed_result* out) {
    if (!ctx || !d_reads || !d_read_off || !out || nreads < 0) return MEME_E_ARG;
    int rc = check_opt(opt);
    if (rc) return rc;
    if (!ctx->idx.sa) { meme_set_error("meme_seed_batch: no index loaded"); return MEME_E_STATE; }
    HIP_TRY(hipSetDevice(ctx->device));
    if (nreads == 0) { memset(out, 0, sizeof(*out)); return MEME_OK; }
    i64 max_len = 0;
    if ((rc = device_max_len(ctx, (const i64*)d_read_off, nreads, &max_len))) return rc;
    return launch_seed(ctx, d_reads, (const i64*)d_read_off, nreads, max_len, total_bases, opt, out);
}

extern "C" int meme_seed_batch(meme_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t nreads,
                               const meme_seed_opt* opt, meme_mem_tl* smems, int64_t smem_capacity, int64_t* smem_off,
                               uint64_t* hits, int64_t hit_capacity, int64_t* hit_off, int64_t* total_smems,
                               int64_t* total_hits) {
    if (!ctx || !reads || !read_off || !smems || !smem_off || !hits || !hit_off || nreads < 0) return MEME_E_ARG;
    int rc = check_opt(opt);
    if (rc) return rc;
    if (!ctx->idx.sa) { meme_set_error("meme_seed_batch: no index loaded"); return MEME_E_STATE; }
    HIP_TRY(hipSetDevice(ctx->device));
    if (nreads == 0) { smem_off[0] = 0; hit_off[0] = 0; if (total_smems) *total_smems = 0; if (total_hits) *total_hits = 0; return MEME_OK; }
    const i64 bases = read_off[nreads] - read_off[0];
    if (read_off[0] != 0) { meme_set_error("read_off[0] must be 0"); return MEME_E_ARG; }
    if ((rc = meme_buf_reserve(ctx, ctx->batch.reads, (size_t)bases + 16))) return rc;
    if ((rc = meme_buf_reserve(ctx, ctx->batch.read_off, (size_t)(nreads + 1) * sizeof(i64)))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->batch.reads.p, reads, (size_t)bases, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->batch.read_off.p, read_off, (size_t)(nreads + 1) * sizeof(i64), hipMemcpyHostToDevice, ctx->stream));
    meme_seed_result res;
    i64 max_len = 0;
    for (i64 i = 0; i < nreads; ++i) max_len = read_off[i + 1] - read_off[i] > max_len ? read_off[i + 1] - read_off[i] : max_len;
    rc = launch_seed(ctx, (const uint8_t*)ctx->batch.reads.p, (const i64*)ctx->batch.read_off.p, nreads, max_len, bases, opt, &res);
    if (rc) return rc;
    if (total_smems) *total_smems = res.total_smems;
    if (total_hits) *total_hits = res.total_hits;
    HIP_TRY(hipMemcpyAsync(smem_off, res.d_smem_off, (size_t)(nreads + 1) * sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(hit_off, res.d_hit_off, (size_t)(nreads + 1) * sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
    if (res.total_smems > smem_capacity || res.total_hits > hit_capacity) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        meme_set_error("output buffers too small: need %lld SMEMs and %lld hits", (long long)res.total_smems,
                       (long long)res.total_hits);
        return MEME_E_CAPACITY;
    }
    HIP_TRY(hipMemcpyAsync(smems, res.d_smems, (size_t)res.total_smems * sizeof(meme_mem_tl), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(hits, res.d_hits, (size_t)res.total_hits * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEME_OK;
}

extern "C" int meme_debug_packed_reads(meme_ctx* ctx, uint64_t* out, int64_t capacity_words, int32_t* geom, int64_t* nreads) {
    if (!ctx || !geom || !nreads) return MEME_E_ARG;
    const ResidentBatch& B = ctx->batch;
    if (B.packed_reads <= 0 || !B.packed.p) { meme_set_error("meme_debug_packed_reads: no batch was packed on this ctx"); return MEME_E_STATE; }
    for (int k = 0; k < 3; ++k) geom[k] = B.packed_geom[k];
    *nreads = B.packed_reads;
    if (!out) return MEME_OK;
    const i64 words = B.packed_reads * B.packed_geom[2];
    if (capacity_words < words) { meme_set_error("meme_debug_packed_reads: %lld words needed", (long long)words); return MEME_E_CAPACITY; }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out, B.packed.p, (size_t)words * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEME_OK;
}

extern "C" int meme_debug_reseed_counts(meme_ctx* ctx, int64_t* out, int32_t capacity, int32_t* rounds) {
    if (!ctx || !out || !rounds) return MEME_E_ARG;
    const SeedWs& S = ctx->seed;
    if (S.reseed_rounds <= 0) { meme_set_error("meme_debug_reseed_counts: the last seeding call on this ctx ran no re-seeding kernels"); return MEME_E_STATE; }
    if (capacity < MEME_RESEED_COUNTS) { meme_set_error("meme_debug_reseed_counts: %d values needed", MEME_RESEED_COUNTS); return MEME_E_CAPACITY; }
    static_assert(MEME_RESEED_COUNTS == RESEED_MAX_ROUNDS + 6 && SEED_CTR_RS_NBPROBE - SEED_CTR_RS_ROUND + 1 == MEME_RESEED_COUNTS, "layout of meme_hip.h");
    for (int k = 0; k < MEME_RESEED_COUNTS; ++k) out[k] = S.reseed_counts[k];
    *rounds = S.reseed_rounds;
    return MEME_OK;
}

extern "C" int meme_debug_seed_r3_counts(meme_ctx* ctx, int64_t* out, int32_t capacity) {
    if (!ctx || !out) return MEME_E_ARG;
    const SeedWs& S = ctx->seed;
    if (!S.r3_valid) { meme_set_error("meme_debug_seed_r3_counts: no seeding call on this ctx yet"); return MEME_E_STATE; }
    if (capacity < MEME_R3_COUNTS) { meme_set_error("meme_debug_seed_r3_counts: %d values needed", MEME_R3_COUNTS); return MEME_E_CAPACITY; }
    for (int k = 0; k < MEME_R3_COUNTS; ++k) out[k] = S.r3_counts[k];
    return MEME_OK;
}

// Host-pointer variant whose results land in pinned buffers owned by the ctx (valid until the next seeding call on it):
// no capacity negotiation, and the device-to-host copies are plain DMA transfers.  `reads` / `read_off` may be pageable or
// pinned (meme_host_alloc).  This is the call a chunk-level binding issues once per -K chunk.
// Workspaces and pinned result buffers of a meme_seed_batch_host() + meme_chain_last_batch_host() call of this size, ahead of
// time: pinned host memory takes ~0.4 s per GB to allocate, which a caller can hide behind its index load.  Sizes are estimates
// (12 SMEMs, 24 hits, 3 chains, 6 chained seeds per read); whatever turns out larger grows on first use as before.
extern "C" int meme_seed_reserve(meme_ctx* ctx, int64_t nreads, int64_t total_bases) {
    if (!ctx || nreads < 0 || total_bases < 0) return MEME_E_ARG;
    if (nreads == 0) return MEME_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = (size_t)nreads;
    const i64 len = total_bases / nreads + 32;
    const size_t stride = (size_t)(2 * ((len + 31) / 32 + 2) + 2 * ((len + 63) / 64) + 1);
    int rc;
    ResidentBatch& B = ctx->batch; SeedWs& S = ctx->seed;
    ChainWs& C = ctx->chain; ExtWs& E = ctx->ext;
    struct { DevBuf* b; size_t bytes; } dev[] = {
        {&B.reads, (size_t)total_bases + 16}, {&B.read_off, (n + 1) * 8}, {&S.slot_cnt, n * 4}, {&S.slot_hits, n * 8},
        {&S.slot_loc, n * 8}, {&S.carry, n * 8}, {&S.counters, 2 * SEED_CTRS * 8}, {&S.pend, n * 8}, {&S.blk, n * BLK_PER_READ * 2 * sizeof(BlkRec)}, {&B.packed, n * stride * 8}, {&S.slots[0], n * (size_t)ctx->smem_cap * sizeof(SlotRec)},
        {&B.smem_off, (n + 1) * 8}, {&B.hit_off, (n + 1) * 8}, {&B.smems, n * 12 * sizeof(meme_mem_tl)}, {&B.hits, n * 24 * 8},
        {&C.chains, n * 3 * sizeof(meme_chain)}, {&C.seeds, n * 6 * sizeof(meme_chain_seed)}};
    for (auto& d : dev) if ((rc = meme_buf_reserve(ctx, *d.b, d.bytes))) return rc;
    if ((rc = meme_chain_reserve(ctx, nreads))) return rc;
    struct { HostBuf* b; size_t bytes; } host[] = {
        {&S.h_smem_off, (n + 1) * 8}, {&S.h_hit_off, (n + 1) * 8}, {&S.h_smems, n * 12 * sizeof(meme_mem_tl)}, {&S.h_hits, n * 24 * 8},
        {&C.h_chain_off, (n + 1) * 8}, {&C.h_chains, n * 3 * sizeof(meme_chain)}, {&C.h_seed_off, (n + 1) * 8},
        {&C.h_seeds, n * 6 * sizeof(meme_chain_seed)}, {&C.h_tree, n * 4}, {&C.h_frac, n * 4}, {&C.h_fallback, n}};
    for (auto& h : host) if ((rc = meme_hostbuf_reserve(ctx, *h.b, h.bytes))) return rc;
    // the stages behind seeding (meme_extend_last_batch_host, meme_global_batch_host) at their usual sizes for short reads: 4 alignment
    // records and 4 extension jobs of ~250 sequence bytes per read, one global alignment per 3 reads -- the first chunks of a run
    // otherwise pay for growing these (pinned memory: ~0.4 s per GB)
    struct { DevBuf* b; size_t bytes; } dev2[] = {
        {&E.rmax, n * 3 * 16}, {&E.regs, n * 4 * sizeof(meme_alnreg)}, {&E.order, n * 4 * 4}, {&E.counts, ExtCounts(nullptr, nreads).bytes},
        {&E.pairs_l, n * 2 * sizeof(meme_seqpair)}, {&E.pairs_r, n * 2 * sizeof(meme_seqpair)}, {&E.retry, n * 4 * sizeof(meme_seqpair)},
        {&E.seq, n * 4 * 250}};
    for (auto& d : dev2) if ((rc = meme_buf_reserve(ctx, *d.b, d.bytes))) return rc;
    if ((rc = meme_hostbuf_reserve(ctx, E.h_reg_off, (n + 1) * 8)) || (rc = meme_hostbuf_reserve(ctx, E.h_regs, n * 4 * sizeof(meme_alnreg))) ||
        (rc = meme_hostbuf_reserve(ctx, ctx->gcig.h_res, n / 2 * sizeof(meme_gres))) || (rc = meme_hostbuf_reserve(ctx, ctx->gcig.h_ops, n * 4))) return rc;
    return MEME_OK;
}

// FASTQ letters (or codes) -> base codes in place, as mem_kernel1_core_Learned does it on the host (src/bwamem.cpp:1277-1279:
// c < 4 ? c : nst_nt4_table[c]); 16 bytes per lane (the buffer is padded to a multiple of 16)
__global__ void __launch_bounds__(256) k_ascii_to_codes(uint4* __restrict__ p, i64 nvec) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (i64)gridDim.x * blockDim.x) {
        uint4 v = p[i];
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t o = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t c = (w[k] >> (8 * b)) & 0xffu, u = c & 0xdfu;        // u: upper case
                const uint32_t code = c < 4 ? c : (u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u);
                o |= code << (8 * b);
            }
            w[k] = o;
        }
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        p[i] = v;
    }
}

// reads from the host into HBM + the seeding kernels; `out` (may be null) receives the results in the ctx's pinned buffers
static int seed_host_reads(meme_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t nreads, const meme_seed_opt* opt, const char* who,
                           meme_seed_host_result* out, int64_t* totals, bool ascii = false) {
    if (!ctx || !reads || !read_off || nreads < 0) return MEME_E_ARG;
    int rc = check_opt(opt);
    if (rc) return rc;
    if (!ctx->idx.sa) { meme_set_error("%s: no index loaded", who); return MEME_E_STATE; }
    HIP_TRY(hipSetDevice(ctx->device));
    if (out) {
        memset(out, 0, sizeof(*out));
        if ((rc = meme_hostbuf_reserve(ctx, ctx->seed.h_smem_off, (size_t)(nreads + 1) * sizeof(i64)))) return rc;
        if ((rc = meme_hostbuf_reserve(ctx, ctx->seed.h_hit_off, (size_t)(nreads + 1) * sizeof(i64)))) return rc;
        out->smem_off = (const int64_t*)ctx->seed.h_smem_off.p;
        out->hit_off = (const int64_t*)ctx->seed.h_hit_off.p;
    }
    if (totals) totals[0] = totals[1] = 0;
    ctx->batch.last_seed_reads = 0;
    if (nreads == 0) { if (out) { ((i64*)ctx->seed.h_smem_off.p)[0] = 0; ((i64*)ctx->seed.h_hit_off.p)[0] = 0; } return MEME_OK; }
    if (read_off[0] != 0) { meme_set_error("read_off[0] must be 0"); return MEME_E_ARG; }
    const i64 bases = read_off[nreads];
    if ((rc = meme_buf_reserve(ctx, ctx->batch.reads, (size_t)bases + 16))) return rc;
    if ((rc = meme_buf_reserve(ctx, ctx->batch.read_off, (size_t)(nreads + 1) * sizeof(i64)))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->batch.reads.p, reads, (size_t)bases, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->batch.read_off.p, read_off, (size_t)(nreads + 1) * sizeof(i64), hipMemcpyHostToDevice, ctx->stream));
    if (ascii) {
        const i64 nvec = (bases + 15) / 16;
        i64 cb = (nvec + 255) / 256;
        if (cb > (i64)ctx->n_cus * 16) cb = (i64)ctx->n_cus * 16;
        hipLaunchKernelGGL(k_ascii_to_codes, dim3((unsigned)(cb < 1 ? 1 : cb)), dim3(256), 0, ctx->stream, (uint4*)ctx->batch.reads.p, nvec);
        HIP_TRY(hipGetLastError());
    }
    i64 max_len = 0;
    for (i64 i = 0; i < nreads; ++i) max_len = read_off[i + 1] - read_off[i] > max_len ? read_off[i + 1] - read_off[i] : max_len;
    meme_seed_result res;
    rc = launch_seed(ctx, (const uint8_t*)ctx->batch.reads.p, (const i64*)ctx->batch.read_off.p, nreads, max_len, bases, opt, &res);
    if (rc) return rc;
    if (out) {
        if ((rc = meme_hostbuf_reserve(ctx, ctx->seed.h_smems, (size_t)(res.total_smems + 1) * sizeof(meme_mem_tl)))) return rc;
        if ((rc = meme_hostbuf_reserve(ctx, ctx->seed.h_hits, (size_t)(res.total_hits + 1) * sizeof(u64)))) return rc;
        HIP_TRY(hipMemcpyAsync(ctx->seed.h_smem_off.p, res.d_smem_off, (size_t)(nreads + 1) * sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->seed.h_hit_off.p, res.d_hit_off, (size_t)(nreads + 1) * sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->seed.h_smems.p, res.d_smems, (size_t)res.total_smems * sizeof(meme_mem_tl), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->seed.h_hits.p, res.d_hits, (size_t)res.total_hits * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
        out->smems = (const meme_mem_tl*)ctx->seed.h_smems.p;
        out->hits = (const uint64_t*)ctx->seed.h_hits.p;
        out->total_smems = res.total_smems;
        out->total_hits = res.total_hits;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // (the caller's read buffer is free again)
    if (totals) { totals[0] = res.total_smems; totals[1] = res.total_hits; }
    ctx->batch.last_seed_reads = nreads;
    ctx->batch.reads_resident = true;
    ctx->batch.last_seed_max_len = max_len;
    return MEME_OK;
}

extern "C" int meme_seed_batch_host(meme_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t nreads,
                                    const meme_seed_opt* opt, meme_seed_host_result* out) {
    if (!out) return MEME_E_ARG;
    return seed_host_reads(ctx, reads, read_off, nreads, opt, "meme_seed_batch_host", out, nullptr);
}

extern "C" int meme_seed_batch_resident(meme_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t nreads,
                                        const meme_seed_opt* opt, int64_t* total_smems, int64_t* total_hits) {
    int64_t tot[2] = {0, 0};
    const int rc = seed_host_reads(ctx, reads, read_off, nreads, opt, "meme_seed_batch_resident", nullptr, tot);
    if (total_smems) *total_smems = tot[0];
    if (total_hits) *total_hits = tot[1];
    return rc;
}

// Same, for reads as they stand in the FASTQ file (letters; bytes below 4 are taken as codes): the conversion of
// mem_kernel1_core_Learned (src/bwamem.cpp:1277-1279) runs on the device, so a caller only has to gather the bytes.
extern "C" int meme_seed_batch_resident_ascii(meme_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t nreads,
                                              const meme_seed_opt* opt, int64_t* total_smems, int64_t* total_hits) {
    int64_t tot[2] = {0, 0};
    const int rc = seed_host_reads(ctx, reads, read_off, nreads, opt, "meme_seed_batch_resident_ascii", nullptr, tot, true);
    if (total_smems) *total_smems = tot[0];
    if (total_hits) *total_hits = tot[1];
    return rc;
}
