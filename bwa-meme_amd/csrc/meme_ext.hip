// Seed extension of a whole batch on the device: mem_chain2aln_across_reads_V2 (reference src/bwamem.cpp:2573-3497) behind the chaining
// kernels -- seeds, chains, extension jobs and their sequences never leave HBM; the host receives mem_alnreg_t records.
//
//   k_flt_pose / k_seedsw / k_flt_count / k_flt_move   mem_flt_chained_seeds (:565-598), only for reads it is not a no-op for (long
//                      reads, -W): seeds whose neighbourhood aligns poorly leave their chains before anything is extended
//   k_ext_jobs<false>  per read: the reference span of every chain (:2648-2690 + bns_fetch_seq_v2, src/bntseq.cpp:479-512), the
//                      number of left / right extension jobs and of sequence bytes                                  -> scans
//   k_ext_jobs<true>   per read: one alignment record per chained seed in extension order (best seed of a chain first, :2692-2702),
//                      the left (:2722-2781) and right (:2783-2850) jobs as SeqPair records, their sequences copied from the 2-bit
//                      text and the read (left jobs reversed), the per-chain seed order the purge step walks
//   meme_bsw           k_bsw_lane / k_bsw<LP> on the jobs of one direction and band width (meme_bsw.hip)
//   k_ext_fold<left>   results into the records (:2985-3018 and siblings); jobs whose band was too narrow to a retry list (MAX_BAND_TRY 2)
//   k_ext_h0           start score of the right extension = score after the left one (:3371-3376)
//   k_ext_purge        alignments of seeds an earlier alignment of the read already covers are dropped (:3389-3485)
// The reference's rules -- spans, job geometry, records, fold, purge predicates -- are meme_ext_rules.h's; here is who walks what.
//
// One wavefront per read in the kernels that walk a read's chains (a read has 1 to a few hundred chained seeds: lanes take seeds, the
// wavefront reduces / scans across them, and a repeat-rich read cannot hold 63 others back); one lane per job in the others.
#include <math.h>
#include <string.h>

#include "meme_common.h"
#include "meme_ext_rules.h"

namespace {

struct ExtArgs {
    const uint8_t* reads; const i64* read_off; i64 g0, ns;            // reads [g0, g0 + ns) of the batch
    const i64* chain_off; const meme_chain* chains; const i64* seed_off; const meme_chain_seed* seeds; const float* frac_rep;
    const int* seed_score;            // per chained seed, or null: score = length (what chaining leaves, src/bwamem.cpp:1163)
    const u64* pac; i64 l_pac;
    const i64* contig_off; const int* contig_len;
    meme_ext_opt o;
    i64* rmax;                        // [2 * chain]: reference span of a chain
    meme_alnreg* regs; int* order;    // per chained seed of the batch
    i64 *cntL, *cntR, *cntB;          // per read (from g0): left jobs, right jobs, sequence bytes (k_ext_jobs<false>)
    const i64 *offL, *offR, *offB;    // their exclusive scans over the batch (pointing at read g0)
    i64 job0L, job0R, byte0;          // offsets of this slab's first job / byte (subtracted: SeqPair offsets are 32-bit)
    meme_seqpair* L; meme_seqpair* R; uint8_t* seq;
    // extension in rounds (tuning "ext_rounds"): mode 0 = every chained seed at once (the reference's batch, :2573-3388); 1 = records and the extension
    // order only, no jobs; 2 = jobs of the seeds k_ext_advance selected (sel: per chained seed; act: per read, any selected)
    int mode; const uint8_t* sel; const uint8_t* act; int4* state;
    // round 6: the kernels that walk a read's chains exist in two widths -- a wavefront per read (G = 64) for the reads in `list` (more than
    // EXT_LIGHT chained seeds), and EIGHT LANES per read (G = 8: eight reads per wavefront) for the others, which are the many: a 150-bp read
    // has four chained seeds on average and a wavefront's life is a chain of dependent loads, not work.  list == nullptr: every read of the slab.
    const i64* list; i64 nlist; int light;           // light: G = 8 launch -- reads with more than EXT_LIGHT seeds are skipped (they are in the other launch's list)
};
constexpr int EXT_LIGHT = 8;

// sub-wavefront groups of G lanes (G = 64: the wavefront): ballots, broadcasts and reductions that stay inside the group
template <int G> __device__ __forceinline__ u64 gballot(bool p, int gbase) { const u64 b = __ballot(p); return G == 64 ? b : (b >> gbase) & (((u64)1 << (G & 63)) - 1); }
template <int G> __device__ __forceinline__ i64 group_min(i64 v) { for (int d = G / 2; d >= 1; d >>= 1) { const i64 y = __shfl_xor(v, d); v = y < v ? y : v; } return v; }
template <int G> __device__ __forceinline__ i64 group_max(i64 v) { for (int d = G / 2; d >= 1; d >>= 1) { const i64 y = __shfl_xor(v, d); v = y > v ? y : v; } return v; }

template <bool WRITE, int G>
__global__ void __launch_bounds__(256) k_ext_jobs(ExtArgs A) {
    const i64 it = (i64)blockIdx.x * (256 / G) + threadIdx.x / G;  // a group of G lanes per read (G = 64: a wavefront each, four to a workgroup -- 2 M one-wave workgroups take 4 ms to dispatch)
    if (it >= (A.list ? A.nlist : A.ns)) return;
    const i64 r = A.list ? A.list[it] : A.g0 + it;
    const i64 rl = r - A.g0;                          // read of the slab
    const int lane = threadIdx.x & (G - 1);           // lane of the group
    const int gbase = (threadIdx.x & 63) & ~(G - 1);  // the group's first lane in its wavefront
    const i64 c0 = A.chain_off[r];
    const int nc = (int)(A.chain_off[r + 1] - c0);
    const i64 s0 = A.seed_off[r];
    const int S = (int)(A.seed_off[r + 1] - s0);
    if (A.light && S > EXT_LIGHT) return;             // (the wavefront-per-read launch has it)
    const int l_query = (int)(A.read_off[r + 1] - A.read_off[r]);
    const meme_ext_opt& o = A.o;
    if (A.mode == 2 && !A.act[r]) {                  // nothing of this read in the round
        if (!WRITE && lane == 0) { A.cntL[rl] = 0; A.cntR[rl] = 0; A.cntB[rl] = 0; }
        return;
    }
    if (WRITE ? A.mode == 1 : A.mode == 0) {
        // ---- reference span of every chain: the widest any of its seeds may reach (:2648-2690)
        for (int c = 0; c < nc; ++c) {
            const meme_chain ch = A.chains[c0 + c];
            const meme_chain_seed* sd = A.seeds + s0 + ch.seed_beg;
            i64 b_min = A.l_pac << 1, e_max = 0;
            for (int i = lane; i < ch.n_seeds; i += G) {
                const ExtSpan x = ext_seed_reach(sd[i], l_query, o);
                b_min = x.b < b_min ? x.b : b_min;
                e_max = x.e > e_max ? x.e : e_max;
            }
            i64 rmax0 = group_min<G>(b_min), rmax1 = group_max<G>(e_max);
            const i64 mid = sd[0].rbeg;
            ext_span_finish(rmax0, rmax1, mid, A.l_pac);
            // bns_fetch_seq_v2: the span stays inside the chain's reference sequence (on the strand of its first seed)
            bns_clamp(A.l_pac, A.contig_off[ch.rid], A.contig_len[ch.rid], mid >= A.l_pac, rmax0, rmax1);
            A.rmax[2 * (c0 + c)] = rmax0;
            A.rmax[2 * (c0 + c) + 1] = rmax1;
        }
    }
    // ---- one lane per chained seed: its place in the extension order, its two jobs
    i64 nL = 0, nR = 0, nB = 0;                       // running totals of the read (uniform)
    const bool posing = WRITE && A.mode != 1;
    const i64 jobL0 = posing ? A.offL[rl] - A.job0L : 0, jobR0 = posing ? A.offR[rl] - A.job0R : 0;
    const i64 byte0 = posing ? A.offB[rl] - A.byte0 : 0;
    for (int jb = 0; jb < S; jb += G) {
        const int j = jb + lane;
        const bool valid = j < S;
        int c = 0;
        if (valid) {                                  // the chain of seed j: chains are packed in order, seed_beg ascending
            int lo = 0, hi = nc - 1;
            while (lo < hi) { const int m = (lo + hi + 1) >> 1; if (A.chains[c0 + m].seed_beg <= j) lo = m; else hi = m - 1; }
            c = lo;
        }
        const meme_chain ch = A.chains[c0 + (valid ? c : 0)];
        const meme_chain_seed* sd = A.seeds + s0 + ch.seed_beg;
        const int il = valid ? j - ch.seed_beg : 0;
        const meme_chain_seed t = sd[il];
        const i64 rmax0 = A.rmax[2 * (c0 + c)], rmax1 = A.rmax[2 * (c0 + c) + 1];
        const bool pick = valid && A.mode != 1 && (A.mode == 0 || A.sel[s0 + j]);              // its jobs are posed by this launch
        const ExtGeom g = ext_geom(t, rmax0, rmax1, l_query);       // the flanks the seed has, their lengths and bytes
        const bool hasL = pick && g.sideL, hasR = pick && g.sideR;
        const int bytesL = hasL ? g.bytesL : 0, bytesR = hasR ? g.bytesR : 0;
        const u64 mL = gballot<G>(hasL, gbase), mR = gballot<G>(hasR, gbase), below = ((u64)1 << lane) - 1;
        // exclusive scan of the bytes over the lanes
        int bsum = bytesL + bytesR, bex;
        {
            int x = bsum;
            for (int d = 1; d < G; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d) x += y; }
            bex = x - bsum;
            bsum = __shfl(x, gbase + G - 1);
        }
        if (WRITE && valid && (A.mode != 2 || pick)) {
            // rank among the chain's seeds by (score, index): ks_introsort_64 on score << 32 | index, keys unique (:2692-2699)
            int rank = 0;
            if (A.seed_score) {
                const int* ss = A.seed_score + s0 + ch.seed_beg;
                const int mine = ss[il];
                for (int k = 0; k < ch.n_seeds; ++k) rank += ext_seed_before(ss[k], k, mine, il) ? 1 : 0;
            } else
                for (int k = 0; k < ch.n_seeds; ++k) rank += ext_seed_before(sd[k].len, k, t.len, il) ? 1 : 0;
            if (A.mode != 2) A.order[s0 + ch.seed_beg + rank] = il;
            const i64 reg = s0 + ch.seed_beg + (ch.n_seeds - 1 - rank);        // best seed first
            if (A.mode != 2) A.regs[reg] = ext_record0(t, g.sideL, g.sideR, l_query, o, ch.rid, A.frac_rep[r], (u64)(c0 + c), sd, ch.n_seeds);
            const int idr = (int)(byte0 + nB + bex);
            if (hasL) A.L[jobL0 + nL + __popcll(mL & below)] = ext_pose(t.len * o.a, (int)r, (int)reg, g.l1L, g.l2L, idr);
            if (hasR) A.R[jobR0 + nR + __popcll(mR & below)] = ext_pose(H0, (int)r, (int)reg, g.l1R, g.l2R, idr + bytesL);
        }
        if (WRITE) {
            // the sequences, job after job, 64 lanes x 4 bases per step: left jobs reversed (both sequences run away from the seed)
            const uint8_t* rd = A.reads + A.read_off[r];
            for (int side = 0; side < 2; ++side) {
                u64 m = side ? mR : mL;
                while (m) {
                    const int jl = __builtin_ctzll(m);
                    m &= m - 1;
                    const i64 rbeg = __shfl(t.rbeg, gbase + jl);
                    const int qb = __shfl(t.qbeg, gbase + jl), ln = __shfl(t.len, gbase + jl);
                    const int l1 = __shfl(side ? g.l1R : g.l1L, gbase + jl), l2 = __shfl(side ? g.l2R : g.l2L, gbase + jl);
                    const i64 dst = byte0 + nB + __shfl(bex, gbase + jl) + (side ? __shfl(bytesL, gbase + jl) : 0);
                    uint8_t* dr = A.seq + dst;
                    uint8_t* dq = dr + ext_query_off(l1);
                    for (int i = lane * 4; i < l1; i += 4 * G) {
                        unsigned v = 0;
                        for (int b = 0; b < 4; ++b) {
                            const int k = i + b;
                            const int code = k < l1 ? text_base(A.pac, side ? rbeg + ln + k : rbeg - 1 - k) : 0;
                            v |= (unsigned)code << (8 * b);
                        }
                        *reinterpret_cast<unsigned*>(dr + i) = v;
                    }
                    for (int i = lane * 4; i < l2; i += 4 * G) {
                        unsigned v = 0;
                        for (int b = 0; b < 4; ++b) {
                            const int k = i + b;
                            const int code = k < l2 ? rd[side ? qb + ln + k : qb - 1 - k] : 0;
                            v |= (unsigned)code << (8 * b);
                        }
                        *reinterpret_cast<unsigned*>(dq + i) = v;
                    }
                }
            }
        }
        nL += __popcll(mL); nR += __popcll(mR); nB += bsum;
    }
    if (!WRITE && lane == 0) { A.cntL[rl] = nL; A.cntR[rl] = nR; A.cntB[rl] = nB; }
    if (WRITE && A.mode == 1 && lane == 0) A.state[r] = make_int4(0, nc ? A.chains[c0].n_seeds - 1 : 0, 0, 0);   // k_ext_advance starts at the best seed of the first chain
}

// ---- mem_flt_chained_seeds (src/bwamem.cpp:565-598) ---------------------------------------------------------------------------------
struct FltArgs {
    const i64* read_off; i64 n;
    const i64* chain_off; meme_chain* chains; const i64* seed_off; const meme_chain_seed* seeds;
    i64 l_pac; const i64* contig_off; const int* contig_len; int n_contigs;
    const int* hsp;                  // per read length: min_HSP_score (:582), -1 where the filter does not run (:583)
    int a;
    int* sc;                         // per chained seed: FLT_OFF, -1 (kept without alignment, :502 / :515) or mem_seed_sw's score
    meme_seedsw_job* jobs; unsigned long long* n_jobs;
    i64* cnt;                        // per read: seeds that stay
    const i64* off2;                 // its exclusive scan = the new seed_off
    meme_chain_seed* seeds2; int* score2;
};

// the alignments mem_seed_sw would run (src/bwamem.cpp:494-520, bns_fetch_seq src/bntseq.cpp:541-570): one lane per chained seed
__global__ void __launch_bounds__(64) k_flt_pose(FltArgs A) {
    const i64 r = blockIdx.x;
    if (r >= A.n) return;
    const int lane = threadIdx.x;
    const i64 s0 = A.seed_off[r];
    const int S = (int)(A.seed_off[r + 1] - s0);
    const i64 q0 = A.read_off[r];
    const int l_query = (int)(A.read_off[r + 1] - q0);
    const int hsp = A.hsp[l_query];
    for (int jb = 0; jb < S; jb += 64) {
        const int j = jb + lane;
        bool job = false;
        meme_seedsw_job J;
        if (j < S) {
            int v = FLT_OFF;
            if (hsp >= 0) {
                v = -1;
                const meme_chain_seed t = A.seeds[s0 + j];
                const FltWindow W = flt_window(t, l_query, A.l_pac, A.contig_off, A.contig_len, A.n_contigs, MEME_SEEDSW_MAX);
                job = W.job;
                if (job) { J.rb = W.rb; J.qoff = q0 + W.qb; J.seed = (int)(s0 + j); J.tlen = (short)(W.re - W.rb); J.qlen = (short)(W.qe - W.qb); }
            }
            A.sc[s0 + j] = v;
        }
        const u64 m = __ballot(job);
        if (m) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(A.n_jobs, (unsigned long long)__popcll(m));
            base = __shfl(base, 0);
            if (job) A.jobs[base + __popcll(m & (((u64)1 << lane) - 1))] = J;
        }
    }
}

// seeds that stay: per read (-> scan -> the new seed_off), per chain (n_seeds; seed_beg = the kept seeds of the read's earlier chains)
template <bool MOVE>
__global__ void __launch_bounds__(64) k_flt_apply(FltArgs A) {
    const i64 r = blockIdx.x;
    if (r >= A.n) return;
    const int lane = threadIdx.x;
    const i64 c0 = A.chain_off[r];
    const int nc = (int)(A.chain_off[r + 1] - c0);
    const i64 s0 = A.seed_off[r];
    const int hsp = A.hsp[(int)(A.read_off[r + 1] - A.read_off[r])];
    const i64 d0 = MOVE ? A.off2[r] : 0;
    int kept = 0;                                     // of the read so far (uniform)
    for (int c = 0; c < nc; ++c) {
        const meme_chain ch = A.chains[c0 + c];
        int kc = 0;
        for (int jb = 0; jb < ch.n_seeds; jb += 64) {
            const int j = jb + lane;
            const i64 g = s0 + ch.seed_beg + (j < ch.n_seeds ? j : 0);
            const int v = A.sc[g];
            const bool keep = j < ch.n_seeds && flt_keeps(v, hsp);
            const u64 m = __ballot(keep);
            if (MOVE && keep) {
                const meme_chain_seed t = A.seeds[g];
                const i64 d = d0 + kept + kc + __popcll(m & (((u64)1 << lane) - 1));
                A.seeds2[d] = t;
                A.score2[d] = flt_kept_score(v, t.len, A.a);
            }
            kc += __popcll(m);
        }
        if (MOVE && lane == 0) { A.chains[c0 + c].seed_beg = kept; A.chains[c0 + c].n_seeds = kc; }
        kept += kc;
    }
    if (!MOVE && lane == 0) A.cnt[r] = kept;
}

struct FoldArgs {
    meme_seqpair* pairs; i64 n;
    meme_alnreg* regs; const meme_chain* chains; const i64* seed_off; const meme_chain_seed* seeds; const i64* read_off;
    meme_ext_opt o; int w, last;
    meme_seqpair* retry; unsigned long long* n_retry;
};

// results of one stage into the alignment records (src/bwamem.cpp:2985-3018 left, :3253-3290 right, and their siblings)
template <bool LEFT>
__global__ void __launch_bounds__(256) k_ext_fold(FoldArgs F) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < F.n; i += (i64)gridDim.x * blockDim.x) {
        const meme_seqpair sp = F.pairs[i];
        meme_alnreg& a = F.regs[sp.regid];
        if (ext_fold<LEFT>(a, sp, F.w, F.last, F.o, (int)(F.read_off[sp.seqid + 1] - F.read_off[sp.seqid]))) {
            const meme_chain ch = F.chains[a.c];
            seedcov(a, F.seeds + F.seed_off[sp.seqid] + ch.seed_beg, ch.n_seeds);
        } else F.retry[atomicAdd(F.n_retry, 1ull)] = sp;
    }
}

__global__ void __launch_bounds__(256) k_ext_h0(meme_seqpair* __restrict__ pairs, i64 n, const meme_alnreg* __restrict__ regs) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) pairs[i].h0 = regs[pairs[i].regid].score;
}

struct PurgeArgs {
    const i64* read_off; i64 nreads;
    const i64* chain_off; const meme_chain* chains; const i64* seed_off; const meme_chain_seed* seeds;
    meme_alnreg* regs; int* order;
    meme_ext_opt o;
};

// (:3389-3485) is the seed s -- k-th of its chain's extension order `ord`, `cur` records of the read before it -- dropped?  The group's lanes take the earlier
// records, then the chain's seeds extended before s (later in ord; -1: dropped themselves); every lane of the group returns the same answer
template <int G>
__device__ __forceinline__ bool ext_seed_dropped(const meme_alnreg* av, int cur, const meme_chain_seed& s, const meme_chain_seed* sd, const int* ord, int k, int n_seeds,
                                                 int l_query, const meme_ext_opt& o, int lane, int gbase) {
    // an earlier, surviving alignment that contains the seed and has it within its band on either side?
    bool found = false;
    for (int ib = 0; ib < cur && !found; ib += G) {
        const int i = ib + lane;
        bool hit = false;
        if (i < cur) { const meme_alnreg* p = &av[i]; hit = ext_covers(p->rb, p->re, p->qb, p->qe, p->w, p->seedlen0, s, l_query, o); }
        found = gballot<G>(hit, gbase) != 0;
    }
    if (!found) return false;
    // (almost) contained -- unless a long, overlapping, better seed of the chain on another diagonal says otherwise
    bool other = false;
    for (int ub = k + 1; ub < n_seeds && !other; ub += G) {
        const int u = ub + lane;
        const bool hit = u < n_seeds && ord[u] >= 0 && ext_other_diagonal(s, sd[ord[u]]);
        other = gballot<G>(hit, gbase) != 0;
    }
    return !other;
}

// The walk over read r in the order the one-read-at-a-time aligner would have met its seeds -- chain after chain, best seed first -- from rank k_first of chain
// c_first, `cur` seeds met before: dropped seeds are marked (qb = qe = -1; -1 in the order); survivor(c, k, cur, chain, seed) = true ends the walk at a survivor.
// Returns the number of seeds met when the read is walked to its end, -1 when survivor ended it.
template <int G, class F>
__device__ __forceinline__ int ext_walk(const PurgeArgs& P, i64 r, int lane, int gbase, int c_first, int k_first, int cur, const F& survivor) {
    const i64 c0 = P.chain_off[r];
    const int nc = (int)(P.chain_off[r + 1] - c0);
    const i64 s0 = P.seed_off[r];
    const int l_query = (int)(P.read_off[r + 1] - P.read_off[r]);
    meme_alnreg* av = P.regs + s0;                     // av[cur]: record of the seed at hand
    for (int c = c_first; c < nc; ++c) {
        const meme_chain ch = P.chains[c0 + c];
        const meme_chain_seed* sd = P.seeds + s0 + ch.seed_beg;
        int* ord = P.order + s0 + ch.seed_beg;
        for (int k = c == c_first ? k_first : ch.n_seeds - 1; k >= 0; --k, ++cur) {
            const meme_chain_seed s = sd[ord[k]];
            if (ext_seed_dropped<G>(av, cur, s, sd, ord, k, ch.n_seeds, l_query, P.o, lane, gbase)) { av[cur].qb = -1; av[cur].qe = -1; ord[k] = -1; }
            else if (survivor(c, k, cur, ch, s)) return -1;
        }
    }
    return cur;
}

// the reference's batch order: every alignment exists, the whole read is walked
__global__ void __launch_bounds__(256) k_ext_purge(PurgeArgs P) {
    const i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= P.nreads) return;
    if (P.seed_off[r + 1] - P.seed_off[r] < 2) return;            // a lone alignment has nothing before it
    ext_walk<64>(P, r, threadIdx.x & 63, 0, 0, P.chains[P.chain_off[r]].n_seeds - 1, 0, [](int, int, int, const meme_chain&, const meme_chain_seed&) { return false; });
}

// ---- extension in rounds ------------------------------------------------------------------------------------------------------------------
// The reference extends every chained seed of a batch and then drops, read by read and in extension order, the alignments of seeds that an
// earlier SURVIVING alignment of the read covers (:3389-3485); mem_kernel2_core deletes the dropped records at once (src/bwamem.cpp:1680-1693).
// A dropped seed's extension is therefore never looked at, and whether a seed is dropped depends on the survivors before it only: the same
// records come out when a read's seeds are taken in that order, tested first, and extended only if they survive.  k_ext_advance walks a read
// from where it stands: dropped seeds are marked, the first survivor is selected for this round's jobs (ADV_ONE); in the last round every seed
// from the next survivor on is selected at once (ADV_REST: repeat-rich reads have tens of survivors, one round each would be launches without work) and
// ADV_FINISH walks to the end over alignments that then all exist -- which is the reference's own pass from that point on.
enum { ADV_ONE = 0, ADV_REST = 1, ADV_FINISH = 2 };
struct AdvArgs {
    PurgeArgs P; int4* state; uint8_t* sel; uint8_t* act; i64* cntS; int mode;     // cntS: seeds selected per read (summed by a scan: an atomic per read on one address costs 12 ns each)
    const i64* rmax; i64 *cntL, *cntR, *cntB;        // the round's plan as k_ext_jobs<false> would count it: left / right jobs and sequence bytes of the read's selected seeds
    const i64* list; i64 nlist; int light;           // as in ExtArgs: the wavefront-per-read launch walks `list`, the eight-lanes-per-read launch everything with at most EXT_LIGHT seeds
};
template <int G>
__global__ void __launch_bounds__(256) k_ext_advance(AdvArgs V) {
    const PurgeArgs& P = V.P;
    const i64 it = (i64)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (it >= (V.list ? V.nlist : P.nreads)) return;
    const i64 r = V.list ? V.list[it] : it;
    const int lane = threadIdx.x & (G - 1);
    const int gbase = (threadIdx.x & 63) & ~(G - 1);
    const i64 c0 = P.chain_off[r];
    const int nc = (int)(P.chain_off[r + 1] - c0);
    const i64 s0 = P.seed_off[r];
    if (V.light && P.seed_off[r + 1] - s0 > EXT_LIGHT) return;
    const int4 st = V.state[r];                        // x chain, y rank of the next seed in it (-1: the chain is done), z seeds met so far
    if (V.mode != ADV_FINISH && lane == 0) { V.act[r] = 0; V.cntL[r] = 0; V.cntR[r] = 0; V.cntB[r] = 0; V.cntS[r] = 0; }
    if (st.x >= nc) return;
    const int l_query = (int)(P.read_off[r + 1] - P.read_off[r]);
    i64 nL = 0, nR = 0, nB = 0;                        // the round's plan: jobs and bytes of the seeds selected, as k_ext_jobs will pose them
    const auto plan = [&](const meme_chain_seed& t, i64 c) { const ExtGeom g = ext_geom(t, V.rmax[2 * c], V.rmax[2 * c + 1], l_query); nL += g.sideL; nR += g.sideR; nB += g.bytesL + g.bytesR; };
    const int met = ext_walk<G>(P, r, lane, gbase, st.x, st.y, st.z, [&](int c, int k, int cur, const meme_chain& ch, const meme_chain_seed& s) {
        if (V.mode == ADV_FINISH) return false;        // a survivor whose alignment exists
        if (V.mode == ADV_REST) {                      // this survivor and everything behind it go into the round; ADV_FINISH walks on from here
            unsigned long long cnt = 0;
            for (int c2 = c; c2 < nc; ++c2) {
                const meme_chain ch2 = P.chains[c0 + c2];
                const int* ord2 = P.order + s0 + ch2.seed_beg;
                const int k1 = c2 == c ? k : ch2.n_seeds - 1;
                for (int k2 = k1 - lane; k2 >= 0; k2 -= G) {
                    const int il = ord2[k2];
                    V.sel[s0 + ch2.seed_beg + il] = 1;
                    plan(P.seeds[s0 + ch2.seed_beg + il], c0 + c2);
                }
                cnt += k1 + 1;
            }
            for (int d = G / 2; d >= 1; d >>= 1) { nL += __shfl_xor(nL, d); nR += __shfl_xor(nR, d); nB += __shfl_xor(nB, d); }
            if (lane == 0) { V.act[r] = 1; V.state[r] = make_int4(c, k, cur, 0); V.cntS[r] = (i64)cnt; V.cntL[r] = nL; V.cntR[r] = nR; V.cntB[r] = nB; }
            return true;
        }
        if (lane == 0) {                               // this round's seed of the read
            V.sel[s0 + ch.seed_beg + P.order[s0 + ch.seed_beg + k]] = 1;
            V.act[r] = 1;
            V.state[r] = make_int4(c, k - 1, cur + 1, 0);
            V.cntS[r] = 1;
            plan(s, c0 + c);
            V.cntL[r] = nL; V.cntR[r] = nR; V.cntB[r] = nB;
        }
        return true;
    });
    if (met >= 0 && lane == 0) V.state[r] = make_int4(nc, 0, met, 0);
}

// reads with more than EXT_LIGHT chained seeds: the list the wavefront-per-read launches walk (order is irrelevant: everything is indexed by read)
__global__ void __launch_bounds__(256) k_ext_split(const i64* __restrict__ seed_off, i64 n, i64* __restrict__ list, unsigned long long* __restrict__ cnt) {
    for (i64 r0 = (i64)blockIdx.x * 256; r0 < n; r0 += (i64)gridDim.x * 256) {
        const i64 r = r0 + threadIdx.x;
        const bool heavy = r < n && seed_off[r + 1] - seed_off[r] > EXT_LIGHT;
        const u64 m = __ballot(heavy);
        if (m) {
            const int lane = threadIdx.x & 63;
            unsigned long long base = 0;
            if (lane == (int)__builtin_ctzll(m)) base = atomicAdd(cnt, (unsigned long long)__popcll(m));
            base = __shfl(base, (int)__builtin_ctzll(m));
            if (heavy) list[base + __popcll(m & (((u64)1 << lane) - 1))] = r;
        }
    }
}

// tuning "ext_live_only": what mem_kernel2_core does first with the stage's records (src/bwamem.cpp:1680-1693: every record with qe <= qb -- the purged
// ones -- is dropped, the others keep their order) done before the records cross to the host: a read's surviving records counted, then packed.
__global__ void __launch_bounds__(256) k_ext_live_count(const i64* __restrict__ seed_off, const meme_alnreg* __restrict__ regs, i64 n, i64* __restrict__ cnt) {
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < n; r += (i64)gridDim.x * 256) {
        int m = 0;
        for (i64 i = seed_off[r]; i < seed_off[r + 1]; ++i) m += regs[i].qe > regs[i].qb;
        cnt[r] = m;
    }
}
__global__ void __launch_bounds__(256) k_ext_live_pack(const i64* __restrict__ seed_off, const meme_alnreg* __restrict__ regs, i64 n, const i64* __restrict__ live_off,
                                                       meme_alnreg* __restrict__ out) {
    static_assert(sizeof(meme_alnreg) == 7 * 16, "record copied as seven 16-byte words");
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < n; r += (i64)gridDim.x * 256) {
        i64 o = live_off[r];
        if (o == live_off[r + 1]) continue;
        for (i64 i = seed_off[r]; i < seed_off[r + 1]; ++i) {
            if (!(regs[i].qe > regs[i].qb)) continue;
            const uint4* s = (const uint4*)&regs[i];
            uint4* d = (uint4*)&out[o++];
#pragma unroll
            for (int k = 0; k < 7; ++k) d[k] = s[k];
        }
    }
}

// measurement (tuning "ext_census"): jobs whose query equals the first len2 bases of the target (no ambiguous base) -- the jobs a closed form
// could answer without the DP (score = h0 + len2 * a).  SMEM seeds end on a mismatch or at a read end, so few are expected.
__global__ void __launch_bounds__(256) k_ext_census(const meme_seqpair* __restrict__ pairs, i64 n, const uint8_t* __restrict__ seq, int w, unsigned long long* __restrict__ cnt) {
    __shared__ unsigned long long acc[11];
    if (threadIdx.x < 11) acc[threadIdx.x] = 0;
    __syncthreads();
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (i64)gridDim.x * blockDim.x) {
        const meme_seqpair P = pairs[k];
        // [1] cells of the band-limited matrix (rows = target bases, columns = query bases within w of the diagonal)
        unsigned long long cells = 0;
        for (int i = 0; i < P.len1; ++i) {
            const int beg = i > w ? i - w : 0, end = i + w + 1 < P.len2 ? i + w + 1 : P.len2;
            if (end > beg) cells += (unsigned)(end - beg);
        }
        atomicAdd(&acc[1], cells);
        // [2..10] LDS size class of the lane-per-pair kernel (LANE_CLS_Q, meme_bsw.hip)
        const int q = P.len2;
        const int c = q <= 30 ? 0 : q <= 62 ? 1 : q <= 94 ? 2 : q <= 126 ? 3 : q <= 158 ? 4 : q <= 222 ? 5 : q <= 318 ? 6 : q <= 600 ? 7 : 8;
        atomicAdd(&acc[2 + c], 1ull);
        // [0] query == first len2 target bases
        if (P.len2 > P.len1) continue;
        const uint8_t* qq = seq + P.idq;
        const uint8_t* tt = seq + P.idr;
        bool same = true;
        for (int i = 0; same && i < P.len2; ++i) same = qq[i] == tt[i] && qq[i] < 4;
        if (same) atomicAdd(&acc[0], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < 11 && acc[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], acc[threadIdx.x]);
}

// ---- the host side: meme_extend_last_batch_host in phases around one ExtRun ----------------------------------------------------------
struct ExtRun {
    meme_ctx* ctx; const meme_chain_opt* copt; const meme_ext_opt* eopt; int32_t n_contigs;
    i64 n, n_chains, n_seeds;                       // reads, chains, chained seeds (before the filter) of the batch
    ExtCounts ec = ExtCounts(nullptr, 0);
    ExtArgs A;                                      // what every launch of k_ext_jobs starts from: the batch, the records, the counts
    meme_bsw_opt bsw[2];                            // left / right (bswLeft / bswRight, src/bwamem.cpp:2953-2959)
    unsigned long long* ctr = nullptr;              // ExtWs::counters
    bool flt_read = true;                           // false: the seed filter ran and its two totals have yet to cross to the host
    i64 h_flt[2] = {0, 0};                          // chained seeds after the filter, alignments it ran
    i64 n_heavy = 0; const i64* d_heavy = nullptr;  // reads with more than EXT_LIGHT chained seeds (tuning "ext_split")
    i64 tot[3] = {0, 0, 0};                         // the plan's totals: left jobs, right jobs, sequence bytes
    std::vector<i64> h_off;                         // the plan's three offset columns on the host (more than one slab only)
    i64 n_pairs = 0, n_retried = 0, n_calls = 0, n_seeds_ext = 0;   // n_seeds_ext: chained seeds whose extension jobs ran
    float bsw_ms = 0.f;
};
struct Slab { i64 g0, g1, n[3], first[3]; };        // reads [g0, g1): its left jobs, right jobs and sequence bytes, and the batch's before it

int ext_check(meme_ctx* ctx, const meme_contig* contigs, int32_t n_contigs, const meme_chain_opt* copt, const meme_ext_opt* eopt, meme_ext_host_result* out) {
    if (!ctx || !contigs || n_contigs < 1 || !copt || !eopt || !out) { meme_set_error("meme_extend_last_batch_host: null argument"); return MEME_E_ARG; }
    if (copt->max_occ < 1 || copt->l_pac < 1 || eopt->e_del < 1 || eopt->e_ins < 1 || eopt->w < 1) { meme_set_error("meme_extend_last_batch_host: bad options"); return MEME_E_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    const i64 n = ctx->batch.last_seed_reads;
    if (n <= 0 || !ctx->batch.smem_off.p || !ctx->batch.read_off.p || !ctx->batch.reads.p || !ctx->batch.reads_resident) {
        meme_set_error("meme_extend_last_batch_host: no seeded batch on this ctx (a seeding call has to stage the reads; meme_chain_batch_host brings seeds only)");
        return MEME_E_STATE;
    }
    if (copt->l_pac * 2 != ctx->idx.n) { meme_set_error("meme_extend_last_batch_host: l_pac does not match the loaded index"); return MEME_E_ARG; }
    if (ctx->max_batch > 0 && n > ctx->max_batch) { meme_set_error("meme_extend_last_batch_host: %lld reads exceed the ctx's max_batch of %lld", (long long)n, (long long)ctx->max_batch); return MEME_E_CAPACITY; }
    return MEME_OK;
}
// the stage's events and counters; what every launch starts from (chaining's seeds until the filter has had its say)
int ext_begin(ExtRun& R) {
    meme_ctx* ctx = R.ctx;
    ExtWs& E = ctx->ext;
    const ChainWs& C = ctx->chain;
    HIP_TRY(E.ev.ensure());
    HIP_TRY(hipEventRecord(E.ev[0], ctx->stream));
    int rc;
    if ((rc = meme_buf_reserve(ctx, E.counters, EXT_CTR_BYTES))) return rc;
    R.ctr = E.counters.as<unsigned long long>();
    R.h_flt[0] = R.n_seeds;
    const ContigTab ct(ctx->contigs.dev.p, R.n_contigs);      // (meme_chain_run has just asked for it: the table of this call's contigs)
    ExtArgs& A = R.A;
    memset(&A, 0, sizeof(A));
    A.reads = ctx->batch.reads.as<const uint8_t>(); A.read_off = ctx->batch.read_off.as<const i64>(); A.g0 = 0; A.ns = R.n;
    A.chain_off = C.chain_off(); A.chains = C.chains.as<const meme_chain>(); A.seed_off = C.seed_off(R.n); A.seeds = C.seeds.as<const meme_chain_seed>(); A.frac_rep = C.frac.as<const float>();
    A.pac = ctx->idx.pac; A.l_pac = R.copt->l_pac;
    A.contig_off = ct.off; A.contig_len = ct.len;
    A.o = *R.eopt;
    return MEME_OK;
}
// behind the filter: the records, the extension order and the per-read counts; the banded-SW options of the two sides
int ext_workspace(ExtRun& R) {
    meme_ctx* ctx = R.ctx;
    ExtWs& E = ctx->ext;
    const meme_ext_opt* eopt = R.eopt;
    ExtArgs& A = R.A;
    int rc;
    if ((rc = meme_buf_reserve(ctx, E.rmax, (size_t)(R.n_chains + 1) * 16)) || (rc = meme_buf_reserve(ctx, E.regs, (size_t)(R.n_seeds + 1) * sizeof(meme_alnreg))) ||
        (rc = meme_buf_reserve(ctx, E.order, (size_t)(R.n_seeds + 1) * 4)) || (rc = meme_buf_reserve(ctx, E.counts, ExtCounts(nullptr, R.n).bytes))) return rc;
    R.ec = ExtCounts(E.counts.p, R.n);
    A.rmax = E.rmax.as<i64>(); A.regs = E.regs.as<meme_alnreg>(); A.order = E.order.as<int>();
    A.cntL = R.ec.cnt[EXT_L]; A.cntR = R.ec.cnt[EXT_R]; A.cntB = R.ec.cnt[EXT_B];
    meme_bsw_opt& bl = R.bsw[0];
    memset(&bl, 0, sizeof(bl));
    bl.o_del = eopt->o_del; bl.e_del = eopt->e_del; bl.o_ins = eopt->o_ins; bl.e_ins = eopt->e_ins; bl.zdrop = eopt->zdrop; bl.a = eopt->a; bl.b = eopt->b;
    R.bsw[1] = bl;
    R.bsw[0].end_bonus = eopt->pen_clip5;
    R.bsw[1].end_bonus = eopt->pen_clip3;
    if (ctx->ext_census) HIP_TRY(hipMemsetAsync(R.ctr + EXT_CTR_CENSUS, 0, 11 * 8, ctx->stream));
    return MEME_OK;
}
PurgeArgs purge_args(const ExtRun& R) {      // the purge's view of the same arrays
    const ExtArgs& A = R.A;
    PurgeArgs P;
    P.read_off = A.read_off; P.nreads = R.n; P.chain_off = A.chain_off; P.chains = A.chains; P.seed_off = A.seed_off; P.seeds = A.seeds; P.regs = A.regs; P.order = A.order; P.o = *R.eopt;
    return P;
}
// mem_flt_chained_seeds: the read lengths it runs for and their thresholds, evaluated the way the reference's host code does (:579-583: float coefficients, double min_l,
// libm's log; never with reads below ~760 bases unless -W is given); the windows posed, aligned (seed SW), the seeds below their bar taken out of their chains: the stage goes
// on with the seeds, offsets and scores the filter made
int ext_filter(ExtRun& R) {
    meme_ctx* ctx = R.ctx;
    ExtWs& E = ctx->ext;
    const i64 n = R.n, n_seeds = R.n_seeds, max_len = ctx->batch.last_seed_max_len;
    bool flt = false;
    std::vector<int> hsp((size_t)max_len + 2, -1);
    for (i64 l = 2; l <= max_len; ++l) {
        const int l_query = (int)l;
        const double min_l = R.copt->min_chain_weight ? 1.1f * R.copt->min_chain_weight : 5.5f * log(l_query);     // MEM_HSP_COEF, MEM_MINSC_COEF (:252-253)
        if (min_l > 0.05f * l_query) continue;                                                                        // MEM_SEEDSW_COEF (:254)
        hsp[(size_t)l] = (int)(R.eopt->a * min_l + .499);
        if (hsp[(size_t)l] < 0) hsp[(size_t)l] = 0;
        flt = true;
    }
    if (!flt || n_seeds <= 0) return MEME_OK;
    if (n_seeds >= 0x7fffffff) { meme_set_error("meme_extend_last_batch_host: %lld chained seeds in one batch", (long long)n_seeds); return MEME_E_CAPACITY; }
    int rc;
    if ((rc = meme_buf_reserve(ctx, E.flt_sc, (size_t)(n_seeds + 1) * 4)) || (rc = meme_buf_reserve(ctx, E.flt_jobs, (size_t)(n_seeds + 1) * sizeof(meme_seedsw_job))) ||
        (rc = meme_buf_reserve(ctx, E.flt_cnt, CountScan(nullptr, n).bytes)) || (rc = meme_buf_reserve(ctx, E.flt_seeds, (size_t)(n_seeds + 1) * sizeof(meme_chain_seed))) ||
        (rc = meme_buf_reserve(ctx, E.flt_score, (size_t)(n_seeds + 1) * 4)) || (rc = meme_buf_reserve(ctx, E.flt_hsp, hsp.size() * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(E.flt_hsp.p, hsp.data(), hsp.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(R.ctr + EXT_CTR_FLT_JOBS, 0, 8, ctx->stream));
    const CountScan fc(E.flt_cnt.p, n);
    FltArgs F;
    memset(&F, 0, sizeof(F));
    F.read_off = R.A.read_off; F.n = n; F.chain_off = R.A.chain_off; F.chains = ctx->chain.chains.as<meme_chain>(); F.seed_off = R.A.seed_off; F.seeds = R.A.seeds;
    F.l_pac = R.A.l_pac; F.contig_off = R.A.contig_off; F.contig_len = R.A.contig_len; F.n_contigs = R.n_contigs;
    F.hsp = E.flt_hsp.as<const int>(); F.a = R.eopt->a; F.sc = E.flt_sc.as<int>(); F.jobs = E.flt_jobs.as<meme_seedsw_job>(); F.n_jobs = R.ctr + EXT_CTR_FLT_JOBS;
    F.cnt = fc.cnt; F.off2 = fc.off; F.seeds2 = E.flt_seeds.as<meme_chain_seed>(); F.score2 = E.flt_score.as<int>();
    hipLaunchKernelGGL(k_flt_pose, dim3((unsigned)n), dim3(64), 0, ctx->stream, F);
    if ((rc = meme_seedsw_launch(ctx, F.jobs, F.n_jobs, n_seeds, F.sc, R.eopt))) return rc;
    hipLaunchKernelGGL((k_flt_apply<false>), dim3((unsigned)n), dim3(64), 0, ctx->stream, F);
    if ((rc = meme_scan_exclusive(ctx, fc.cnt, fc.off, n))) return rc;
    hipLaunchKernelGGL((k_flt_apply<true>), dim3((unsigned)n), dim3(64), 0, ctx->stream, F);
    HIP_TRY(hipGetLastError());
    R.A.seed_off = F.off2; R.A.seeds = F.seeds2; R.A.seed_score = F.score2;
    R.flt_read = false;
    return MEME_OK;
}
// light and heavy reads (tuning "ext_split"): the list of reads with more than EXT_LIGHT chained seeds; everything else runs eight lanes per read
int ext_split(ExtRun& R) {
    meme_ctx* ctx = R.ctx;
    if (!ctx->ext_split) return MEME_OK;
    int rc;
    if ((rc = meme_buf_reserve(ctx, ctx->ext.heavy, (size_t)(R.n + 1) * 8))) return rc;
    unsigned long long* d_nheavy = R.ctr + EXT_CTR_HEAVY;
    HIP_TRY(hipMemsetAsync(d_nheavy, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_ext_split, dim3(grid_blocks(R.n, 256)), dim3(256), 0, ctx->stream, R.A.seed_off, R.n, ctx->ext.heavy.as<i64>(), d_nheavy);
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, d_nheavy, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    R.n_heavy = (i64)h; R.d_heavy = ctx->ext.heavy.as<const i64>();
    return MEME_OK;
}
// A kernel that walks reads (k_ext_jobs, k_ext_advance; k64 / k8: its G = 64 and G = 8 instances) over `ns` reads: one launch of a wavefront per read, or -- tuning
// "ext_split", and the reads are the whole batch -- eight lanes per light read + a wavefront per read of the heavy list
template <class Args> void launch_walk(const ExtRun& R, void (*k64)(Args), void (*k8)(Args), Args X, i64 ns, bool whole_batch) {
    const hipStream_t st = R.ctx->stream;
    X.list = nullptr; X.nlist = 0; X.light = 0;
    if (!(R.ctx->ext_split && whole_batch)) { hipLaunchKernelGGL(k64, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, st, X); return; }
    X.light = 1;
    hipLaunchKernelGGL(k8, dim3((unsigned)((ns + 31) / 32)), dim3(256), 0, st, X);
    if (R.n_heavy > 0) { X.light = 0; X.list = R.d_heavy; X.nlist = R.n_heavy; hipLaunchKernelGGL(k64, dim3((unsigned)((R.n_heavy + 3) / 4)), dim3(256), 0, st, X); }
}
void launch_jobs(const ExtRun& R, const ExtArgs& X, bool write) {      // the reads [X.g0, X.g0 + X.ns)
    void (*const k64)(ExtArgs) = write ? k_ext_jobs<true, 64> : k_ext_jobs<false, 64>;
    void (*const k8)(ExtArgs) = write ? k_ext_jobs<true, 8> : k_ext_jobs<false, 8>;
    launch_walk(R, k64, k8, X, X.ns, X.g0 == 0 && X.ns == R.n);
}
// the plan of the seeds `A.mode` / `A.sel` name: job and byte counts of every read (in rounds k_ext_advance has counted), their scans and totals.
// *n_sel: what k_ext_advance selected for this round.  The filter's two totals ride along with the first plan's.
int ext_plan(ExtRun& R, i64* n_sel) {
    meme_ctx* ctx = R.ctx;
    int rc;
    if (R.A.mode != 2) launch_jobs(R, R.A, false);
    for (int k = 0; k < 3; ++k) if ((rc = meme_scan_exclusive(ctx, R.ec.cnt[k], R.ec.off[k], R.n))) return rc;      // (all three queued before the first total is fetched)
    for (int k = 0; k < 3; ++k) HIP_TRY(hipMemcpyAsync(&R.tot[k], R.ec.off[k] + R.n, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (n_sel && (rc = meme_scan_total(ctx, R.ec.cntS, R.ec.offS, R.n, n_sel))) return rc;
    if (!R.flt_read) {
        HIP_TRY(hipMemcpyAsync(&R.h_flt[0], R.A.seed_off + R.n, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(&R.h_flt[1], R.ctr + EXT_CTR_FLT_JOBS, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    R.flt_read = true;
    return MEME_OK;
}
// Slabs: runs of whole reads whose jobs stay within lim[k] per column, at least one read each.  off[k][0..n]: the plan's scans, so reads [g0, g) hold off[k][g] - off[k][g0].
bool slab_fits(const i64* const off[3], const i64 lim[3], i64 g0, i64 g) { return off[0][g] - off[0][g0] <= lim[0] && off[1][g] - off[1][g0] <= lim[1] && off[2][g] - off[2][g0] <= lim[2]; }
i64 next_slab(const i64* const off[3], i64 n, i64 g0, const i64 lim[3]) {      // the end of the slab that starts at read g0
    i64 g1 = g0 + 1;
    while (g1 < n && slab_fits(off, lim, g0, g1 + 1)) {
        i64 step = 1;                               // gallop to the slab's end
        while (g1 + 2 * step < n && slab_fits(off, lim, g0, g1 + 2 * step + 1)) step *= 2;
        g1 += step;
    }
    return g1;
}
// one slab: its jobs and their sequences written (SeqPair offsets are 32-bit: they count from the slab's first job and byte), the census, then banded SW left and right with
// the band doubled once where the reference doubles it, results folded into the records
int ext_slab(ExtRun& R, const Slab& S) {
    meme_ctx* ctx = R.ctx;
    ExtWs& E = ctx->ext;
    const i64 nL = S.n[EXT_L], nR = S.n[EXT_R], nmax = nL > nR ? nL : nR;
    int rc;
    if ((rc = meme_buf_reserve(ctx, E.pairs_l, (size_t)(nL + 1) * sizeof(meme_seqpair))) || (rc = meme_buf_reserve(ctx, E.pairs_r, (size_t)(nR + 1) * sizeof(meme_seqpair))) ||
        (rc = meme_buf_reserve(ctx, E.retry, ExtRetry(nullptr, nmax).bytes)) || (rc = meme_buf_reserve(ctx, E.seq, (size_t)S.n[EXT_B] + 256))) return rc;
    const ExtRetry retry(E.retry.p, nmax);
    ExtArgs X = R.A;
    X.g0 = S.g0; X.ns = S.g1 - S.g0;
    // (the scans cover the whole batch: a slab's first read has its own offsets to subtract)
    X.offL = R.ec.off[EXT_L] + S.g0; X.offR = R.ec.off[EXT_R] + S.g0; X.offB = R.ec.off[EXT_B] + S.g0;
    X.job0L = S.first[EXT_L]; X.job0R = S.first[EXT_R]; X.byte0 = S.first[EXT_B];
    X.L = E.pairs_l.as<meme_seqpair>(); X.R = E.pairs_r.as<meme_seqpair>(); X.seq = E.seq.as<uint8_t>();
    launch_jobs(R, X, true);
    HIP_TRY(hipGetLastError());
    unsigned long long *d_census = R.ctr + EXT_CTR_CENSUS, *d_nretry = R.ctr + EXT_CTR_RETRY;
    if (ctx->ext_census) {
        if (nL) hipLaunchKernelGGL(k_ext_census, dim3(grid_blocks(nL, 256)), dim3(256), 0, ctx->stream, (const meme_seqpair*)X.L, nL, (const uint8_t*)X.seq, R.eopt->w, d_census);
        if (nR) hipLaunchKernelGGL(k_ext_census, dim3(grid_blocks(nR, 256)), dim3(256), 0, ctx->stream, (const meme_seqpair*)X.R, nR, (const uint8_t*)X.seq, R.eopt->w, d_census);
    }
    for (int dir = 0; dir < 2; ++dir) {
        meme_seqpair* P = dir == 0 ? X.L : X.R;
        i64 np = dir == 0 ? nL : nR;
        if (dir == 1 && np > 0) hipLaunchKernelGGL(k_ext_h0, dim3(grid_blocks(np, 256)), dim3(256), 0, ctx->stream, P, np, (const meme_alnreg*)X.regs);
        for (int attempt = 0; attempt < EXT_BAND_TRIES && np > 0; ++attempt) {
            const int w = R.eopt->w << attempt;
            if ((rc = meme_bsw_launch(ctx, P, X.seq, X.seq, (int)np, w, &R.bsw[dir], (int)ctx->batch.last_seed_max_len))) return rc;
            HIP_TRY(hipMemsetAsync(d_nretry, 0, 8, ctx->stream));
            FoldArgs F;
            F.pairs = P; F.n = np; F.regs = X.regs; F.chains = X.chains; F.seed_off = X.seed_off; F.seeds = X.seeds; F.read_off = X.read_off;
            F.o = *R.eopt; F.w = w; F.last = attempt + 1 == EXT_BAND_TRIES;
            F.retry = retry.half[attempt & 1]; F.n_retry = d_nretry;
            if (dir == 0) hipLaunchKernelGGL((k_ext_fold<true>), dim3(grid_blocks(np, 256)), dim3(256), 0, ctx->stream, F);
            else hipLaunchKernelGGL((k_ext_fold<false>), dim3(grid_blocks(np, 256)), dim3(256), 0, ctx->stream, F);
            unsigned long long h_retry = 0;
            HIP_TRY(hipMemcpyAsync(&h_retry, d_nretry, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            { float ms = 0.f; if (meme_bsw_last_ms(ctx, &ms) == hipSuccess) R.bsw_ms += ms; }
            R.n_pairs += np; ++R.n_calls;
            if (attempt > 0) R.n_retried += np;
            P = F.retry;
            np = (i64)h_retry;
        }
    }
    return MEME_OK;
}
// the planned jobs, slab after slab.  One slab takes the whole batch unless its jobs exceed the ctx's ext_slab_jobs per side or ext_slab_bytes of sequence;
// only then do the per-read offsets cross to the host.
int ext_slabs(ExtRun& R) {
    meme_ctx* ctx = R.ctx;
    const i64 n = R.n, lim[3] = {ctx->ext_slab_jobs, ctx->ext_slab_jobs, ctx->ext_slab_bytes};
    if (R.tot[EXT_L] + R.tot[EXT_R] == 0) return MEME_OK;
    int rc;
    if (R.tot[EXT_L] <= lim[EXT_L] && R.tot[EXT_R] <= lim[EXT_R] && R.tot[EXT_B] <= lim[EXT_B]) return ext_slab(R, Slab{0, n, {R.tot[0], R.tot[1], R.tot[2]}, {0, 0, 0}});
    if (!R.ec.adjacent(n)) { meme_set_error("meme_extend_last_batch_host: the offset columns of ExtCounts are not adjacent"); return MEME_E_STATE; }
    R.h_off.resize((size_t)(3 * (n + 1)));
    HIP_TRY(hipMemcpyAsync(R.h_off.data(), R.ec.off[0], R.h_off.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const i64* const off[3] = {R.h_off.data(), R.h_off.data() + (n + 1), R.h_off.data() + 2 * (n + 1)};
    for (i64 g0 = 0; g0 < n;) {
        Slab S;
        S.g0 = g0; S.g1 = next_slab(off, n, g0, lim);
        for (int k = 0; k < 3; ++k) { S.n[k] = off[k][S.g1] - off[k][g0]; S.first[k] = off[k][g0]; }
        if (S.n[EXT_B] >= ((i64)1 << 31)) { meme_set_error("a read's extension jobs need more than 2 GiB of sequence"); return MEME_E_CAPACITY; }
        if ((rc = ext_slab(R, S))) return rc;
        g0 = S.g1;
    }
    return MEME_OK;
}
// the reference's batch: every chained seed extended, then the purge
int ext_batch(ExtRun& R) {
    int rc;
    R.A.mode = 0;
    if ((rc = ext_plan(R, nullptr)) || (rc = ext_slabs(R))) return rc;
    hipLaunchKernelGGL(k_ext_purge, dim3((unsigned)((R.n + 3) / 4)), dim3(256), 0, R.ctx->stream, purge_args(R));
    HIP_TRY(hipGetLastError());
    R.n_seeds_ext = R.h_flt[0];
    return MEME_OK;
}
// in rounds (see k_ext_advance): records + extension order first, then `rounds` rounds of one seed per read, one round with everything still ahead
int ext_rounds(ExtRun& R, i64 rounds) {
    meme_ctx* ctx = R.ctx;
    ExtArgs& A = R.A;
    int rc;
    if ((rc = meme_buf_reserve(ctx, ctx->ext.rounds, ExtRounds(nullptr, R.n, R.n_seeds).bytes))) return rc;
    const ExtRounds er(ctx->ext.rounds.p, R.n, R.n_seeds);
    AdvArgs V;
    V.P = purge_args(R); V.state = er.state; V.act = er.act; V.sel = er.sel; V.cntS = R.ec.cntS;
    V.rmax = A.rmax; V.cntL = A.cntL; V.cntR = A.cntR; V.cntB = A.cntB;
    A.mode = 1; A.state = V.state;
    launch_jobs(R, A, true);
    A.sel = V.sel; A.act = V.act;
    for (i64 t = 0; t <= rounds; ++t) {
        HIP_TRY(hipMemsetAsync(V.sel, 0, (size_t)R.n_seeds, ctx->stream));
        V.mode = t < rounds ? ADV_ONE : ADV_REST;
        launch_walk(R, k_ext_advance<64>, k_ext_advance<8>, V, R.n, true);
        A.mode = 2;
        i64 h_sel = 0;
        if ((rc = ext_plan(R, &h_sel)) || (rc = ext_slabs(R))) return rc;
        R.n_seeds_ext += h_sel;
        if (h_sel == 0) break;                      // every read has been walked to its end
    }
    V.mode = ADV_FINISH;
    launch_walk(R, k_ext_advance<64>, k_ext_advance<8>, V, R.n, true);
    HIP_TRY(hipGetLastError());
    return MEME_OK;
}
// hand-over: one record per chained seed, or (tuning "ext_live_only") the surviving ones counted, packed and copied; then the result
int ext_hand_over(ExtRun& R, meme_ext_host_result* out) {
    meme_ctx* ctx = R.ctx;
    ExtWs& E = ctx->ext;
    const i64 n = R.n, n_seeds = R.h_flt[0];        // chained seeds behind the filter
    const meme_alnreg* regs = R.A.regs;
    int rc;
    if ((rc = meme_hostbuf_reserve(ctx, E.h_reg_off, (size_t)(n + 1) * 8))) return rc;
    i64 n_out = n_seeds;                            // records that cross to the host
    if (ctx->ext_live_only) {
        if ((rc = meme_buf_reserve(ctx, E.live_cnt, CountScan(nullptr, n).bytes))) return rc;
        const CountScan lc(E.live_cnt.p, n);
        hipLaunchKernelGGL(k_ext_live_count, dim3(grid_blocks(n, 256)), dim3(256), 0, ctx->stream, R.A.seed_off, regs, n, lc.cnt);
        if ((rc = meme_scan_exclusive(ctx, lc.cnt, lc.off, n))) return rc;
        HIP_TRY(hipMemcpyAsync(E.h_reg_off.p, lc.off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        n_out = E.h_reg_off.as<const i64>()[n];
        if ((rc = meme_buf_reserve(ctx, E.live_regs, (size_t)(n_out + 1) * sizeof(meme_alnreg))) || (rc = meme_hostbuf_reserve(ctx, E.h_regs, (size_t)(n_out + 1) * sizeof(meme_alnreg)))) return rc;
        hipLaunchKernelGGL(k_ext_live_pack, dim3(grid_blocks(n, 256)), dim3(256), 0, ctx->stream, R.A.seed_off, regs, n, (const i64*)lc.off, E.live_regs.as<meme_alnreg>());
        HIP_TRY(hipGetLastError());
        if (n_out) HIP_TRY(hipMemcpyAsync(E.h_regs.p, E.live_regs.p, (size_t)n_out * sizeof(meme_alnreg), hipMemcpyDeviceToHost, ctx->stream));
    } else {
        if ((rc = meme_hostbuf_reserve(ctx, E.h_regs, (size_t)(n_seeds + 1) * sizeof(meme_alnreg)))) return rc;
        HIP_TRY(hipMemcpyAsync(E.h_reg_off.p, R.A.seed_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (n_seeds) HIP_TRY(hipMemcpyAsync(E.h_regs.p, regs, (size_t)n_seeds * sizeof(meme_alnreg), hipMemcpyDeviceToHost, ctx->stream));
    }
    unsigned long long h_census[11] = {0};
    if (ctx->ext_census) HIP_TRY(hipMemcpyAsync(h_census, R.ctr + EXT_CTR_CENSUS, 11 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    out->n_exact_prefix = ctx->ext_census ? (int64_t)h_census[0] : -1;
    out->census_band_cells = ctx->ext_census ? (int64_t)h_census[1] : -1;
    for (int c = 0; c < 9; ++c) out->census_class[c] = ctx->ext_census ? (int64_t)h_census[2 + c] : -1;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, E.ev[0], E.ev[1]));
    out->nreads = n; out->reg_off = E.h_reg_off.as<const int64_t>(); out->regs = E.h_regs.as<const meme_alnreg>(); out->total_regs = n_out; out->total_seeds = n_seeds; out->n_ext_seeds = R.n_seeds_ext;
    out->total_chains = R.n_chains; out->n_pairs = R.n_pairs; out->n_retried = R.n_retried; out->n_bsw_calls = R.n_calls;
    out->n_flt_jobs = R.h_flt[1]; out->n_flt_dropped = R.n_seeds - n_seeds;
    out->n_tier2 = ctx->tm.chain_tier2_reads; out->chain_ms = ctx->tm.chain_kernel_ms; out->ext_ms = ms; out->bsw_ms = R.bsw_ms;
    return MEME_OK;
}

}  // namespace

extern "C" int meme_extend_last_batch_host(meme_ctx* ctx, const meme_contig* contigs, int32_t n_contigs, const meme_chain_opt* copt,
                                           const meme_ext_opt* eopt, meme_ext_host_result* out) {
    int rc;
    if ((rc = ext_check(ctx, contigs, n_contigs, copt, eopt, out))) return rc;
    i64 tot[2];
    if ((rc = meme_chain_run(ctx, contigs, n_contigs, copt, tot))) return rc;
    ExtRun R;
    R.ctx = ctx; R.copt = copt; R.eopt = eopt; R.n_contigs = n_contigs;
    R.n = ctx->batch.last_seed_reads; R.n_chains = tot[0]; R.n_seeds = tot[1];
    if ((rc = ext_begin(R)) || (rc = ext_filter(R)) || (rc = ext_workspace(R)) || (rc = ext_split(R))) return rc;
    const i64 rounds = ctx->ext_live_only ? ctx->ext_rounds : 0;
    if ((rc = rounds <= 0 ? ext_batch(R) : ext_rounds(R, rounds))) return rc;
    HIP_TRY(hipEventRecord(ctx->ext.ev[1], ctx->stream));
    return ext_hand_over(R, out);
}
