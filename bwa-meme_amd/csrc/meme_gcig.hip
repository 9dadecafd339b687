// Banded global alignment with traceback -- the CIGAR kernel of the SAM phase: ksw_global2 (reference src/ksw.cpp:560-670)
// as bwa_gen_cigar2 (src/bwa.cpp:274-362) calls it from mem_reg2aln (src/bwamem.cpp:2314-2380) for every alignment that is written out.
//
// One wavefront per alignment; the lanes take the query columns of the band (64 at a time), the target rows run in sequence:
//   M(i,j)   = H(i-1,j-1) + S(i,j)                         lane-parallel (H of the row above, shifted by one column, in LDS)
//   E(i+1,j) = max{M(i,j) - gapo_del, E(i,j)} - gape_del    lane-parallel (E stays with its column)
//   F(i,j+1) = max{M(i,j) - gapo_ins, F(i,j)} - gape_ins    along the row: a max-plus prefix scan over the lanes, carried across chunks
//   H(i,j)   = max{M, E, F}; the direction byte of the cell (h from M/E/F, e opened or extended, f opened or extended) goes to the
//   backtrack matrix exactly as the reference stores it, and the backtrack walks it the reference's way -- so that ties (M over E over F)
//   and with them the placement of gaps in the CIGAR come out the same.
// What decides that placement is not stated here: the scoring entry, bwa_gen_cigar2's band, the band of a row and the borders of the matrix, the cell,
// the walk back and the writer of its operations are meme_gcig_rules.h (plain values; tests/test_gcig_rules_model.py runs them on the CPU), and
// both DP kernels, k_cjob_prep and k_gcig_nogap call them.  This file holds what needs the lanes, once each: F's scan (gcig_fscan), the NM / MD
// emitter (gcig_md) and the decimal writer (gcig_put_num); and where each kernel keeps H, E, the sequences and the direction bytes.
// Sequences are not shipped: a job names a read of the batch resident on the ctx, its query span, and a span of the fwd+rc text (2-bit
// pac64 in HBM); alignments on the reverse strand have both sequences reversed, as bwa_gen_cigar2 does to keep gaps left-aligned.
#include <string.h>

#include "meme_common.h"
#include "meme_gcig_rules.h"

namespace {

struct GcigArgs {
    const meme_gjob* jobs; i64 njobs;
    const uint8_t* reads; const i64* read_off; const u64* pac;
    meme_bsw_opt o;                          // o_del, e_del, o_ins, e_ins, a, b (zdrop / end_bonus unused)
    const i64* zoff; uint8_t* z;             // backtrack matrices: n_col * tlen bytes per job
    const i64* coff; uint32_t* cig;          // CIGAR scratch: qlen + tlen + 2 operations per job, filled from the back
    meme_gres* res;                          // score, n_cigar, (cigar_off = first operation inside the job's scratch, for the pack kernel)
    // bwa_gen_cigar2 whole (meme_gen_cigar_batch_host): NM and the MD string of every job; null for the plain ksw_global2 call
    const i64* mdoff; char* md;              // MD scratch: 2 * (qlen + tlen) + 16 bytes per job
    int32_t* nm; int32_t* mdlen;
    int zcap;                                // backtrack matrices of at most this many bytes stay in LDS (0: all in global memory)
    const i64* dp_list;                      // jobs that need the kernel below (the rest were answered by k_gcig_nogap), or null: all
    i64 list_first;                          // k_gcig / k_gcig_grp: this launch's jobs are dp_list[list_first ..) (the list is ordered by class: 16-lane, 32-lane, whole wavefront)
    int grp_qcap, grp_tcap, grp_z;           // k_gcig_grp: bytes of LDS per group for the query, the target and the backtrack matrix
    const u64* packed; int pW, pMW, pstride; // the batch's packed reads (2 bits per base + N masks, k_pack_reads): what k_gcig_nogap compares
};

// F's scan (gcig_scan_key / gcig_scan_f of the rules): the maximum of the keys of the lanes BELOW each lane of a group of G (a group's lane 0 does not use
// it), in the register file: row_shr 1/2/4/8, row_bcast15 into rows 1,3 (G >= 32), row_bcast31 into rows 2,3 (G == 64), then wave_shr:1 -- as ds_bpermute
// shuffles the eight steps were eight LDS round trips on the row's dependent chain, 1 000 of its 1 200 cycles.  Every lane of the wavefront takes part.
#define GCIG_DPP(src_, ctrl_, rowmask_) __builtin_amdgcn_update_dpp(GCIG_SCAN_FLOOR, (src_), (ctrl_), (rowmask_), 0xF, false)
template <int G>
__device__ __forceinline__ int gcig_fscan(int key) {
    int sg = key, y;
    y = GCIG_DPP(sg, 0x111, 0xF); sg = sg > y ? sg : y;
    y = GCIG_DPP(sg, 0x112, 0xF); sg = sg > y ? sg : y;
    y = GCIG_DPP(sg, 0x114, 0xF); sg = sg > y ? sg : y;
    y = GCIG_DPP(sg, 0x118, 0xF); sg = sg > y ? sg : y;
    if (G >= 32) { y = GCIG_DPP(sg, 0x142, 0xA); sg = sg > y ? sg : y; }
    if (G == 64) { y = GCIG_DPP(sg, 0x143, 0xC); sg = sg > y ? sg : y; }
    return GCIG_DPP(sg, 0x138, 0xF);
}

// kputw: v >= 0 in decimal at out[len ..), written where `store`; returns the number of its digits
__device__ __forceinline__ int gcig_put_num(char* out, int len, int v, bool store) {
    char buf[12];
    int l = 0;
    do { buf[l++] = (char)('0' + v % 10); v /= 10; } while (v);
    if (store) for (int i = 0; i < l; ++i) out[len + i] = buf[l - 1 - i];
    return l;
}

// NM and MD (src/bwa.cpp:322-355) by a group of G lanes (lane gl of the group whose first lane is gbase; gmask: G ones) from a job's n operations in
// CIGAR order over the (possibly reversed) query qs and target tbase(position).  Matches are compared G bases at a time -- one ballot, then only the
// mismatches are visited --, deleted bases are written by the lanes side by side; the text of the string is identical on every lane of the group, the lane
// with `store` writes it.
struct GcigMd { int nm, len; };
template <int G, class T>
__device__ __forceinline__ GcigMd gcig_md(const uint32_t* ops, int n, const uint8_t* qs, T&& tbase, bool rev, int gl, int gbase, unsigned long long gmask, bool store, char* out) {
    const char* const b2c = rev ? "TGCAN" : "ACGTN";
    int len = 0, x = 0, y = 0, u = 0, n_mm = 0, n_gap = 0;
    for (int k = 0; k < n; ++k) {
        const int op = (int)(ops[k] & 0xf), l = (int)(ops[k] >> 4);
        if (op == 0) {
            for (int i0 = 0; i0 < l; i0 += G) {
                const int i = i0 + gl;
                const bool in = i < l;
                int tb = 0, qb = 0;
                if (in) { tb = tbase(y + i); qb = qs[x + i]; }
                unsigned long long mask = (__ballot(in && tb != qb) >> gbase) & gmask;
                int pos0 = 0;
                while (mask) {
                    const int b = __builtin_ctzll(mask);
                    u += b - pos0;
                    len += gcig_put_num(out, len, u, store);
                    const int t = __shfl(tb, gbase + b);
                    if (store) out[len] = b2c[t];
                    ++len; ++n_mm; u = 0; pos0 = b + 1;
                    mask &= mask - 1;
                }
                u += (l - i0 < G ? l - i0 : G) - pos0;
            }
            x += l; y += l;
        } else if (op == 2) {
            if (k > 0 && k < n - 1) {        // (a deletion at either end of the CIGAR is not reported: mem_reg2aln squeezes it out)
                len += gcig_put_num(out, len, u, store);
                if (store) out[len] = '^';
                ++len;
                for (int i = gl; i < l; i += G) out[len + i] = b2c[tbase(y + i)];
                len += l; u = 0; n_gap += l;
            }
            y += l;
        } else { x += l; n_gap += l; }
    }
    len += gcig_put_num(out, len, u, store);
    if (store) out[len] = 0;
    return {n_mm + n_gap, len};
}

// The whole-wavefront kernel described above (`k_gcig` in the comments of this file).
__global__ void __launch_bounds__(64) k_gcig_t(GcigArgs A) {
    extern __shared__ int lds[];             // hA[qlen + 2] | hB[qlen + 2] | e[qlen + 2] | query bytes (as ints, 4 per word)
    if ((i64)blockIdx.x >= A.njobs) return;
    const i64 jb = A.dp_list ? A.dp_list[A.list_first + blockIdx.x] : (i64)blockIdx.x;
    const int lane = threadIdx.x;
    const meme_gjob J = A.jobs[jb];
    const int qlen = J.qlen, tlen = J.tlen, w = J.w;
    int* hA = lds;
    int* hB = hA + qlen + 2;
    int* eE = hB + qlen + 2;
    uint8_t* qs = reinterpret_cast<uint8_t*>(eE + qlen + 2);
    uint8_t* ts = qs + ((qlen + 3) & ~3);    // the target bases in row order: a row must not wait for a load from the text (1-2 us each, 250 in a row)
    uint8_t* zl = ts + ((tlen + 3) & ~3);    // the backtrack matrix, when it fits (A.zcap bytes): the walk back is one dependent load per step
    const uint8_t* rd = A.reads + A.read_off[J.read] + J.qb;
    const auto text_at = [&](int p) -> int { return text_base(A.pac, J.rev ? J.rb + tlen - 1 - p : J.rb + p); };
    const auto tbase = [&](int p) -> int { return w >= 0 ? (int)ts[p] : text_at(p); };      // (the gap-free shortcut does not load ts)
    for (int j = lane; j < qlen; j += 64) qs[j] = J.rev ? rd[qlen - 1 - j] : rd[j];
    if (w >= 0) for (int i = lane; i < tlen; i += 64) ts[i] = (uint8_t)text_at(i);
    GcigOps ops{A.cig + A.coff[jb], qlen + tlen + 2, true};      // every lane the same walk, every lane stores the same words
    int score;
    if (w < 0) {
        // bwa_gen_cigar2's gap-free shortcut (src/bwa.cpp:295-304: equal lengths and w_ == 0): one M operation, the score summed
        __syncthreads();
        int part = 0;
        for (int j = lane; j < qlen; j += 64) part += gcig_score(text_at(j), qs[j], A.o.a, A.o.b);
        for (int d = 32; d; d >>= 1) part += __shfl_xor(part, d);
        score = part;
        ops.push(0, qlen);
        ops.flush();
    } else {
    const int oe_del = A.o.o_del + A.o.e_del, oe_ins = A.o.o_ins + A.o.e_ins, e_del = A.o.e_del, e_ins = A.o.e_ins;
    const int n_col = gcig_n_col(qlen, w);
    uint8_t* z = (i64)n_col * tlen <= A.zcap ? zl : A.z + A.zoff[jb];
    int* hp = hA;                            // H(i-1, j-1) at [j]
    int* hn = hB;
    for (int j = lane; j <= qlen; j += 64) {
        hA[j] = gcig_row0(j, w, A.o.o_ins, e_ins);
        eE[j] = GCIG_MINUS_INF;
    }
    __syncthreads();
    for (int i = 0; i < tlen; ++i) {
        const int tb = ts[i];
        const int beg = gcig_beg(i, w), end = gcig_end(i, w, qlen);
        int f_in = GCIG_MINUS_INF;                                    // F(i, first column of the chunk)
        const int h_in = gcig_left(i, beg, A.o.o_del, e_del);
        if (lane == 0 && beg <= qlen) hn[beg] = h_in;                 // (beg > qlen cannot happen for bands the host check admits: w >= |tlen - qlen|)
        uint8_t* zi = z + (i64)i * n_col;
        for (int cb = beg; cb < end; cb += 64) {
            const int j = cb + lane;
            const bool in = j < end;
            int m = GCIG_MINUS_INF, e = GCIG_MINUS_INF;
            if (in) {
                m = hp[j] + gcig_score(tb, qs[j], A.o.a, A.o.b);
                e = eE[j];
            }
            const int f = gcig_scan_f(gcig_fscan<64>(gcig_scan_key(in, m, oe_ins, e_ins, lane)), f_in, e_ins, lane);
            const GcigCell c = gcig_cell(m, e, f, oe_del, e_del, oe_ins, e_ins);
            if (in) { eE[j] = c.e; hn[j + 1] = c.h; zi[j - beg] = (uint8_t)c.d; }
            f_in = __builtin_amdgcn_readlane(c.f, 63);                // carry to the next chunk: F(i, cb + 64)
        }
        if (lane == 0) eE[end] = GCIG_MINUS_INF;                         // eh[end].e (:649); eh[end].h was stored by the row's last column
        __syncthreads();
        int* tsw = hp; hp = hn; hn = tsw;
    }
    score = hp[qlen];
    __threadfence();
    __syncthreads();
    // The walk is the same on every lane: the byte it reads goes through readfirstlane so that i, k, `which` and the addresses live in scalar
    // registers.  Measured (profiles/r05_gcig.md): 21-29 % fewer VALU instructions per job and NO change in the kernel's time -- so the kernel is not
    // bound by VALU issue; what it IS bound by is open (four explanations refuted, same file).  Kept because it is exact and costs nothing.
    // A matrix in global memory is walked through a window in LDS: the rows [win_lo, win_hi) the walk is about to cross are fetched by the
    // whole wavefront at once (a walk straight on HBM is 500 dependent loads of a microsecond each -- ten times the DP above it).  The refill's barriers
    // stand under conditions that are the same on every lane (zi comes from i, k and `which`), as the walk's loop does.
    const bool windowed = z != zl && A.zcap >= 2 * n_col + 8;
    const int win_rows = windowed ? (A.zcap - 8) / n_col : 0;
    i64 win_base = 0, win_b0 = (i64)n_col * tlen;        // zl[x - win_base] = z[x] for the bytes [win_b0, ..) of the window
    gcig_walk<i64>(tlen, qlen, w, n_col, [&](i64 zi) -> int {
        if (!windowed) return __builtin_amdgcn_readfirstlane((int)z[zi]);
        if (zi < win_b0) {
            __syncthreads();
            const int row = (int)(zi / n_col);      // (the walk's clamps can leave row i)
            const int win_lo = row - win_rows + 1 > 0 ? row - win_rows + 1 : 0;
            const i64 b0 = (i64)win_lo * n_col, b1 = (i64)(row + 1) * n_col;
            win_b0 = b0;
            const uint8_t* src = z + b0;
            const int shift = (int)(reinterpret_cast<uintptr_t>(src) & 3);      // dword loads from the aligned address below
            const unsigned* src4 = reinterpret_cast<const unsigned*>(src - shift);
            unsigned* dst4 = reinterpret_cast<unsigned*>(zl);
            const int nd = (int)((b1 - b0 + shift + 3) >> 2);
            for (int d = lane; d < nd; d += 64) dst4[d] = src4[d];
            win_base = b0 - shift;
            __syncthreads();
        }
        return __builtin_amdgcn_readfirstlane((int)zl[zi - win_base]);
    }, ops);
    }
    if (lane == 0) { meme_gres R; R.score = score; R.n_cigar = ops.n; R.cigar_off = ops.cigar_off(); A.res[jb] = R; }
    if (!A.md) return;
    __threadfence();
    __syncthreads();
    const GcigMd M = gcig_md<64>(ops.cg + ops.cigar_off(), ops.n, qs, tbase, J.rev != 0, lane, 0, ~0ull, lane == 0, A.md + A.mdoff[jb]);
    if (lane == 0) { A.nm[jb] = M.nm; A.mdlen[jb] = M.len; }
}

// Several jobs per wavefront (round 6).  k_gcig above gives a job all 64 lanes and runs its rows one after the other; the bands bwa_gen_cigar2
// computes for short reads are 5-15 columns wide, so ~9 of the 64 lanes work and the kernel's time follows its instruction count
// (profiles/r05_gcig.md).  Here a job whose band has at most G columns (G = 16, 32 or 64: one, two or four DPP rows; G = 64 is one job per wavefront
// again, without the chunk loop and with the rings) takes a GROUP of G lanes and a wavefront runs 64 / G jobs side by side: the same instruction
// stream, 4 or 2 jobs per instruction.  A row is ONE chunk (end - beg <= 2w + 1 <= G), so F's scan stays inside the group's DPP rows and carries
// nothing in.  H and E live in rings of 2G entries (a row reads what the row before wrote inside its band, never beyond: indices modulo the ring),
// the backtrack matrix (<= G x tlen bytes) always in LDS; the walk back runs per lane, identical within a group.  The rules, the scan and the
// emitter are k_gcig's -- so the same CIGAR, NM and MD.
template <int G>
__global__ void __launch_bounds__(64) k_gcig_grp(GcigArgs A) {
    extern __shared__ int lds[];
    constexpr int NG = 64 / G, R = 2 * G, RM = R - 1;
    constexpr unsigned long long GMASK = G == 64 ? ~0ull : G == 32 ? 0xffffffffull : 0xffffull;
    const int lane = threadIdx.x, sub = lane / G, gl = lane % G, gbase = sub * G;
    const i64 slot = (i64)blockIdx.x * NG + sub;
    const bool live = slot < A.njobs;
    const i64 jb = live ? A.dp_list[A.list_first + slot] : 0;
    meme_gjob J;
    if (live) J = A.jobs[jb];
    else { J.rb = 0; J.read = 0; J.qb = 0; J.qlen = 0; J.tlen = 0; J.w = 0; J.rev = 0; }
    const int qlen = J.qlen, tlen = J.tlen, w = J.w;
    const int stride = 3 * R + ((A.grp_qcap + A.grp_tcap + A.grp_z) >> 2);          // ints per group
    int* hA = lds + sub * stride;
    int* hB = hA + R;
    int* eE = hB + R;
    uint8_t* qs = reinterpret_cast<uint8_t*>(eE + R);
    uint8_t* ts = qs + A.grp_qcap;
    uint8_t* zl = ts + A.grp_tcap;
    if (live) {
        const uint8_t* rd = A.reads + A.read_off[J.read] + J.qb;
        // (the strand picks the 32-bit index, not one of two 64-bit addresses: in the loops' eight unrolled copies that is two VGPRs of the kernel)
        for (int j = gl; j < qlen; j += G) qs[j] = rd[J.rev ? qlen - 1 - j : j];
        for (int i = gl; i < tlen; i += G) ts[i] = (uint8_t)text_base(A.pac, J.rb + (J.rev ? tlen - 1 - i : i));
    }
    GcigOps ops{A.cig + (live ? A.coff[jb] : 0), qlen + tlen + 2, gl == 0};         // every lane of the group the same walk (a dead group: no cell, no operation)
    const int oe_del = A.o.o_del + A.o.e_del, oe_ins = A.o.o_ins + A.o.e_ins, e_del = A.o.e_del, e_ins = A.o.e_ins;
    const int n_col = gcig_n_col(qlen, w);
    // The first row: the columns row 0 can read.  The cells left of the band and E above a column the band has just reached are not kept in the rings: H(i-1, -1)
    // is arithmetic (gcig_corner) and E of a column at or beyond the previous row's end (gcig_end_above) is -inf -- two
    // single-lane stores per row less, and every load of a row is unconditional (lanes beyond the band compute on whatever the ring holds and store nothing).
    for (int j = gl + 1; j <= qlen && j <= w + 1; j += G) hA[j & RM] = gcig_row0(j, w, A.o.o_ins, e_ins);
    int tl_max = tlen;
    for (int d = 32; d >= G; d >>= 1) { const int o = __shfl_xor(tl_max, d); tl_max = tl_max > o ? tl_max : o; }
    __syncthreads();
    int* hp = hA;
    int* hn = hB;
    for (int i = 0; i < tl_max; ++i) {
        const bool row = i < tlen;
        const int tb = ts[i < tlen ? i : 0];
        const int beg = gcig_beg(i, w), end = gcig_end(i, w, qlen), end_prev = gcig_end_above(i, w, qlen);
        const int j = beg + gl;
        const bool in = row && j < end;
        const int qb = qs[j];
        const int hprev = hp[j & RM], eprev = eE[j & RM];
        const int sc = gcig_score(tb, qb, A.o.a, A.o.b);
        const int m = (j == 0 ? gcig_corner(i, A.o.o_del, e_del) : hprev) + sc;
        const int e = j >= end_prev ? GCIG_MINUS_INF : eprev;
        const int f = gcig_scan_f(gcig_fscan<G>(gcig_scan_key(in, m, oe_ins, e_ins, gl)), GCIG_MINUS_INF, e_ins, gl);
        const GcigCell c = gcig_cell(m, e, f, oe_del, e_del, oe_ins, e_ins);
        if (in) { eE[j & RM] = c.e; hn[(j + 1) & RM] = c.h; zl[i * n_col + gl] = (uint8_t)c.d; }
        __syncthreads();
        if (row) { int* tsw = hp; hp = hn; hn = tsw; }
    }
    const int score = live ? hp[qlen & RM] : 0;
    gcig_walk<int>(tlen, qlen, w, n_col, [&](int zi) -> int { return zl[zi]; }, ops);
    if (live && gl == 0) { meme_gres Rr; Rr.score = score; Rr.n_cigar = ops.n; Rr.cigar_off = ops.cigar_off(); A.res[jb] = Rr; }
    if (!A.md) return;
    __threadfence();
    __syncthreads();
    const GcigMd M = gcig_md<G>(ops.cg + ops.cigar_off(), ops.n, qs, [&](int p) -> int { return ts[p]; }, J.rev != 0, gl, gbase, GMASK, live && gl == 0,
                                A.md + (live ? A.mdoff[jb] : 0));
    if (live && gl == 0) { A.nm[jb] = M.nm; A.mdlen[jb] = M.len; }
}

// bwa_gen_cigar2's gap-free shortcut (src/bwa.cpp:295-304) for the jobs of a batch that take it, ONE LANE per job: the query span against
// the text 32 bases per XOR on the packed reads k_pack_reads left on the ctx (2 bits per base, N as A with a mask beside it) and the 2-bit
// text -- score, the one M operation, NM and the MD string (visited mismatch by mismatch, in the reversed order on the reverse strand).
// A batch of 150-bp reads with 1 % errors poses 70 % of its calls this way; a wavefront-wide block each (k_gcig) cost 70 ns per job.
constexpr int NOGAP_MAX_LEN = 500;           // reads beyond LEARNED_MAX_READ_LEN are not packed: k_gcig takes their jobs
__device__ __forceinline__ bool nogap_fast(const meme_gjob& J, const i64* read_off) {
    return J.w < 0 && read_off[J.read + 1] - read_off[J.read] <= NOGAP_MAX_LEN;
}
__global__ void __launch_bounds__(256) k_gcig_nogap(GcigArgs A) {
    for (i64 jb = (i64)blockIdx.x * blockDim.x + threadIdx.x; jb < A.njobs; jb += (i64)gridDim.x * blockDim.x) {
        const meme_gjob J = A.jobs[jb];
        if (!nogap_fast(J, A.read_off)) continue;
        const int qlen = J.qlen;
        const u64* fw = A.packed + (i64)J.read * A.pstride;
        const u64* nmask = fw + 2 * A.pW;
        const bool has_n = (fw[A.pstride - 1] >> 31) & 1ull;
        char* out = A.md ? A.md + A.mdoff[jb] : nullptr;
        const char* const b2c = J.rev ? "TGCA" : "ACGT";
        const int nblk = (qlen + 31) >> 5;
        int len = 0, n_mm = 0, n_n = 0, last = J.rev ? qlen : -1;
        for (int kk = 0; kk < nblk; ++kk) {
            const int k = J.rev ? nblk - 1 - kk : kk;
            const int p0 = J.qb + 32 * k, nvalid = qlen - 32 * k < 32 ? qlen - 32 * k : 32;
            const int wi = p0 >> 5, sh = (p0 & 31) * 2;
            const u64 q = sh ? (fw[wi] << sh) | (fw[wi + 1] >> (64 - sh)) : fw[wi];
            const u64 t = extract32(A.pac, J.rb + 32 * k);
            const u64 x = q ^ t;
            u64 y = (x | (x >> 1)) & 0x5555555555555555ull;                     // bit 62 - 2i: base i of the block differs
            if (has_n) {
                const int mw = p0 >> 6, ms = p0 & 63;
                u64 nb = nmask[mw] >> ms;
                if (ms > 32 && mw + 1 < A.pMW) nb |= nmask[mw + 1] << (64 - ms);
                unsigned nbits = (unsigned)(nb & 0xffffffffull);
                if (nvalid < 32) nbits &= (1u << nvalid) - 1u;
                n_n += __popc(nbits);
                while (nbits) { const int i = __ffs((int)nbits) - 1; nbits &= nbits - 1; y |= 1ull << (62 - 2 * i); }
            }
            if (nvalid < 32) y &= ~0ull << (2 * (32 - nvalid));
            n_mm += __popcll(y);
            if (out)
                while (y) {
                    const int i = J.rev ? 31 - (__builtin_ctzll(y) >> 1) : (__clzll((long long)y) >> 1);
                    y &= ~(1ull << (62 - 2 * i));
                    const int j = 32 * k + i;
                    len += gcig_put_num(out, len, J.rev ? last - j - 1 : j - last - 1, true);
                    out[len++] = b2c[(int)(t >> (62 - 2 * i)) & 3];
                    last = j;
                }
        }
        if (out) { len += gcig_put_num(out, len, J.rev ? last : qlen - last - 1, true); out[len] = 0; A.nm[jb] = n_mm; A.mdlen[jb] = len; }
        const int cap = qlen + J.tlen + 2;
        A.cig[A.coff[jb] + cap - 1] = (unsigned)qlen << 4;
        meme_gres R;
        R.score = A.o.a * (qlen - n_mm) - A.o.b * (n_mm - n_n) - n_n;            // bwa_fill_scmat: match a, mismatch -b, an ambiguous base -1
        R.n_cigar = 1; R.cigar_off = cap - 1;
        A.res[jb] = R;
    }
}

// the operations of every job, densely packed in job order (they were pushed back to front: already in CIGAR order)
__global__ void __launch_bounds__(256) k_gcig_pack(const meme_gres* __restrict__ res, const i64* __restrict__ coff, const uint32_t* __restrict__ cig,
                                                    const i64* __restrict__ ooff, i64 njobs, uint32_t* __restrict__ out) {
    for (i64 jb = (i64)blockIdx.x * blockDim.x + threadIdx.x; jb < njobs; jb += (i64)gridDim.x * blockDim.x) {
        const meme_gres R = res[jb];
        const uint32_t* src = cig + coff[jb] + R.cigar_off;
        uint32_t* dst = out + ooff[jb];
        for (int k = 0; k < R.n_cigar; ++k) dst[k] = src[k];
    }
}
// per job: the kernel that takes it -- isdp: k_gcig (a wavefront), is16 / is32: k_gcig_grp<16 / 32> (a group of lanes; z16 / z32 = bytes of LDS a group has for
// the backtrack matrix, 0: the class is not used), none: k_gcig_nogap -- and the sizes of its scratch
__global__ void __launch_bounds__(256) k_gcig_sizes(const meme_gjob* __restrict__ jobs, i64 njobs, const i64* __restrict__ read_off, bool fast, int zcap, int z16, int z32, int z64, i64* __restrict__ zsz,
                                                     i64* __restrict__ csz, i64* __restrict__ msz, i64* __restrict__ isdp, i64* __restrict__ is16, i64* __restrict__ is32, i64* __restrict__ is64) {
    for (i64 jb = (i64)blockIdx.x * blockDim.x + threadIdx.x; jb < njobs; jb += (i64)gridDim.x * blockDim.x) {
        const meme_gjob J = jobs[jb];
        const bool dp = !(fast && nogap_fast(J, read_off));
        const i64 n_col = gcig_n_col(J.qlen, J.w);
        const bool g16 = dp && J.w >= 0 && n_col <= 16 && n_col * J.tlen <= z16;
        const bool g32 = dp && !g16 && J.w >= 0 && n_col <= 32 && n_col * J.tlen <= z32;
        const bool g64 = dp && !g16 && !g32 && J.w >= 0 && n_col <= 64 && n_col * J.tlen <= z64;
        is16[jb] = g16; is32[jb] = g32; is64[jb] = g64;
        isdp[jb] = dp && !g16 && !g32 && !g64;                               // 1: the job goes to k_gcig
        zsz[jb] = J.w < 0 || g16 || g32 || g64 || n_col * J.tlen <= zcap ? 0 : (n_col * J.tlen + 15) & ~(i64)15;   // (w < 0: the gap-free shortcut, no matrix; small matrices stay in LDS)
        csz[jb] = J.qlen + J.tlen + 2;
        if (msz) msz[jb] = 2 * ((i64)J.qlen + J.tlen) + 16;                // an MD string never has more than two characters per base
    }
}
// the list the three kernels draw from: the 16-lane jobs, then the 32-lane jobs, then the whole-wavefront jobs, each in job order
__global__ void __launch_bounds__(256) k_gcig_dplist(const i64* __restrict__ isdp, const i64* __restrict__ dpoff, const i64* __restrict__ is16, const i64* __restrict__ o16,
                                                      const i64* __restrict__ is32, const i64* __restrict__ o32, const i64* __restrict__ is64, const i64* __restrict__ o64, i64 njobs,
                                                      i64* __restrict__ list) {
    const i64 n16 = o16[njobs], n32 = o32[njobs], n64 = o64[njobs];
    for (i64 jb = (i64)blockIdx.x * blockDim.x + threadIdx.x; jb < njobs; jb += (i64)gridDim.x * blockDim.x) {
        if (is16[jb]) list[o16[jb]] = jb;
        else if (is32[jb]) list[n16 + o32[jb]] = jb;
        else if (is64[jb]) list[n16 + n32 + o64[jb]] = jb;
        else if (isdp[jb]) list[n16 + n32 + n64 + dpoff[jb]] = jb;
    }
}
__global__ void __launch_bounds__(256) k_gcig_ncig(const meme_gres* __restrict__ res, i64 njobs, i64* __restrict__ ncig) {
    for (i64 jb = (i64)blockIdx.x * blockDim.x + threadIdx.x; jb < njobs; jb += (i64)gridDim.x * blockDim.x) ncig[jb] = res[jb].n_cigar;
}
__global__ void __launch_bounds__(256) k_gcig_fix(meme_gres* __restrict__ res, const i64* __restrict__ ooff, i64 njobs) {
    for (i64 jb = (i64)blockIdx.x * blockDim.x + threadIdx.x; jb < njobs; jb += (i64)gridDim.x * blockDim.x) res[jb].cigar_off = ooff[jb];
}

// what the host loop cannot see: a job's query span against the length of the read it names
__global__ void __launch_bounds__(256) k_gcig_check(const meme_gjob* __restrict__ jobs, i64 njobs, const i64* __restrict__ read_off, i64* __restrict__ bad) {
    for (i64 jb = (i64)blockIdx.x * blockDim.x + threadIdx.x; jb < njobs; jb += (i64)gridDim.x * blockDim.x) {
        const meme_gjob J = jobs[jb];
        if ((i64)J.qb + J.qlen > read_off[J.read + 1] - read_off[J.read]) atomicMin((unsigned long long*)bad, (unsigned long long)jb);
    }
}

// bwa_gen_cigar2's own preamble (src/bwa.cpp:288-316) for a batch of its calls: the strand from rb, and gcig_band -- the gap-free shortcut (band -1 here)
// or the band it hands to ksw_global2
__global__ void __launch_bounds__(256) k_cjob_prep(const meme_cjob* __restrict__ cj, i64 njobs, i64 l_pac, meme_bsw_opt o, meme_gjob* __restrict__ jobs) {
    for (i64 jb = (i64)blockIdx.x * blockDim.x + threadIdx.x; jb < njobs; jb += (i64)gridDim.x * blockDim.x) {
        const meme_cjob C = cj[jb];
        meme_gjob J;
        J.rb = C.rb; J.read = C.read; J.qb = C.qb; J.qlen = C.qlen; J.tlen = C.tlen; J.rev = C.rb >= l_pac ? 1 : 0;
        J.w = gcig_band(C.qlen, C.tlen, C.w_, o);
        jobs[jb] = J;
    }
}
// packed MD strings (NUL-terminated, job order) + the per-job result records of meme_gen_cigar_batch_host
__global__ void __launch_bounds__(256) k_md_sizes(const int32_t* __restrict__ mdlen, i64 njobs, i64* __restrict__ sz) {
    for (i64 jb = (i64)blockIdx.x * blockDim.x + threadIdx.x; jb < njobs; jb += (i64)gridDim.x * blockDim.x) sz[jb] = (i64)mdlen[jb] + 1;
}
__global__ void __launch_bounds__(256) k_md_pack(const meme_gres* __restrict__ res, const int32_t* __restrict__ nm, const int32_t* __restrict__ mdlen, const i64* __restrict__ mdoff,
                                                  const char* __restrict__ md, const i64* __restrict__ poff, i64 njobs, char* __restrict__ out, meme_cres* __restrict__ cres) {
    for (i64 jb = (i64)blockIdx.x * blockDim.x + threadIdx.x; jb < njobs; jb += (i64)gridDim.x * blockDim.x) {
        const int l = mdlen[jb];
        const char* src = md + mdoff[jb];
        char* dst = out + poff[jb];
        for (int k = 0; k <= l; ++k) dst[k] = src[k];
        meme_cres R;
        R.score = res[jb].score; R.n_cigar = res[jb].n_cigar; R.nm = nm[jb]; R.md_len = l; R.cigar_off = res[jb].cigar_off; R.md_off = poff[jb];
        cres[jb] = R;
    }
}

// The batch from the jobs in ctx->gcig.jobs (device) to packed results: scratch sizes and kernel classes (gcig_plan), the alignment kernels (gcig_align), the packed
// operations and MD strings (gcig_pack).  with_md: NM + MD of every job (meme_gen_cigar_batch_host).
struct GcigRun {
    i64 njobs; int qmax, tmax; const meme_bsw_opt* opt; bool with_md; const char* who;
    size_t lds_base; int zcap, grp_qcap, grp_tcap, grp_z[3];     // LDS of k_gcig_t without its matrix, the matrix bytes it keeps; of k_gcig_grp<16 / 32 / 64>: query, target, matrix bytes
    i64 tz = 0, tc = 0, tm = 0, ndp = 0, ngrp[3] = {0, 0, 0};    // bytes of matrices, CIGAR words, MD bytes; jobs of k_gcig_t and of the three group classes
    i64 tops = 0, tmd = 0;                                        // packed operations, packed MD bytes
};
constexpr int Z_LDS_WINDOW = 2048;          // ... and when matrices do not fit anyway: the window the walk back reads them through
constexpr int Z_LDS_CAP = 8192;             // a 250-row matrix of up to 32 band columns: the bands bwa_gen_cigar2 computes for reads with a few small indels
// Several jobs per wavefront for narrow bands (k_gcig_grp; tuning "gcig_groups" = 0: every job a wavefront): lanes, jobs per wavefront, the most matrix bytes a group keeps, the
// LDS a wavefront's groups may take (24 KB: six wavefronts per CU and more).  Per group: rings for H and E, the query, the target and a matrix of `lanes` columns x the longest target.
// (bands of 65-128 columns as one chunk, two columns per lane, were measured and removed: profiles/r06_gcig.md)
constexpr struct { int lanes, per_wave, zmax, lds_max; } GCIG_GRP[3] = {{16, 4, 4096, 24 * 1024}, {32, 2, 8192, 24 * 1024}, {64, 1, 12288, 16 * 1024}};
size_t grp_lds(const GcigRun& R, int g) { return (size_t)GCIG_GRP[g].per_wave * ((size_t)3 * 2 * GCIG_GRP[g].lanes * 4 + R.grp_qcap + R.grp_tcap + R.grp_z[g]); }

// sizing and classing: LDS per job, the per-job scratch sizes and kernel classes, their scans and totals, the scratch itself
int gcig_plan(meme_ctx* ctx, GcigRun& R) {
    int rc;
    const i64 njobs = R.njobs;
    R.lds_base = (size_t)(3 * (R.qmax + 2)) * 4 + (size_t)((R.qmax + 3) & ~3) + (size_t)((R.tmax + 3) & ~3);
    // The LDS kept per job for its backtrack matrix or window (tuning "gcig_zcap" overrides; 0: none).  Measured on two read classes only
    // (profiles/r05_gcig.md, 400 k calls each): where a typical matrix -- the rows of the longest target x the ~33 band columns bwa_gen_cigar2 computes
    // for a read with a few small indels -- fits, keeping it whole pays (150 bp: 7.1 ms against 9.8 without); where it does not, only the window is used
    // and a small one leaves room for more wavefronts (250 bp: 47.5 ms with 2 KB against 52.9 with 8 KB).
    const int zauto = (size_t)R.tmax * 33 <= (size_t)Z_LDS_CAP ? Z_LDS_CAP : Z_LDS_WINDOW;
    const int zwant = ctx->gcig_zcap >= 0 ? (int)ctx->gcig_zcap : zauto;
    R.zcap = R.lds_base + (size_t)zwant <= 32 * 1024 ? zwant : 0;          // (long reads: their rows fill the LDS, the matrix stays in global memory)
    GcigWs& G = ctx->gcig;
    if ((rc = meme_buf_reserve(ctx, G.cols, GcigCols(nullptr, njobs).bytes)) || (rc = meme_buf_reserve(ctx, G.res, (size_t)njobs * sizeof(meme_gres)))) return rc;
    const GcigCols gc(G.cols.p, njobs);
    R.grp_qcap = (R.qmax + 3) & ~3; R.grp_tcap = (R.tmax + 3) & ~3;
    for (int g = 0; g < 3; ++g) {
        int& z = R.grp_z[g];
        z = ctx->gcig_groups ? ((GCIG_GRP[g].lanes * R.tmax + 3) & ~3) : 0;
        if (z > GCIG_GRP[g].zmax) z = GCIG_GRP[g].zmax;
        if (grp_lds(R, g) > (size_t)GCIG_GRP[g].lds_max) z = 0;
    }
    // the gap-free shortcut on the packed reads the seeding call left on the ctx (reads of at most 500 bases)
    const bool fast = ctx->batch.packed.p != nullptr && ctx->batch.last_seed_max_len > 0;
    const meme_gjob* jobs = G.jobs.as<const meme_gjob>();
    const i64* read_off = ctx->batch.read_off.as<const i64>();
    HIP_TRY(hipMemsetAsync(gc.bad, 0xff, 8, ctx->stream));
    hipLaunchKernelGGL(k_gcig_check, dim3(grid_blocks(njobs, 256)), dim3(256), 0, ctx->stream, jobs, njobs, read_off, gc.bad);
    hipLaunchKernelGGL(k_gcig_sizes, dim3(grid_blocks(njobs, 256)), dim3(256), 0, ctx->stream, jobs, njobs, read_off, fast, R.zcap, R.grp_z[0], R.grp_z[1], R.grp_z[2], gc.zsz, gc.csz,
                       R.with_md ? gc.msz : (i64*)nullptr, gc.isdp, gc.is16, gc.is32, gc.is64);
    if ((rc = meme_scan_exclusive(ctx, gc.zsz, gc.zoff, njobs)) || (rc = meme_scan_exclusive(ctx, gc.csz, gc.coff, njobs)) || (rc = meme_scan_exclusive(ctx, gc.isdp, gc.dpoff, njobs)) ||
        (rc = meme_scan_exclusive(ctx, gc.is16, gc.o16, njobs)) || (rc = meme_scan_exclusive(ctx, gc.is32, gc.o32, njobs)) || (rc = meme_scan_exclusive(ctx, gc.is64, gc.o64, njobs))) return rc;
    hipLaunchKernelGGL(k_gcig_dplist, dim3(grid_blocks(njobs, 256)), dim3(256), 0, ctx->stream, (const i64*)gc.isdp, (const i64*)gc.dpoff, (const i64*)gc.is16, (const i64*)gc.o16,
                       (const i64*)gc.is32, (const i64*)gc.o32, (const i64*)gc.is64, (const i64*)gc.o64, njobs, gc.dplist);
    if (R.with_md && (rc = meme_scan_exclusive(ctx, gc.msz, gc.moff, njobs))) return rc;
    // (every scan is queued before the first total is fetched: a fetch makes the host wait for the stream)
    i64 bad = -1;
    const struct { i64* h; const i64* d; } back[8] = {{&R.ngrp[2], gc.o64 + njobs}, {&R.ndp, gc.dpoff + njobs}, {&R.ngrp[0], gc.o16 + njobs}, {&R.ngrp[1], gc.o32 + njobs},
                                                      {&R.tz, gc.zoff + njobs}, {&R.tc, gc.coff + njobs}, {R.with_md ? &R.tm : nullptr, gc.moff + njobs}, {&bad, gc.bad}};
    for (const auto& b : back) if (b.h) HIP_TRY(hipMemcpyAsync(b.h, b.d, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (bad >= 0) {
        meme_set_error("%s: job %lld names a query span beyond the end of read it refers to", R.who, (long long)bad);
        return MEME_E_ARG;
    }
    const size_t need = (size_t)R.tz + (size_t)R.tc * 4 + (size_t)R.tm;
    size_t free_b = 0;
    if (!meme_fits_free_hbm(need, G.z.cap + G.cig.cap + G.md.cap, &free_b)) {
        meme_set_error("%s: %lld alignments need %.1f GB of backtrack matrices, more than half of the free HBM: submit fewer at a time", R.who, (long long)njobs, need / 1e9);
        return MEME_E_CAPACITY;
    }
    if ((rc = meme_buf_reserve(ctx, G.z, (size_t)R.tz + 64)) || (rc = meme_buf_reserve(ctx, G.cig, (size_t)(R.tc + 1) * 4))) return rc;
    if (R.with_md && ((rc = meme_buf_reserve(ctx, G.md, (size_t)R.tm + 64)) || (rc = meme_buf_reserve(ctx, G.nm, (size_t)njobs * 8 + 64)))) return rc;
    return MEME_OK;
}

// the alignment launches: the gap-free shortcut over everything no class took, the three group classes off their table, a wavefront per job for the rest of the DP list
int gcig_align(meme_ctx* ctx, const GcigRun& R) {
    GcigWs& G = ctx->gcig;
    const GcigCols gc(G.cols.p, R.njobs);
    const i64 njobs = R.njobs, n_grp = R.ngrp[0] + R.ngrp[1] + R.ngrp[2];
    const int pW = (int)((ctx->batch.last_seed_max_len + 31) / 32) + 2, pMW = (int)((ctx->batch.last_seed_max_len + 63) / 64);      // PackGeom of the seeded batch (meme_seed.hip)
    GcigArgs A;
    A.jobs = G.jobs.as<const meme_gjob>(); A.njobs = njobs; A.reads = ctx->batch.reads.as<const uint8_t>(); A.read_off = ctx->batch.read_off.as<const i64>(); A.pac = ctx->idx.pac;
    A.o = *R.opt; A.zoff = gc.zoff; A.z = G.z.as<uint8_t>(); A.coff = gc.coff; A.cig = G.cig.as<uint32_t>(); A.res = G.res.as<meme_gres>();
    A.mdoff = gc.moff; A.md = R.with_md ? G.md.as<char>() : nullptr;
    A.nm = R.with_md ? G.nm.as<int32_t>() : nullptr; A.mdlen = R.with_md ? G.nm.as<int32_t>() + njobs : nullptr;
    A.zcap = R.zcap; A.dp_list = nullptr; A.packed = ctx->batch.packed.as<const u64>(); A.pW = pW; A.pMW = pMW; A.pstride = 2 * pW + 2 * pMW + 1;
    A.list_first = 0; A.grp_qcap = R.grp_qcap; A.grp_tcap = R.grp_tcap; A.grp_z = 0;
    if (R.ndp + n_grp < njobs) hipLaunchKernelGGL(k_gcig_nogap, dim3(grid_blocks(njobs, 256)), dim3(256), 0, ctx->stream, A);
    GcigArgs D = A;
    D.dp_list = gc.dplist;
    for (int g = 0; g < 3; ++g) {              // the DP list holds the classes one after the other
        D.njobs = R.ngrp[g]; D.grp_z = R.grp_z[g];
        const dim3 grid((unsigned)((D.njobs + GCIG_GRP[g].per_wave - 1) / GCIG_GRP[g].per_wave));
        if (D.njobs > 0 && g == 0) hipLaunchKernelGGL(k_gcig_grp<16>, grid, dim3(64), grp_lds(R, g), ctx->stream, D);
        if (D.njobs > 0 && g == 1) hipLaunchKernelGGL(k_gcig_grp<32>, grid, dim3(64), grp_lds(R, g), ctx->stream, D);
        if (D.njobs > 0 && g == 2) hipLaunchKernelGGL(k_gcig_grp<64>, grid, dim3(64), grp_lds(R, g), ctx->stream, D);
        D.list_first += D.njobs;
    }
    i64* cj = ctx->tm.gcig_class_jobs;
    cj[0] = R.ngrp[0]; cj[1] = R.ngrp[1]; cj[2] = R.ndp; cj[3] = njobs - R.ndp - n_grp; cj[4] = R.ngrp[2]; cj[5] = 0;
    if (R.ndp > 0) {
        D.njobs = R.ndp; D.grp_z = 0;
        const size_t lds = R.lds_base + (size_t)R.zcap;
        if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)k_gcig_t, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_gcig_t, dim3((unsigned)R.ndp), dim3(64), lds, ctx->stream, D);
    }
    HIP_TRY(hipGetLastError());
    return MEME_OK;
}

// operations (and MD strings) of the jobs packed in job order
int gcig_pack(meme_ctx* ctx, GcigRun& R) {
    GcigWs& G = ctx->gcig;
    const GcigCols gc(G.cols.p, R.njobs);
    const i64 njobs = R.njobs;
    const int32_t* nm = G.nm.as<const int32_t>();       // nm, then mdlen (with_md)
    const dim3 grid(grid_blocks(njobs, 256)), block(256);
    int rc;
    hipLaunchKernelGGL(k_gcig_ncig, grid, block, 0, ctx->stream, G.res.as<const meme_gres>(), njobs, gc.ncig);
    if ((rc = meme_scan_exclusive(ctx, gc.ncig, gc.ooff, njobs))) return rc;
    if (R.with_md) {
        hipLaunchKernelGGL(k_md_sizes, grid, block, 0, ctx->stream, nm + njobs, njobs, gc.psz);
        if ((rc = meme_scan_exclusive(ctx, gc.psz, gc.poff, njobs))) return rc;
    }
    HIP_TRY(hipMemcpyAsync(&R.tops, gc.ooff + njobs, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (R.with_md) HIP_TRY(hipMemcpyAsync(&R.tmd, gc.poff + njobs, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if ((rc = meme_buf_reserve(ctx, G.ops, (size_t)(R.tops + 1) * 4))) return rc;
    hipLaunchKernelGGL(k_gcig_pack, grid, block, 0, ctx->stream, G.res.as<const meme_gres>(), (const i64*)gc.coff, G.cig.as<const uint32_t>(), (const i64*)gc.ooff, njobs, G.ops.as<uint32_t>());
    hipLaunchKernelGGL(k_gcig_fix, grid, block, 0, ctx->stream, G.res.as<meme_gres>(), (const i64*)gc.ooff, njobs);
    if (R.with_md) {
        if ((rc = meme_buf_reserve(ctx, G.md_packed, (size_t)R.tmd + 64)) || (rc = meme_buf_reserve(ctx, G.cres, (size_t)njobs * sizeof(meme_cres)))) return rc;
        hipLaunchKernelGGL(k_md_pack, grid, block, 0, ctx->stream, G.res.as<const meme_gres>(), nm, nm + njobs, (const i64*)gc.moff, G.md.as<const char>(), (const i64*)gc.poff, njobs,
                           G.md_packed.as<char>(), G.cres.as<meme_cres>());
    }
    HIP_TRY(hipGetLastError());
    return MEME_OK;
}

// what both entry points do with the staged jobs: the three parts between the stage's events, then the per-job records (`rec` bytes each, in `d_res`), the packed
// operations and the packed MD strings to the host; *ms: the stage's time
int gcig_run(meme_ctx* ctx, GcigRun& R, const DevBuf& d_res, size_t rec, float* ms) {
    GcigWs& G = ctx->gcig;
    int rc;
    if ((rc = gcig_plan(ctx, R)) || (rc = gcig_align(ctx, R)) || (rc = gcig_pack(ctx, R))) return rc;
    HIP_TRY(hipEventRecord(G.ev[1], ctx->stream));
    if ((rc = meme_hostbuf_reserve(ctx, G.h_res, (size_t)R.njobs * rec)) || (rc = meme_hostbuf_reserve(ctx, G.h_ops, (size_t)(R.tops + 1) * 4)) ||
        (R.with_md && (rc = meme_hostbuf_reserve(ctx, G.h_md, (size_t)R.tmd + 64)))) return rc;
    HIP_TRY(hipMemcpyAsync(G.h_res.p, d_res.p, (size_t)R.njobs * rec, hipMemcpyDeviceToHost, ctx->stream));
    if (R.tops) HIP_TRY(hipMemcpyAsync(G.h_ops.p, G.ops.p, (size_t)R.tops * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (R.tmd) HIP_TRY(hipMemcpyAsync(G.h_md.p, G.md_packed.p, (size_t)R.tmd, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipEventElapsedTime(ms, G.ev[0], G.ev[1]));
    return MEME_OK;
}

int gcig_preamble(meme_ctx* ctx, const void* jobs, int64_t njobs, const meme_bsw_opt* opt, const void* out, const char* who) {
    if (!ctx || !jobs || njobs < 0 || !opt || !out) { meme_set_error("%s: null argument", who); return MEME_E_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    if (njobs == 0) return MEME_OK;
    const i64 nreads = ctx->batch.last_seed_reads;
    if (nreads <= 0 || !ctx->batch.reads.p || !ctx->batch.read_off.p || !ctx->idx.pac || !ctx->batch.reads_resident) { meme_set_error("%s: no seeded batch on this ctx (the jobs name its reads)", who); return MEME_E_STATE; }
    if (opt->e_del < 1 || opt->e_ins < 1) { meme_set_error("%s: gap extension penalties must be positive", who); return MEME_E_ARG; }
    if (ctx->max_batch > 0 && njobs > ctx->max_batch) { meme_set_error("%s: %lld jobs exceed the ctx's max_batch of %lld", who, (long long)njobs, (long long)ctx->max_batch); return MEME_E_CAPACITY; }
    HIP_TRY(ctx->gcig.ev.ensure());
    return MEME_OK;
}

}  // namespace

extern "C" int meme_global_batch_host(meme_ctx* ctx, const meme_gjob* jobs, int64_t njobs, const meme_bsw_opt* opt, meme_gres_host* out) {
    static const char* const who = "meme_global_batch_host";
    int rc;
    if ((rc = gcig_preamble(ctx, jobs, njobs, opt, out, who))) return rc;
    memset(out, 0, sizeof(*out));
    if (njobs == 0) return MEME_OK;
    const i64 nreads = ctx->batch.last_seed_reads;
    int qmax = 0, tmax = 0;
    for (i64 k = 0; k < njobs; ++k) {
        const meme_gjob& J = jobs[k];
        // (the band must reach the matrix's last cell, w >= |tlen - qlen|, as every band bwa_gen_cigar2 computes does, src/bwa.cpp:306-316:
        // below that ksw_global2 walks rows without cells, which this kernel does not restate)
        if (J.read < 0 || J.read >= nreads || J.qb < 0 || J.qlen < 1 || J.tlen < 1 || J.w < 0 || J.rb < 0 || J.rb + J.tlen > ctx->idx.n || J.qlen > 65535 || J.tlen > 65535 ||
            J.w < (J.tlen > J.qlen ? J.tlen - J.qlen : J.qlen - J.tlen)) {
            meme_set_error("%s: job %lld is malformed (read %d, query %d+%d, target %lld+%d, band %d)", who, (long long)k, J.read, J.qb, J.qlen, (long long)J.rb, J.tlen, J.w);
            return MEME_E_ARG;
        }
        qmax = J.qlen > qmax ? J.qlen : qmax;
        tmax = J.tlen > tmax ? J.tlen : tmax;
    }
    GcigWs& G = ctx->gcig;
    if ((rc = meme_buf_reserve(ctx, G.jobs, (size_t)njobs * sizeof(meme_gjob)))) return rc;
    HIP_TRY(hipMemcpyAsync(G.jobs.p, jobs, (size_t)njobs * sizeof(meme_gjob), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->gcig.ev[0], ctx->stream));
    GcigRun R{njobs, qmax, tmax, opt, false, who};
    float ms = 0.f;
    if ((rc = gcig_run(ctx, R, G.res, sizeof(meme_gres), &ms))) return rc;
    out->njobs = njobs; out->res = G.h_res.as<const meme_gres>(); out->cigars = G.h_ops.as<const uint32_t>(); out->total_ops = R.tops; out->kernel_ms = ms;
    return MEME_OK;
}

extern "C" int meme_gen_cigar_batch_host(meme_ctx* ctx, const meme_cjob* jobs, int64_t njobs, const meme_bsw_opt* opt, meme_cres_host* out) {
    static const char* const who = "meme_gen_cigar_batch_host";
    int rc;
    if ((rc = gcig_preamble(ctx, jobs, njobs, opt, out, who))) return rc;
    memset(out, 0, sizeof(*out));
    if (njobs == 0) return MEME_OK;
    const i64 nreads = ctx->batch.last_seed_reads, l_pac = ctx->idx.n >> 1;
    int qmax = 0, tmax = 0;
    for (i64 k = 0; k < njobs; ++k) {
        const meme_cjob& J = jobs[k];
        // what bwa_gen_cigar2 itself rejects (src/bwa.cpp:285: empty spans, a target bridging the two strands) is not a job
        if (J.read < 0 || J.read >= nreads || J.qb < 0 || J.qlen < 1 || J.tlen < 1 || J.w_ < 0 || J.rb < 0 || J.rb + J.tlen > ctx->idx.n || J.qlen > 65535 || J.tlen > 65535 ||
            (J.rb < l_pac && J.rb + J.tlen > l_pac)) {
            meme_set_error("%s: job %lld is malformed (read %d, query %d+%d, target %lld+%d, w_ %d)", who, (long long)k, J.read, J.qb, J.qlen, (long long)J.rb, J.tlen, J.w_);
            return MEME_E_ARG;
        }
        qmax = J.qlen > qmax ? J.qlen : qmax;
        tmax = J.tlen > tmax ? J.tlen : tmax;
    }
    GcigWs& G = ctx->gcig;
    if ((rc = meme_buf_reserve(ctx, G.jobs, (size_t)njobs * sizeof(meme_gjob))) || (rc = meme_buf_reserve(ctx, G.cjobs, (size_t)njobs * sizeof(meme_cjob)))) return rc;
    HIP_TRY(hipMemcpyAsync(G.cjobs.p, jobs, (size_t)njobs * sizeof(meme_cjob), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->gcig.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_cjob_prep, dim3(grid_blocks(njobs, 256)), dim3(256), 0, ctx->stream, (const meme_cjob*)G.cjobs.p, (i64)njobs, l_pac, *opt, (meme_gjob*)G.jobs.p);
    GcigRun R{njobs, qmax, tmax, opt, true, who};
    float ms = 0.f;
    if ((rc = gcig_run(ctx, R, G.cres, sizeof(meme_cres), &ms))) return rc;
    out->njobs = njobs; out->res = G.h_res.as<const meme_cres>(); out->cigars = G.h_ops.as<const uint32_t>(); out->total_ops = R.tops; out->md = G.h_md.as<const char>(); out->md_bytes = R.tmd;
    out->kernel_ms = ms;
    return MEME_OK;
}
