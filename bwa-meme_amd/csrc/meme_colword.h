// Column words of the lane-per-job Smith-Waterman kernels (k_bsw_lane / k_bsw_lane_circ of meme_bsw.hip, k_kswv / k_seedsw of meme_kswv.hip),
// device only.  A lane keeps the state of DP column j in one 32-bit LDS word, laid out [column][lane] (bank-conflict free whatever column each
// lane is at): the query code in the low byte, then two 12-bit fields.  Which two values the fields hold, and the recurrence, is each kernel's own
// (k_kswv and k_seedsw share cw_gotoh_cell).
#pragma once
#include "meme_common.h"

typedef __attribute__((address_space(3))) unsigned int* lds_u32;

__device__ __forceinline__ int max3_i32(int a, int b, int c) { int d; asm("v_max3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }

// {code, lo in bits 8..19, hi in bits 20..31}
__device__ __forceinline__ unsigned cw_pack(int lo, int hi, unsigned code) { return ((unsigned)lo << 8) | ((unsigned)hi << 20) | code; }
// the same for the inner loop, two instructions: (hi << 12 | lo), then its three low bytes above the low byte of the old word
__device__ __forceinline__ unsigned cw_repack(int lo, int hi, unsigned old) {
    unsigned x, w;
    asm("v_lshl_or_b32 %0, %1, 12, %2" : "=v"(x) : "v"(hi), "v"(lo));
    asm("v_perm_b32 %0, %1, %2, %3" : "=v"(w) : "v"(x), "v"(old), "s"(0x06050400u));
    return w;
}

// A row's substitution scores as a byte table indexed by the query code: codes 0..3 in the word built here (the target base's own slot holds the
// match score; a row on an N scores `ambiguous` throughout), codes 4.. in byte 0.. of the caller's tab_hi.  Scores are signed bytes.
__device__ __forceinline__ unsigned cw_score_tab(int tb, int match, int mismatch, int ambiguous) {
    const unsigned mm4 = (unsigned)(mismatch & 0xff) * 0x01010101u, am4 = (unsigned)(ambiguous & 0xff) * 0x01010101u;
    return tb > 3 ? am4 : (mm4 & ~(0xffu << (8 * tb))) | ((unsigned)(match & 0xff) << (8 * tb));
}
// the score of the column whose word is `cw`: v_perm_b32 picks byte `code` of {tab_hi, tab_lo} (selector byte 0; the other result bytes are not looked at)
__device__ __forceinline__ int cw_score(unsigned tab_hi, unsigned tab_lo, unsigned cw) { return (int)(signed char)(__builtin_amdgcn_perm(tab_hi, tab_lo, cw) & 0xffu); }

// One Gotoh cell of a local alignment on a column word {code, H(i-1, j), the gap state that travels down the column}; the gap state that travels along the
// row (`along`) and the diagonal stay in registers.  Gap states are opened from H and never negative.  H(i, j) goes to `seen` (the caller's row maximum), the
// column's next word to `slot`.  CAPPED: diagonal + score saturates at `cap` (the unsigned bytes of the reference's int8 lanes).
template <bool CAPPED, class Seen> __device__ __forceinline__ void cw_gotoh_cell(lds_u32 slot, unsigned cur, unsigned tab_hi, unsigned tab_lo, int cap, int& diag, int& along,
                                                                                 int oe_down, int e_down, int oe_along, int e_along, const Seen& seen) {
    const int hold = (int)((cur >> 8) & 0xfffu), down = (int)(cur >> 20);
    int m = diag + cw_score(tab_hi, tab_lo, cur);
    if (CAPPED) m = m < cap ? m : cap;
    const int h = max3_i32(m, along, down);
    seen(h);
    const int down2 = max3_i32(h - oe_down, down - e_down, 0);      // (in this order: with the row's state first k_kswv's row loop measured 1 % slower)
    along = max3_i32(h - oe_along, along - e_along, 0);
    *slot = cw_repack(h, down2, cur);
    diag = hold;
}

// A row's maximum and its column travel as one key (h << 10 | column term), one accumulator per position of the four-cell unrolled loop, each
// holding the column term of its trip's FIRST cell: position p is `step` * p further (step = 1: column, rightmost wins; -1: 1023 - column, first wins)
__device__ __forceinline__ int cw_join_keys(int mk0, int mk1, int mk2, int mk3, int step) {
    mk1 += step; mk2 += 2 * step; mk3 += 3 * step;
    const int ka = mk0 > mk1 ? mk0 : mk1, kb = mk2 > mk3 ? mk2 : mk3;
    return ka > kb ? ka : kb;
}

// the largest v of the wavefront's 64 lanes, in every lane
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int y = __shfl_xor(v, d); v = v > y ? v : y; }
    return v;
}
