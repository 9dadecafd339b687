// The rules of ksw_global2 (reference src/ksw.cpp:560-670) under bwa_gen_cigar2 (src/bwa.cpp:262-316) that decide the placement of a gap in a
// CIGAR, written ONCE on plain values: the scoring entry, the band, the borders of the matrix, the cell with its direction byte, the walk back
// and the writer of its operations.  The kernels of meme_gcig.hip differ in who computes a row's cells and where H, E and the direction bytes
// live (a wavefront in 64-column chunks, a group of lanes on rings), not in these.  F's scan over the lanes, the NM / MD emitter and the
// decimal writer need the lanes and stay in meme_gcig.hip; what the scan is fed and how F is read off it is here (gcig_scan_key / gcig_scan_f).
#pragma once
#include <stdint.h>

#include "meme_hip.h"
#include "meme_ksort.h"      // KS_HD

constexpr int GCIG_MINUS_INF = -0x40000000;       // src/ksw.cpp:546
constexpr int GCIG_SCAN_FLOOR = -2000000000;      // the scan key of a lane without a cell: below every cell's (those stay near GCIG_MINUS_INF), above INT_MIN

// bwa_fill_scmat (src/bwa.cpp:262-270) for a target and a query code
KS_HD int gcig_score(int tb, int qb, int a, int b) { return (tb > 3 || qb > 3) ? -1 : (tb == qb ? a : -b); }

// bwa_gen_cigar2's preamble (src/bwa.cpp:294, 305-314): -1 for the gap-free shortcut, else the band ksw_global2 gets
KS_HD int gcig_band(int qlen, int tlen, int w_, const meme_bsw_opt& o) {
    if (qlen == tlen && w_ == 0) return -1;
    const int max_ins = (int)((double)(((qlen + 1) >> 1) * o.a - o.o_ins) / o.e_ins + 1.);
    const int max_del = (int)((double)(((qlen + 1) >> 1) * o.a - o.o_del) / o.e_del + 1.);
    int max_gap = max_ins > max_del ? max_ins : max_del;
    max_gap = max_gap > 1 ? max_gap : 1;
    const int dl = tlen > qlen ? tlen - qlen : qlen - tlen;
    int w = (max_gap + dl + 1) >> 1;
    w = w < w_ ? w : w_;
    return w > dl + 3 ? w : dl + 3;
}

// columns of the backtrack matrix (:568) and the band [beg, end) of row i (:594-595)
KS_HD int gcig_n_col(int qlen, int w) { return qlen < 2 * w + 1 ? qlen : 2 * w + 1; }
KS_HD int gcig_beg(int i, int w) { return i > w ? i - w : 0; }
KS_HD int gcig_end(int i, int w, int qlen) { return i + w + 1 < qlen ? i + w + 1 : qlen; }

// The borders.  H(-1, j - 1), what eh[j].h holds before row 0 (:586-589); H(i, beg - 1), what h1 starts row i from (:596), and the same as the
// cell (i, 0) reads it, H(i - 1, -1); the end of the row above: E(i, j) of a column at or beyond it is GCIG_MINUS_INF (:589, :649).
KS_HD int gcig_row0(int j, int w, int o_ins, int e_ins) { return j == 0 ? 0 : (j <= w ? -(o_ins + e_ins * j) : GCIG_MINUS_INF); }
KS_HD int gcig_left(int i, int beg, int o_del, int e_del) { return beg == 0 ? -(o_del + e_del * (i + 1)) : GCIG_MINUS_INF; }
KS_HD int gcig_corner(int i, int o_del, int e_del) { return i == 0 ? 0 : gcig_left(i - 1, 0, o_del, e_del); }      // (gcig_row0(0) = 0)
KS_HD int gcig_end_above(int i, int w, int qlen) { return i == 0 ? 0 : gcig_end(i - 1, w, qlen); }

// the cell (:611-629) from M(i,j), E(i,j), F(i,j): H(i,j), the direction byte f<<4 | e<<2 | h, E(i+1,j), F(i,j+1).  Ties: M over E over F, open over extend.
struct GcigCell { int h; unsigned d; int e, f; };
KS_HD GcigCell gcig_cell(int m, int e, int f, int oe_del, int e_del, int oe_ins, int e_ins) {
    GcigCell c;
    c.d = m >= e ? 0u : 1u;
    c.h = m >= e ? m : e;
    c.d = c.h >= f ? c.d : 2u;
    c.h = c.h >= f ? c.h : f;
    int t = m - oe_del;
    c.e = e - e_del;
    c.d |= c.e > t ? 1u << 2 : 0u;
    c.e = c.e > t ? c.e : t;
    t = m - oe_ins;
    c.f = f - e_ins;
    c.d |= c.f > t ? 2u << 4 : 0u;
    c.f = c.f > t ? c.f : t;
    return c;
}

// F along a row without the chain of :626-628.  With the columns of a chunk numbered c = 0, 1, ... and `carry` = F at column 0:
//   F(c) = max( carry - c * e_ins , max_{k < c} (M(k) - oe_ins - (c - 1 - k) * e_ins) )
// so the lanes scan key(k) = M(k) - oe_ins + k * e_ins for its running maximum (columns outside the row: the floor) and column c reads F off
// `below`, the maximum over k < c.  (F(i, beg) = -inf: a row's first chunk carries GCIG_MINUS_INF, a later one the chunk before's last F(i, j+1).)
KS_HD int gcig_scan_key(bool in, int m, int oe_ins, int e_ins, int c) { return in ? m - oe_ins + c * e_ins : GCIG_SCAN_FLOOR; }
KS_HD int gcig_scan_f(int below, int carry, int e_ins, int c) {
    const int own = below - (c - 1) * e_ins, far = carry - c * e_ins;
    return c == 0 ? carry : (own > far ? own : far);
}

// The operations of the walk, merged while equal (push_cigar, :548-558) and written back to front into the job's cap = qlen + tlen + 2 words, so
// that they stand in CIGAR order without :664's reversal: cg[cap - n ..) when done.  store: whether this caller (lane) writes.
struct GcigOps {
    uint32_t* cg; int cap; bool store;
    int n = 0, last_op = -1;
    unsigned cur = 0;
    KS_HD void flush() { if (last_op >= 0) { if (store) cg[cap - 1 - n] = cur; ++n; } }
    KS_HD void push(int op, int len) {
        if (last_op == op) cur += (unsigned)len << 4;
        else { flush(); cur = (unsigned)len << 4 | (unsigned)op; last_op = op; }
    }
    KS_HD int cigar_off() const { return cap - n; }
};

// the backtrack (:653-663).  zbyte(x): the direction byte at index x of the n_col x tlen matrix (the walk clamps x into it: where the reference would read
// outside its allocation, this reads the first or last byte); I: the type the index is computed in (int where the matrix is known to be small).
template <class I, class Z>
KS_HD void gcig_walk(int tlen, int qlen, int w, int n_col, Z&& zbyte, GcigOps& ops) {
    int i = tlen - 1, k = gcig_end(i, w, qlen) - 1, which = 0;
    const I zsize = (I)n_col * tlen;
    while (i >= 0 && k >= 0) {
        I zi = (I)i * n_col + (k - gcig_beg(i, w));
        if (zi < 0) zi = 0;
        if (zi >= zsize) zi = zsize - 1;
        which = zbyte(zi) >> (which << 1) & 3;
        if (which == 0) { ops.push(0, 1); --i; --k; }
        else if (which == 1) { ops.push(2, 1); --i; }
        else { ops.push(1, 1); --k; }
    }
    if (i >= 0) ops.push(2, i + 1);
    if (k >= 0) ops.push(1, k + 1);
    ops.flush();
}
