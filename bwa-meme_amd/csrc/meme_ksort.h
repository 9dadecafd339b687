// klib's ks_introsort, ks_combsort and __ks_insertsort (reference src/ksort.h), restated ONCE for every place that has to leave elements of equal
// key where klib leaves them: the same comparisons and swaps in the same order.  Sequential code for the host and the device (one lane, or all
// lanes of a wavefront doing the same stores); tests/test_introsort_model.py compiles this file with g++ and holds it against its Python model.
//
//   A   the array: `T get(int i) const` and `void set(int i, T v)` (a pointer, a strided pointer, parallel arrays ...)
//   LT  `bool operator()(const T& a, const T& b) const`: a sorts before b
//   ST  ks_introsort's explicit stack of (left, right, depth), owned by the caller: `void push(int l, int r, int d)`, `bool pop(int& l, int& r, int& d)`
//       (false = empty).  A range is pushed only when it has more than 16 elements, and the smaller side is always taken first: at most log2(n / 16) + 1 entries are live.
#pragma once

#if defined(__HIPCC__)
#define KS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KS_HD inline
#endif

template <class T> struct KsPtr {            // a plain array
    T* p;
    KS_HD T get(int i) const { return p[i]; }
    KS_HD void set(int i, T v) const { p[i] = v; }
};

template <class A> KS_HD void ks_swap(const A& a, int i, int j) { const auto x = a.get(i), y = a.get(j); a.set(i, y); a.set(j, x); }

template <class A, class LT> KS_HD void ks_insertsort(const A& a, int s, int t, const LT& lt) {      // __ks_insertsort on [s, t)
    for (int i = s + 1; i < t; ++i)
        for (int j = i; j > s && lt(a.get(j), a.get(j - 1)); --j) ks_swap(a, j, j - 1);
}

template <class A, class LT> KS_HD void ks_combsort(const A& a, int s, int n, const LT& lt) {        // ks_combsort on [s, s + n)
    const double shrink = 1.2473309501039786540366528676643;
    bool do_swap;
    int gap = n;
    do {
        if (gap > 2) { gap = (int)(gap / shrink); if (gap == 9 || gap == 10) gap = 11; }
        do_swap = false;
        for (int i = s; i < s + n - gap; ++i) { const int j = i + gap; if (lt(a.get(j), a.get(i))) { ks_swap(a, i, j); do_swap = true; } }
    } while (do_swap || gap > 2);
    if (gap != 1) ks_insertsort(a, s, s + n, lt);
}

// ks_introsort on [0, n): two elements are compared and swapped; otherwise quicksort around the median of first / middle / last, sub-ranges of at
// most 16 elements are left to the closing insertion sort, comb sort takes a range over when the depth budget (2 log2 n) is spent.
template <class A, class LT, class ST> KS_HD void ks_introsort(const A& a, int n, const LT& lt, ST& stack) {
    if (n < 1) return;
    if (n == 2) { if (lt(a.get(1), a.get(0))) ks_swap(a, 0, 1); return; }
    int d;
    for (d = 2; (1 << d) < n; ++d) {}
    d <<= 1;
    int s = 0, t = n - 1;
    for (;;) {
        if (s < t) {
            if (--d == 0) { ks_combsort(a, s, t - s + 1, lt); t = s; continue; }
            int i = s, j = t, k = i + ((j - i) >> 1) + 1;
            if (lt(a.get(k), a.get(i))) { if (lt(a.get(k), a.get(j))) k = j; }
            else k = lt(a.get(j), a.get(i)) ? i : j;
            const auto rp = a.get(k);
            if (k != t) ks_swap(a, k, t);
            for (;;) {
                do ++i; while (lt(a.get(i), rp));
                do --j; while (i <= j && lt(rp, a.get(j)));
                if (j <= i) break;
                ks_swap(a, i, j);
            }
            ks_swap(a, i, t);
            if (i - s > t - i) {
                if (i - s > 16) stack.push(s, i - 1, d);
                s = t - i > 16 ? i + 1 : t;
            } else {
                if (t - i > 16) stack.push(i + 1, t, d);
                t = i - s > 16 ? i - 1 : s;
            }
        } else {
            if (!stack.pop(s, t, d)) { ks_insertsort(a, 0, n, lt); return; }
        }
    }
}
