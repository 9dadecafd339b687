"""klib's ks_introsort (reference src/ksort.h; what mem_chain_flt sorts chains with, src/bwamem.cpp:80, 631), modelled here in Python on
(weight, id) pairs, against the two forms the chaining stage runs; chains of EQUAL weight must come out in the same order, because the
filter that follows depends on it.
 * The sequential sort, written once in bwa-meme_amd/csrc/meme_ksort.h (ks_introsort, ks_combsort, ks_insertsort over an array with get / set, a
   less-than functor and the caller's stack): the lane tier (k_chain) and the B-tree tier (k_chain_wave) of meme_chain.hip run it whole, the
   LDS tier (wave_introsort_lds) its comb-sort fallback.  The header is compiled here with g++ and has to give the model's order, also on the
   monotone and tied inputs that spend the depth budget and enter the comb sort (random inputs never do).  The rules of the reference the tiers
   share (meme_chain_rules.h) are compiled along with it; tests/test_gpu_chain.py checks them through the kernels.
 * The wave-parallel formulation of the LDS tier (par below): each Hoare partition step from the two lists of scan stops (up-scan stops at
   weight <= pivot, down-scan at weight >= pivot; the k-th swap pairs the k-th stop from the left with the k-th from the right while the left
   one lies before the right one; the loop ends on a position that follows from the lists), the closing insertion sort as a stable sort.
(The device kernels themselves are checked against the reference's chains in tests/test_gpu_chain.py.)"""
import ctypes as C
import os
import subprocess

import random
def lt(a,b): return a[0] > b[0]
def insertsort(a,s,t):
    for i in range(s+1,t):
        j=i
        while j> s and lt(a[j],a[j-1]):
            a[j],a[j-1]=a[j-1],a[j]; j-=1
COMB_CALLS = [0]           # times the model entered the comb sort
def combsort(a,s,n):
    COMB_CALLS[0] += 1
    shrink=1.2473309501039786540366528676643
    gap=n
    while True:
        if gap>2:
            gap=int(gap/shrink)
            if gap in (9,10): gap=11
        do_swap=False
        for i in range(s, s+n-gap):
            j=i+gap
            if lt(a[j],a[i]): a[i],a[j]=a[j],a[i]; do_swap=True
        if not (do_swap or gap>2): break
    if gap!=1: insertsort(a,s,s+n)
def klib(a):
    a=a[:]; n=len(a)
    if n<1: return a
    if n==2:
        if lt(a[1],a[0]): a[0],a[1]=a[1],a[0]
        return a
    d=2
    while (1<<d) < n: d+=1
    d<<=1
    s=0;t=n-1;stack=[]
    while True:
        if s<t:
            d-=1
            if d==0:
                combsort(a,s,t-s+1); t=s; continue
            i=s;j=t;k=i+((j-i)>>1)+1
            if lt(a[k],a[i]):
                if lt(a[k],a[j]): k=j
            else: k = i if lt(a[j],a[i]) else j
            rp=a[k]
            if k!=t: a[k],a[t]=a[t],a[k]
            while True:
                i+=1
                while lt(a[i],rp): i+=1
                j-=1
                while i<=j and lt(rp,a[j]): j-=1
                if j<=i: break
                a[i],a[j]=a[j],a[i]
            a[i],a[t]=a[t],a[i]
            if i-s > t-i:
                if i-s>16: stack.append((s,i-1,d))
                s = i+1 if t-i>16 else t
            else:
                if t-i>16: stack.append((i+1,t,d))
                t = i-1 if i-s>16 else s
        else:
            if not stack:
                insertsort(a,0,n); return a
            s,t,d=stack.pop()
def par(a):
    a=a[:]; n=len(a)
    if n<1: return a
    if n==2:
        if a[1][0]>a[0][0]: a[0],a[1]=a[1],a[0]
        return a
    d=2
    while (1<<d) < n: d+=1
    d<<=1
    s=0;t=n-1;stack=[]
    while True:
        if s<t:
            d-=1
            if d==0:
                combsort(a,s,t-s+1); t=s; continue
            k=s+((t-s)>>1)+1
            wi,wj,wk=a[s][0],a[t][0],a[k][0]
            if wk>wi:
                if wk>wj: k=t
            else: k = s if wj>wi else t
            rpw=a[k][0]
            if k!=t: a[k],a[t]=a[t],a[k]
            L=[p for p in range(s+1,t+1) if a[p][0]<=rpw]
            R=[p for p in range(t-1,s,-1) if a[p][0]>=rpw]
            mm=0
            while mm<min(len(L),len(R)) and L[mm]<R[mm]: mm+=1
            for q in range(mm): a[L[q]],a[R[q]]=a[R[q]],a[L[q]]
            i=L[mm]
            if mm>=1 and R[mm-1]<i: i=R[mm-1]
            a[i],a[t]=a[t],a[i]
            if i-s > t-i:
                if i-s>16: stack.append((s,i-1,d))
                s = i+1 if t-i>16 else t
            else:
                if t-i>16: stack.append((i+1,t,d))
                t = i-1 if i-s>16 else s
        else:
            if not stack:
                # stable sort by descending weight
                order=sorted(range(n), key=lambda e:(-a[e][0], e))
                return [a[e] for e in order]
            s,t,d=stack.pop()


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 3, 16, 17, 33, 34, 40, 64, 100, 256, 300, 1024, 1300]
FAMILIES = {"n-i": lambda n, i: n - i, "i": lambda n, i: i, "(n-i)//2": lambda n, i: (n - i) // 2, "(n-i)//3": lambda n, i: (n - i) // 3, "i//2": lambda n, i: i // 2}


def random_cases():
    random.seed(3)
    for it in range(3000):
        n = random.randint(1, 400)
        rng = random.choice([1, 2, 4, 20, 1000])
        yield (n, rng), [(random.randint(0, rng), i) for i in range(n)]


def monotone_cases():
    for name, f in FAMILIES.items():
        for n in SIZES:
            yield (name, n), [(f(n, i), i) for i in range(n)]


def pipe_cases():
    for n in (400, 1000):
        yield ("organ pipe", n), [(min(i, n - 1 - i), i) for i in range(n)]
        yield ("inverted organ pipe", n), [(max(i, n - 1 - i), i) for i in range(n)]


def stable(arr): return sorted(arr, key=lambda e: -e[0])


_REFERENCE = {}
def reference(family):
    """(what, input, klib's result, whether the model entered the comb sort) for every case of a family, computed once"""
    if family not in _REFERENCE:
        out = []
        for what, arr in {"random": random_cases, "monotone": monotone_cases, "pipe": pipe_cases}[family]():
            COMB_CALLS[0] = 0
            want = klib(arr)
            out.append((what, arr, want, COMB_CALLS[0] > 0))
        _REFERENCE[family] = out
    return _REFERENCE[family]


def test_parallel_formulation_of_klib_introsort_keeps_the_order_of_ties():
    for family in ("random", "monotone", "pipe"):
        for what, arr, want, _ in reference(family):
            assert par(arr) == want, what


def test_monotone_inputs_reach_the_combsort_branch_and_ties_show_there():
    assert not any(entered for _, _, _, entered in reference("random"))          # (why the families below are needed)
    entering = [what for what, _, _, entered in reference("monotone") if entered]
    assert len(entering) >= 10, entering
    assert ("n-i", 33) in entering and ("(n-i)//2", 40) in entering
    (arr, want, entered), = [(arr, want, entered) for what, arr, want, entered in reference("monotone") if what == ("(n-i)//2", 40)]
    assert entered and want != stable(arr)                                        # the order of ties that klib leaves is observable there


def test_shared_sort_header_equals_the_model(tmp_path):
    src = tmp_path / "t_ksort.cpp"
    src.write_text('''#include <vector>
#include "meme_chain_rules.h"
typedef unsigned long long u64;
struct ByWeight { bool operator()(u64 a, u64 b) const { return (a >> 32) > (b >> 32); } };
struct VecStack {
    std::vector<int> v;
    void push(int l, int r, int d) { v.push_back(l); v.push_back(r); v.push_back(d); }
    bool pop(int& l, int& r, int& d) { if (v.empty()) return false; d = v.back(); v.pop_back(); r = v.back(); v.pop_back(); l = v.back(); v.pop_back(); return true; }
};
extern "C" int t_introsort(u64* a, int n) { VecStack st; ks_introsort(KsPtr<u64>{a}, n, ByWeight(), st); return (int)st.v.size(); }
extern "C" void t_combsort(u64* a, int s, int n) { ks_combsort(KsPtr<u64>{a}, s, n, ByWeight()); }
''')
    so = str(tmp_path / "libt_ksort.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"),
                    str(src), "-o", so], check=True)
    lib = C.CDLL(so)

    def keys(arr): return (C.c_uint64 * len(arr))(*[(w << 32) | i for w, i in arr])
    def pairs(buf): return [(int(k) >> 32, int(k) & 0xffffffff) for k in buf]

    for family in ("random", "monotone", "pipe"):
        for what, arr, want, _ in reference(family):
            buf = keys(arr)
            assert lib.t_introsort(buf, len(arr)) == 0, what                     # (the stack comes back empty)
            assert pairs(buf) == want, what
    # ks_combsort on a range inside an array: the range as the model leaves it, nothing outside it touched
    random.seed(5)
    for n in range(2, 65):
        for rng in (1, 3, 50):
            arr = [(random.randint(0, rng), i) for i in range(n + 7)]
            want = arr[:]
            combsort(want, 3, n)
            buf = keys(arr)
            lib.t_combsort(buf, 3, n)
            assert pairs(buf) == want, (n, rng)
