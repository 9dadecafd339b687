"""Workload and plain-Python model of pair scoring: mem_pair (reference src/bwamem_pair.cpp:372-433), the second step of mem_sam_pe -- the one the
device stage meme_pair_batch_host runs.

workload(): a list of batches (a call of the stage each: records, offsets, n_pri, the four orientations, the id of pair 0), over the three contigs of
the fixture genome.  The first batch is the workload of tests/primary_gen.py as the primary stage leaves it, paired as the reads come: real record
shapes, mostly unpairable.  The others are synthetic: every orientation alone alive, alone failed and all failed, with distances at low - 1, low, high
and high + 1, mates on two contigs and at a contig's first base, both strands on either side of l_pac; pairs of 2, 8, 9, 64, 65, 257 and 520 keys (the
last beyond the heavy tier's LDS cap); scores that would be negative, |ns| at which erfc underflows, std == 0, candidates of equal q that the hash
orders, sub - q at tmp and tmp + 1; ids 0, 2^23 - 1, 2^23 (where id << 8 turns negative), 2^31 + 5 and near 2^40.  Two pairs hold two candidates of
equal q AND equal hash word, which the candidate's (k, i) then orders: pair ids 7553733 (candidates at sorted positions (0, 3) and (4, 6)) and
16244286 ((0, 1) and (8, 9)), found by a search of the 2^24 values `id << 8` takes over the candidates of twelve keys.  Inputs are regenerated from
seeds; tests/golden/pair_golden.npz holds the compiled reference's outputs.

model(): the function restated line by line -- the backward loop with its break, the y[] array, the two sorts -- with its branch counts.  log and erfc
are the C library's through ctypes (CPython's math.erfc is its own code).  Pair p of a batch has id id_base + p."""
import ctypes
import ctypes.util
import math
import os
from fractions import Fraction

import numpy as np

import primary_gen as PG
from common import GOLDEN

M64 = (1 << 64) - 1
INT_MIN = -(1 << 31)
L_PAC = 300000
CONTIGS = [(0, 100000, 0), (100000, 100000, 0), (200000, 100000, 1)]      # the fixture genome's (tests/finish_gen.py: workload()["contigs"])
SIZES = (2, 8, 9, 64, 65, 257, 520)                                       # keys of a pair the workload holds; the last is beyond the heavy tier's LDS cap
LDS_KEYS = 512                                                            # that cap (tuning key pair_lds_keys: its default)
EQUAL_HASH = {7553733: ((0, 3), (4, 6)), 16244286: ((0, 1), (8, 9))}      # pair id -> two candidates (k, i) whose hash words are equal
_CACHE = {}

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in ("log", "erfc"):
    getattr(_libm, _f).restype = ctypes.c_double
    getattr(_libm, _f).argtypes = [ctypes.c_double]
M_SQRT1_2 = 0.70710678118654752440


def default_opt(**kw):
    """mem_opt_init (reference src/bwamem.cpp:126-162)"""
    o = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1)
    o.update(kw)
    return o


# options besides the defaults under which the model is compared with the compiled reference, and the device stage with the model
OTHER = {"a-2": dict(a=2, b=8), "gaps-del": dict(o_del=12, e_del=3), "gaps-ins": dict(o_ins=2, e_ins=1, o_del=2, e_del=1, b=1), "mismatch": dict(b=14)}


def penalty(dist, avg, std, a):
    """.721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * opt->a (:407-408), by the C library"""
    num = float(dist) - avg
    if std == 0.0:
        ns = math.nan if num == 0.0 or math.isnan(num) else math.copysign(math.inf, num)
    else:
        ns = num / std
    return .721 * _libm.log(2. * _libm.erfc(abs(ns) * M_SQRT1_2)) * a


def c_int(v):
    """(int)v as x86's cvttsd2si leaves it: INT_MIN for a NaN, an infinity and everything outside the range"""
    if v != v or v in (math.inf, -math.inf) or v >= 2147483648.0 or v <= -2147483649.0:
        return INT_MIN
    return int(v)


def idx_of(pair_id):
    """`id << 8` on the int the prototype truncates the id to, as a 64-bit operand of ^"""
    w = ((pair_id & 0xffffffff) << 8) & 0xffffffff
    return (w - (1 << 32)) & M64 if w >> 31 else w


def _ulps(x, n):
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def counters():
    C = dict(n_called=0, n_cand=0, n_with_cand=0, n_break=0, n_low_skip=0, n_which_skip=0, n_failed_skip=0, n_no_hit=0, n_neg_q=0, n_underflow=0, n_nan=0, n_tie_q=0,
             n_tie_hash=0, n_sub_at_tmp=0, n_sub_over_tmp=0, n_two_contigs=0, n_first_base=0, n_rev=0, n_fwd=0, n_at_l_pac=0, n_below_l_pac=0, n_idx_negative=0, n_id_high=0,
             n_at_low=0, n_at_high=0, n_below_low=0, n_above_high=0, n_unstable=0, n_multi=0, n_beyond_lds=0)
    for d in range(4):
        C["n_dir%d" % d] = 0
    return C


def mem_pair(o, pes, a, n_pri, pair_id, C, check=False):
    """mem_pair: a = the records of the two ends as lists of (rb, rid, score); -> (ret, sub, n_sub, z, u.n).  check: every q is also evaluated with the penalty moved by
    8 ulp either way and with `x * a + s` as one fused multiply-add; C["n_unstable"] counts the candidates where that changes q."""
    v = []
    for r in range(2):
        for i in range(n_pri[r]):
            rb, rid, score = a[r][i]
            x = rb if rb < L_PAC else (L_PAC << 1) - 1 - rb
            x = ((rid << 32) & M64) | ((x - CONTIGS[rid][0]) & M64)
            v.append((x, ((score << 32) & M64) | i << 2 | (rb >= L_PAC) << 1 | r))
            C["n_first_base"] += (x & 0xffffffff) == 0
            C["n_rev" if rb >= L_PAC else "n_fwd"] += 1
            C["n_at_l_pac"] += rb == L_PAC
            C["n_below_l_pac"] += rb == L_PAC - 1
    C["n_two_contigs"] += len({x >> 32 for x, _ in v}) > 1
    v.sort()                                                      # ks_introsort_128: pair64_lt is a strict total order here (every y is distinct)
    u = []
    y = [-1, -1, -1, -1]
    idx = idx_of(pair_id)
    for i in range(len(v)):
        for r in range(2):
            d = r << 1 | (v[i][1] >> 1 & 1)
            if pes[d][2]:
                C["n_failed_skip"] += 1
                continue
            which = r << 1 | ((v[i][1] & 1) ^ 1)
            if y[which] < 0:
                C["n_no_hit"] += 1
                continue
            k = y[which]
            while k >= 0:
                if (v[k][1] & 3) != which:
                    C["n_which_skip"] += 1
                    k -= 1
                    continue
                dist = v[i][0] - v[k][0]                          # (never negative: the keys are sorted)
                if dist > pes[d][1]:
                    C["n_break"] += 1
                    C["n_above_high"] += dist == pes[d][1] + 1
                    break
                if dist < pes[d][0]:
                    C["n_low_skip"] += 1
                    C["n_below_low"] += dist == pes[d][0] - 1
                    k -= 1
                    continue
                s = (v[i][1] >> 32) + (v[k][1] >> 32)
                t = penalty(dist, pes[d][3], pes[d][4], 1)
                T = t * o["a"]
                q = c_int(float(s) + T + .499)
                if check:
                    for T2 in (_ulps(T, 8), _ulps(T, -8)) if T == T and abs(T) != math.inf else ():
                        C["n_unstable"] += c_int(float(s) + T2 + .499) != q
                    if t == t and abs(t) != math.inf:
                        C["n_unstable"] += c_int(float(Fraction(t) * o["a"] + s) + .499) != q
                C["n_underflow"] += T == -math.inf
                C["n_nan"] += T != T
                C["n_neg_q"] += INT_MIN < q < 0
                C["n_dir%d" % d] += 1
                C["n_at_low"] += dist == pes[d][0]
                C["n_at_high"] += dist == pes[d][1]
                if q < 0:
                    q = 0
                py = (k << 32) | i
                u.append(((q << 32) | (PG.hash_64(py ^ idx) & 0xffffffff), py))
                k -= 1
        y[v[i][1] & 3] = i
    C["n_called"] += 1
    C["n_cand"] += len(u)
    z = [-1, -1]
    if u:
        tmp = max(o["a"] + o["b"], o["o_del"] + o["e_del"], o["o_ins"] + o["e_ins"])
        u.sort()
        i, k = u[-1][1] >> 32, u[-1][1] & 0xffffffff
        z[v[i][1] & 1] = (v[i][1] & 0xffffffff) >> 2
        z[v[k][1] & 1] = (v[k][1] & 0xffffffff) >> 2
        ret = u[-1][0] >> 32
        sub = u[-2][0] >> 32 if len(u) > 1 else 0
        n_sub = 0
        for j in range(len(u) - 2, -1, -1):
            if sub - (u[j][0] >> 32) <= tmp:
                n_sub += 1
            C["n_sub_at_tmp"] += sub - (u[j][0] >> 32) == tmp
            C["n_sub_over_tmp"] += sub - (u[j][0] >> 32) == tmp + 1
        C["n_with_cand"] += 1
        C["n_multi"] += len(u) > 2
        if len(u) > 1:
            C["n_tie_hash"] += u[-1][0] == u[-2][0]
            C["n_tie_q"] += u[-1][0] >> 32 == u[-2][0] >> 32 and u[-1][0] != u[-2][0]
    else:
        ret = sub = n_sub = 0
    C["n_idx_negative"] += idx >> 63
    C["n_id_high"] += pair_id >= 1 << 31
    C["n_beyond_lds"] += len(v) > LDS_KEYS
    return ret, sub, n_sub, z, len(u)


def model(B, opt=None, check=False, C=None):
    """a batch of workload() -> dict(score, sub, n_sub, n_cand (int32 per pair), z (pairs x 2), status (zeros: the model runs what the reference can), counters)"""
    o = opt or default_opt()
    C = counters() if C is None else C
    off, n_pri = B["reg_off"], B["n_pri"]
    npairs = (off.shape[0] - 1) // 2
    rb, rid, score = B["regs"]["rb"].tolist(), B["regs"]["rid"].tolist(), B["regs"]["score"].tolist()
    out = {k: np.zeros(npairs, np.int32) for k in ("score", "sub", "n_sub", "n_cand")}
    out["z"] = np.full((npairs, 2), -1, np.int32)
    out["status"] = np.zeros(npairs, np.uint8)
    for p in range(npairs):
        n = [int(n_pri[2 * p]), int(n_pri[2 * p + 1])]
        if n[0] == 0 or n[1] == 0:                               # (mem_sam_pe calls mem_pair only where both ends have records, :931)
            continue
        a = [[(rb[k], rid[k], score[k]) for k in range(int(off[2 * p + r]), int(off[2 * p + r]) + n[r])] for r in range(2)]
        out["score"][p], out["sub"][p], out["n_sub"][p], out["z"][p], out["n_cand"][p] = mem_pair(o, B["pes"], a, n, B["id_base"] + p, C, check)
    out["counters"] = C
    return out


# ---- the workload ------------------------------------------------------------------------------------------------------------------------
# (low, high, failed, avg, std) of FF, FR, RF, RR
PES = [(10, 400, 0, 200.0, 60.0), (50, 650, 0, 350.0, 50.0), (0, 300, 0, 120.0, 40.0), (20, 500, 0, 250.0, 70.0)]


def _with(pes, **kw):
    """PES with failed flags (failed=(...)), or a field of every orientation replaced (std=..., avg=...)"""
    out = []
    for d, (lo, hi, f, avg, std) in enumerate(pes):
        out.append((lo, hi, int(d in kw["failed"]) if "failed" in kw else f, kw.get("avg", avg), kw.get("std", std)))
    return out


def rec(rid, kp, rev, score, length=100):
    """a record whose key position (its forward position within contig rid) is kp, on the reverse strand if rev"""
    f = CONTIGS[rid][0] + kp
    rb = 2 * L_PAC - 1 - f if rev else f
    return dict(rb=rb, re=rb + length, qb=0, qe=length, rid=rid, score=score, truesc=score, secondary=-1, secondary_all=-1, seedlen0=19, w=100, n_comp_is_alt=1, seedcov=length // 2)


def _orientation_pairs(pes, rng):
    """for every orientation (strand of the earlier key, strand of the later) and which end comes first: the later key at low - 1, low, inside, high and high + 1"""
    pairs = []
    for sk in (0, 1):
        for si in (0, 1):
            lo, hi = pes[sk << 1 | si][0], pes[sk << 1 | si][1]
            for first_end in (0, 1):
                for dist in (lo - 1, lo, (lo + hi) // 2, int(rng.integers(lo, hi + 1)), hi, hi + 1):
                    if dist < 0:
                        continue
                    base = int(rng.integers(2000, 90000))
                    rid = int(rng.integers(0, 3))
                    k, i = rec(rid, base, sk, int(rng.integers(30, 150))), rec(rid, base + dist, si, int(rng.integers(30, 150)))
                    ends = [[k], [i]] if first_end == 0 else [[i], [k]]
                    if rng.random() < 0.3:                       # a second record on one end, out of every range
                        ends[int(rng.integers(0, 2))].append(rec(rid, base + 5000, int(rng.integers(0, 2)), 40))
                    pairs.append(ends)
    return pairs


def _random_pair(rng, n0, n1, span, rids=(0,), scores=(30, 150)):
    ends = []
    for n in (n0, n1):
        ends.append([rec(int(rng.choice(rids)), 1000 + int(rng.integers(0, span)), int(rng.integers(0, 2)), int(rng.integers(*scores))) for _ in range(n)])
    return ends


def _sized_pair(rng, m):
    """m keys, about half on either end, close enough together that most keys have candidates"""
    n0 = m // 2 if m > 2 else 1
    return _random_pair(rng, n0, m - n0, 700 if m < 100 else 1500)


def _edge_pairs(rng):
    pairs = []
    for _ in range(6):
        pairs.append([[rec(0, 500, 0, 80)], [rec(1, 800, 1, 70)]])                                  # mates on two contigs: the distance is beyond every high
        pairs.append([[rec(0, 99990, 0, 80)], [rec(1, 60, 1, 70)]])                                 # ... 170 bases apart in the genome, all the same
    for rid in (0, 1, 2):
        pairs.append([[rec(rid, 0, 0, 90)], [rec(rid, 300, 1, 90)]])                                # the first base of a contig
        pairs.append([[rec(rid, 300, 0, 90)], [rec(rid, 0, 1, 90)], ])                              # ... as the reverse mate's key: a candidate of RF at 300 (its high)
        pairs.append([[rec(rid, 0, 1, 60), rec(rid, 0, 0, 50)], [rec(rid, 0, 0, 55), rec(rid, 120, 1, 45)]])       # equal x: y orders the keys
    pairs.append([[rec(2, 99999, 0, 100, length=1)], [rec(2, 99999 - 200, 0, 90)]])                 # rb = l_pac - 1: the last forward base
    pairs.append([[rec(2, 99999, 1, 100)], [rec(2, 99999 - 300, 0, 90)]])                           # rb = l_pac: the first reverse base
    pairs.append([[rec(2, 99999, 1, 100), rec(2, 99999, 0, 100, length=1)], [rec(2, 99999 - 300, 0, 90), rec(2, 99999 - 100, 1, 95)]])
    pairs.append([[rec(0, 0, 1, 100)], [rec(0, 250, 1, 90)]])                                       # rb = 2 l_pac - 1: the last reverse base
    for k in range(10):                                          # records behind n_pri do not take part: the only proper mate is one of them
        pairs.append({"ends": [[rec(0, 5000, 0, 100), rec(0, 5350, 1, 90)], [rec(0, 40000, 1, 80), rec(0, 5350 + k, 1, 99)]], "n_pri": [1 + k % 2, 1]})
    for k in range(6):                                           # an end without records that take part: the reference does not call the function
        pairs.append({"ends": [[rec(0, 5000, 0, 100)], [rec(0, 5350, 1, 90)]], "n_pri": [(0, 1, 0)[k % 3], (1, 0, 0)[k % 3]]})
    pairs.append([[], [rec(0, 5350, 1, 90)]])
    pairs.append([[], []])
    return pairs


def _score_pairs(rng, tmp):
    """one record on end 0 and several on end 1 at the mean distance of FR (the penalty is .721 log 2 there: q is the sum of the scores): the q of the candidates by choice"""
    pairs = []

    def fan(scores, s0=50, at=350):
        order = rng.permutation(len(scores))
        return [[rec(0, 3000, 0, s0)], [rec(0, 3000 + at, 1, int(scores[j])) for j in order]]
    for _ in range(12):
        pairs.append(fan([60, 50, 50 - tmp]))                    # sub - q == tmp: counted
        pairs.append(fan([60, 50, 50 - tmp - 1]))                # tmp + 1: not counted
        pairs.append(fan([60, 50, 50 - tmp, 50 - tmp - 1, 50, 49, 20]))
        pairs.append(fan([60, 60]))                              # equal q: the hash orders the two
        pairs.append(fan([60, 60, 60, 60]))
        pairs.append(fan([70]))                                  # a single candidate: sub 0
    for _ in range(12):                                          # small scores far from the mean: q would be negative
        pairs.append([[rec(0, 3000, 0, int(rng.integers(0, 6)))], [rec(0, 3000 + int(rng.choice([50, 60, 640, 650])), 1, int(rng.integers(0, 6)))]])
        pairs.append([[rec(0, 3000, 0, 0)], [rec(0, 3350, 1, 0)]])                                   # scores 0 at the mean: q 0 from .9988
    return pairs


def _equal_hash_pair(pair_id):
    """the pair whose id is pair_id: fillers keep the candidates where EQUAL_HASH puts them (end 0: forward keys; end 1: reverse keys, and forward fillers; FR alone is alive)"""
    (k1, i1), (k2, i2) = EQUAL_HASH[pair_id]
    m = i2 + 1
    ends = [[], []]
    for p in range(m):
        cluster = 0 if p <= i1 else 1
        kp = 2000 + 40000 * cluster + 10 * p                     # ascending with p; the clusters lie far beyond high of each other
        if p in (k1, k2):
            ends[0].append(rec(0, kp, 0, 70))
        elif p in (i1, i2):
            ends[1].append(rec(0, 2000 + 40000 * cluster + 10 * (k1 if cluster == 0 else k2) + 350, 1, 60))      # 350 behind its k: equal scores and distances, equal q
        else:
            ends[1].append(rec(0, kp, 0, 80))
    return ends


def _batch(name, pairs, pes, id_base):
    from pymeme import hipapi
    rows, counts, n_pri = [], [], []
    for pr in pairs:
        ends = pr["ends"] if isinstance(pr, dict) else pr
        for r in range(2):
            rows += ends[r]
            counts.append(len(ends[r]))
            n_pri.append(pr["n_pri"][r] if isinstance(pr, dict) else len(ends[r]))
    regs = np.zeros(len(rows), hipapi.ALNREG)
    if rows:
        for f in rows[0]:
            regs[f] = [x[f] for x in rows]
    regs["c"] = np.arange(len(rows))
    return {"name": name, "regs": regs, "reg_off": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), "n_pri": np.array(n_pri, np.int32), "pes": pes, "id_base": id_base}


def workload():
    """-> list of batches: dict(name, regs (hipapi.ALNREG), reg_off, n_pri, pes (four (low, high, failed, avg, std)), id_base); contigs and l_pac are CONTIGS and L_PAC"""
    if "w" in _CACHE:
        return _CACHE["w"]
    rng = np.random.default_rng(20231)
    PW, G = PG.workload(), PG.golden()
    n = (PW["reg_off"].shape[0] - 1) // 2 * 2
    W = [{"name": "primary", "regs": PG.FG.take(G["regs"], np.arange(int(PW["reg_off"][n]))), "reg_off": PW["reg_off"][:n + 1].astype(np.int64), "n_pri": G["n_pri"][:n].astype(np.int32),
          "pes": [(0, 3000, 0, 500.0, 300.0), (50, 650, 0, 350.0, 50.0), (0, 2000, 0, 300.0, 150.0), (20, 1500, 0, 250.0, 70.0)], "id_base": 0}]
    tmp = 7
    # orientations: all alive, each alone failed, each alone alive, all failed; ids around 2^23
    masks = [()] + [(d,) for d in range(4)] + [tuple(x for x in range(4) if x != d) for d in range(4)] + [(0, 1, 2, 3)]
    for j, failed in enumerate(masks):
        pes = _with(PES, failed=failed)
        W.append(_batch("orient-" + "".join(map(str, failed)), _orientation_pairs(pes, rng) + [_sized_pair(rng, m) for m in (2, 8, 9, 16)], pes, (1 << 23) - 20 - 7 * j))
    W.append(_batch("edges", _edge_pairs(rng), PES, 0))
    W.append(_batch("sizes", [_sized_pair(rng, m) for m in SIZES for _ in range(3 if m < 300 else 1)] + [_random_pair(rng, 4, 4, 600, rids=(0, 1, 2)) for _ in range(60)], PES, (1 << 31) + 5))
    W.append(_batch("scores", _score_pairs(rng, tmp), PES, (1 << 40) - 40))
    W.append(_batch("scores-2^23", _score_pairs(rng, tmp), PES, (1 << 23) - 30))
    narrow = _with(PES, std=1.0)                                 # |ns| up to 300: erfc underflows, log(0) is -inf and q is 0; nearer the mean q would be negative
    W.append(_batch("underflow", [_random_pair(rng, 3, 3, 500, scores=(0, 40)) for _ in range(60)] + _orientation_pairs(narrow, rng), narrow, 77))
    zero = _with(PES, std=0.0)                                   # std == 0: ns is an infinity, or 0 / 0 at the mean
    W.append(_batch("std-0", [[[rec(0, 3000, 0, 50)], [rec(0, 3000 + d, 1, 60)]] for d in (350, 349, 351, 50, 650, 350)] + [_random_pair(rng, 3, 3, 500) for _ in range(30)] +
                    [[[rec(0, 7000, 0, 50), rec(0, 7010, 0, 40)], [rec(0, 7210, 0, 60), rec(0, 7200, 0, 45)]]], zero, 5))      # (FF: its mean is 200)
    only_fr = _with(PES, failed=(0, 2, 3))
    for pair_id in EQUAL_HASH:
        before = [_sized_pair(rng, m) for m in (2, 3, 8)]
        W.append(_batch("equal-hash-%d" % pair_id, before + [_equal_hash_pair(pair_id)] + [_sized_pair(rng, 4)], only_fr, pair_id - len(before)))
    _CACHE["w"] = W
    return W


def modelled():
    """the model's result on every batch of the workload with default options, the generator's checks on, and the counters of all batches together (computed once)"""
    if "m" not in _CACHE:
        C = counters()
        _CACHE["m"] = ([model(B, check=True, C=C) for B in workload()], C)
    return _CACHE["m"]


def floors(C, W):
    """the floors the workload was built to meet -> list of the ones it misses"""
    want = [("n_called", 1500), ("n_with_cand", 400), ("n_cand", 20000), ("n_break", 500), ("n_low_skip", 100), ("n_which_skip", 1000), ("n_failed_skip", 500), ("n_no_hit", 1000),
            ("n_neg_q", 20), ("n_underflow", 100), ("n_nan", 2), ("n_tie_q", 20), ("n_tie_hash", 2), ("n_sub_at_tmp", 20), ("n_sub_over_tmp", 20), ("n_two_contigs", 30),
            ("n_first_base", 9), ("n_rev", 1000), ("n_fwd", 1000), ("n_at_l_pac", 2), ("n_below_l_pac", 2), ("n_idx_negative", 100), ("n_id_high", 100), ("n_at_low", 30),
            ("n_at_high", 30), ("n_below_low", 15), ("n_above_high", 15), ("n_multi", 100), ("n_beyond_lds", 1)] + [("n_dir%d" % d, 200) for d in range(4)]
    missed = ["%s = %d < %d" % (k, C[k], v) for k, v in want if C[k] < v]
    m = set()
    for B in W:
        k = B["n_pri"][0::2] + B["n_pri"][1::2]
        m |= set(k[(B["n_pri"][0::2] > 0) & (B["n_pri"][1::2] > 0)].tolist())
    missed += ["no pair of %d keys" % k for k in SIZES if k not in m]
    ids = {B["id_base"] + p for B in W for p in range((B["reg_off"].shape[0] - 1) // 2)}
    missed += ["no pair with id %d" % k for k in (0, (1 << 23) - 1, 1 << 23, (1 << 31) + 5, (1 << 40) - 1) + tuple(EQUAL_HASH) if k not in ids]
    return missed


RESULT = ("score", "sub", "n_sub", "z")         # what the reference returns (n_cand, u.n, is the model's)


def golden():
    """tests/golden/pair_golden.npz: the compiled reference's outputs on the workload -> list of dict(score, sub, n_sub, z), a batch each"""
    G = np.load(os.path.join(GOLDEN, "pair_golden.npz"))
    out, at = [], 0
    for B in workload():
        n = (B["reg_off"].shape[0] - 1) // 2
        out.append({"score": G["score"][at:at + n], "sub": G["sub"][at:at + n], "n_sub": G["n_sub"][at:at + n], "z": G["z"][at:at + n]})
        at += n
    assert at == G["score"].shape[0], "the fixture is not of this workload"
    return out


def same(got, want, fields=RESULT):
    """exact equality of the fields, pair by pair; None or the first difference"""
    for f in fields:
        x, y = np.asarray(got[f]), np.asarray(want[f])
        if x.shape != y.shape:
            return "%s: shape %r, expected %r" % (f, x.shape, y.shape)
        bad = np.nonzero((x != y).reshape(x.shape[0], -1).any(axis=1))[0]
        if bad.size:
            p = int(bad[0])
            return "%s of pair %d: %r, expected %r (%d pairs differ)" % (f, p, x[p].tolist(), y[p].tolist(), bad.size)
    return None


def piece(B, p0, p1):
    """pairs [p0, p1) of a batch as a batch of their own (id_base moves with them)"""
    off = B["reg_off"]
    b, e = int(off[2 * p0]), int(off[2 * p1])
    return {"name": B["name"], "regs": PG.FG.take(B["regs"], np.arange(b, e)), "reg_off": off[2 * p0:2 * p1 + 1] - b, "n_pri": B["n_pri"][2 * p0:2 * p1], "pes": B["pes"], "id_base": B["id_base"] + p0}


def part(res, p0, p1):
    return {f: res[f][p0:p1] for f in res if f != "counters" and hasattr(res[f], "shape")}
