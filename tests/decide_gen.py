"""Workload and plain-Python model of the pairing decision: what mem_sam_pe does behind mem_pair (reference src/bwamem_pair.cpp:536-590, and its no_pairing
block's choice of records and flag, :632-648) -- the step the device stage meme_pair_decide_batch_* runs.

workload(): a list of batches of PRE-PRIMARY records (the reference's function marks primaries itself, and marking marked records again would count sub_n
twice): dict(name, regs, reg_off, pes, id_base = the id of pair 0, opt = the options that differ from the defaults).  Every record lies inside one contig
on one strand, spans as many query bases as reference bases (20 .. 250, truesc perfect: mem_reg2aln then writes an all-M CIGAR and the SAM position is the
record's own, which is how the fixture's generator finds a reported record by position and strand), and no two records of a read share contig, strand
and leftmost base.  The genome is that of tests/pair_gen.py (three contigs, the third ALT) with random bases from a seed, the reads random bases.

chain(B): the three models one behind the other as the stages chain -- tests/primary_gen.py (ids 2 P + r), tests/pair_gen.py (ids P + p), decide() here.
decide(): the block restated line by line on post-primary records and mem_pair's outputs; log is the C library's through ctypes.  direct(): batches that
no reference run can produce -- a pair-stage status, n_sub + 1 beyond the table of logarithms, an is_alt bit cleared behind n_pri -- for the stage alone.
"""
import ctypes
import ctypes.util
import os

import numpy as np

import pair_gen as QG
import primary_gen as PG
from common import GOLDEN

L_PAC, CONTIGS = QG.L_PAC, QG.CONTIGS
NAMES = ("c0", "c1", "c2alt")
READ_LEN = 250
SIZES = (1, 2, 8, 9, 63, 64, 65, 130, 520)        # records of a read the workload holds
LOG_TABLE = PG.LOG_TABLE
F32 = np.float32
_CACHE = {}

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.log.restype = ctypes.c_double
_libm.log.argtypes = [ctypes.c_double]

# (low, high, failed, avg, std) of FF, FR, RF, RR
PES = [(10, 400, 0, 200.0, 60.0), (10, 900, 0, 350.0, 50.0), (0, 300, 0, 120.0, 40.0), (20, 500, 0, 250.0, 70.0)]


def default_opt(**kw):
    """mem_opt_init (reference src/bwamem.cpp:126-162), the fields the three steps read"""
    o = dict(PG.default_opt(), pen_unpaired=17, no_pairing=0)
    o.update(kw)
    return o


def c_int(v):
    return int(v)                                    # (int) of a double truncates towards zero; every value here is far inside the int range


def raw_mapq(diff, a):
    return c_int(6.02 * diff / a + .499)


def infer_dir(b1, b2):
    """mem_infer_dir, :58-65"""
    r1, r2 = b1 >= L_PAC, b2 >= L_PAC
    p2 = b2 if r1 == r2 else (L_PAC << 1) - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), (p2 - b1 if p2 > b1 else b1 - p2)


class _Rec:
    __slots__ = ("qb", "qe", "rb", "re", "rid", "score", "is_alt", "sub", "csub", "sub_n", "secondary", "secondary_all", "frac_rep", "f32")


def _recs(regs, b, e):
    out = []
    for k in range(b, e):
        r = regs[k]
        p = _Rec()
        for f in ("qb", "qe", "rb", "re", "rid", "score", "sub", "csub", "sub_n", "secondary", "secondary_all"):
            setattr(p, f, int(r[f]))
        p.is_alt = (int(r["n_comp_is_alt"]) >> 30) & 3
        p.f32 = F32(r["frac_rep"])
        p.frac_rep = float(p.f32)
        out.append(p)
    return out


def counters():
    keys = ("path0", "path1", "path2", "path3", "cause_n_pri", "cause_score", "cause_flag", "multi0_only", "multi1_only", "o_eq_un", "o_eq_un1", "subo_below", "subo_above", "n_sub0", "n_sub1",
            "n_sub_large", "q_pe_clamp0", "q_pe_clamp60", "frac_float", "c_parent0", "c_parent1", "arm_se", "arm_pe", "arm_40", "csub_cap", "swap", "swap_k_neg", "swap_k_alt",
            "sib_before", "sib_after", "alt_yes", "alt_low", "alt_secondary", "alt_not_alt", "which0", "which_alt", "which_none", "np_flag", "np_low", "np_high", "np_failed", "np_rid",
            "np_dir0", "np_dir1", "np_dir2", "np_dir3", "status1")
    return {k: 0 for k in keys}


def decide_pair(o, pes, a, n_pri, score, sub, n_sub, z, C):
    """the block for one pair: a = the records of the two ends (lists of _Rec, changed in place) -> (path, sel, q_se, q_pe, flag, alt, beyond)"""
    T = o["T"]

    def no_pairing(path):                            # :632-648
        which = [-1, -1]
        for i in range(2):
            if a[i]:
                if a[i][0].score >= T:
                    which[i] = 0
                elif n_pri[i] < len(a[i]) and a[i][n_pri[i]].score >= T:
                    which[i] = n_pri[i]
            C["which0" if which[i] == 0 else "which_alt" if which[i] > 0 else "which_none"] += 1
        rid = [a[i][which[i]].rid if which[i] >= 0 else -1 for i in range(2)]
        flag = 1
        if not o["no_pairing"] and rid[0] == rid[1] and rid[0] >= 0:
            d, dist = infer_dir(a[0][0].rb, a[1][0].rb)
            if not pes[d][2] and pes[d][0] <= dist <= pes[d][1]:
                flag |= 2
                C["np_flag"] += 1
                C["np_dir%d" % d] += 1
            C["np_failed"] += bool(pes[d][2])
            C["np_low"] += dist == pes[d][0] - 1
            C["np_high"] += dist == pes[d][1] + 1
        elif not o["no_pairing"] and min(rid) >= 0:
            C["np_rid"] += 1
        return path, which, [0, 0], 0, flag, [-1, -1], False

    if o["no_pairing"]:                              # :533
        C["path0"] += 1
        C["cause_flag"] += 1
        return no_pairing(0)
    if not (n_pri[0] and n_pri[1] and score > 0):    # :536
        C["path0"] += 1
        C["cause_n_pri" if not (n_pri[0] and n_pri[1]) else "cause_score"] += 1
        return no_pairing(0)
    multi = [0, 0]
    for i in range(2):                               # :541-545
        j = 1
        while j < n_pri[i]:
            if a[i][j].secondary < 0 and a[i][j].score >= T:
                break
            j += 1
        multi[i] = 1 if j < n_pri[i] else 0
    if multi[0] or multi[1]:
        C["path1"] += 1
        C["multi0_only"] += multi == [1, 0]
        C["multi1_only"] += multi == [0, 1]
        return no_pairing(1)
    score_un = a[0][0].score + a[1][0].score - o["pen_unpaired"]
    C["o_eq_un"] += score == score_un
    C["o_eq_un1"] += score == score_un + 1
    C["subo_below"] += sub < score_un
    C["subo_above"] += sub > score_un
    C["n_sub0"] += n_sub == 0
    C["n_sub1"] += n_sub == 1
    C["n_sub_large"] += n_sub >= 20
    subo = sub if sub > score_un else score_un
    q_pe = raw_mapq(score - subo, o["a"])
    beyond = False
    if n_sub > 0:
        if n_sub + 1 >= LOG_TABLE:
            beyond = True
        else:
            q_pe -= c_int(4.343 * _libm.log(float(n_sub + 1)) + .499)
    C["q_pe_clamp0"] += q_pe < 0
    C["q_pe_clamp60"] += q_pe > 60
    q_pe = min(max(q_pe, 0), 60)
    f = a[0][0].f32 + a[1][0].f32                    # float + float, as x86-64 evaluates it
    wide = c_int(q_pe * (1. - .5 * (a[0][0].frac_rep + a[1][0].frac_rep)) + .499)
    q_pe = c_int(q_pe * (1. - .5 * float(f)) + .499)
    C["frac_float"] += wide != q_pe
    q_se = [0, 0]
    for i in range(2):                               # a logarithm of mem_approx_mapq_se beyond the table, asked before any record changes (sub: as :563-564 will leave it)
        c = a[i][z[i]] if score > score_un else a[i][0]
        sub_c = a[i][c.secondary].score if score > score_un and c.secondary >= 0 else c.sub
        if c.sub_n > 0 and c.sub_n + 1 >= LOG_TABLE and max(sub_c if sub_c else o["min_seed_len"] * o["a"], c.csub) < c.score:
            beyond = True
    if beyond:
        return 0, [-1, -1], [0, 0], 0, 1, [-1, -1], True
    if score > score_un:                             # :559-575
        path, flag = 3, 3
        z = [int(z[0]), int(z[1])]
        for i in range(2):
            c = a[i][z[i]]
            if c.secondary >= 0:
                c.sub = a[i][c.secondary].score
                c.secondary = -2
                C["c_parent%d" % i] += 1
            q = PG.mapq_se(o, c)
            C["arm_se" if q > q_pe else "arm_pe" if q_pe < q + 40 else "arm_40"] += 1
            q = q if q > q_pe else q_pe if q_pe < q + 40 else q + 40
            cap = raw_mapq(c.score - c.csub, o["a"])
            C["csub_cap"] += cap < q
            q_se[i] = q if q < cap else cap
    else:                                            # :576-580
        path, flag, z = 2, 1, [0, 0]
        q_se = [PG.mapq_se(o, a[0][0]), PG.mapq_se(o, a[1][0])]
    alt = [-1, -1]
    for i in range(2):                               # :581-590
        k = a[i][z[i]].secondary_all
        if 0 <= k < n_pri[i]:
            assert a[i][k].secondary_all < 0
            C["swap"] += 1
            sib = [j for j, p in enumerate(a[i]) if p.secondary_all == k and j != z[i]]
            C["sib_before"] += any(j < z[i] for j in sib)
            C["sib_after"] += any(j > z[i] for j in sib)
            for j, p in enumerate(a[i]):
                if p.secondary_all == k or j == k:
                    p.secondary_all = z[i]
            a[i][z[i]].secondary_all = -1
        else:
            C["swap_k_neg" if k < 0 else "swap_k_alt"] += 1
        if n_pri[i] < len(a[i]):                     # :603-605
            p = a[i][n_pri[i]]
            if p.score < T:
                C["alt_low"] += 1
            elif p.secondary >= 0:
                C["alt_secondary"] += 1
            elif not p.is_alt:
                C["alt_not_alt"] += 1
            else:
                alt[i] = n_pri[i]
                C["alt_yes"] += 1
    C["path%d" % path] += 1
    return path, z, q_se, q_pe, flag, alt, False


OUT = ("path", "sel", "q_se", "q_pe", "flag", "alt", "status")
MARKS = ("sub", "secondary", "secondary_all")


def decide(regs, reg_off, n_pri, pair, pes, opt=None, C=None):
    """post-primary records, mem_pair's outputs (score, sub, n_sub, z, status) -> dict(OUT..., regs: the changed copy, counters)"""
    o = opt or default_opt()
    C = counters() if C is None else C
    npairs = (reg_off.shape[0] - 1) // 2
    out = {"path": np.zeros(npairs, np.int32), "sel": np.full((npairs, 2), -1, np.int32), "q_se": np.zeros((npairs, 2), np.int32), "q_pe": np.zeros(npairs, np.int32),
           "flag": np.ones(npairs, np.int32), "alt": np.full((npairs, 2), -1, np.int32), "status": np.zeros(npairs, np.uint8), "regs": regs.copy(), "counters": C}
    for p in range(npairs):
        if pair["status"][p]:
            out["status"][p] = 1
            C["status1"] += 1
            continue
        b = [int(reg_off[2 * p]), int(reg_off[2 * p + 1]), int(reg_off[2 * p + 2])]
        a = [_recs(regs, b[0], b[1]), _recs(regs, b[1], b[2])]
        path, sel, q_se, q_pe, flag, alt, beyond = decide_pair(o, pes, a, [int(n_pri[2 * p]), int(n_pri[2 * p + 1])], int(pair["score"][p]), int(pair["sub"][p]), int(pair["n_sub"][p]),
                                                               pair["z"][p], C)
        if beyond:
            out["status"][p] = 1
            C["status1"] += 1
            continue
        out["path"][p], out["sel"][p], out["q_se"][p], out["q_pe"][p], out["flag"][p], out["alt"][p] = path, sel, q_se, q_pe, flag, alt
        for i in range(2):
            for j, r in enumerate(a[i]):
                for f in MARKS:
                    out["regs"][f][b[i] + j] = getattr(r, f)
    return out


def stage_opts(o):
    """the model's options -> (primary, pair, decide) keyword arguments of hipapi.default_*_opt"""
    pri = {k: o[k] for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "min_seed_len", "T", "mask_level", "mapQ_coef_len", "mapQ_coef_fac", "primary5")}
    pair = {k: o[k] for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins")}
    dec = {k: o[k] for k in ("a", "b", "pen_unpaired", "T", "min_seed_len", "mapQ_coef_len", "mapQ_coef_fac", "no_pairing")}
    return pri, pair, dec


def chain(B, C=None):
    """a batch of workload() through the three models -> dict(primary: PG.model's result, pair: QG.model's, decide: decide()'s)"""
    o = default_opt(**B["opt"])
    n = B["reg_off"].shape[0] - 1
    pm = PG.model(B["regs"], B["reg_off"], 2 * B["id_base"] + np.arange(n), o)
    assert not pm["status"].any()
    qm = QG.model({"regs": pm["regs"], "reg_off": B["reg_off"], "n_pri": pm["n_pri"], "pes": B["pes"], "id_base": B["id_base"]}, {k: o[k] for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins")})
    return {"primary": pm, "pair": qm, "decide": decide(pm["regs"], B["reg_off"], pm["n_pri"], qm, B["pes"], o, C)}


# ---- the workload ------------------------------------------------------------------------------------------------------------------------------
def rec(rid, kp, rev, score, qb=0, length=100, csub=0, sub_n=0, frac=0.0):
    """a pre-primary record whose key position (tests/pair_gen.py: rec) is kp in contig rid: query [qb, qb + length), as many reference bases, truesc perfect"""
    r = QG.rec(rid, kp, rev, score, length)
    r.update(qb=qb, qe=qb + length, truesc=length, csub=csub, sub_n=sub_n, frac_rep=frac, n_comp_is_alt=(CONTIGS[rid][2] << 30) | 1, seedcov=length // 2,
             sub=5, alt_sc=3, secondary=7, secondary_all=9)       # (stale marks: the primary step resets them)
    assert 20 <= length <= 250 and qb + length <= READ_LEN and (kp >= length - 1 if rev else kp + length <= CONTIGS[rid][1])
    return r


def leftmost(r):
    """(rid, strand, leftmost forward base within the contig): what a SAM line shows of a record"""
    rev = r["rb"] >= L_PAC
    return int(r["rid"]), int(rev), int((2 * L_PAC - r["re"] if rev else r["rb"]) - CONTIGS[int(r["rid"])][0])


def _distinct(ends):
    for e in ends:
        keys = [leftmost(r) for r in e]
        assert len(set(keys)) == len(keys), "two records of a read at one place"
    return ends


def _fr(rng, s0=100, s1=90, dist=350, rid=0, **kw):
    """a forward record on end 0 and a reverse one on end 1, `dist` behind it: one candidate of FR"""
    x = int(rng.integers(400, 60000))
    return [[rec(rid, x, 0, s0, **kw)], [rec(rid, x + dist, 1, s1, **kw)]]


def _fill(rng, end, n, x, parent_q=(0, 100), scores=(5, 28), rid=0, span=4000):
    """n more records on an end, all overlapping the record at query parent_q (secondaries of it, below T), around key position x"""
    have = {leftmost(r) for r in end}
    while n > 0:
        length = int(rng.integers(60, parent_q[1] - parent_q[0] + 1))
        r = rec(rid, x + int(rng.integers(-span, span)), int(rng.integers(0, 2)), int(rng.integers(*scores)), qb=parent_q[0] + int(rng.integers(0, parent_q[1] - parent_q[0] - length + 1)), length=length)
        if leftmost(r) not in have:
            have.add(leftmost(r))
            end.append(r)
            n -= 1
    return end


def _find_frac(rng):
    """(q, f0, f1): q_pe before :556 and two frac_rep whose float sum gives another q_pe than their double sum; q from what one candidate gives (6.02 d)"""
    for _ in range(400000):
        q = int(rng.choice([6, 12, 18, 24, 30, 36, 42, 48, 54, 60]))
        n = int(rng.integers(q // 2, q))
        t = 2. * (1. - (n + .501) / q)                # the sum at which q (1 - .5 s) + .499 crosses n + 1
        f0 = F32(rng.uniform(0.05, 0.95) * t)
        f1 = F32(t - float(f0))
        for _ in range(int(rng.integers(0, 4))):
            f1 = np.nextafter(f1, F32(rng.choice([0.0, 1.0])))
        wide = c_int(q * (1. - .5 * (float(f0) + float(f1))) + .499)
        if 0 < f1 < 1 and c_int(q * (1. - .5 * float(f0 + f1)) + .499) != wide:
            return q, float(f0), float(f1)
    return None


def _pairs_paths(rng):
    P = []
    for _ in range(30):
        P.append(_fr(rng, int(rng.integers(40, 150)), int(rng.integers(40, 150)), int(rng.integers(250, 450))))          # near the mean: the paired alignment preferred
        P.append(_fr(rng, int(rng.integers(40, 150)), int(rng.integers(40, 150)), int(rng.choice([20, 30, 700, 850]))))   # far from it: the unpaired one
        P.append(_fr(rng, 100, 90, 2000))                                                                                 # no candidate: o = 0
        P.append([[rec(0, 5000, 0, 80)], [rec(1, 5300, 1, 70)]])                                                          # two contigs
    for k in range(12):                              # an end without records, or without primaries (ALT only)
        P.append([[], [rec(0, 5000, 1, 80)]] if k % 3 == 0 else [[rec(0, 5000, 0, 80)], []] if k % 3 == 1 else [[], []])
        P.append([[rec(2, 5000 + k, 0, 25 + k)], [rec(2, 5300, 1, 70)]])                                                   # n_pri 0, 0; the ALT records' distance in range: the flag, by FR
        P.append([[rec(2, 5000, 0, 60)], [rec(0, 5300 + k, 1, 70)]])
    return P


def _pairs_scores(rng, pes):
    """o against score_un by the distance: one candidate, q = s0 + s1 + (int)(T + .499) with T from the table of FR"""
    P = []
    lo, hi, _, avg, std = pes[1]
    want = {}
    for dist in range(lo, hi + 1):
        d = QG.c_int(190. + QG.penalty(dist, avg, std, 1) + .499) - 190
        want.setdefault(d, dist)
    for d in (-17, -16, -15, -12, -8, -7, -1, 0, -18, -19, -30):
        if d in want:
            for _ in range(4):
                P.append(_fr(rng, 100, 90, want[d], csub=int(rng.choice([0, 0, 85, 95])), frac=float(F32(rng.choice([0, 0.25, 0.6])))))
    assert -17 in want and -16 in want
    found = _find_frac(rng)
    assert found is not None, "no frac_rep pair whose float sum changes q_pe"
    q, f0, f1 = found
    d = {6 * k: k for k in range(1, 10)}.get(q, 10)   # o - score_un
    for _ in range(3):
        e = _fr(rng, 100, 90, want[d - 17])
        e[0][0]["frac_rep"], e[1][0]["frac_rep"] = f0, f1
        P.append(e)
    return P


def _pairs_secondary(rng):
    """the better pairing goes through a secondary record of an end: c[i] has a parent, and the swap makes it the primary"""
    P = []
    for k in range(40):
        x = int(rng.integers(6000, 50000))
        e0 = [rec(0, x, 0, 100, csub=int(rng.choice([0, 60, 99])), sub_n=int(rng.choice([0, 0, 3])))]
        e1 = [rec(0, x + 30000, 1, 95), rec(0, x + 350, 1, int(rng.integers(35, 94)), qb=int(rng.integers(0, 30)), length=int(rng.integers(80, 101)))]      # the far record scores more; the near one is its secondary
        n_sib = (0, 1, 3, 7)[k % 4]
        _fill(rng, e1, n_sib, x + 30000, scores=(5, 94 if k % 8 < 4 else 30))       # siblings: other secondaries of the same parent, before and after z by score
        if k % 5 == 0:                               # both ends
            e0 += [rec(0, x + 60000 if x < 30000 else x - 5000, 0, 120)]
        if k % 7 == 0:                               # an ALT record behind the primaries: reported, below T, or a secondary of a primary
            e1.append(rec(2, 7000 + k, 0, (50, 20, 40)[k // 7 % 3], qb=(120, 120, 0)[k // 7 % 3], length=100))
        P.append([e0, e1] if k % 2 == 0 else [e1, e0])
    for k in range(12):                              # z's parent is an ALT record: k >= n_pri, no swap
        x = int(rng.integers(6000, 50000))
        P.append([[rec(0, x, 0, 100)], [rec(2, 3000 + k, 0, 120), rec(0, x + 350, 1, 80)]])
    return P


def _pairs_multi(rng, pes):
    """an end with a second primary of score >= T: left through is_multi; the flag of no_pairing by record 0 of either end"""
    P = []
    for sk in (0, 1):
        for si in (0, 1):
            d = sk << 1 | si
            lo, hi = pes[d][0], pes[d][1]
            for dist in (lo - 1, lo, (lo + hi) // 2, hi, hi + 1):
                if dist < 0:
                    continue
                for multi_end in (0, 1):
                    x = int(rng.integers(3000, 40000))
                    A, B = rec(0, x, sk, 100), rec(0, x + dist, si, 90)
                    M = rec(0, x + 50000, 0, 60, qb=120, length=100)                     # a second primary
                    Cc = rec(0, x + 50350, 1, 40, qb=10, length=80)                      # ... and its mate, a secondary of the other end's record 0: o > 0 whatever A and B do
                    ends = [[A, M], [B, Cc]]
                    if multi_end:                    # the second primary on end 1, its mate a secondary of end 0's record 0
                        ends = [[A, rec(0, x + 50350, 1, 40, qb=10, length=80)], [B, rec(0, x + 50000, 0, 60, qb=120, length=100)]]
                    P.append(ends)
    for k in range(8):                               # different rid, and which = the ALT record / none under a multi end
        x = int(rng.integers(3000, 40000))
        P.append([[rec(0, x, 0, 100), rec(0, x + 50000, 0, 60, qb=120, length=100)], [rec(1, x + 350, 1, 90), rec(0, x + 50350, 1, 40, qb=10, length=80)]])
        P.append([[rec(0, x, 0, 29), rec(2, x + 100, 0, 60, qb=120, length=100)], [rec(0, x + 20000, 1, 90)]])          # record 0 below T, the ALT record above: which = n_pri
        P.append([[rec(0, x, 0, 29), rec(2, x + 100, 0, 28, qb=120, length=100)], [rec(0, x + 20000, 1, 25)]])          # none
    return P


def _pairs_sizes(rng):
    """reads of every size of SIZES: one primary, a second at times, and secondaries of the first; mates that pair with a secondary of the big read"""
    P = []
    for m in SIZES:
        for v in range(3 if m < 200 else 1):
            x = int(rng.integers(8000, 50000))
            big = [rec(0, x + 30000, 0, 100)]
            if m >= 2:
                big.append(rec(0, x, 0, int(rng.integers(35, 95)), qb=int(rng.integers(0, 20)), length=int(rng.integers(80, 101))))
            _fill(rng, big, m - len(big), x, scores=(5, 95 if v else 28))
            if v == 2 and m >= 9:
                big.append(rec(2, 9000 + m, 0, 50, qb=130, length=100))
                big.pop(2)
            other = [rec(0, x + 350, 1, 90)]
            if v == 1:
                _fill(rng, other, min(m, 130) - 1, x + 350, scores=(5, 60))
            P.append([big, other] if v != 1 else [other, big])
    for k in range(6):                               # many mates of nearly the best score at nearly the best distance: n_sub large
        x = int(rng.integers(8000, 50000))
        e1 = [rec(0, x + 350, 1, 90)] + [rec(0, x + 352 + j, 1, 84 + j % 6, qb=j % 20, length=80) for j in range(25 + 10 * k)]
        P.append([[rec(0, x, 0, 100)], e1] if k % 2 else [e1, [rec(0, x, 0, 100)]])
    return P


def _pairs_random(rng, n):
    P = []
    for _ in range(n):
        ends = []
        x = int(rng.integers(8000, 50000))
        for i in range(2):
            e = []
            for j in range(int(rng.integers(1, 3))):
                e.append(rec(int(rng.choice([0, 0, 0, 2])), x + int(rng.integers(0, 600)), int(rng.integers(0, 2)), int(rng.integers(20, 120)), qb=130 * j, length=int(rng.integers(60, 120)),
                             csub=int(rng.choice([0, 0, 30, 80])), sub_n=int(rng.choice([0, 0, 2])), frac=float(F32(rng.choice([0, 0, 0.3, 0.9])))))
            _fill(rng, e, int(rng.integers(0, 12)), x + 300, scores=(5, 110), span=700)
            ends.append(e)
        P.append(ends)
    return P


def _batch(name, pairs, pes, id_base, **opt):
    B = QG._batch(name, [_distinct(p) for p in pairs], pes, id_base)
    del B["n_pri"]                                   # (pre-primary: n_pri comes out of the primary step)
    B["opt"] = opt
    B["regs"]["truesc"] = B["regs"]["truesc"] * opt.get("a", 1)       # (perfect under the batch's match score)
    return B


def workload():
    if "w" in _CACHE:
        return _CACHE["w"]
    rng = np.random.default_rng(61803)
    W = [_batch("paths", _pairs_paths(rng), PES, 0),
         _batch("scores", _pairs_scores(rng, PES), PES, 1000),
         _batch("secondary", _pairs_secondary(rng), PES, (1 << 23) - 10),
         _batch("multi", _pairs_multi(rng, PES), PES, 5000),
         _batch("multi-failed", _pairs_multi(rng, QG._with(PES, failed=(1, 2))), QG._with(PES, failed=(1, 2)), 6000),
         _batch("sizes", _pairs_sizes(rng), PES, 7000),
         _batch("random", _pairs_random(rng, 250), PES, 9000),
         _batch("one", _pairs_random(rng, 1), PES, 3),
         _batch("a-2", _pairs_random(rng, 60) + _pairs_scores(rng, PES)[:20], PES, 11000, a=2, b=8),
         _batch("pen-9", _pairs_random(rng, 60) + _pairs_secondary(rng)[:20], PES, 12000, pen_unpaired=9),
         _batch("T-50", _pairs_random(rng, 60) + _pairs_multi(rng, PES)[:30], PES, 13000, T=50),
         _batch("no-pairing", _pairs_random(rng, 40) + _pairs_paths(rng)[:30], PES, 14000, no_pairing=1)]
    _CACHE["w"] = W
    return W


def modelled():
    """chain() of every batch, and the counters of all batches together (computed once)"""
    if "m" not in _CACHE:
        C = counters()
        _CACHE["m"] = ([chain(B, C) for B in workload()], C)
    return _CACHE["m"]


def floors(C, W):
    """the floors the workload was built to meet -> list of the ones it misses"""
    want = [("path0", 100), ("path1", 60), ("path2", 40), ("path3", 150), ("cause_n_pri", 20), ("cause_score", 40), ("cause_flag", 60), ("multi0_only", 15), ("multi1_only", 15),
            ("o_eq_un", 4), ("o_eq_un1", 4), ("subo_below", 100), ("subo_above", 20), ("n_sub0", 100), ("n_sub1", 10), ("n_sub_large", 3), ("q_pe_clamp0", 30), ("q_pe_clamp60", 50),
            ("frac_float", 3), ("c_parent0", 10), ("c_parent1", 15), ("arm_se", 20), ("arm_pe", 20), ("arm_40", 10), ("csub_cap", 10), ("swap", 40), ("swap_k_neg", 200),
            ("swap_k_alt", 10), ("sib_before", 5), ("sib_after", 5), ("alt_yes", 5), ("alt_low", 2), ("alt_secondary", 2), ("which0", 200), ("which_alt", 6), ("which_none", 20),
            ("np_flag", 20), ("np_low", 4), ("np_high", 4), ("np_failed", 4), ("np_rid", 8)] + [("np_dir%d" % d, 3) for d in range(4)]
    missed = ["%s = %d < %d" % (k, C[k], v) for k, v in want if C[k] < v]
    sizes = set()
    for B in W:
        sizes |= set(np.diff(B["reg_off"]).tolist())
    missed += ["no read of %d records" % m for m in SIZES if m not in sizes]
    missed += ["no batch with %s" % k for k in ("a", "pen_unpaired", "T", "no_pairing") if not any(k in B["opt"] for B in W)]
    return missed


def direct():
    """batches for the stage alone (post-primary records and pair outputs handed in as they are): dict(name, regs, reg_off, n_pri, pair, pes, opt).  `status`: pairs of the
    "secondary" batch, of which one gets a pair-stage status, one n_sub = 65535 (n_sub + 1 is beyond the table) and one a record 0 with sub_n = 65535; `not-alt`: pairs whose
    record n_pri has its is_alt bit cleared (the primary step never leaves that)"""
    if "d" in _CACHE:
        return _CACHE["d"]
    W, (M, _) = workload(), modelled()
    out = []
    k = [B["name"] for B in W].index("secondary")
    B, m = W[k], M[k]
    pair = {f: m["pair"][f].copy() for f in ("score", "sub", "n_sub", "z", "status")}
    regs = m["primary"]["regs"].copy()
    p3 = np.nonzero(m["decide"]["path"] == 3)[0]
    pair["status"][p3[1]] = 1
    pair["n_sub"][p3[3]] = 65535
    pair["n_sub"][p3[4]] = 65534                      # (the last argument inside the table)
    def reaches(p):                                   # record z[0] of pair p has no parent and a quality that reaches the logarithm of sub_n + 1
        c = regs[int(B["reg_off"][2 * p]) + int(pair["z"][p][0])]
        return c["secondary"] < 0 and max(int(c["sub"]) or 19, int(c["csub"])) < c["score"]
    p6 = next(int(p) for p in p3[6:] if reaches(p))
    r = int(B["reg_off"][2 * p6]) + int(pair["z"][p6][0])
    regs["sub_n"][r] = 65535
    out.append({"name": "status", "regs": regs, "reg_off": B["reg_off"], "n_pri": m["primary"]["n_pri"], "pair": pair, "pes": B["pes"], "opt": {}, "expect_status1": sorted([int(p3[1]), int(p3[3]), p6])})
    regs = m["primary"]["regs"].copy()
    n_pri = m["primary"]["n_pri"]
    hit = 0
    for r in range(B["reg_off"].shape[0] - 1):
        b, e = int(B["reg_off"][r]), int(B["reg_off"][r + 1])
        if b + n_pri[r] < e:
            regs["n_comp_is_alt"][b + n_pri[r]] &= 0x3fffffff
            hit += 1
    assert hit >= 5
    out.append({"name": "not-alt", "regs": regs, "reg_off": B["reg_off"], "n_pri": n_pri, "pair": {f: m["pair"][f] for f in ("score", "sub", "n_sub", "z", "status")}, "pes": B["pes"], "opt": {}})
    _CACHE["d"] = out
    return out


def direct_modelled():
    if "dm" not in _CACHE:
        _CACHE["dm"] = [decide(D["regs"], D["reg_off"], D["n_pri"], D["pair"], D["pes"], default_opt(**D["opt"])) for D in direct()]
    return _CACHE["dm"]


# ---- genome and reads (what the reference's SAM step reads; the stages do not) --------------------------------------------------------------------
def genome():
    """L_PAC random bases (codes 0..3) and their pac image (four bases a byte, the first in the high bits: _get_pac)"""
    if "g" not in _CACHE:
        codes = np.random.default_rng(4242).integers(0, 4, L_PAC).astype(np.uint8)
        c = codes.reshape(-1, 4)
        _CACHE["g"] = (codes, (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8))
    return _CACHE["g"]


def read_codes(B, r):
    return np.random.default_rng(1000003 * B["id_base"] + r).integers(0, 4, READ_LEN).astype(np.uint8)


# ---- what the reference shows, and what the model says it shows -----------------------------------------------------------------------------------
OBS = ("n_lines", "flag0", "mapq0", "rec0", "mate")         # per read: SAM lines, FLAG and MAPQ of the first, the record it reports (-1: unmapped), the mate's record (-1: unmapped)


def observables_agree(B, m, obs, marks):
    """the reference's observables of a batch (obs: OBS -> int array per read; marks: MARKS -> array per record, behind the call) against chain()'s result m
    -> None or the first difference"""
    d = m["decide"]
    for f in MARKS:
        bad = np.nonzero(d["regs"][f] != marks[f])[0]
        if bad.size:
            return "%s of record %d: model %d, reference %d" % (f, bad[0], d["regs"][f][bad[0]], marks[f][bad[0]])
    for p in range(d["path"].shape[0]):
        for i in range(2):
            r = 2 * p + i
            if bool(obs["flag0"][r] & 2) != bool(d["flag"][p] & 2):
                return "proper-pair bit of read %d: model flag %d, reference FLAG %d" % (r, d["flag"][p], obs["flag0"][r])
            if obs["mate"][r] != d["sel"][p][1 - i]:
                return "mate record of read %d: model %d, reference %d (path %d)" % (r, d["sel"][p][1 - i], obs["mate"][r], d["path"][p])
            if d["path"][p] >= 2:
                got = (int(obs["rec0"][r]), int(obs["mapq0"][r]), int(obs["n_lines"][r]))
                want = (int(d["sel"][p][i]), int(d["q_se"][p][i]) & 0xff, 1 + int(d["alt"][p][i] >= 0))      # (mem_aln_t keeps eight bits of mapq: the cap is negative where csub > score)
                if got != want:
                    return "read %d (path %d): record, MAPQ, lines %r, model %r" % (r, d["path"][p], got, want)
    return None


def golden():
    """tests/golden/decide_golden.npz -> list of (obs, marks), a batch each"""
    G = np.load(os.path.join(GOLDEN, "decide_golden.npz"))
    out, at_r, at_k = [], 0, 0
    for B in workload():
        n, k = B["reg_off"].shape[0] - 1, B["regs"].shape[0]
        out.append(({f: G[f][at_r:at_r + n] for f in OBS}, {f: G[f][at_k:at_k + k] for f in MARKS}))
        at_r += n
        at_k += k
    assert at_r == G["n_lines"].shape[0] and at_k == G["sub"].shape[0], "the fixture is not of this workload"
    return out


def same(got, want, fields=OUT):
    return QG.same(got, want, fields)
