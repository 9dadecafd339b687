"""Workload and plain-Python model of primary marking and mapping quality: mem_mark_primary_se with mem_mark_primary_se_core (reference
src/bwamem.cpp:1974-2046), mem_reorder_primary5 (:2078-2100) and mem_approx_mapq_se (:2052-2076) -- the first and the third step of mem_sam_pe,
the ones the device stage meme_primary_batch_host runs.

workload(): the records tests/golden/finish_golden.npz holds (what mem_sort_dedup_patch_mate_sort leaves: exactly what the stage is handed) plus
synthetic reads for what they do not reach -- lists of non-overlapping primaries of 63, 64, 65 and 130 members (spans of 3 bases tile a
500-base read) with later records that overlap members of every 64-member chunk, reads of 8, 9, 64 and 65 records, quality inputs on both
sides of l = 50, sub >= score, csub > sub, sub_n > 0, qualities clipped at 60 and at 0, frac_rep of 0 and above, score 0, and one read with a
70 000-base reference span (beyond the stage's log table: status).  Inputs are regenerated from seeds; tests/golden/primary_golden.npz holds
the compiled reference's outputs.

model(): the functions restated step by step -- numpy.float32 for the overlap test, math.log and Python floats (IEEE double, no contraction)
for the quality -- with their branch counts.  Read r of a batch has id id_base + r (mem_mark_primary_se's `id`: record i hashes id + i)."""
import math
import os
from fractions import Fraction

import numpy as np

import finish_gen as FG
from common import GOLDEN

F32 = np.float32
INT_MAX = 2147483647
M64 = (1 << 64) - 1
LIST_LENGTHS = (63, 64, 65, 130)
READ_COUNTS = (8, 9, 64, 65)
ID_BASE = 1000              # the fixture: read r has id ID_BASE + r
OUT_FIELDS = ("sub", "alt_sc", "sub_n", "secondary", "secondary_all", "hash")      # what the functions write; every other field travels with its record
_CACHE = {}


def default_opt(**kw):
    """mem_opt_init (reference src/bwamem.cpp:126-162)"""
    o = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, min_seed_len=19, T=30, mask_level=0.5, mapQ_coef_len=50.0, mapQ_coef_fac=0, primary5=0)
    o.update(kw)
    if "mapQ_coef_fac" not in kw:
        o["mapQ_coef_fac"] = int(math.log(float(F32(o["mapQ_coef_len"]))))     # (:150: mapQ_coef_fac = log(mapQ_coef_len), an int)
    return o


# options besides the defaults under which the model is compared with the compiled reference, and the device stage with the model
OTHER = {"mask-0.3": dict(mask_level=0.3), "mask-0.95": dict(mask_level=0.95), "penalties": dict(a=2, b=3, o_del=4, e_del=2, o_ins=5, e_ins=1), "primary5": dict(primary5=1),
         "id-2^40": dict(id_base=(1 << 40) - 77)}


def split_other(name):
    """-> (model / stage options, id_base) of an entry of OTHER"""
    kw = dict(OTHER[name])
    id_base = kw.pop("id_base", ID_BASE)
    return kw, id_base


def hash_64(key):
    """reference src/utils.h:117"""
    key &= M64
    key = (key + (~(key << 32) & M64)) & M64
    key ^= key >> 22
    key = (key + (~(key << 13) & M64)) & M64
    key ^= key >> 8
    key = (key + (key << 3)) & M64
    key ^= key >> 15
    key = (key + (~(key << 27) & M64)) & M64
    key ^= key >> 31
    return key


class _Rec:
    __slots__ = ("src", "qb", "qe", "rb", "re", "score", "is_alt", "sub", "alt_sc", "csub", "sub_n", "secondary", "secondary_all", "hash", "frac_rep")


def _core(o, a, n, C):
    """mem_mark_primary_se_core over a[0..n)"""
    tmp = max(o["a"] + o["b"], o["o_del"] + o["e_del"], o["o_ins"] + o["e_ins"])
    ml = F32(o["mask_level"])
    z = [0]
    for i in range(1, n):
        p = a[i]
        for j in z:
            q = a[j]
            b_max = max(q.qb, p.qb)
            e_min = min(q.qe, p.qe)
            if e_min > b_max:
                min_l = min(p.qe - p.qb, q.qe - q.qb)
                lhs, rhs = F32(e_min - b_max), F32(min_l) * ml
                C["n_boundary"] += bool(lhs == rhs)
                if lhs >= rhs:
                    if q.sub == 0:
                        q.sub = p.score
                    if q.score - p.score <= tmp and (q.is_alt or not p.is_alt):
                        q.sub_n += 1
                    p.secondary = j
                    break
        else:
            z.append(i)
    C["z_max"] = max(C["z_max"], len(z))


def _mark(o, a, rid, C):
    """mem_mark_primary_se: a (list of _Rec, reordered in place) -> n_pri"""
    n = len(a)
    if n == 0:
        return 0
    n_pri = 0
    for i, p in enumerate(a):
        p.sub = p.alt_sc = 0
        p.secondary = p.secondary_all = -1
        p.hash = hash_64(rid + i)
        n_pri += not p.is_alt
    C["n_hash_reads"] += len({(p.score, p.is_alt) for p in a}) < n
    a.sort(key=lambda p: (-p.score, p.is_alt, p.hash))            # alnreg_hlt: a strict total order (hash_64 is a bijection)
    _core(o, a, n, C)
    for i, p in enumerate(a):
        p.secondary_all = i
        if not p.is_alt and p.secondary >= 0 and a[p.secondary].is_alt:
            p.alt_sc = a[p.secondary].score
            C["n_alt_sc"] += 1
    if n_pri < n:
        C["n_alt_and_pri" if n_pri else "n_alt_only"] += 1
        if n_pri > 0:
            a.sort(key=lambda p: (p.is_alt, -p.score, p.hash))    # alnreg_hlt2
        z = [0] * n
        for i, p in enumerate(a):
            z[p.secondary_all] = i
        for p in a:
            if p.secondary >= 0:
                p.secondary_all = z[p.secondary]
                if p.is_alt:
                    p.secondary = INT_MAX
            else:
                p.secondary_all = -1
        if n_pri > 0:
            for p in a[:n_pri]:
                p.sub, p.secondary = 0, -1
            _core(o, a, n_pri, C)                                 # (sub_n is not reset: counted twice, as the reference does)
    else:
        for p in a:
            p.secondary_all = p.secondary
    return n_pri


def _reorder5(T, a, C):
    """mem_reorder_primary5"""
    cand = [k for k, p in enumerate(a) if p.secondary < 0 and not p.is_alt and p.score >= T]
    if len(cand) <= 1:
        return
    left_k = min(cand, key=lambda k: (a[k].qb, k))
    assert a[0].secondary < 0
    if left_k == 0:
        return
    C["n_reordered"] += 1
    a[0], a[left_k] = a[left_k], a[0]
    for p in a[1:]:
        if p.secondary == 0:
            p.secondary = left_k
        elif p.secondary == left_k:
            p.secondary = 0
        if p.secondary_all == 0:
            p.secondary_all = left_k
        elif p.secondary_all == left_k:
            p.secondary_all = 0


def _fma(x, y, z):
    """x * y + z rounded once (what a compiler that contracts the expression evaluates)"""
    return float(Fraction(x) * Fraction(y) + Fraction(z))


def mapq_se(o, p, C=None, fused=False):
    """mem_approx_mapq_se, the mapQ_coef_len > 0 branch; fused: every `x * y + .499` as one fused multiply-add"""
    mad = _fma if fused else (lambda x, y, z: x * y + z)
    sub = p.sub if p.sub else o["min_seed_len"] * o["a"]
    if p.csub > sub:
        sub = p.csub
        if C is not None:
            C["q_csub"] += 1
    if sub >= p.score:
        if C is not None:
            C["q_zero"] += 1
        return 0
    l = max(p.qe - p.qb, p.re - p.rb)
    identity = 1. - float(l * o["a"] - p.score) / (o["a"] + o["b"]) / l
    assert p.score != 0 and o["mapQ_coef_len"] > 0
    if F32(l) < F32(o["mapQ_coef_len"]):
        tmp = 1.
        key = "q_short"
    else:
        tmp = o["mapQ_coef_fac"] / math.log(l)
        key = "q_long"
    tmp *= identity * identity
    mapq = int(mad(6.02 * (p.score - sub) / o["a"] * tmp, tmp, .499))
    if p.sub_n > 0:
        mapq -= int(mad(4.343, math.log(p.sub_n + 1), .499))
    if C is not None:
        C[key] += 1
        C["q_sub_n"] += p.sub_n > 0
        C["q_clip60"] += mapq > 60
        C["q_clip0"] += mapq < 0
        C["q_frac"] += p.frac_rep > 0
        C["q_frac0"] += p.frac_rep == 0
    mapq = min(max(mapq, 0), 60)
    return int(mad(float(mapq), 1. - p.frac_rep, .499))


def counters():
    return dict(n_alt_and_pri=0, n_alt_only=0, n_alt_sc=0, n_secondary=0, n_hash_reads=0, n_boundary=0, z_max=0, n_reordered=0, q_zero=0, q_short=0, q_long=0, q_sub_n=0, q_clip60=0,
                q_clip0=0, q_frac=0, q_frac0=0, q_csub=0, n_status=0, n_fma_differs=0)


LOG_TABLE = 65536           # the stage's table of log((double)k): arguments beyond it set the read's status


def model(regs, reg_off, ids, opt=None, both=False):
    """regs (hipapi.ALNREG) per read, ids[r] = the read's id -> dict(regs: the records in final order, n_pri, mapq (uint8 per record), status
    (per read: 1 where a quality needs a logarithm beyond the stage's table -- its qualities are unspecified there), counters).  both: every
    quality is also evaluated with its multiply-adds fused; counters["n_fma_differs"] counts the records where that changes it."""
    o = opt or default_opt()
    n = reg_off.shape[0] - 1
    C = counters()
    cols = {f: regs[f].tolist() for f in ("qb", "qe", "rb", "re", "score", "csub", "sub_n", "n_comp_is_alt")}
    frac = regs["frac_rep"].astype(np.float64).tolist()
    src, rows, n_pri, mapq, status = [], [], np.zeros(n, np.int32), [], np.zeros(n, np.uint8)
    for r in range(n):
        a = []
        for k in range(int(reg_off[r]), int(reg_off[r + 1])):
            p = _Rec()
            p.src, p.qb, p.qe, p.rb, p.re, p.score, p.csub, p.sub_n, p.frac_rep = k, cols["qb"][k], cols["qe"][k], cols["rb"][k], cols["re"][k], cols["score"][k], cols["csub"][k], cols["sub_n"][k], frac[k]
            p.is_alt = (cols["n_comp_is_alt"][k] >> 30) & 3
            a.append(p)
        n_pri[r] = _mark(o, a, int(ids[r]), C)
        if o["primary5"]:
            _reorder5(o["T"], a, C)
        for p in a:
            l = max(p.qe - p.qb, p.re - p.rb)
            sub = max(p.sub if p.sub else o["min_seed_len"] * o["a"], p.csub)
            if sub < p.score and ((not F32(l) < F32(o["mapQ_coef_len"]) and l >= LOG_TABLE) or (p.sub_n > 0 and p.sub_n + 1 >= LOG_TABLE)):
                status[r] = 1
            q = mapq_se(o, p, C)
            if both and mapq_se(o, p, None, fused=True) != q:
                C["n_fma_differs"] += 1
            mapq.append(q)
            C["n_secondary"] += p.secondary >= 0
            src.append(p.src)
            rows.append(p)
        C["n_status"] += int(status[r])
    out = FG.take(regs, np.array(src, np.int64))
    for f in ("sub", "alt_sc", "sub_n", "secondary", "secondary_all"):
        out[f] = [getattr(p, f) for p in rows]
    out["hash"] = np.array([p.hash for p in rows], np.uint64)
    return {"regs": out, "n_pri": n_pri, "mapq": np.array(mapq, np.int64).astype(np.uint8), "status": status, "counters": C}


# ---- the workload ------------------------------------------------------------------------------------------------------------------------
def _rec(qb, qe, score, rb=None, re=None, alt=0, sub_n=0, csub=0, frac=0.0, rid=0):
    rb = 100000 + 7 * qb if rb is None else rb
    return dict(qb=qb, qe=qe, rb=rb, re=rb + (qe - qb) if re is None else re, score=score, truesc=score, rid=2 if alt else rid, csub=csub, sub_n=sub_n, frac_rep=frac,
                n_comp_is_alt=(alt << 30) | 1, w=100, seedcov=(qe - qb) // 2, seedlen0=19, sub=5, alt_sc=3, secondary=7, secondary_all=9)   # (stale sub, alt_sc, secondary, secondary_all: the stage resets them)


def _synthetic():
    rng = np.random.default_rng(977)
    reads = []
    for m in LIST_LENGTHS:                       # m non-overlapping primaries in score order unrelated to their position, then records that overlap members of every chunk of the list
        for variant in range(3):
            scores = rng.permutation(m) + 100 if variant < 2 else np.full(m, 150)          # (all equal: the hash alone orders the list)
            recs = [_rec(3 * k, 3 * k + 3, int(scores[k]), alt=int(variant == 1 and k % 5 == 0)) for k in range(m)]
            for k in sorted({0, 1, m // 2, 62, 63, 64, m - 2, m - 1} & set(range(m))):
                recs.append(_rec(3 * k, 3 * k + 3, int(rng.integers(60, 100)), alt=int(rng.integers(0, 2)) if variant == 1 else 0))          # the member's own span
                recs.append(_rec(3 * k + 1, min(3 * k + 7, 3 * m), int(rng.integers(60, 100))))                                             # two (three) members: the first in list order takes it
            recs.append(_rec(0, 3 * m, 99))                                                     # the whole read: min_l = 3, every member overlaps
            recs.append(_rec(3 * m, 3 * m + 40, 50))                                            # and one more member
            order = rng.permutation(len(recs))
            reads.append([recs[k] for k in order])
    for n in READ_COUNTS + (1, 2, 3, 5, 7, 8, 9, 12, 20, 40, 100):                              # generic reads: few distinct scores, spans that overlap around the mask level
        for rep in range(6):
            rl = int(rng.integers(80, 501))
            recs = []
            for k in range(n):
                ql = int(rng.integers(10, rl // 2 + 1))
                qb = int(rng.integers(0, rl - ql + 1)) // 5 * 5
                alt = int(rng.random() < (0.0, 0.3, 1.0, 0.3, 0.6, 0.0)[rep])
                qe = qb + ql // 5 * 5 + 5
                rb = 100000 + int(rng.integers(0, 5000))
                recs.append(_rec(qb, qe, int(rng.integers(25, 32 + 4 * rep)), alt=alt, sub_n=int(rng.integers(0, 3)), csub=int(rng.integers(0, 30)),
                                 frac=float(rng.choice([0.0, 0.0, 0.125, 0.5])), rb=rb, re=rb + qe - qb + int(rng.integers(0, 30)) * int(rng.random() < 0.3)))
            reads.append(recs)
    for it in range(240):                        # qualities: one or two records per read
        l = (48, 49, 50, 51, 52, 100, 150, 400)[it % 8]
        kind = it // 8 % 6
        frac = float((0.0, 0.0, 0.25, 0.75)[it // 48 % 4])
        if kind == 0:      # a clean hit: clipped at 60 above l = 50 or so
            recs = [_rec(0, l, l, frac=frac)]
        elif kind == 1:    # mismatches: identity below 1
            recs = [_rec(0, l, l - int(rng.integers(5, 25)), frac=frac, re=100000 + l + int(rng.integers(0, 6)))]
        elif kind == 2:    # sub >= score (by csub, by the default sub = min_seed_len * a) and score 0
            recs = [_rec(0, l, (0, 10, 19, 25)[it % 4], csub=(0, 0, 0, 25 + it % 2)[it % 4], frac=frac)]
        elif kind == 3:    # csub > sub, just below the score
            recs = [_rec(0, l, l - 3, csub=l - 4 - it % 7, frac=frac)]
        elif kind == 4:    # sub_n > 0 from the input and from a close second hit; small scores: the penalty takes the quality below 0
            recs = [_rec(0, l, 21 + it % 9 if it % 2 else l, sub_n=int(rng.integers(1, 400)), frac=frac), _rec(2, l, 20 if it % 2 else l - 3)]
        else:              # a secondary hit sets sub
            recs = [_rec(0, l, l, frac=frac), _rec(0, l - 5, l - 5 - it % 11), _rec(l, l + 30, 30)]
        reads.append(recs)
    reads.append([_rec(0, 100, 100, rb=200000, re=270000), _rec(0, 60, 40)])                   # a 70 000-base reference span: beyond the table of logarithms
    reads.append([])
    return reads


def workload():
    """-> dict: regs (hipapi.ALNREG), reg_off, ids (per read, ID_BASE + r), n_fixture (reads taken from finish_golden.npz, the first ones), status_read (the read with the 70 000-base span)"""
    if "w" in _CACHE:
        return _CACHE["w"]
    from pymeme import hipapi
    fin, fin_off, _ = FG.golden()
    syn_reads = _synthetic()
    rows = [x for recs in syn_reads for x in recs]
    syn = np.zeros(len(rows), hipapi.ALNREG)
    for f in rows[0]:
        syn[f] = [x[f] for x in rows]
    syn["c"] = np.arange(len(rows)) + (1 << 40)
    syn["hash"] = 12345                          # (stale: the stage writes it)
    syn["flg"] = np.arange(len(rows)) % 3
    regs = np.concatenate([fin, syn])
    regs = FG.take(regs, np.arange(regs.shape[0]))
    syn_off = np.cumsum([len(x) for x in syn_reads]).astype(np.int64)
    reg_off = np.concatenate([np.asarray(fin_off, np.int64), fin_off[-1] + syn_off])
    n = reg_off.shape[0] - 1
    W = {"regs": regs, "reg_off": reg_off, "ids": np.arange(n, dtype=np.int64) + ID_BASE, "n_fixture": fin_off.shape[0] - 1, "status_read": n - 2}
    _CACHE["w"] = W
    return W


def modelled():
    """the model's result on the workload with default options (computed once)"""
    if "m" not in _CACHE:
        W = workload()
        _CACHE["m"] = model(W["regs"], W["reg_off"], W["ids"], both=True)
    return _CACHE["m"]


def floors(C, regs_off):
    """the floors the workload was built to meet -> list of the ones it misses"""
    n = np.diff(regs_off)
    want = [("n_alt_and_pri", 500), ("n_alt_only", 900), ("n_alt_sc", 600), ("n_secondary", 4000), ("n_hash_reads", 400), ("n_boundary", 5), ("z_max", 130)] + \
           [(k, 50) for k in ("q_zero", "q_short", "q_long", "q_sub_n", "q_clip60", "q_clip0", "q_frac", "q_frac0", "q_csub")] + [("n_status", 1)]
    missed = ["%s = %d < %d" % (k, C[k], v) for k, v in want if C[k] < v]
    missed += ["no read of %d records" % k for k in READ_COUNTS if k not in set(n.tolist())]
    return missed


def golden():
    """tests/golden/primary_golden.npz: the compiled reference's outputs on the workload -> dict(regs, n_pri, mapq)"""
    G = np.load(os.path.join(GOLDEN, "primary_golden.npz"))
    W = workload()
    regs = FG.take(W["regs"], G["src"])
    for k, f in enumerate(OUT_FIELDS[:-1]):
        regs[f] = G["cols"][:, k]
    regs["hash"] = G["hash"]
    return {"regs": regs, "n_pri": G["n_pri"], "mapq": G["mapq"]}


def same(got, want, reg_off, skip_mapq_of=()):
    """exact equality of every field of every record, n_pri and the qualities (but those of the reads in skip_mapq_of); None or the first difference"""
    from pymeme import hipapi
    for f in hipapi.ALNREG.names:
        x, y = (got["regs"][f].view(np.uint32), want["regs"][f].view(np.uint32)) if f == "frac_rep" else (got["regs"][f], want["regs"][f])
        bad = np.nonzero(x != y)[0]
        if bad.size:
            k = int(bad[0])
            return "field %s of record %d (read %d): %r, expected %r (%d records differ)" % (f, k, int(np.searchsorted(reg_off, k, "right")) - 1, x[k], y[k], bad.size)
    if not np.array_equal(got["n_pri"], want["n_pri"]):
        return "n_pri differs at read %d" % int(np.nonzero(np.asarray(got["n_pri"]) != np.asarray(want["n_pri"]))[0][0])
    keep = np.ones(got["mapq"].shape[0], bool)
    for r in skip_mapq_of:
        keep[reg_off[r]:reg_off[r + 1]] = False
    bad = np.nonzero((np.asarray(got["mapq"]) != np.asarray(want["mapq"])) & keep)[0]
    if bad.size:
        k = int(bad[0])
        return "mapq of record %d (read %d): %d, expected %d (%d differ)" % (k, int(np.searchsorted(reg_off, k, "right")) - 1, got["mapq"][k], want["mapq"][k], bad.size)
    return None
