"""Workload and plain-Python model of mate rescue's record updates: what mem_sam_pe_batch_post does with the kswr_t results before it marks primaries (reference
src/bwamem_pair.cpp:851-921, with mem_matesw_batch_post :1225-1334, mem_matesw_batch_post_mate_sort :1337-1485, mem_sort_dedup_patch src/bwamem.cpp:385-446 and
mem_dedup_patch :258-308 as they run with bns == 0) -- the step the device stage meme_rescue_batch_* runs.  It sits behind nothing and in front of the primary, pair and
decide models.

workload(): batches on tests/pair_gen.py's geometry (300 kbp, three contigs, the third ALT; the bases are tests/decide_gen.py's genome): dict(name, regs, reg_off, ums,
read_len, reads, read_off, pes, opt, gar, gar_off, job_off, jobs, res).  Family A ("genuine"): pairs sampled inside pes, one end with a record at its true place, the
other with none or with decoys; gar and the jobs are posed by pose() here -- mem_sam_pe_batch_pre restated, which the fixture's generator holds against the compiled
reference's own posing -- and res is the compiled reference's kswv on those jobs, kept in tests/golden/rescue_golden.npz.  Family B ("directed"): the same kind of poses
with SYNTHETIC kswr_t values, made while the model walks, that reach each branch.  In every batch of workload() no walk asks for a result gar does not hold (pairs
where one would are dropped when the batch is made, and modelled() asserts it); status 1, status 2 and refused arguments are direct()'s, for the stage alone.

model(): the loop and the two post functions line by line, klib's introsort from tests/finish_gen.py, numpy.float32 for the redundancy test."""
import os

import numpy as np

import decide_gen as DG
import pair_gen as QG
from common import GOLDEN
from finish_gen import ks_introsort, take

L_PAC, CONTIGS = QG.L_PAC, QG.CONTIGS
PES = DG.PES
F32 = np.float32
LDS_RECS = 128                                       # tuning key rescue_lds_recs: its default; the tests lower it to 16 and 1
SIZES = (0, 1, 2, 8, 63, 64, 65, 130)                # records of a list the workload holds
KSWR = np.dtype([(n, "<i4") for n in ("score", "te", "qe", "score2", "te2", "tb", "qb")])
_CACHE = {}


def default_opt(**kw):
    """mem_opt_init (reference src/bwamem.cpp:126-162), the fields the step reads; batch_reads: BATCH_SIZE of worker_sam"""
    o = dict(a=1, pen_unpaired=17, max_matesw=50, min_seed_len=19, batch_reads=512, max_chain_gap=10000, mask_level_redun=0.95)
    o.update(kw)
    return o


# ---- the rules the posing step and the post functions share ------------------------------------------------------------------------------------
def infer_dir(b1, b2):
    return DG.infer_dir(b1, b2)


def skip_mask(pes, rb, mate_rbs):
    skip = [1 if pes[r][2] else 0 for r in range(4)]
    for b2 in mate_rbs:                              # :1244-1249
        r, dist = infer_dir(rb, b2)
        if pes[r][0] <= dist <= pes[r][1]:
            skip[r] = 1
    return skip


def window(r, pes, rb_a, l_ms):
    """:1263-1280 -> (is_rev, rb, re, rid of the clamp or None where rb >= re)"""
    is_rev = (r >> 1) != (r & 1)
    is_larger = not (r >> 1)
    lo, hi = pes[r][0], pes[r][1]
    if not is_rev:
        rb = rb_a + lo if is_larger else rb_a - hi
        re = (rb_a + hi if is_larger else rb_a - lo) + l_ms
    else:
        rb = (rb_a + lo if is_larger else rb_a - hi) - l_ms
        re = rb_a + hi if is_larger else rb_a - lo
    raw = (rb, re)
    rb, re = max(rb, 0), min(re, L_PAC << 1)
    rid = None
    if rb < re:                                      # bns_fetch_seq (src/bntseq.cpp:541-570): the sequence of the midpoint, its strand
        mid = (rb + re) >> 1
        rev = mid >= L_PAC
        f = (L_PAC << 1) - 1 - mid if rev else mid
        rid = max(k for k in range(len(CONTIGS)) if CONTIGS[k][0] <= f)
        fb, fe = CONTIGS[rid][0], CONTIGS[rid][0] + CONTIGS[rid][1]
        if rev:
            fb, fe = (L_PAC << 1) - fe, (L_PAC << 1) - fb
        rb, re = max(rb, fb), min(re, fe)
    return is_rev, rb, re, rid, raw


def anchors_of(recs, o):
    """indices of the records looked at: within pen_unpaired of the first (:854-857), the first max_matesw of them (:877, :898)"""
    out = [k for k, x in enumerate(recs) if x.score >= recs[0].score - o["pen_unpaired"]]
    return out[:o["max_matesw"]], len(out)


class Rec:
    __slots__ = ("rb", "re", "qb", "qe", "rid", "score", "csub", "seedcov", "n_comp", "is_alt", "src", "n_comp_in")


def recs_of(regs, b, e):
    out = []
    for k in range(b, e):
        x = Rec()
        for f in ("rb", "re", "qb", "qe", "rid", "score", "csub", "seedcov"):
            setattr(x, f, int(regs[f][k]))
        w = int(regs["n_comp_is_alt"][k]) & 0xffffffff
        x.n_comp, x.is_alt, x.src = w & 0x3fffffff, w >> 30, k
        out.append(x)
    return out


# ---- the posing step (mem_sam_pe_batch_pre :660-716 with mem_matesw_batch_pre :1060-1223), for gar and the jobs ------------------------------------
def pose(B):
    """-> gar (int32), gar_off, job_off (int64, per worker batch), jobs: list of (read of the mate, window rb, len1, is_rev) in posing order"""
    o = default_opt(**B["opt"])
    off, n = B["reg_off"], B["reg_off"].shape[0] - 1
    gar, gar_off, job_off, jobs = [], [0], [0], []
    for r in range(n):
        if r and r % o["batch_reads"] == 0:
            gar_off.append(len(gar))
            job_off.append(len(jobs))
        m = r ^ 1
        a, ma = recs_of(B["regs"], int(off[r]), int(off[r + 1])), recs_of(B["regs"], int(off[m]), int(off[m + 1]))
        l_ms = int(B["read_len"][m])
        for k in (anchors_of(a, o)[0] if a else []):
            skip = skip_mask(B["pes"], a[k].rb, [x.rb for x in ma])
            rid = -1
            for d in range(4):
                idx = -1
                if not skip[d] and sum(skip) != 4:
                    is_rev, rb, re, got, _ = window(d, B["pes"], a[k].rb, l_ms)
                    rid = rid if got is None else got
                    if a[k].rid == rid and re - rb >= o["min_seed_len"]:
                        idx = len(jobs) - job_off[-1]
                        jobs.append((m, rb, re - rb, int(is_rev)))
                gar.append(idx)
    gar_off.append(len(gar))
    job_off.append(len(jobs))
    return np.array(gar, np.int32), np.array(gar_off, np.int64), np.array(job_off, np.int64), jobs


def job_sequences(B, jobs):
    """the jobs' windows and queries back to back: (KSWV_JOB records, ref bytes, query bytes), as mem_matesw_batch_pre stores them"""
    from oracle_py import KSWV_JOB_DTYPE
    g = DG.genome()[0]
    both = np.concatenate([g, (3 - g)[::-1]])
    kj = np.zeros(len(jobs), KSWV_JOB_DTYPE)
    ref, qer, o = [], [], default_opt(**B["opt"])
    ir = iq = 0
    for k, (m, rb, len1, is_rev) in enumerate(jobs):
        ms = B["reads"][int(B["read_off"][m]):int(B["read_off"][m + 1])]
        q = np.where(ms < 4, 3 - ms, 4)[::-1].astype(np.uint8) if is_rev else ms
        l_ms = ms.shape[0]
        kj[k] = (ir, iq, len1, l_ms, 0x40000 | 0x80000 | (0x10000 if l_ms * o["a"] < 250 else 0) | (o["min_seed_len"] * o["a"]), 0)
        ref.append(both[rb:rb + len1])
        qer.append(q)
        ir += len1
        iq += l_ms
    cat = lambda xs: np.concatenate(xs).astype(np.uint8) if xs else np.zeros(0, np.uint8)
    return kj, cat(ref), cat(qer)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def counters():
    keys = ("path_ms", "path_plain", "lost_ms_end0", "lost_ms_end1", "beyond_pen", "beyond_max", "skip_all", "posed0", "posed1", "posed2", "posed3", "refused_edge", "refused_strand",
            "low_score", "qb_neg", "is_rev0", "is_rev1", "ins_head", "ins_mid", "ins_tail", "resort", "pushed_removed", "orig_removed", "identical", "ncomp_reset", "ncomp_kept_single",
            "skip_by_pushed", "sw_no_push", "sw0_ms", "later_batch", "n_wave", "n_tested", "n_pushed", "n_removed", "status1")
    return {k: 0 for k in keys}


_lt_re = lambda x, y: x.re < y.re
_lt_score = lambda x, y: x.score > y.score or (x.score == y.score and (x.rb < y.rb or (x.rb == y.rb and x.qb < y.qb)))


def _gone(x, C):
    C["pushed_removed" if x.src < 0 else "orig_removed"] += 1


def _dedup_patch(a, o, C):
    """mem_dedup_patch with bns == 0 (:258-308): mem_patch_reg returns 0 (:200)"""
    if len(a) <= 1:
        C["ncomp_kept_single"] += len(a)
        return a
    mlr, gap = F32(o["mask_level_redun"]), o["max_chain_gap"]
    for x in a:
        C["ncomp_reset"] += x.n_comp != 1
        x.n_comp = 1
    for i in range(1, len(a)):
        p = a[i]
        if p.rid != a[i - 1].rid or p.rb >= a[i - 1].re + gap:
            continue
        j = i - 1
        while j >= 0 and p.rid == a[j].rid and p.rb < a[j].re + gap:
            q = a[j]
            j -= 1
            if q.qe == q.qb:
                continue
            or_ = q.re - p.rb
            oq = q.qe - p.qb if q.qb < p.qb else p.qe - q.qb
            mr, mq = min(q.re - q.rb, p.re - p.rb), min(q.qe - q.qb, p.qe - p.qb)
            if F32(or_) > mlr * F32(mr) and F32(oq) > mlr * F32(mq):
                if p.score < q.score:
                    p.qe = p.qb
                    break
                q.qe = q.qb
    for x in a:
        if not x.qe > x.qb:
            _gone(x, C)
    return [x for x in a if x.qe > x.qb]


def _identical(a, C):
    for i in range(1, len(a)):
        if a[i].score == a[i - 1].score and a[i].rb == a[i - 1].rb and a[i].qb == a[i - 1].qb:
            a[i].qe = a[i].qb
            C["identical"] += 1
            _gone(a[i], C)
    return a[:1] + [x for x in a[1:] if x.qe > x.qb]


def _sort_dedup_patch(a, o, C):
    """mem_sort_dedup_patch with bns == 0 (:385-446)"""
    if len(a) <= 1:
        C["ncomp_kept_single"] += len(a)
        return a
    ks_introsort(a, _lt_re)
    a = _dedup_patch(a, o, C)
    ks_introsort(a, _lt_score)
    return _identical(a, C)


def rescue_list(o, pes, ma, anchors_end, mate_sort, l_ms, job, C, probe=None):
    """the loop of one i (:864-907) on ma = a[!i] (a list of Rec, changed and returned) with the records of a[i] as they were handed over.  job(q, d, window rb, len1,
    is_rev, ma) -> the kswr_t as a dict, or None where gar holds none.  -> (list, status)"""
    if not anchors_end:                              # b[i].n == 0
        return ma, 0
    looked, n_b = anchors_of(anchors_end, o)
    C["beyond_pen"] += len(anchors_end) - n_b
    C["beyond_max"] += n_b - len(looked)
    if mate_sort:
        ks_introsort(ma, _lt_re)                     # :875
    swcount = 0
    for q, k in enumerate(looked):
        a = anchors_end[k]
        skip = skip_mask(pes, a.rb, [x.rb for x in ma])
        if any(skip[r] and not skip_mask(pes, a.rb, [x.rb for x in ma if x.src >= 0])[r] for r in range(4)):
            C["skip_by_pushed"] += 1
        n, rid = 0, -1
        if sum(skip) == 4:
            C["skip_all"] += 1
            continue
        for r in range(4):
            if skip[r]:
                continue
            is_rev, rb, re, got, raw = window(r, pes, a.rb, l_ms)
            rid = rid if got is None else got
            if a.rid == rid and re - rb >= o["min_seed_len"]:
                aln = job(q, r, rb, re - rb, is_rev, ma)
                if aln is None:
                    return None, 1
                C["posed%d" % r] += 1
                if aln["score"] >= o["min_seed_len"] and aln["qb"] >= 0:
                    b = Rec()
                    b.rid, b.is_alt = a.rid, a.is_alt
                    b.qb = l_ms - (aln["qe"] + 1) if is_rev else aln["qb"]
                    b.qe = l_ms - aln["qb"] if is_rev else aln["qe"] + 1
                    b.rb = (L_PAC << 1) - (rb + aln["te"] + 1) if is_rev else rb + aln["tb"]
                    b.re = (L_PAC << 1) - (rb + aln["tb"]) if is_rev else rb + aln["te"] + 1
                    b.score, b.csub, b.n_comp, b.src = aln["score"], aln["score2"], 0, -1
                    b.seedcov = min(b.re - b.rb, b.qe - b.qb) >> 1
                    C["is_rev%d" % int(is_rev)] += 1
                    C["n_pushed"] += 1
                    if not mate_sort:                # :1315-1322
                        i = next((i for i in range(len(ma)) if ma[i].score < b.score), len(ma))
                        C["ins_head" if i == 0 and ma else "ins_tail" if i == len(ma) else "ins_mid"] += 1
                        ma.insert(i, b)
                    else:                            # :1431-1474
                        resort, i = 0, 0
                        while i < len(ma):
                            if ma[i].re == b.re:
                                resort = 1
                                break
                            if ma[i].re > b.re:
                                break
                            i += 1
                        if resort:
                            C["resort"] += 1
                            ks_introsort(ma, _lt_score)
                            ma[:] = _identical(ma, C)
                            i = next((i for i in range(len(ma)) if ma[i].score < b.score), len(ma))
                            ma.insert(i, b)
                            ks_introsort(ma, _lt_re)
                        else:
                            ma.insert(i, b)
                else:
                    C["low_score" if aln["score"] < o["min_seed_len"] else "qb_neg"] += 1
                n += 1
            else:
                if raw[0] < 0 or raw[1] > (L_PAC << 1) or (raw[0] < L_PAC < raw[1]):
                    C["refused_strand"] += 1
                else:
                    C["refused_edge"] += 1
            if n:
                ma[:] = _dedup_patch(ma, o, C) if mate_sort else _sort_dedup_patch(ma, o, C)
        C["n_tested"] += n
        swcount += n
    if mate_sort:
        if swcount > 0:
            if not any(x.src < 0 for x in ma):
                C["sw_no_push"] += 1
            ma[:] = _sort_dedup_patch(ma, o, C)
        else:
            C["sw0_ms"] += 1
            ks_introsort(ma, _lt_score)
    return ma, 0


def cursors(B, o):
    """per read: (worker batch, first gar entry of its records looked at relative to the batch's gar, how many are looked at)"""
    off, n = B["reg_off"], B["reg_off"].shape[0] - 1
    out, cur = [], 0
    for r in range(n):
        if r % o["batch_reads"] == 0:
            cur = 0
        a = recs_of(B["regs"], int(off[r]), int(off[r + 1]))
        na = len(anchors_of(a, o)[0]) if a else 0
        out.append((r // o["batch_reads"], cur, na))
        cur += 4 * na
    return out


def model(B, C=None, synth=None, walk_all=False, walk_all_status=False):
    """the stage on a batch -> dict(regs, reg_off, status, counters).  synth(r, q, d, rb, len1, is_rev, ma) makes a result where the batch has none yet (the workload's
    generator); walk_all: lists the stage does not walk (no result can be pushed, off the mate-sort path) are walked too and must come out unchanged;
    walk_all_status: they are walked too and report what the reference's walk would meet (1 where it asks for a result gar does not hold)."""
    o = default_opt(**B["opt"])
    C = counters() if C is None else C
    off, n = B["reg_off"], B["reg_off"].shape[0] - 1
    cur = cursors(B, o)
    rows, out_off, status = [], np.zeros(n + 1, np.int64), np.zeros(n, np.uint8)
    C0 = dict(C)
    for r in range(n):
        m = r ^ 1
        ma, anc = recs_of(B["regs"], int(off[r]), int(off[r + 1])), recs_of(B["regs"], int(off[m]), int(off[m + 1]))
        b, g, na = cur[m]
        g0, j0, nj = int(B["gar_off"][b]), int(B["job_off"][b]), int(B["job_off"][b + 1] - B["job_off"][b])
        posed = sum(int(B["gar"][g0 + g + e]) >= 0 for e in range(4 * na))
        mate_sort = bool(B["ums"][r]) and bool(B["ums"][m])
        listed = posed > 0 or (mate_sort and len(anc) > 0 and len(ma) > 1)

        def job(q, d, rb, len1, is_rev, lst):
            idx = int(B["gar"][g0 + g + 4 * q + d])
            if idx < 0 or idx >= nj:
                return None
            if synth is not None:
                synth(r, j0 + idx, rb, len1, is_rev, lst)
            return {f: int(B["res"][f][j0 + idx]) for f in KSWR.names}

        if listed or walk_all or walk_all_status:
            Cr = dict(C)
            n_in = len(ma)
            before = [x.src for x in ma]
            got, st = rescue_list(o, B["pes"], ma, anc, mate_sort, int(B["read_len"][r]), job, C)
            if not listed and not walk_all_status:
                assert st == 0 and [x.src for x in got] == before, "a list the stage does not walk changes (read %d of %s)" % (r, B["name"])
            if st:
                for k in C:
                    C[k] = Cr[k]                     # (the stage counts nothing of a list it hands back)
                C["status1"] += 1
                status[r] = 1
                got = None
            elif listed:
                C["n_wave"] += 1
                C["n_removed"] += n_in + (C["n_pushed"] - Cr["n_pushed"]) - len(got)
                C["path_ms" if mate_sort else "path_plain"] += 1
                if r // o["batch_reads"] > 0:
                    C["later_batch"] += 1
            if listed and st:
                C["n_wave"] += 1
        else:
            got = ma
        if not mate_sort and B["ums"][r] != B["ums"][m]:
            C["lost_ms_end%d" % (r & 1 if not B["ums"][r] else m & 1)] += 1
        if got is None:
            rows += [(x.src, None) for x in recs_of(B["regs"], int(off[r]), int(off[r + 1]))]
            out_off[r + 1] = out_off[r] + (off[r + 1] - off[r])
        else:
            rows += [(x.src, x) for x in got]
            out_off[r + 1] = out_off[r] + len(got)
    from pymeme import hipapi
    out = np.zeros(len(rows), hipapi.ALNREG)
    old = np.array([k for k, (s, x) in enumerate(rows) if s >= 0], np.int64)
    if old.size:
        src = take(B["regs"], np.array([rows[k][0] for k in old], np.int64))
        for f in hipapi.ALNREG.names:
            out[f][old] = src[f]
    for k, (s, x) in enumerate(rows):
        if x is None:
            continue                                 # status 1: as it went in, flg included
        out["flg"][k] = 0
        if s >= 0:
            out["qe"][k] = x.qe
            out["n_comp_is_alt"][k] = np.array(((int(out["n_comp_is_alt"][k]) & 0xc0000000) | x.n_comp) & 0xffffffff, np.uint32).view(np.int32)
        else:
            for f in ("rb", "re", "qb", "qe", "rid", "score", "csub", "seedcov"):
                out[f][k] = getattr(x, f)
            out["secondary"][k] = -1
            out["n_comp_is_alt"][k] = np.array(((x.is_alt << 30) | x.n_comp) & 0xffffffff, np.uint32).view(np.int32)
    stage = {k: C[k] - C0[k] for k in ("n_wave", "n_tested", "n_pushed", "n_removed")}      # (of this batch: C may run over several)
    return {"regs": out, "reg_off": out_off, "status": status, "counters": C, "stage": stage}


# ---- the workload ------------------------------------------------------------------------------------------------------------------------------
def _revcomp(x):
    return np.where(x > 3, x, 3 - x)[::-1].astype(np.uint8)


def _rec(rid, fpos, rev, length, score=None, qb=0, rl=None, **kw):
    """a record of `length` bases whose leftmost forward base is fpos in contig rid, on the reverse strand if rev: as many reference as query bases, truesc perfect"""
    f = CONTIGS[rid][0] + fpos
    rb = 2 * L_PAC - (f + length) if rev else f
    r = dict(rb=rb, re=rb + length, qb=qb, qe=qb + length, rid=rid, score=length if score is None else score, truesc=length, secondary=-1, secondary_all=-1, seedlen0=19, w=100,
             n_comp_is_alt=(CONTIGS[rid][2] << 30) | 1, seedcov=length // 2, flg=3, sub=0, csub=0)
    r.update(kw)
    assert 0 <= fpos and fpos + length <= CONTIGS[rid][1]
    return r


def _sorted(recs):
    return sorted(recs, key=lambda x: (-x["score"], x["rb"], x["qb"]))


def _distinct_re(recs):
    seen = set()
    for x in recs:
        while x["re"] in seen:
            x["re"] += 1
        seen.add(x["re"])
    return recs


def _genuine_pair(rng, g, variant, n_decoy=0, near_edge=None):
    """one true FR pair: end 0 forward at x, end 1 the reverse complement `dist` behind it, a few mismatches; which records exist is the variant's"""
    rid = int(rng.integers(0, 3))
    l0, l1 = int(rng.choice([100, 125, 150, 260])), int(rng.choice([100, 125, 150]))
    dist = int(rng.integers(120, 700))
    clen = CONTIGS[rid][1]
    if near_edge == "origin":                        # the first bases of the text: a window towards smaller coordinates is cut at the strand's start
        rid, clen = 0, CONTIGS[0][1]
        x = int(rng.integers(0, 15))
    elif near_edge == "contig":
        x = int(rng.integers(0, 200))
    elif near_edge == "end":
        x = clen - max(dist + l1, l0) - int(rng.integers(0, 60))
    else:
        x = int(rng.integers(1500, clen - 2500))
    base = CONTIGS[rid][0]
    r0 = g[base + x:base + x + l0].copy()
    r1 = _revcomp(g[base + x + dist:base + x + dist + l1])
    for rd in (r0, r1):
        for p in rng.integers(0, rd.shape[0], int(rng.integers(0, 4))):
            rd[p] = (rd[p] + 1) & 3
    true0 = _rec(rid, x, 0, l0, score=l0 - int(rng.integers(0, 12)))
    true1 = _rec(rid, x + dist, 1, l1, score=l1 - int(rng.integers(0, 12)))

    def decoys(k, rl, top):
        out = []
        for _ in range(k):
            c = int(rng.integers(0, 3))
            ln = int(rng.integers(30, min(rl, 100)))
            out.append(_rec(c, int(rng.integers(100, CONTIGS[c][1] - 400)), int(rng.integers(0, 2)), ln, score=int(rng.integers(max(20, top - 30), top + 1)) if rng.random() < 0.5 else int(rng.integers(19, 40)),
                            qb=int(rng.integers(0, rl - ln + 1)), n_comp_is_alt=(CONTIGS[c][2] << 30) | int(rng.integers(1, 4))))
        return out

    if variant == 0:
        ends = [[true0], []]
    elif variant == 1:
        ends = [[true0], decoys(1 + n_decoy, l1, 60)]
    elif variant == 2:
        ends = [[true0] + decoys(n_decoy, l0, true0["score"]), [true1] + decoys(n_decoy, l1, true1["score"])]
    elif variant == 3:
        ends = [[], [true1]]
    elif variant == 4:
        ends = [[true0] + decoys(2 + n_decoy, l0, true0["score"]), decoys(n_decoy, l1, 50)]
    else:
        ends = [decoys(1 + n_decoy, l0, 70), [true1] + decoys(n_decoy, l1, 60)]
    return {"ends": [_distinct_re(_sorted(e)) for e in ends], "reads": [r0, r1]}


def _identical_pair(rng, g, want="identical"):
    """directed: end 1 holds a record X at dist high + 5 behind the anchor (FF: outside the statistics, inside the window), and behind X's end a record Z of another
    sequence: a result equal to X in score, rb and qb with its end behind Z's is never compared with X by the walk and leaves in the identical-hit pass"""
    P = _genuine_pair(rng, g, 0)
    a = P["ends"][0][0]
    rid, x = a["rid"], a["rb"] - CONTIGS[a["rid"]][0]
    l1 = P["reads"][1].shape[0]
    X = _rec(rid, x + PES[0][1] + 5, 0, 60, score=50, qb=3)
    Z = _rec(rid, x + PES[0][1] + 5 + 21, 0, 40, score=30)       # (its end one base behind X's)
    Z["rid"] = (rid + 1) % 3
    P["ends"][1] = [X, Z] if want else [X]           # (want None: X alone, for results that are redundant with an original record)
    P["want"] = want
    return P


def _assemble(name, pairs, pes, ums_of, **opt):
    from pymeme import hipapi
    rows, counts, reads, ums = [], [], [], []
    for k, P in enumerate(pairs):
        u = ums_of(k)
        for e in range(2):
            rows += P["ends"][e]
            counts.append(len(P["ends"][e]))
            reads.append(P["reads"][e])
            ums.append(u[e])
    regs = np.zeros(len(rows), hipapi.ALNREG)
    for f in (rows[0] if rows else ()):
        regs[f] = [x.get(f, 0) for x in rows]
    regs["c"] = 7000 + np.arange(len(rows))          # (dead fields that tell a record from its copies and from a new one)
    regs["hash"] = 11 + np.arange(len(rows))
    regs["frac_rep"] = 0.25
    B = {"name": name, "regs": regs, "reg_off": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), "ums": np.array(ums, np.uint8),
         "read_len": np.array([len(x) for x in reads], np.int32), "reads": np.concatenate(reads) if reads else np.zeros(0, np.uint8),
         "read_off": np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.int64), "pes": pes, "opt": opt, "pairs": pairs}
    B["gar"], B["gar_off"], B["job_off"], B["jobs"] = pose(B)
    B["res"] = np.zeros(len(B["jobs"]), KSWR)
    return B


def _synth_for(B, rng):
    """synthetic kswr_t values made while the model walks: each job's result once, by a pattern that looks at the list as it stands"""
    done = set()
    o = default_opt(**B["opt"])

    def put(j, rb_w, is_rev, l_ms, nrb, nre, nqb, nqe, score, score2):
        if is_rev:
            v = dict(qe=l_ms - nqb - 1, qb=l_ms - nqe, te=2 * L_PAC - nrb - 1 - rb_w, tb=2 * L_PAC - nre - rb_w)
        else:
            v = dict(qb=nqb, qe=nqe - 1, tb=nrb - rb_w, te=nre - 1 - rb_w)
        B["res"][j] = (score, v["te"], v["qe"], score2, -1, v["tb"], v["qb"])

    def synth(r, j, rb_w, len1, is_rev, ma):
        if j in done:
            return
        done.add(j)
        l_ms = int(B["read_len"][r])
        lo, hi = (2 * L_PAC - (rb_w + len1), 2 * L_PAC - rb_w) if is_rev else (rb_w, rb_w + len1)      # where a new record can lie
        inside = [x for x in ma if lo <= x.rb and x.re <= hi and x.qe <= l_ms]
        want = B["pairs"][r // 2].get("want")
        pat = rng.random()
        if want == "identical" and inside:
            x = inside[0]
            return put(j, rb_w, is_rev, l_ms, x.rb, x.re + 2, x.qb, x.qe, x.score, 0)
        if pat < 0.08:
            return put(j, rb_w, is_rev, l_ms, lo, lo + 30, 0, 30, int(rng.integers(0, o["min_seed_len"])), 0)
        if pat < 0.14:
            B["res"][j] = (int(rng.integers(19, 60)), 40, 30, 0, -1, -1, -1)                          # qb < 0: "something goes wrong"
            return
        if inside and pat < 0.55:
            x = inside[int(rng.integers(0, len(inside)))]
            kind = int(rng.choice([0, 1, 1, 2, 3]))
            if kind == 0 and x.re - 25 > lo:         # the same end, another start: the resort branch on the mate-sort path
                return put(j, rb_w, is_rev, l_ms, x.re - 25, x.re, 0, 25, int(rng.integers(19, 26)), int(rng.integers(0, 19)))
            if kind == 1:                            # redundant with x, the better of the two
                return put(j, rb_w, is_rev, l_ms, x.rb, x.re, x.qb, x.qe, x.score + int(rng.integers(0, 6)), 0)
            if kind == 2:                            # redundant with x, the worse
                return put(j, rb_w, is_rev, l_ms, x.rb, x.re, x.qb, x.qe, max(19, x.score - int(rng.integers(1, 6))), 0)
        ln = int(rng.integers(19, min(l_ms, len1) + 1))
        s = lo + int(rng.integers(0, len1 - ln + 1))
        qb = int(rng.integers(0, l_ms - ln + 1))
        put(j, rb_w, is_rev, l_ms, s, s + ln, qb, qb + ln, int(rng.integers(19, ln + 1)), int(rng.integers(0, 19)))

    return synth


def _settle(name, pairs, pes, ums_of, rng, genuine_res=None, keep=None, **opt):
    """the batch of those pairs whose walks ask for no result gar does not hold (B["keep"]: their indices); family B's results are made on the way.  keep: the indices
    a run with the compiled reference's kswv found for a batch of family A (the fixture's)"""
    idx = list(range(len(pairs)))
    if keep is not None:
        ums_list = [ums_of(k) for k in keep]
        B = _assemble(name, [pairs[k] for k in keep], pes, lambda k: ums_list[k], **opt)
        B["res"], B["keep"] = genuine_res(B), list(keep)
        return B
    for _ in range(6):
        B = _assemble(name, pairs, pes, ums_of, **opt)
        B["keep"] = idx
        if genuine_res is not None:
            B["res"] = genuine_res(B)
            m = model(B, walk_all=True)
        else:
            m = model(B, synth=_synth_for(B, np.random.default_rng(int(rng.integers(1 << 30)))), walk_all=True)
        bad = {int(r) // 2 for r in np.nonzero(m["status"])[0]}
        if not bad:
            return B
        left = [k for k in range(len(pairs)) if k not in bad]
        ums_list = [ums_of(k) for k in left]
        pairs, ums_of, idx = [pairs[k] for k in left], (lambda k, u=ums_list: u[k]), [idx[k] for k in left]
    raise AssertionError("the batch %s does not settle" % name)


UMS = ((1, 1), (1, 1), (0, 1), (1, 0), (0, 0), (1, 1), (0, 0))
FAMILY_A = ("A-genuine", "A-matesw-1", "A-small-batches")


def _pairs_for(rng, g, n, sizes=False, edges=False):
    out = []
    for k in range(n):
        v = k % 6
        out.append(_genuine_pair(rng, g, v, n_decoy=int(rng.integers(0, 4)), near_edge=("contig", "end")[k & 1] if edges and k % 5 == 0 else None))
    if edges:
        out += [_genuine_pair(rng, g, k & 1, near_edge="origin") for k in range(8)]
    if sizes:
        for m in SIZES[3:] + (3,):
            for v in (1, 2, 4):
                out.append(_genuine_pair(rng, g, v, n_decoy=m - 1))
    return out


def build(genuine_res, keep=None):
    """every batch of the workload; genuine_res(B) -> family A's kswr_t records (the compiled reference's kswv for the generator, the fixture's for everybody else);
    keep: name of a family A batch -> the pairs the generator's run kept"""
    keep = keep or {}
    rng = np.random.default_rng(271828)
    g = DG.genome()[0]
    u = lambda k: UMS[k % len(UMS)]
    failed = QG._with(PES, failed=(0, 2))
    W = [_settle("A-genuine", _pairs_for(rng, g, 150, sizes=True, edges=True), PES, u, rng, genuine_res, keep.get("A-genuine")),
         _settle("A-matesw-1", _pairs_for(rng, g, 60), PES, u, rng, genuine_res, keep.get("A-matesw-1"), max_matesw=1, pen_unpaired=40),
         _settle("A-small-batches", _pairs_for(rng, g, 50), PES, u, rng, genuine_res, keep.get("A-small-batches"), batch_reads=4, max_matesw=2, pen_unpaired=30),
         _settle("B-directed", _pairs_for(rng, g, 260, sizes=True, edges=True) + [_identical_pair(rng, g) for _ in range(12)] + [_identical_pair(rng, g, None) for _ in range(40)], PES, u, rng),
         _settle("B-batches-6", _pairs_for(rng, g, 120), PES, u, rng, batch_reads=6, pen_unpaired=25),
         _settle("B-failed", _pairs_for(rng, g, 60), failed, u, rng, batch_reads=4, max_matesw=2),
         _settle("B-one", _pairs_for(rng, g, 1), PES, u, rng),
         _settle("B-two", _pairs_for(rng, g, 2), PES, u, rng, batch_reads=2),
         _settle("B-three", _pairs_for(rng, g, 3), PES, u, rng, batch_reads=4),
         _settle("B-matesw-0", _pairs_for(rng, g, 30), PES, u, rng, max_matesw=0),
         _settle("B-all-failed", _pairs_for(rng, g, 16), QG._with(PES, failed=(0, 1, 2, 3)), u, rng)]
    return W


def golden():
    return np.load(os.path.join(GOLDEN, "rescue_golden.npz"))


WHOLE_ID_BASE = 500                                  # pair p of a batch has id WHOLE_ID_BASE + p in the whole reference call and in the chained stages


def chain(B, m):
    """a batch of family A behind its rescue result m through the three models that follow, as the stages chain (tests/decide_gen.py: chain) -> dict(primary, pair, decide)"""
    import primary_gen as PG
    o = DG.default_opt(pen_unpaired=default_opt(**B["opt"])["pen_unpaired"])
    n = B["reg_off"].shape[0] - 1
    pm = PG.model(m["regs"], m["reg_off"], 2 * WHOLE_ID_BASE + np.arange(n), o)
    assert not pm["status"].any()
    qm = QG.model({"regs": pm["regs"], "reg_off": m["reg_off"], "n_pri": pm["n_pri"], "pes": B["pes"], "id_base": WHOLE_ID_BASE}, {k: o[k] for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins")})
    return {"primary": pm, "pair": qm, "decide": DG.decide(pm["regs"], m["reg_off"], pm["n_pri"], qm, B["pes"], o), "opt": o}


def whole_agrees(B, m, obs, whole):
    """the reference's whole call on a batch of family A (obs: DG.OBS per read; whole: dict(regs, reg_off) behind it) against chain() behind the rescue result m
    -> None or the first difference"""
    ch = chain(B, m)
    d = same(whole, {"regs": ch["decide"]["regs"], "reg_off": m["reg_off"], "status": whole["status"]})
    return d or DG.observables_agree(B, ch, obs, {f: whole["regs"][f] for f in DG.MARKS})


def golden_whole():
    """name of a family A batch -> (obs, dict(regs, reg_off, status)): what the reference's whole call left, from the fixture"""
    from pymeme import hipapi
    G, out, at_k, at_r = golden(), {}, 0, 0
    for B in workload():
        if B["name"] not in FAMILY_A:
            continue
        n = B["reg_off"].shape[0] - 1
        off = G["whole_reg_off"][at_r + len(out):at_r + len(out) + n + 1]
        k = int(off[n])
        regs = np.zeros(k, hipapi.ALNREG)
        for c, f in enumerate(FIELDS):
            regs[f] = G["whole_cols"][at_k:at_k + k, c]
        regs["frac_rep"] = G["whole_frac_rep_bits"][at_k:at_k + k].view(np.float32)
        out[B["name"]] = ({f: G["whole_" + f][at_r:at_r + n] for f in DG.OBS}, {"regs": regs, "reg_off": off, "status": np.zeros(n, np.uint8)})
        at_k += k
        at_r += n
    return out


def workload():
    """the batches, family A's results from the fixture (made by the compiled reference's kswv; tests/golden/make_rescue_golden.py)"""
    if "w" not in _CACHE:
        G = golden()
        at = [0]

        def from_fixture(B):
            n = len(B["jobs"])
            res = np.zeros(n, KSWR)
            for k, f in enumerate(KSWR.names):
                res[f] = G["a_res"][at[0]:at[0] + n, k]
            at[0] += n
            return res
        _CACHE["w"] = build(from_fixture, {name: G["a_keep_" + name].tolist() for name in FAMILY_A})
    return _CACHE["w"]


def modelled():
    """model() of every batch and the counters of all batches together (computed once); no list of the workload may have status 1"""
    if "m" not in _CACHE:
        C = counters()
        M = [model(B, C) for B in workload()]
        assert not any(m["status"].any() for m in M), "a walk of the parity batches asks for a result gar does not hold"
        _CACHE["m"] = (M, C)
    return _CACHE["m"]


def floors(C, W):
    """the floors the workload was built to meet -> list of the ones it misses"""
    want = [("path_ms", 60), ("path_plain", 60), ("lost_ms_end0", 20), ("lost_ms_end1", 20), ("beyond_pen", 20), ("beyond_max", 20), ("skip_all", 5), ("posed0", 50), ("posed1", 50),
            ("posed2", 50), ("posed3", 50), ("refused_edge", 3), ("refused_strand", 3), ("low_score", 20), ("qb_neg", 15), ("is_rev0", 50), ("is_rev1", 50), ("ins_head", 20), ("ins_mid", 20),
            ("ins_tail", 20), ("resort", 5), ("pushed_removed", 20), ("orig_removed", 10), ("identical", 3), ("ncomp_reset", 20), ("ncomp_kept_single", 10), ("skip_by_pushed", 10),
            ("sw_no_push", 3), ("sw0_ms", 10), ("later_batch", 30)]
    missed = ["%s = %d < %d" % (k, C[k], v) for k, v in want if C[k] < v]
    sizes = set()
    for B in W:
        sizes |= set(np.diff(B["reg_off"]).tolist())
    missed += ["no list of %d records" % m for m in SIZES if m not in sizes]
    if not any(m > LDS_RECS for m in sizes):
        missed.append("no list beyond rescue_lds_recs")
    for k in ("batch_reads", "max_matesw", "pen_unpaired"):
        if not any(k in B["opt"] for B in W):
            missed.append("no batch with " + k)
    return missed


FIELDS = ("rb", "re", "qb", "qe", "rid", "c", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w", "seedcov", "secondary", "secondary_all", "seedlen0", "n_comp_is_alt", "hash", "flg")


def same(got, want):
    """exact equality of offsets, status and every field of every record; None or the first difference"""
    if not np.array_equal(got["reg_off"], want["reg_off"]):
        bad = np.nonzero(np.asarray(got["reg_off"]) != np.asarray(want["reg_off"]))[0] if len(got["reg_off"]) == len(want["reg_off"]) else [0]
        return "offsets differ from read %d on" % (int(bad[0]) - 1)
    if not np.array_equal(got["status"], want["status"]):
        return "status differs at read %d" % int(np.nonzero(np.asarray(got["status"]) != np.asarray(want["status"]))[0][0])
    for f in FIELDS:
        bad = np.nonzero(got["regs"][f] != want["regs"][f])[0]
        if bad.size:
            k = int(bad[0])
            return "field %s of record %d (read %d): %r, expected %r" % (f, k, int(np.searchsorted(want["reg_off"], k, "right")) - 1, got["regs"][f][k], want["regs"][f][k])
    if not np.array_equal(got["regs"]["frac_rep"].view(np.uint32), want["regs"]["frac_rep"].view(np.uint32)):
        return "frac_rep differs"
    return None




# ---- batches for the stage alone ------------------------------------------------------------------------------------------------------------------
def direct():
    """status 1: pairs of "A-genuine" where a result a walk reaches is taken out of gar (-1) or points outside the batch's jobs, the pairs around them untouched"""
    if "d" in _CACHE:
        return _CACHE["d"]
    W, (M, _) = workload(), modelled()
    B = dict(W[0])
    B["name"] = "status1"
    gar = B["gar"].copy()
    o = default_opt(**B["opt"])
    cur = cursors(B, o)
    hit = []
    for r in range(2, B["reg_off"].shape[0] - 3):
        b, g, na = cur[r ^ 1]
        es = [e for e in range(4 * na) if gar[int(B["gar_off"][b]) + g + e] >= 0]
        # a list with two results or more: one is taken away, another stays, so that the stage still walks it
        if len(es) >= 2 and all(abs(r // 2 - h // 2) > 1 for h in hit) and len(hit) < 6:
            gar[int(B["gar_off"][b]) + g + es[0]] = -1 if len(hit) & 1 else 1 << 20
            hit.append(r)
    B["gar"] = gar
    B["expect_status1"] = hit
    # "unposed": lists all of whose results are taken out of gar.  Nothing can be pushed into them, so the stage does not walk them off the mate-sort path (and on it only
    # where they hold two records or more): they report 0 and come back as they went in with flg = 0, although the reference would call ksw_align2 for them
    U = dict(W[0])
    U["name"] = "unposed"
    gar = U["gar"].copy()
    taken = []
    for r in range(2, U["reg_off"].shape[0] - 3):
        b, g, na = cur[r ^ 1]
        g0 = int(U["gar_off"][b]) + g
        if (gar[g0:g0 + 4 * na] >= 0).any() and all(abs(r // 2 - h // 2) > 1 for h in taken) and len(taken) < 12:
            gar[g0:g0 + 4 * na] = -1
            taken.append(r)
    U["gar"] = gar
    U["unposed"] = taken
    _CACHE["d"] = [U, B]
    return _CACHE["d"]


def direct_modelled():
    if "dm" not in _CACHE:
        out = []
        for B in direct():
            m = model(B)
            got = sorted(int(r) for r in np.nonzero(m["status"] == 1)[0])
            if B["name"] == "unposed":
                quiet = [r for r in B["unposed"] if r not in got]      # not walked: status 0 where the reference's walk would ask for a result
                assert set(got) <= set(B["unposed"]) and len(quiet) >= 3, (got, B["unposed"])
            else:
                assert set(got) <= set(B["expect_status1"]) and len(got) >= 3, (got, B["expect_status1"])
            out.append(m)
        _CACHE["dm"] = out
    return _CACHE["dm"]
