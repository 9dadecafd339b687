"""Workload and plain-Python model of record finishing: the tail of mem_kernel2_core (reference src/bwamem.cpp:1681-1719) -- the compaction
of a read's alignment records to the live ones, mem_sort_dedup_patch_mate_sort (:312-383, with mem_patch_reg :194-244) and the is_alt flag.
It is the one function between two device stages (seed extension, the SAM-phase stages) without a device counterpart; this is its oracle
and its fixture, for the stage that will take it to the device.

workload(): reads of 150-500 bases on the 3-contig fixture genome (the chaining / extension fixtures' genome, third contig flagged ALT) with the
records the function is handed, in four parts -- `sort` (live counts at every edge of klib's introsort, heavy ties in `re`, exact
duplicates in (score, rb, qb)), `redundant` (pairs whose overlap sits on the float boundary of the redundancy test), `patch` (colinear records
around an indel on both strands: merged, chained, rejected, on both sides of every bar of mem_patch_reg) and `real` (the records of
tests/golden/ext_golden.npz).  Inputs are regenerated from seeds; tests/golden/finish_golden.npz holds the compiled reference's outputs.

model(): the function restated step by step -- klib's ks_introsort, numpy.float32 for the redundancy test, Python floats (IEEE double, no
contraction) for mem_patch_reg, oracle_py.gen_cigar2 for the patch's score -- with its branch counts."""
import os

import numpy as np

from common import GOLDEN, ext_golden_inputs

ALT_CONTIG = 2
SORT_COUNTS = (0, 1, 2, 3, 4, 16, 17, 18, 33, 64, 65, 130, 300)
_CACHE = {}


# ---- klib ksort.h: ks_introsort with its comb sort and insertion sort, on a Python list, `lt` = __sort_lt ----------------------------------
def _insertsort(a, s, t, lt):
    for i in range(s + 1, t):
        j = i
        while j > s and lt(a[j], a[j - 1]):
            a[j], a[j - 1] = a[j - 1], a[j]
            j -= 1


def _combsort(a, s, n, lt):
    shrink = 1.2473309501039786540366528676643
    gap = n
    while True:
        if gap > 2:
            gap = int(gap / shrink)
            if gap in (9, 10):
                gap = 11
        do_swap = False
        for i in range(s, s + n - gap):
            j = i + gap
            if lt(a[j], a[i]):
                a[i], a[j] = a[j], a[i]
                do_swap = True
        if not (do_swap or gap > 2):
            break
    if gap != 1:
        _insertsort(a, s, s + n, lt)


def ks_introsort(a, lt):
    n = len(a)
    if n < 1:
        return
    if n == 2:
        if lt(a[1], a[0]):
            a[0], a[1] = a[1], a[0]
        return
    d = 2
    while (1 << d) < n:
        d += 1
    d <<= 1
    s, t, stack = 0, n - 1, []
    while True:
        if s < t:
            d -= 1
            if d == 0:
                _combsort(a, s, t - s + 1, lt)
                t = s
                continue
            i, j = s, t
            k = i + ((j - i) >> 1) + 1
            if lt(a[k], a[i]):
                if lt(a[k], a[j]):
                    k = j
            else:
                k = i if lt(a[j], a[i]) else j
            rp = a[k]
            if k != t:
                a[k], a[t] = a[t], a[k]
            while True:
                i += 1
                while lt(a[i], rp):
                    i += 1
                j -= 1
                while i <= j and lt(rp, a[j]):
                    j -= 1
                if j <= i:
                    break
                a[i], a[j] = a[j], a[i]
            a[i], a[t] = a[t], a[i]
            if i - s > t - i:
                if i - s > 16:
                    stack.append((s, i - 1, d))
                s = i + 1 if t - i > 16 else t
            else:
                if t - i > 16:
                    stack.append((i + 1, t, d))
                t = i - 1 if i - s > 16 else s
        else:
            if not stack:
                _insertsort(a, 0, n, lt)
                return
            s, t, d = stack.pop()


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class _Rec:
    __slots__ = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "csub", "seedcov", "w", "n_comp", "src")


F32 = np.float32
PATCH_MAX_R_BW = float(F32(0.05))
PATCH_MAX_R_BW2 = float(F32(0.05) * F32(2))
PATCH_MIN_SC_RATIO = float(F32(0.90))


def default_opt(**kw):
    o = dict(w=100, max_chain_gap=10000, a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, mask_level_redun=0.95)
    o.update(kw)
    return o


def _patch(o, l_pac, text, query, a, b, C):
    """mem_patch_reg: (score, w) -- score 0: no merge"""
    import oracle_py as O
    if a.rb < l_pac and b.rb >= l_pac:
        return 0, 0
    if a.qb >= b.qb or a.qe >= b.qe or a.re >= b.re:
        return 0, 0
    w = abs((a.re - b.rb) - (a.qe - b.qb))
    r = abs((a.re - b.rb) / float(b.re - a.rb) - (a.qe - b.qb) / float(b.qe - a.qb))
    if a.re < b.rb or a.qe < b.qb:
        if w > o["w"] << 1 or r >= PATCH_MAX_R_BW:
            return 0, 0
    elif w > o["w"] << 2 or r >= PATCH_MAX_R_BW2:
        return 0, 0
    w += a.w + b.w
    w = min(w, o["w"] << 2)
    C["n_patch_jobs"] += 1
    got = O.gen_cigar2(text, l_pac, query[a.qb:b.qe], a.rb, b.re, w, a=o["a"], b=o["b"], o_del=o["o_del"], e_del=o["e_del"], o_ins=o["o_ins"], e_ins=o["e_ins"])
    assert got is not None
    score = got[0]
    q_s = int(float(b.qe - a.qb) / ((b.qe - b.qb) + (a.qe - a.qb)) * (b.score + a.score) + .499)
    r_s = int(float(b.re - a.rb) / ((b.re - b.rb) + (a.re - a.rb)) * (b.score + a.score) + .499)
    den = max(q_s, r_s)
    ratio = score / float(den) if den else (float("nan") if score == 0 else float("inf") * score)
    if ratio < PATCH_MIN_SC_RATIO:
        C["n_ratio_rejected"] += 1
        return 0, w
    return score, w


def model(regs, reg_off, reads, read_off, text, l_pac, contig_alt, opt=None):
    """-> (records left, offsets, useMateSort, counters)"""
    from pymeme import hipapi
    o = opt or default_opt()
    mlr = F32(o["mask_level_redun"])
    gap = o["max_chain_gap"]
    n = reg_off.shape[0] - 1
    C = dict(n_in=0, n_redundant=0, n_patch_jobs=0, n_patched=0, n_ratio_rejected=0, n_identical=0, n_ums0=0, n_above_17=0, n_rounds_max=0)
    out_src, out_rows, off, ums = [], [], np.zeros(n + 1, np.int64), np.ones(n, np.uint8)
    cols = {f: regs[f].tolist() for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "csub", "seedcov", "w", "n_comp_is_alt")}
    for r in range(n):
        a = []
        for k in range(int(reg_off[r]), int(reg_off[r + 1])):
            if cols["qe"][k] > cols["qb"][k]:
                x = _Rec()
                for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "csub", "seedcov", "w"):
                    setattr(x, f, cols[f][k])
                x.n_comp = cols["n_comp_is_alt"][k] & 0x3fffffff
                x.src = k
                a.append(x)
        C["n_in"] += len(a)
        C["n_above_17"] += len(a) > 17
        if len(a) > 1:
            query = reads[read_off[r]:read_off[r + 1]]
            jobs0 = C["n_patch_jobs"]
            ks_introsort(a, lambda x, y: x.re < y.re)
            for x in a:
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
                    mr = min(q.re - q.rb, p.re - p.rb)
                    mq = min(q.qe - q.qb, p.qe - p.qb)
                    if F32(or_) > mlr * F32(mr) and F32(oq) > mlr * F32(mq):
                        C["n_redundant"] += 1
                        if p.score < q.score:
                            p.qe = p.qb
                            break
                        q.qe = q.qb
                    elif q.rb < p.rb:
                        score, w = _patch(o, l_pac, text, query, q, p, C)
                        if score > 0:
                            C["n_patched"] += 1
                            p.n_comp += q.n_comp + 1
                            p.seedcov = max(p.seedcov, q.seedcov)
                            p.sub = max(p.sub, q.sub)
                            p.csub = max(p.csub, q.csub)
                            p.qb, p.rb = q.qb, q.rb
                            p.truesc = p.score = score
                            p.w = w
                            q.qb = q.qe
            C["n_rounds_max"] = max(C["n_rounds_max"], C["n_patch_jobs"] - jobs0)
            a = [x for x in a if x.qe > x.qb]
            if any(a[i].re == a[i + 1].re for i in range(len(a) - 1)):
                ums[r] = 0
                C["n_ums0"] += 1
            ks_introsort(a, lambda x, y: x.score > y.score or (x.score == y.score and (x.rb < y.rb or (x.rb == y.rb and x.qb < y.qb))))
            for i in range(1, len(a)):
                if a[i].score == a[i - 1].score and a[i].rb == a[i - 1].rb and a[i].qb == a[i - 1].qb:
                    a[i].qe = a[i].qb
                    C["n_identical"] += 1
            a = a[:1] + [x for x in a[1:] if x.qe > x.qb]
        for x in a:
            out_src.append(x.src)
            out_rows.append(x)
        off[r + 1] = off[r] + len(a)
    out = take(regs, np.array(out_src, np.int64))
    for f in ("rb", "re", "qb", "qe", "score", "truesc", "sub", "csub", "seedcov", "w"):
        out[f] = [getattr(x, f) for x in out_rows]
    word = out["n_comp_is_alt"].astype(np.int64) & 0xffffffff
    word = (word & 0xc0000000) | np.array([x.n_comp & 0x3fffffff for x in out_rows], np.int64)
    alt = np.asarray(contig_alt, np.int64)
    hit = (out["rid"] >= 0) & (alt[np.maximum(out["rid"], 0)] != 0)
    word[hit] = (word[hit] & 0x3fffffff) | (1 << 30)
    out["n_comp_is_alt"] = word.astype(np.uint32).view(np.int32)
    return out, off, ums, C


# ---- the workload ------------------------------------------------------------------------------------------------------------------------
def _revcomp(x):
    return np.where(x > 3, x, 3 - x)[::-1].astype(np.uint8)


def take(regs, idx):
    """regs[idx] in the 112-byte layout of meme_alnreg (numpy's own indexing packs a padded record type)"""
    from pymeme import hipapi
    out = np.zeros(len(idx), hipapi.ALNREG)
    for f in hipapi.ALNREG.names:
        out[f] = regs[f][idx]
    return out


class _Build:
    def __init__(self, g, l_pac, contig_off, contig_len):
        self.g, self.l_pac, self.coff, self.clen = g, l_pac, contig_off, contig_len
        self.reads, self.recs, self.part = [], [], []

    def rid_of(self, rb, re):
        f0, f1 = (rb, re) if rb < self.l_pac else (2 * self.l_pac - re, 2 * self.l_pac - rb)
        for k in range(len(self.coff)):
            if self.coff[k] <= f0 and f1 <= self.coff[k] + self.clen[k]:
                return k
        return -1

    def rec(self, rb, re, qb, qe, score=None, rid=None, w=100, sub=0, csub=0, seedcov=None, rev=False, read_len=0):
        if rev:                                    # the same alignment seen from the other strand
            rb, re, qb, qe = 2 * self.l_pac - re, 2 * self.l_pac - rb, read_len - qe, read_len - qb
        score = qe - qb if score is None else score
        return dict(rb=rb, re=re, qb=qb, qe=qe, rid=self.rid_of(rb, re) if rid is None else rid, score=score, truesc=score, sub=sub, csub=csub,
                    seedcov=(qe - qb) // 2 if seedcov is None else seedcov, w=w)

    def add(self, part, read, recs):
        self.reads.append(np.ascontiguousarray(read, np.uint8))
        self.recs.append(recs)
        self.part.append(part)


def _sort_part(B, rng):
    """live counts at the edges; `ties`: few distinct end positions; `dups`: copies equal in (score, rb, qb) kept apart by a record of another
    sequence between them in the order by end (the walk never compares them: they meet in the identical-hit pass)"""
    L = B.l_pac
    for n in SORT_COUNTS:
        for variant in ("ties", "dups"):
            for rep in range(2):
                rl = int(rng.integers(150, 501))
                base = int(rng.integers(2000, 90000)) + (L if rep else 0)
                read = B.g[base % L:base % L + rl] if not rep else _revcomp(B.g[2 * L - base - rl:2 * L - base])
                recs = []
                ends = base + rng.integers(60, 60 + max(4, n // 4), size=max(n, 1))
                for k in range(n):
                    ql = int(rng.integers(20, min(rl, 140)))
                    qb = int(rng.integers(0, rl - ql + 1))
                    re = int(ends[rng.integers(0, ends.shape[0])]) + (int(rng.integers(0, 400)) if variant == "dups" else 0)
                    rb = re - ql - int(rng.integers(-3, 4))
                    rid = int(rng.integers(0, 3)) if rng.random() < 0.6 else None
                    recs.append(B.rec(rb, re, qb, qb + ql, score=int(rng.integers(18, 40)), rid=rid, sub=int(rng.integers(0, 20)), csub=int(rng.integers(0, 10)), w=int(rng.choice([100, 200]))))
                if variant == "dups" and n >= 2:
                    for k in range(1, n, 2):          # every second record a copy of its predecessor in (score, rb, qb), on another sequence
                        recs[k]["score"] = recs[k]["truesc"] = recs[k - 1]["score"]
                        recs[k]["rb"], recs[k]["qb"] = recs[k - 1]["rb"], recs[k - 1]["qb"]
                        recs[k]["re"] = max(recs[k]["re"], recs[k]["rb"] + 1)
                        recs[k]["qe"] = max(recs[k]["qe"], recs[k]["qb"] + 1)
                        recs[k]["rid"] = (recs[k - 1]["rid"] + 1) % 3
                # dead records between the live ones (qe <= qb: purged by the extension stage, dropped by the compaction)
                mixed = []
                for x in recs:
                    if rng.random() < 0.2:
                        mixed.append(dict(x, qb=-1, qe=-1))
                    mixed.append(x)
                B.add("sort", read, mixed)


def _redundant_part(B, rng):
    """two records whose overlap on the reference (query fully shared) or on the query (reference fully shared) is round(0.95 * len) - 1, that,
    + 1 for the shorter length len: or_ > 0.95f * len is evaluated in float (0.95f * 100 is exactly 95.0f: 95 is NOT redundant)"""
    for ln in (20, 100, 200, 500):
        for d in (-1, 0, 1):
            ov = int(round(0.95 * ln)) + d
            for rel in (-1, 0, 1):
                for side in ("ref", "query"):
                    for rev in (False, True):
                        rl = 500
                        p0 = int(rng.integers(2000, 90000)) + 100000 * int(rng.integers(0, 3))
                        read = B.g[p0:p0 + rl]
                        if side == "ref":          # reference spans of ln bases overlapping by ov, query spans nearly the same
                            q = B.rec(p0, p0 + ln, 0, 60, score=50, rev=rev, read_len=rl)
                            p = B.rec(p0 + ln - ov, p0 + 2 * ln - ov, 1, 61, score=50 + rel, rev=rev, read_len=rl)
                        else:                      # query spans of ln bases (at most the read) overlapping by ov, reference spans nearly the same
                            lq = min(ln, 250)
                            ovq = int(round(0.95 * lq)) + d
                            q = B.rec(p0, p0 + 300, 0, lq, score=50, rev=rev, read_len=rl)
                            p = B.rec(p0 + 1, p0 + 301, lq - ovq, 2 * lq - ovq, score=50 + rel, rev=rev, read_len=rl)
                        B.add("redundant", _revcomp(read) if rev else read, [p, q] if rng.random() < 0.5 else [q, p])


def _patch_part(B, rng):
    g = B.g

    def spot(span):                                 # a stretch inside one contig
        c = int(rng.integers(0, 3))
        return int(B.coff[c]) + int(rng.integers(500, int(B.clen[c]) - span - 500))

    def pieces(kinds, lens, gaps, junk=0):
        """read = pieces of the genome separated by deletions (kind 'D': gap bases of the reference skipped), insertions ('I': gap random bases
        in the read) or `junk` unrelated bases on both; returns (read, [(rb, re, qb, qe)] of the pieces, forward strand)"""
        p = spot(sum(lens) + sum(gaps) + junk * len(gaps) + 10)
        read, spans, q = [], [], 0
        for k, ln in enumerate(lens):
            read.append(g[p:p + ln])
            spans.append((p, p + ln, q, q + ln))
            p += ln
            q += ln
            if k < len(gaps):
                if junk:
                    read.append(rng.integers(0, 4, size=junk).astype(np.uint8))
                    p += junk
                    q += junk
                if kinds[k] == "D":
                    p += gaps[k]
                else:
                    read.append(rng.integers(0, 4, size=gaps[k]).astype(np.uint8))
                    q += gaps[k]
        return np.concatenate(read), spans

    def emit(read, spans, rev, shuffle=True, **kw):
        rl = read.shape[0]
        recs = [B.rec(*s, rev=rev, read_len=rl, **kw) for s in spans]
        if shuffle:
            rng.shuffle(recs)
        B.add("patch", _revcomp(read) if rev else read, recs)

    for it in range(150):                           # merged: two pieces around an indel of 1-25 bases
        rev = bool(it & 1)
        d = 1 + it % 25
        l1, l2 = int(rng.integers(150, 235)), int(rng.integers(150, 235))
        read, spans = pieces("D" if it % 4 < 2 else "I", [l1, l2], [d])
        if it % 3 == 0:                             # the pieces as the extension would leave them: overlapping by a few bases on both
            ov = int(rng.integers(1, 6))
            spans[0] = (spans[0][0], spans[0][1] + ov, spans[0][2], spans[0][3] + ov)
        emit(read, spans, rev, w=int(rng.choice([100, 120])))
    for it in range(60):                            # chained a -> b -> c
        rev = bool(it & 1)
        read, spans = pieces(rng.choice(["D", "I"], size=2), [int(rng.integers(90, 150)) for _ in range(3)], [int(rng.integers(1, 9)) for _ in range(2)])
        emit(read, spans, rev)
    for it in range(80):                            # rejected by the 0.90 score ratio: unrelated bases between the pieces
        rev = bool(it & 1)
        read, spans = pieces("D", [int(rng.integers(100, 200)), int(rng.integers(100, 200))], [int(rng.integers(0, 4))], junk=int(rng.integers(40, 70)))
        emit(read, spans, rev)
    # the bars of mem_patch_reg.  The records need not be alignments of their reads: the spans are set to sit on either side of a bar.
    for rev in (False, True):
        for w_need in (199, 200, 201):              # w == opt->w << 1, no overlap: the reference gap is w_need longer than the query gap
            p = spot(12000)
            read = g[p:p + 400]
            emit(read, [(p, p + 4000, 0, 200), (p + 4000 + w_need, p + 9000, 200, 400)], rev)
        for w_need in (399, 400, 401):              # w == opt->w << 2, overlapping on both: by w_need + 20 on the reference and 20 on the query
            p = spot(12000)
            read = g[p:p + 400]
            emit(read, [(p, p + 5000, 0, 210), (p + 5000 - (w_need + 20), p + 10000, 190, 400)], rev)
        for gp in (19, 20, 21):                     # relative bandwidth at 0.05 (a float constant: 20 / 400 = 0.05 < 0.05f), no overlap
            p = spot(2000)
            read = np.concatenate([g[p:p + 190], g[p + 190 + gp:p + 190 + gp + 190]])
            emit(read, [(p, p + 190, 0, 190), (p + 190 + gp, p + 400, 190, 380 - gp + 0)], rev)
        for x in (39, 40, 41):                      # ... and at 0.10 with both overlapping: x / 400 on the reference, none on the query side of the difference
            p = spot(2000)
            read = g[p:p + 300]
            emit(read, [(p, p + 200 + x, 0, 150), (p + 200, p + 400, 150, 300)], rev)
        for it in range(6):
            p = spot(12000)
            read = g[p:p + 300]
            if it == 0:   # not colinear: the later piece of the reference is the earlier piece of the read
                emit(read, [(p, p + 140, 150, 290), (p + 150, p + 300, 0, 150)], rev)
            elif it == 1:   # different strands, inside the window: the end of the forward strand and the start of the reverse strand (the last contig on both)
                L = B.l_pac
                B.add("patch", g[L - 400:L - 100], [B.rec(L - 400, L - 260, 0, 140), B.rec(L + 100, L + 250, 150, 300)])
            elif it == 2:   # different sequences: across a contig boundary
                e = int(B.coff[1])
                B.add("patch", g[e - 150:e + 150], [B.rec(e - 150, e - 5, 0, 145, rev=rev, read_len=300), B.rec(e + 5, e + 150, 155, 300, rev=rev, read_len=300)])
            elif it == 3:   # outside the max_chain_gap window
                emit(read, [(p, p + 140, 0, 140), (p + 140 + 10000, p + 10300, 150, 300)], rev)
            elif it == 4:   # just inside it
                emit(read, [(p, p + 140, 0, 140), (p + 140 + 9999, p + 10300, 150, 300)], rev)
            else:           # a lone record and none at all
                emit(read, [(p, p + 300, 0, 300)], rev)
                B.add("patch", read, [])


def workload():
    """-> dict: reads, read_off, regs (hipapi.ALNREG), reg_off, part (per read), text, l_pac, contigs [(offset, len, is_alt)], genome, first_real (index of the first
    read of the `real` part: the reads of common.ext_golden_inputs() in their order)"""
    if "w" in _CACHE:
        return _CACHE["w"]
    from pymeme import hipapi
    I = ext_golden_inputs()
    G = np.load(os.path.join(GOLDEN, "ext_golden.npz"))
    g, l_pac = I["genome"], int(I["l_pac"])
    B = _Build(g, l_pac, [int(x) for x in I["contig_off"]], [int(x) for x in I["contig_len"]])
    rng = np.random.default_rng(4242)
    _sort_part(B, rng)
    _redundant_part(B, rng)
    _patch_part(B, rng)
    first_real = len(B.reads)
    rows = [x for recs in B.recs for x in recs]
    syn = np.zeros(len(rows), hipapi.ALNREG)
    for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "csub", "seedcov", "w"):
        syn[f] = [x[f] for x in rows]
    syn["seedlen0"] = 19
    syn["secondary"] = -1
    syn["c"] = np.arange(len(rows))                 # (a dead field: tells a record from its copies)
    syn["frac_rep"] = 0.25
    real = np.zeros(G["regs"].shape[0], hipapi.ALNREG)   # the golden extension records, live and purged, as meme_extend_last_batch_host leaves them
    import oracle_py as O
    for k, f in enumerate(O.ALNREG_FIELDS):
        real[f] = G["regs"][:, k]
    real["frac_rep"] = G["frac_rep_bits"].view(np.float32)
    reads = B.reads + I["reads_list"]
    read_off = np.zeros(len(reads) + 1, np.int64)
    read_off[1:] = np.cumsum([len(r) for r in reads])
    syn_off = np.concatenate([[0], np.cumsum([len(x) for x in B.recs])]).astype(np.int64)
    W = {"reads": np.concatenate(reads), "read_off": read_off, "regs": take(np.concatenate([syn, real]), np.arange(syn.shape[0] + real.shape[0])), "reg_off": np.concatenate([syn_off, syn_off[-1] + G["reg_off"][1:]]),
         "part": B.part + ["real"] * len(I["reads_list"]), "text": I["text"], "l_pac": l_pac, "genome": g, "first_real": first_real,
         "contigs": [(int(o), int(l), 1 if k == ALT_CONTIG else 0) for k, (o, l) in enumerate(zip(I["contig_off"], I["contig_len"]))]}
    _CACHE["w"] = W
    return W


def golden():
    G = np.load(os.path.join(GOLDEN, "finish_golden.npz"))
    from pymeme import hipapi
    regs = np.zeros(G["cols"].shape[0], hipapi.ALNREG)
    for k, f in enumerate(GOLDEN_FIELDS):
        regs[f] = G["cols"][:, k]
    regs["frac_rep"] = G["frac_rep_bits"].view(np.float32)
    return regs, G["reg_off"], G["use_mate_sort"]


GOLDEN_FIELDS = ("rb", "re", "qb", "qe", "rid", "c", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w", "seedcov", "secondary", "secondary_all", "seedlen0", "n_comp_is_alt",
                 "hash", "flg")


def same_records(got, got_off, got_ums, want, want_off, want_ums):
    """exact equality of every field, the offsets and the flag; returns None or a description of the first difference"""
    if not np.array_equal(got_off, want_off):
        r = int(np.nonzero(np.asarray(got_off) != np.asarray(want_off))[0][0]) - 1 if len(got_off) == len(want_off) else -1
        return "offsets differ from read %d on" % r
    for f in GOLDEN_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        if bad.size:
            k = int(bad[0])
            return "field %s of record %d (read %d): %r, expected %r" % (f, k, int(np.searchsorted(want_off, k, "right")) - 1, got[f][k], want[f][k])
    if not np.array_equal(got["frac_rep"].view(np.uint32), want["frac_rep"].view(np.uint32)):
        return "frac_rep differs"
    if not np.array_equal(got_ums, want_ums):
        return "useMateSort differs at read %d" % int(np.nonzero(np.asarray(got_ums) != np.asarray(want_ums))[0][0])
    return None
