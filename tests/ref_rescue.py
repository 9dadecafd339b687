"""ctypes driver of the COMPILED REFERENCE's own mate-rescue post functions (oracle/_ref/libbwa_pic.so exports every symbol; TEST INFRASTRUCTURE ONLY), two ways.  Piecewise:
mem_matesw_batch_post, mem_matesw_batch_post_mate_sort, sort_alnreg_re, sort_alnreg_score and mem_sort_dedup_patch themselves, by mangled name, inside a restatement of
the forty lines of mem_sam_pe_batch_post around them (reference src/bwamem_pair.cpp:851-921).  What comes back are the records RIGHT BEHIND rescue, before the primary
marking.  The lists live in libc's heap (kv_push reallocs them); the bntseq_t is made here as tests/ref_decide.py makes it, the pac is tests/decide_gen.py's genome.
Whole (Reference.run_whole): mem_sam_pe_batch_post itself per pair, with MEM_F_ALL set and MEM_F_NO_RESCUE clear -- rescue, primary marking, mem_pair, the decision and the
SAM lines in one call; gar goes through a zeroed buffer that stands for mem_cache (seqPairArrayAux is its first member, src/bwamem.h:198-200; tid 0), gcnt is the caller's
and starts at 0 with every worker batch.  What comes back: every record behind the whole function and the observables of tests/decide_gen.py (OBS), the records a SAM line
names found by position and strand.  This is the one check that does not share the restated loop with the model.
pose() and kswv() are the compiled reference's posing and Smith-Waterman (oracle/ref_stage_shim.cpp), batch by batch, for the fixture's generator."""
import ctypes as C

import numpy as np

import decide_gen as DG
import ref_finish
import ref_py
import rescue_gen as RG
from ref_decide import MEM_F_ALL, MEM_F_NO_RESCUE, Bseq1
from ref_pair import AlnregV, PeStat

POST = "_Z21mem_matesw_batch_postPK9mem_opt_tPK8bntseq_tPKhPK12mem_pestat_tPK12mem_alnreg_tiS6_P12mem_alnreg_vPP6kswr_tiPiP9mem_cache"
POST_MS = "_Z31mem_matesw_batch_post_mate_sortPK9mem_opt_tPK8bntseq_tPKhPK12mem_pestat_tPK12mem_alnreg_tiS6_P12mem_alnreg_vPP6kswr_tiPiP9mem_cache"
# (opt, bns, pac, pes[4], const mem_alnreg_t* a, int l_ms, const uint8_t* ms, mem_alnreg_v* ma, kswr_t** myaln, int32_t gcnt, int32_t* gar, mem_cache*) -> int
POST_WHOLE = "_Z21mem_sam_pe_batch_postPK9mem_opt_tPK8bntseq_tPKhPK12mem_pestat_tmP7bseq1_tP12mem_alnreg_vPP6kswr_tP9mem_cacheRii"
# (opt, bns, pac, pes[4], uint64_t id, bseq1_t s[2], mem_alnreg_v a[2], kswr_t** myaln, mem_cache*, int32_t& gcnt, int tid) -> int
SORT_RE, SORT_SCORE = "_Z14sort_alnreg_reiP12mem_alnreg_t", "_Z17sort_alnreg_scoreiP12mem_alnreg_t"
SORT_DEDUP_PATCH = "_Z20mem_sort_dedup_patchPK9mem_opt_tPK8bntseq_tPKhPhiP12mem_alnreg_t"


class Reference:
    def __init__(self, **fields):
        L = ref_finish.lib()
        self.opt = L._Z12mem_opt_initv()
        o = self.opt.contents
        assert (o.a, o.pen_unpaired, o.min_seed_len, o.max_matesw, o.max_chain_gap) == (1, 17, 19, 50, 10000), "mem_opt_t layout"
        for k, v in fields.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        self.anns = (ref_finish.BntAnn * len(DG.CONTIGS))()
        self.names = [n.encode() for n in DG.NAMES]
        for k, (off, ln, alt) in enumerate(DG.CONTIGS):
            self.anns[k].offset, self.anns[k].len, self.anns[k].is_alt, self.anns[k].name, self.anns[k].anno = off, ln, alt, self.names[k], b""
        self.bns = ref_finish.BntSeq()
        self.bns.l_pac, self.bns.n_seqs, self.bns.anns = DG.L_PAC, len(DG.CONTIGS), C.cast(self.anns, C.POINTER(ref_finish.BntAnn))
        self.pac = DG.genome()[1]
        self.post, self.post_ms = getattr(L, POST), getattr(L, POST_MS)
        for f in (self.post, self.post_ms):
            f.restype = C.c_int
            f.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.sort_re, self.sort_score, self.sdp = getattr(L, SORT_RE), getattr(L, SORT_SCORE), getattr(L, SORT_DEDUP_PATCH)
        for f in (self.sort_re, self.sort_score):
            f.restype = None
            f.argtypes = [C.c_int, C.c_void_p]
        self.sdp.restype = C.c_int
        self.sdp.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        libc = C.CDLL(None)
        self.malloc, self.free = libc.malloc, libc.free
        self.malloc.restype = C.c_void_p
        self.malloc.argtypes = [C.c_size_t]
        self.free.argtypes = [C.c_void_p]

    def run(self, B):
        """a batch of tests/rescue_gen.py -> dict(regs, reg_off): every list as the loop leaves it"""
        o = self.opt.contents
        d = RG.default_opt(**B["opt"])
        o.pen_unpaired, o.max_matesw, o.min_seed_len, o.max_chain_gap, o.mask_level_redun = d["pen_unpaired"], d["max_matesw"], d["min_seed_len"], d["max_chain_gap"], d["mask_level_redun"]
        regs, off = B["regs"], B["reg_off"]
        assert regs.dtype.itemsize == 112 and regs.flags["C_CONTIGUOUS"]
        n = off.shape[0] - 1
        pes = (PeStat * 4)(*[PeStat(lo, hi, f, avg, std) for lo, hi, f, avg, std in B["pes"]])
        res = np.ascontiguousarray(B["res"])
        gar = np.ascontiguousarray(B["gar"])
        out, out_off = [], np.zeros(n + 1, np.int64)
        gcnt = 0
        opt, bns, pac = C.cast(self.opt, C.c_void_p), C.addressof(self.bns), self.pac.ctypes.data
        for p in range(n // 2):
            if (2 * p) % d["batch_reads"] == 0:
                gcnt = 0
            bt = 2 * p // d["batch_reads"]
            myaln = C.c_void_p(res.ctypes.data + 28 * int(B["job_off"][bt]))
            gar_p = gar.ctypes.data + 4 * int(B["gar_off"][bt])
            cnt = [int(off[2 * p + i + 1] - off[2 * p + i]) for i in range(2)]
            a = (AlnregV * 2)()
            seqs = [np.ascontiguousarray(B["reads"][int(B["read_off"][2 * p + i]):int(B["read_off"][2 * p + i + 1])]).copy() for i in range(2)]
            b = []
            for i in range(2):
                src = ref_finish.take(regs, np.arange(int(off[2 * p + i]), int(off[2 * p + i + 1])))
                a[i].n, a[i].m, a[i].a = cnt[i], max(cnt[i], 1), self.malloc(112 * max(cnt[i], 1))
                a[i].useMateSort = bool(B["ums"][2 * p + i])
                C.memmove(a[i].a, src.ctypes.data, 112 * cnt[i])
                b.append(ref_finish.take(src, np.nonzero(src["score"] >= src["score"][0] - o.pen_unpaired)[0]) if cnt[i] else src)      # :854-857
            for i in range(2):                                                     # :859-862
                v = np.frombuffer((C.c_char * (112 * cnt[i])).from_address(a[i].a), dtype=regs.dtype) if cnt[i] else None
                if v is not None:
                    v["flg"] = 0
            mate_sort = bool(a[0].useMateSort) and bool(a[1].useMateSort)          # :865-871
            for i in range(2):
                ma = a[1 - i]
                l_ms, ms = int(seqs[1 - i].shape[0]), seqs[1 - i].ctypes.data
                if mate_sort:
                    if b[i].shape[0] > 0:
                        self.sort_re(C.c_int(ma.n), ma.a)
                        swcount = 0
                        for j in range(min(b[i].shape[0], o.max_matesw)):
                            swcount += self.post_ms(opt, bns, pac, C.addressof(pes), b[i].ctypes.data + 112 * j, l_ms, ms, C.addressof(ma), C.addressof(myaln), gcnt, gar_p, None)
                            gcnt += 4
                        if swcount > 0:
                            ma.n = self.sdp(opt, None, None, None, C.c_int(ma.n), ma.a)
                        else:
                            self.sort_score(C.c_int(ma.n), ma.a)
                else:
                    for j in range(min(b[i].shape[0], o.max_matesw)):
                        self.post(opt, bns, pac, C.addressof(pes), b[i].ctypes.data + 112 * j, l_ms, ms, C.addressof(ma), C.addressof(myaln), gcnt, gar_p, None)
                        gcnt += 4
            for i in range(2):
                m = int(a[i].n)
                got = np.frombuffer(C.string_at(a[i].a, 112 * m), dtype=regs.dtype).copy() if m else regs[:0].copy()
                out.append(got)
                out_off[2 * p + i + 1] = out_off[2 * p + i] + m
                self.free(a[i].a)
        allr = np.concatenate(out) if out else regs[:0].copy()
        return {"regs": ref_finish.take(allr, np.arange(allr.shape[0])), "reg_off": out_off, "status": np.zeros(n, np.uint8)}


    def run_whole(self, B):
        """a batch of family A -> (obs: DG.OBS -> int array per read, dict(regs, reg_off): every record behind the whole function); pair p has id RG.WHOLE_ID_BASE + p"""
        R = self
        L = ref_finish.lib()
        fn = getattr(L, POST_WHOLE)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 5 + [C.c_int]
        o = R.opt.contents
        d = RG.default_opt(**B["opt"])
        o.pen_unpaired, o.max_matesw, o.min_seed_len, o.max_chain_gap, o.mask_level_redun = d["pen_unpaired"], d["max_matesw"], d["min_seed_len"], d["max_chain_gap"], d["mask_level_redun"]
        L.bwa_fill_scmat(o.a, o.b, C.addressof(o.mat))
        o.flag = (o.flag | MEM_F_ALL) & ~MEM_F_NO_RESCUE
        regs, off = B["regs"], B["reg_off"]
        n = off.shape[0] - 1
        pes = (PeStat * 4)(*[PeStat(lo, hi, f, avg, std) for lo, hi, f, avg, std in B["pes"]])
        res, gar = np.ascontiguousarray(B["res"]), np.ascontiguousarray(B["gar"])
        mmc = (C.c_void_p * (1 << 17))()
        out, out_off = [], np.zeros(n + 1, np.int64)
        obs = {f: np.zeros(n, np.int32) for f in DG.OBS}
        gcnt = C.c_int32(0)
        opt, bns, pac = C.cast(R.opt, C.c_void_p), C.addressof(R.bns), R.pac.ctypes.data
        for p in range(n // 2):
            if (2 * p) % d["batch_reads"] == 0:
                gcnt.value = 0
            bt = 2 * p // d["batch_reads"]
            myaln = C.c_void_p(res.ctypes.data + 28 * int(B["job_off"][bt]))
            mmc[0] = gar.ctypes.data + 4 * int(B["gar_off"][bt])
            cnt = [int(off[2 * p + i + 1] - off[2 * p + i]) for i in range(2)]
            a = (AlnregV * 2)()
            seqs = [np.ascontiguousarray(B["reads"][int(B["read_off"][2 * p + i]):int(B["read_off"][2 * p + i + 1])]).copy() for i in range(2)]
            for i in range(2):
                src = ref_finish.take(regs, np.arange(int(off[2 * p + i]), int(off[2 * p + i + 1])))
                a[i].n, a[i].m, a[i].a = cnt[i], max(cnt[i], 1), R.malloc(112 * max(cnt[i], 1))
                a[i].useMateSort = bool(B["ums"][2 * p + i])
                C.memmove(a[i].a, src.ctypes.data, 112 * cnt[i])
            s = (Bseq1 * 2)(*[Bseq1(int(seqs[i].shape[0]), 2 * p + i, b"pair%d" % p, None, seqs[i].ctypes.data, None, None) for i in range(2)])
            fn(opt, bns, pac, C.addressof(pes), C.c_uint64(RG.WHOLE_ID_BASE + p), C.addressof(s), C.addressof(a), C.addressof(myaln), C.addressof(mmc), C.addressof(gcnt), 0)
            got = []
            for i in range(2):
                m = int(a[i].n)
                g = np.frombuffer(C.string_at(a[i].a, 112 * m), dtype=regs.dtype).copy() if m else regs[:0].copy()
                got.append(g)
                out.append(g)
                out_off[2 * p + i + 1] = out_off[2 * p + i] + m
                R.free(a[i].a)
            for r in range(2):
                text = C.string_at(s[r].sam).decode()
                R.free(s[r].sam)
                where = [{DG.leftmost(got[e][k]): k for k in range(got[e].shape[0])} for e in range(2)]
                lines = text.rstrip("\n").split("\n")
                f = lines[0].split("\t")
                flag, rname, pos, mapq, rnext, pnext = int(f[1]), f[2], int(f[3]), int(f[4]), f[6], int(f[7])
                rid = DG.NAMES.index(rname) if rname != "*" else -1
                rid2 = rid if rnext == "=" else DG.NAMES.index(rnext) if rnext != "*" else -1
                k = 2 * p + r
                obs["n_lines"][k], obs["flag0"][k], obs["mapq0"][k] = len(lines), flag, mapq
                obs["rec0"][k] = -1 if flag & 4 else where[r].get((rid, int(bool(flag & 16)), pos - 1), -2)
                obs["mate"][k] = -1 if flag & 8 else where[1 - r].get((rid2, int(bool(flag & 32)), pnext - 1), -2)
        allr = np.concatenate(out) if out else regs[:0].copy()
        return obs, {"regs": ref_finish.take(allr, np.arange(allr.shape[0])), "reg_off": out_off, "status": np.zeros(n, np.uint8)}


def pose(B):
    """the compiled reference's mem_sam_pe_batch_pre, worker batch by worker batch -> (gar, gar_off, job_off, [(KSWV jobs, ref bytes, query bytes) per batch])"""
    from oracle_py import MATE_REG_DTYPE
    o = RG.default_opt(**B["opt"])
    n = B["reg_off"].shape[0] - 1
    mr = np.zeros(B["regs"].shape[0], MATE_REG_DTYPE)
    for f in ("rb", "rid", "score"):
        mr[f] = B["regs"][f]
    g = DG.genome()[0]
    gar, gar_off, job_off, parts = [], [0], [0], []
    for first in range(0, n, o["batch_reads"]):
        count = min(o["batch_reads"], n - first)
        ga, jobs, ref, qer = ref_py.matesw_pose(g, RG.L_PAC, [c[0] for c in RG.CONTIGS], [c[1] for c in RG.CONTIGS], B["reads"], B["read_off"], first, count, mr, B["reg_off"],
                                                [p[:3] for p in B["pes"]], a=o["a"], pen_unpaired=o["pen_unpaired"], max_matesw=o["max_matesw"], min_seed_len=o["min_seed_len"])
        gar.append(ga)
        gar_off.append(gar_off[-1] + ga.shape[0])
        job_off.append(job_off[-1] + jobs.shape[0])
        parts.append((jobs, ref, qer))
    return np.concatenate(gar) if gar else np.zeros(0, np.int32), np.array(gar_off, np.int64), np.array(job_off, np.int64), parts


def kswv(parts):
    """the compiled reference's kswv on the posed jobs of every worker batch -> KSWR records in posing order"""
    out = [ref_py.kswv_batch(jobs, ref, qer) for jobs, ref, qer in parts if jobs.shape[0]]
    res = np.zeros(sum(x.shape[0] for x in out), RG.KSWR)
    at = 0
    for x in out:
        for f in RG.KSWR.names:
            res[f][at:at + x.shape[0]] = x[f]
        at += x.shape[0]
    return res
