"""ctypes driver of the COMPILED REFERENCE's own mem_sam_pe (oracle/_ref/libbwa_pic.so exports every symbol; TEST INFRASTRUCTURE ONLY), called per pair with
opt->flag |= MEM_F_NO_RESCUE | MEM_F_ALL, so that neither mate rescue nor mem_gen_alt runs: the function then marks primaries, calls mem_pair, decides
(reference src/bwamem_pair.cpp:523-658) and writes the SAM lines of both ends.  The bntseq_t is made here (anns with offset, len, is_alt and name), the pac
is packed from tests/decide_gen.py's genome, the two bseq1_t carry equal names and code sequences.  What comes back: the records as the call leaves them,
and per end the number of SAM lines, FLAG and MAPQ of the first, the record it reports and the record its mate fields point to, both found by position and
strand (tests/decide_gen.py: leftmost)."""
import ctypes as C

import numpy as np

import decide_gen as DG
import ref_finish
from ref_pair import AlnregV, PeStat

MEM_SAM_PE = "_Z10mem_sam_pePK9mem_opt_tPK8bntseq_tPKhPK12mem_pestat_tmP7bseq1_tP12mem_alnreg_v"
# (const mem_opt_t*, const bntseq_t*, const uint8_t* pac, const mem_pestat_t[4], uint64_t id, bseq1_t[2], mem_alnreg_v[2]) -> int
MEM_F_NOPAIRING, MEM_F_ALL, MEM_F_NO_RESCUE = 0x4, 0x8, 0x20


class Bseq1(C.Structure):           # bseq1_t, src/bwa.h:68-71
    _fields_ = [("l_seq", C.c_int), ("id", C.c_int), ("name", C.c_char_p), ("comment", C.c_char_p), ("seq", C.c_void_p), ("qual", C.c_char_p), ("sam", C.c_void_p)]


class Reference:
    """The reference's options: mem_opt_init, the two flags, then the fields given (mem_opt_t names; no_pairing sets MEM_F_NOPAIRING)."""

    def __init__(self, no_pairing=0, **fields):
        L = ref_finish.lib()
        self.opt = L._Z12mem_opt_initv()
        o = self.opt.contents
        assert (o.a, o.b, o.pen_unpaired, o.T, o.min_seed_len, o.mapQ_coef_fac) == (1, 4, 17, 30, 19, 3), "mem_opt_t layout"
        for k, v in fields.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        L.bwa_fill_scmat(o.a, o.b, C.addressof(o.mat))
        o.flag |= MEM_F_NO_RESCUE | MEM_F_ALL | (MEM_F_NOPAIRING if no_pairing else 0)
        self.names = [n.encode() for n in DG.NAMES]
        self.anns = (ref_finish.BntAnn * len(DG.CONTIGS))()
        for k, (off, ln, alt) in enumerate(DG.CONTIGS):
            self.anns[k].offset, self.anns[k].len, self.anns[k].is_alt, self.anns[k].name, self.anns[k].anno = off, ln, alt, self.names[k], b""
        self.bns = ref_finish.BntSeq()
        self.bns.l_pac, self.bns.n_seqs, self.bns.anns = DG.L_PAC, len(DG.CONTIGS), C.cast(self.anns, C.POINTER(ref_finish.BntAnn))
        self.pac = DG.genome()[1]
        self.fn = getattr(L, MEM_SAM_PE)
        self.fn.restype = C.c_int
        self.fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        self.free = C.CDLL(None).free
        self.free.argtypes = [C.c_void_p]

    def run(self, B):
        """a batch of tests/decide_gen.py -> (obs: DG.OBS -> int array per read, regs: the records behind the calls)"""
        regs, off = B["regs"].copy(), B["reg_off"]
        assert regs.dtype.itemsize == 112 and regs.flags["C_CONTIGUOUS"]
        n = off.shape[0] - 1
        obs = {f: np.zeros(n, np.int32) for f in DG.OBS}
        pes = (PeStat * 4)(*[PeStat(lo, hi, f, avg, std) for lo, hi, f, avg, std in B["pes"]])
        base = regs.ctypes.data
        for p in range(n // 2):
            cnt = [int(off[2 * p + r + 1] - off[2 * p + r]) for r in range(2)]
            a = (AlnregV * 2)(*[AlnregV(cnt[r], cnt[r], base + 112 * int(off[2 * p + r])) for r in range(2)])
            seqs = [DG.read_codes(B, 2 * p + r) for r in range(2)]
            s = (Bseq1 * 2)(*[Bseq1(DG.READ_LEN, 2 * p + r, b"pair%d" % p, None, seqs[r].ctypes.data, None, None) for r in range(2)])
            self.fn(C.cast(self.opt, C.c_void_p), C.addressof(self.bns), self.pac.ctypes.data, C.addressof(pes), C.c_uint64(B["id_base"] + p), C.addressof(s), C.addressof(a))
            assert (a[0].n, a[1].n) == tuple(cnt)
            for r in range(2):
                text = C.string_at(s[r].sam).decode()
                self.free(s[r].sam)
                where = [{DG.leftmost(regs[k]): k - int(off[2 * p + e]) for k in range(int(off[2 * p + e]), int(off[2 * p + e + 1]))} for e in range(2)]
                lines = text.rstrip("\n").split("\n")
                f = lines[0].split("\t")
                flag, rname, pos, mapq, rnext, pnext = int(f[1]), f[2], int(f[3]), int(f[4]), f[6], int(f[7])
                rid = DG.NAMES.index(rname) if rname != "*" else -1
                rid2 = rid if rnext == "=" else DG.NAMES.index(rnext) if rnext != "*" else -1
                k = 2 * p + r
                obs["n_lines"][k], obs["flag0"][k], obs["mapq0"][k] = len(lines), flag, mapq
                obs["rec0"][k] = -1 if flag & 4 else where[r][(rid, int(bool(flag & 16)), pos - 1)]
                obs["mate"][k] = -1 if flag & 8 else where[1 - r][(rid2, int(bool(flag & 32)), pnext - 1)]
        return obs, regs
