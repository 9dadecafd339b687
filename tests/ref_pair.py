"""ctypes driver of the COMPILED REFERENCE's own mem_pair (oracle/_ref/libbwa_pic.so exports every symbol; TEST INFRASTRUCTURE ONLY), called per pair as
mem_sam_pe calls it (reference src/bwamem_pair.cpp:931): only where both ends have records that take part, z preset to -1.  The bntseq_t is made here --
l_pac and an anns array with the contigs' offsets are all the function reads of it; pac and the two bseq1_t are not read."""
import ctypes as C
import time

import numpy as np

import ref_finish

MEM_PAIR = "_Z8mem_pairPK9mem_opt_tPK8bntseq_tPKhPK12mem_pestat_tP7bseq1_tP12mem_alnreg_viPiSE_SE_SE_"
# (const mem_opt_t*, const bntseq_t*, const uint8_t*, const mem_pestat_t[4], bseq1_t[2], mem_alnreg_v[2], int id, int* sub, int* n_sub, int z[2], int n_pri[2]) -> int


class AlnregV(C.Structure):         # mem_alnreg_v as the reference is built (MATE_SORT=1), src/bwamem.h:166-173: mem_pair takes an array of two
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p), ("pad", C.c_size_t * 4), ("useMateSort", C.c_bool)]


class PeStat(C.Structure):          # mem_pestat_t, src/bwamem.h:175
    _fields_ = [("low", C.c_int), ("high", C.c_int), ("failed", C.c_int), ("avg", C.c_double), ("std", C.c_double)]


assert C.sizeof(PeStat) == 32 and C.sizeof(AlnregV) == 64


class Reference:
    """The reference's options: mem_opt_init, then the fields given (mem_opt_t names); contigs: (offset, len, is_alt)."""

    def __init__(self, contigs, l_pac, **fields):
        L = ref_finish.lib()
        self.opt = L._Z12mem_opt_initv()
        o = self.opt.contents
        assert (o.a, o.b, o.o_del, o.e_del, o.o_ins, o.e_ins) == (1, 4, 6, 1, 6, 1), "mem_opt_t layout"
        for k, v in fields.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        self.anns = (ref_finish.BntAnn * len(contigs))()
        for k, (off, ln, alt) in enumerate(contigs):
            self.anns[k].offset, self.anns[k].len, self.anns[k].is_alt = off, ln, alt
        self.bns = ref_finish.BntSeq()
        self.bns.l_pac, self.bns.n_seqs, self.bns.anns = l_pac, len(contigs), C.cast(self.anns, C.POINTER(ref_finish.BntAnn))
        self.fn = getattr(L, MEM_PAIR)
        self.fn.restype = C.c_int
        self.fn.argtypes = [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 4

    def run(self, B):
        """a batch of tests/pair_gen.py -> dict(score, sub, n_sub, z, seconds: time spent inside the reference's function)"""
        regs, off = B["regs"], B["reg_off"]
        assert regs.dtype.itemsize == 112 and regs.flags["C_CONTIGUOUS"]
        npairs = (off.shape[0] - 1) // 2
        out = {k: np.zeros(npairs, np.int32) for k in ("score", "sub", "n_sub")}
        out["z"] = np.full((npairs, 2), -1, np.int32)
        pes = (PeStat * 4)(*[PeStat(lo, hi, f, avg, std) for lo, hi, f, avg, std in B["pes"]])
        base = regs.ctypes.data
        before = regs.tobytes()
        spent = 0.0
        for p in range(npairs):
            n = [int(B["n_pri"][2 * p]), int(B["n_pri"][2 * p + 1])]
            if n[0] == 0 or n[1] == 0:
                continue
            a = (AlnregV * 2)(*[AlnregV(int(off[2 * p + r + 1] - off[2 * p + r]), int(off[2 * p + r + 1] - off[2 * p + r]), base + 112 * int(off[2 * p + r])) for r in range(2)])
            n_pri = (C.c_int * 2)(*n)
            z = (C.c_int * 2)(-1, -1)
            sub, n_sub = C.c_int(-9), C.c_int(-9)
            pair_id = (B["id_base"] + p) & 0xffffffff                         # (the prototype's int: the id is truncated at the call)
            t0 = time.perf_counter()
            ret = self.fn(C.cast(self.opt, C.c_void_p), C.addressof(self.bns), None, C.addressof(pes), None, C.addressof(a), C.c_int(pair_id - (1 << 32) if pair_id >> 31 else pair_id),
                          C.addressof(sub), C.addressof(n_sub), C.addressof(z), C.addressof(n_pri))
            spent += time.perf_counter() - t0
            out["score"][p], out["sub"][p], out["n_sub"][p], out["z"][p] = ret, sub.value, n_sub.value, (z[0], z[1])
        assert regs.tobytes() == before                                       # the records are read only
        out["seconds"] = spent
        return out
