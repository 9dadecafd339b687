"""ctypes driver of the COMPILED REFERENCE's own mem_mark_primary_se, mem_reorder_primary5 and mem_approx_mapq_se (oracle/_ref/libbwa_pic.so exports
every symbol; TEST INFRASTRUCTURE ONLY), called per read as worker_sam and mem_sam_pe call them (reference src/bwamem.cpp:1907-1911,
src/bwamem_pair.cpp:923-929, src/bwamem.cpp:2332): mark, reorder under MEM_F_PRIMARY5, then one quality per record.  No index is needed."""
import ctypes as C
import time

import numpy as np

import ref_finish

MARK_PRIMARY = "_Z19mem_mark_primary_sePK9mem_opt_tiP12mem_alnreg_tl"      # (const mem_opt_t*, int, mem_alnreg_t*, int64_t) -> int
APPROX_MAPQ = "_Z18mem_approx_mapq_sePK9mem_opt_tPK12mem_alnreg_t"         # (const mem_opt_t*, const mem_alnreg_t*) -> int
REORDER_PRIMARY5 = "_Z20mem_reorder_primary5iP12mem_alnreg_v"              # (int, mem_alnreg_v*)


class AlnregV(C.Structure):         # mem_alnreg_v, src/bwamem.h:167
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


class Reference:
    """The reference's options: mem_opt_init, then the fields given (mem_opt_t names; primary5 is not one of them: an argument of run)."""

    def __init__(self, **fields):
        L = ref_finish.lib()
        self.L = L
        self.opt = L._Z12mem_opt_initv()
        o = self.opt.contents
        assert (o.a, o.b, o.min_seed_len, o.T, o.mapQ_coef_fac) == (1, 4, 19, 30, 3) and abs(o.mask_level - 0.5) < 1e-6 and abs(o.mapQ_coef_len - 50) < 1e-6, "mem_opt_t layout"
        for k, v in fields.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        self.mark = getattr(L, MARK_PRIMARY)
        self.mark.restype = C.c_int
        self.mark.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        self.mapq = getattr(L, APPROX_MAPQ)
        self.mapq.restype = C.c_int
        self.mapq.argtypes = [C.c_void_p, C.c_void_p]
        self.reorder = getattr(L, REORDER_PRIMARY5)
        self.reorder.restype = None
        self.reorder.argtypes = [C.c_int, C.c_void_p]

    def run(self, regs, reg_off, ids, primary5=False):
        """regs (hipapi.ALNREG = mem_alnreg_t, 112 bytes) per read, ids[r] = the read's id -> dict(regs in final order, n_pri, mapq (int32: what the function returns),
        seconds: time spent inside the reference's functions)"""
        assert regs.dtype.itemsize == 112 and regs.flags["C_CONTIGUOUS"]
        out = regs.copy()
        n = reg_off.shape[0] - 1
        n_pri, mapq = np.zeros(n, np.int32), np.zeros(out.shape[0], np.int32)
        base = out.ctypes.data
        opt, T = C.cast(self.opt, C.c_void_p), int(self.opt.contents.T)
        spent = 0.0
        for r in range(n):
            b, e = int(reg_off[r]), int(reg_off[r + 1])
            t0 = time.perf_counter()
            n_pri[r] = self.mark(opt, e - b, base + 112 * b, int(ids[r]))
            if primary5 and e > b:
                v = AlnregV(e - b, e - b, base + 112 * b)
                self.reorder(T, C.addressof(v))
            for k in range(b, e):
                mapq[k] = self.mapq(opt, base + 112 * k)
            spent += time.perf_counter() - t0
        return {"regs": out, "n_pri": n_pri, "mapq": mapq, "seconds": spent}
