"""ctypes driver of the COMPILED REFERENCE's own mem_sort_dedup_patch_mate_sort (oracle/_ref/libbwa_pic.so exports every symbol; TEST
INFRASTRUCTURE ONLY): the function as mem_kernel2_core calls it (reference src/bwamem.cpp:1681-1719) -- the compaction to the live records
in front of it, the is_alt loop behind it -- on the bntseq_t that bns_restore reads from an index prefix and the bytes of its .pac file."""
import ctypes as C
import os

import numpy as np

from ref_py import REF_DIR

SORT_DEDUP_PATCH = "_Z30mem_sort_dedup_patch_mate_sortPK9mem_opt_tPK8bntseq_tPKhPhiP12mem_alnreg_tPb"      # (const mem_opt_t*, const bntseq_t*, const uint8_t*, uint8_t*, int, mem_alnreg_t*, bool*)


def take(regs, idx):
    """regs[idx] in the 112-byte layout of mem_alnreg_t (numpy's own indexing packs a padded record type)"""
    from pymeme import hipapi
    out = np.zeros(len(idx), hipapi.ALNREG)
    for f in hipapi.ALNREG.names:
        out[f] = regs[f][idx]
    assert out.dtype.itemsize == 112 and out.flags["C_CONTIGUOUS"]
    return out


class MemOpt(C.Structure):          # mem_opt_t, reference src/bwamem.h:82-114
    _fields_ = [(n, C.c_int) for n in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "pen_unpaired", "pen_clip5", "pen_clip3", "w", "zdrop")] + \
               [("max_mem_intv", C.c_uint64)] + [(n, C.c_int) for n in ("T", "flag", "min_seed_len", "min_chain_weight", "max_chain_extend")] + \
               [("split_factor", C.c_float)] + [(n, C.c_int) for n in ("split_width", "max_occ", "max_chain_gap", "n_threads")] + [("chunk_size", C.c_int64)] + \
               [(n, C.c_float) for n in ("mask_level", "drop_ratio", "XA_drop_ratio", "mask_level_redun", "mapQ_coef_len")] + \
               [(n, C.c_int) for n in ("mapQ_coef_fac", "max_ins", "max_matesw", "max_XA_hits", "max_XA_hits_alt")] + [("mat", C.c_int8 * 25)]


class BntAnn(C.Structure):          # bntann1_t, src/bntseq.h:41-48
    _fields_ = [("offset", C.c_int64), ("len", C.c_int32), ("n_ambs", C.c_int32), ("gi", C.c_uint32), ("is_alt", C.c_int32), ("name", C.c_char_p), ("anno", C.c_char_p)]


class BntSeq(C.Structure):          # bntseq_t, src/bntseq.h:56-64
    _fields_ = [("l_pac", C.c_int64), ("n_seqs", C.c_int32), ("seed", C.c_uint32), ("anns", C.POINTER(BntAnn)), ("n_holes", C.c_int32), ("ambs", C.c_void_p), ("fp_pac", C.c_void_p)]


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        # (the library leaves two profiling globals to its executable; oracle/ref_stage_shim.cpp's library defines them and brings libbwa_pic.so with it)
        C.CDLL(os.path.join(REF_DIR, "libstage_ref.so"), mode=C.RTLD_GLOBAL)
        L = C.CDLL(os.path.join(REF_DIR, "libbwa_pic.so"))
        L._Z12mem_opt_initv.restype = C.POINTER(MemOpt)
        L.bns_restore.restype = C.POINTER(BntSeq)
        L.bns_restore.argtypes = [C.c_char_p]
        L.bwa_fill_scmat.argtypes = [C.c_int, C.c_int, C.c_void_p]
        getattr(L, SORT_DEDUP_PATCH).restype = C.c_int
        getattr(L, SORT_DEDUP_PATCH).argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


class Reference:
    """The reference's options (mem_opt_init, then the fields given), its view of the index at `prefix` and the packed text; alt: contigs flagged ALT."""

    def __init__(self, prefix, alt=(), **fields):
        L = lib()
        self.opt = L._Z12mem_opt_initv()
        o = self.opt.contents
        # the layout above against the reference's own defaults on both sides of every float / 64-bit member
        assert (o.a, o.b, o.w, o.zdrop, o.max_mem_intv, o.min_seed_len, o.split_width, o.max_occ, o.max_chain_gap, o.chunk_size, o.max_matesw, o.max_XA_hits_alt) == \
               (1, 4, 100, 100, 20, 19, 10, 500, 10000, 10000000, 50, 200), "mem_opt_t layout"
        assert abs(o.mask_level_redun - 0.95) < 1e-6 and abs(o.split_factor - 1.5) < 1e-6 and o.mat[0] == 1 and o.mat[1] == -4 and o.mat[24] == -1, "mem_opt_t layout"
        for k, v in fields.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        L.bwa_fill_scmat(o.a, o.b, C.addressof(o.mat))
        self.bns = L.bns_restore(prefix.encode())
        assert self.bns, prefix
        b = self.bns.contents
        self.l_pac = int(b.l_pac)
        self.contigs = []
        for k in range(b.n_seqs):
            b.anns[k].is_alt = 1 if k in alt else 0
            self.contigs.append((int(b.anns[k].offset), int(b.anns[k].len), int(b.anns[k].is_alt)))
        self.pac = np.fromfile(prefix + ".pac", np.uint8)
        assert self.pac.shape[0] >= (self.l_pac + 3) // 4

    def finish(self, regs, reg_off, reads, read_off):
        """regs (hipapi.ALNREG = mem_alnreg_t) per read -> (records left, their offsets, useMateSort per read), as mem_kernel2_core's tail leaves them."""
        fn = getattr(lib(), SORT_DEDUP_PATCH)
        n = reg_off.shape[0] - 1
        out, off, ums = [], np.zeros(n + 1, np.int64), np.ones(n, np.uint8)
        alt = np.array([c[2] for c in self.contigs], np.int64)
        for r in range(n):
            a = regs[reg_off[r]:reg_off[r + 1]]
            a = take(a, np.nonzero(a["qe"] > a["qb"])[0])                    # :1689-1694
            q = np.ascontiguousarray(reads[read_off[r]:read_off[r + 1]], dtype=np.uint8).copy()
            flag = C.c_bool(True)                                            # :1687
            m = fn(self.opt, self.bns, C.c_void_p(self.pac.ctypes.data), C.c_void_p(q.ctypes.data), C.c_int(a.shape[0]), C.c_void_p(a.ctypes.data), C.byref(flag)) if a.shape[0] else 0
            assert np.array_equal(q, reads[read_off[r]:read_off[r + 1]])     # (bwa_gen_cigar2 reverses the query in place and back)
            a = a[:m]
            hit = (a["rid"] >= 0) & (alt[np.maximum(a["rid"], 0)] != 0)      # :1711-1719: is_alt = 1 (n_comp:30, is_alt:2)
            a["n_comp_is_alt"][hit] = (a["n_comp_is_alt"][hit] & 0x3fffffff) | (1 << 30)
            out.append(a)
            off[r + 1] = off[r] + m
            ums[r] = 1 if flag.value else 0
        return take(np.concatenate(out), np.arange(int(off[n]))) if n else take(regs, np.zeros(0, np.int64)), off, ums
