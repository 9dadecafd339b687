"""What the pair-scoring tests share beside tests/pair_gen.py: the scalar host driver of bwa-meme_amd/csrc/meme_pair_rules.h (tests/pair_rules_driver.h)
compiled with g++, and the workload with the reference's outputs as one binary file for the driver as a program of its own (scripts/pair_rules_main.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

import pair_gen as QG
from pymeme import hipapi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "tests")]


def build_driver(tmpdir):
    """tests/pair_rules_driver.h as a shared object (g++, contraction off) -> run(batch, exhaustive=False, **opt) = dict(score, sub, n_sub, n_cand, z, status), or None
    where the driver refuses the orientations; exhaustive: every k < i is put to the predicate, none skipped as beyond the reach"""
    src = os.path.join(str(tmpdir), "t_pair_rules.cpp")
    with open(src, "w") as f:
        f.write('#include "pair_rules_driver.h"\n')
    so = os.path.join(str(tmpdir), "libt_pair_rules.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC"] + INCLUDES + [src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.t_pair.restype = C.c_int
    lib.t_pair_exhaustive.restype = None

    def run(B, exhaustive=False, **opt):
        regs, reg_off, n_pri = B["regs"], np.ascontiguousarray(B["reg_off"], np.int64), np.ascontiguousarray(B["n_pri"], np.int32)
        assert regs.dtype == hipapi.ALNREG and regs.flags.c_contiguous
        n = reg_off.shape[0] - 1
        m = n // 2
        out = {k: np.full(m, -7, np.int32) for k in ("score", "sub", "n_sub", "n_cand")}
        out["z"] = np.full((m, 2), -7, np.int32)
        out["status"] = np.full(m, 9, np.uint8)
        contigs = B.get("contigs", QG.CONTIGS)
        arr = (hipapi.Contig * len(contigs))(*[hipapi.Contig(int(o), int(l), int(a)) for o, l, a in contigs])
        o = hipapi.default_pair_opt(**opt)
        lib.t_pair_exhaustive(C.c_int(int(exhaustive)))
        rc = lib.t_pair(hipapi._p(regs), hipapi._p(reg_off), hipapi._p(n_pri), C.c_int64(n), arr, C.c_int32(len(contigs)), C.c_int64(B.get("l_pac", QG.L_PAC)), hipapi.pair_pes(B["pes"]),
                        C.c_int64(int(B["id_base"])), C.byref(o), hipapi._p(out["score"]), hipapi._p(out["sub"]), hipapi._p(out["n_sub"]), hipapi._p(out["n_cand"]), hipapi._p(out["z"]),
                        hipapi._p(out["status"]))
        return out if rc == 0 else None
    return run


def dump(path):
    """the workload and the reference's outputs for scripts/pair_rules_main.cpp: int64 batches; per batch int64 nreads, nregs, id_base, then the four orientations
    (meme_pair_pes), reg_off, n_pri, the records, and score, sub, n_sub, z of the fixture"""
    with open(path, "wb") as f:
        W, G = QG.workload(), QG.golden()
        f.write(np.array([len(W)], np.int64).tobytes())
        for B, g in zip(W, G):
            f.write(np.array([B["reg_off"].shape[0] - 1, B["regs"].shape[0], B["id_base"]], np.int64).tobytes())
            f.write(bytes(hipapi.pair_pes(B["pes"])))
            for a, t in ((B["reg_off"], np.int64), (B["n_pri"], np.int32), (B["regs"], None), (g["score"], np.int32), (g["sub"], np.int32), (g["n_sub"], np.int32), (g["z"], np.int32)):
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())


def build_program(tmpdir, sanitize=True):
    """scripts/pair_rules_main.cpp as a program (with -fsanitize=address,undefined unless told otherwise) -> its path"""
    exe = os.path.join(str(tmpdir), "pair_rules_main")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror"] + flags + INCLUDES + [os.path.join(REPO, "scripts", "pair_rules_main.cpp"), "-o", exe], check=True)
    return exe
