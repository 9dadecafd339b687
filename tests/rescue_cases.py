"""What the tests of mate rescue's record updates share: the batches of tests/rescue_gen.py with the model's results, the stage's options and arguments, the g++
driver of the rules (tests/rescue_rules_driver.h) as a shared object, the dump scripts/rescue_rules_main.cpp reads, and that program's build."""
import ctypes as C
import os
import subprocess

import numpy as np

import rescue_gen as RG
from finish_gen import take
from pymeme import hipapi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "tests")]


def stage_inputs():
    """[(batch, model's result)]: the workload, then the batches for the stage alone"""
    return list(zip(RG.workload(), RG.modelled()[0])) + list(zip(RG.direct(), RG.direct_modelled()))


def rescue_opt(opt):
    o = RG.default_opt(**opt)
    return hipapi.default_rescue_opt(**{k: o[k] for k in ("pen_unpaired", "max_matesw", "min_seed_len", "batch_reads", "max_chain_gap", "mask_level_redun")})


def jobs_of(B):
    return {"gar": B["gar"], "gar_off": B["gar_off"], "job_off": B["job_off"], "res": B["res"]}


def counters_of(m):
    return m["stage"]


def build_driver(tmpdir):
    """tests/rescue_rules_driver.h as a shared object (g++, contraction off) -> run(batch) = dict(regs, reg_off, status, counters), or None where the driver refuses"""
    src = os.path.join(str(tmpdir), "t_rescue_rules.cpp")
    with open(src, "w") as f:
        f.write('#include "rescue_rules_driver.h"\n')
    so = os.path.join(str(tmpdir), "libt_rescue_rules.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC"] + INCLUDES + [src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.t_rescue.restype = C.c_int

    def run(B, **over):
        B = dict(B, **over)
        regs, reg_off = take(B["regs"], np.arange(B["regs"].shape[0])), np.ascontiguousarray(B["reg_off"], np.int64)
        n = reg_off.shape[0] - 1
        ums, rlen = np.ascontiguousarray(B["ums"], np.uint8), np.ascontiguousarray(B["read_len"], np.int32)
        gar, gar_off, job_off = np.ascontiguousarray(B["gar"], np.int32), np.ascontiguousarray(B["gar_off"], np.int64), np.ascontiguousarray(B["job_off"], np.int64)
        res = np.ascontiguousarray(B["res"], hipapi.KSWR)
        out = np.zeros(regs.shape[0] + res.shape[0] + 1, hipapi.ALNREG)
        off, status, ctr = np.full(n + 1, -7, np.int64), np.full(n + 1, 9, np.uint8), np.zeros(4, np.int64)
        pes4 = hipapi.mate_pes(B["pes"])
        arr = hipapi._contig_array(RG.CONTIGS)
        o = rescue_opt(B["opt"])
        rc = lib.t_rescue(hipapi._p(regs), hipapi._p(reg_off), hipapi._p(ums), hipapi._p(rlen), C.c_int64(n), hipapi._p(gar), hipapi._p(gar_off), hipapi._p(job_off), C.c_int64(gar_off.shape[0] - 1),
                          hipapi._p(res), C.c_int64(res.shape[0]), hipapi._p(pes4), arr, C.c_int32(len(RG.CONTIGS)), C.c_int64(RG.L_PAC), C.byref(o), hipapi._p(out), hipapi._p(off), hipapi._p(status),
                          hipapi._p(ctr))
        if rc != 0:
            return None
        return {"regs": take(out, np.arange(int(off[n]))), "reg_off": off, "status": status[:n], "counters": dict(zip(("n_wave", "n_tested", "n_pushed", "n_removed"), [int(x) for x in ctr]))}
    return run


def dump(path):
    """the stage inputs and the model's results for scripts/rescue_rules_main.cpp (its header comment names the layout)"""
    with open(path, "wb") as f:
        S = stage_inputs()
        f.write(np.array([len(S)], np.int64).tobytes())
        contigs = np.zeros(len(RG.CONTIGS), np.dtype([("offset", "<i8"), ("len", "<i4"), ("is_alt", "<i4")]))
        for k, c in enumerate(RG.CONTIGS):
            contigs[k] = c
        for B, m in S:
            f.write(np.array([B["reg_off"].shape[0] - 1, B["regs"].shape[0], B["gar"].shape[0], B["gar_off"].shape[0] - 1, B["res"].shape[0], m["regs"].shape[0]], np.int64).tobytes())
            f.write(bytes(rescue_opt(B["opt"])))
            f.write(hipapi.mate_pes(B["pes"]).tobytes())
            f.write(np.array([len(RG.CONTIGS)], np.int64).tobytes())
            f.write(contigs.tobytes())
            c = counters_of(m)
            for a, t in ((B["reg_off"], np.int64), (B["ums"], np.uint8), (B["read_len"], np.int32), (B["gar"], np.int32), (B["gar_off"], np.int64), (B["job_off"], np.int64), (B["res"], hipapi.KSWR),
                         (take(B["regs"], np.arange(B["regs"].shape[0])), None), (m["reg_off"], np.int64), (m["status"], np.uint8),
                         (np.array([c[k] for k in ("n_wave", "n_tested", "n_pushed", "n_removed")]), np.int64), (take(m["regs"], np.arange(m["regs"].shape[0])), None)):
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())


def build_program(tmpdir, sanitize=True):
    """scripts/rescue_rules_main.cpp as a program (with -fsanitize=address,undefined unless told otherwise) -> its path"""
    exe = os.path.join(str(tmpdir), "rescue_rules_main")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror"] + flags + INCLUDES + [os.path.join(REPO, "scripts", "rescue_rules_main.cpp"), "-o", exe], check=True)
    return exe
