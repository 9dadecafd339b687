"""What the primary-marking tests share beside tests/primary_gen.py: the scalar host driver of bwa-meme_amd/csrc/meme_primary_rules.h (tests/primary_rules_driver.h)
compiled with g++."""
import ctypes as C
import os
import subprocess

import numpy as np

from pymeme import hipapi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmpdir):
    """tests/primary_rules_driver.h as a shared object (g++, contraction off) -> run(regs, reg_off, id_base, **opt) = dict(regs, n_pri, mapq, status, orders), with
    run.mapq(reg, **opt) = (quality, beyond) of one record"""
    src = os.path.join(str(tmpdir), "t_primary_rules.cpp")
    with open(src, "w") as f:
        f.write('#include "primary_rules_driver.h"\n')
    so = os.path.join(str(tmpdir), "libt_primary_rules.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"),
                    "-I" + os.path.join(REPO, "tests"), src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.t_primary.restype = None
    lib.t_primary_orders.restype = C.c_int64
    lib.t_primary_mapq.restype = C.c_int

    def run(regs, reg_off, id_base, **opt):
        reg_off = np.ascontiguousarray(reg_off, np.int64)
        assert regs.dtype == hipapi.ALNREG and regs.flags.c_contiguous
        n = reg_off.shape[0] - 1
        out = np.zeros(regs.shape[0], hipapi.ALNREG)
        n_pri, mapq, status = np.full(n, -7, np.int32), np.full(regs.shape[0], 99, np.uint8), np.full(n, 9, np.uint8)
        o = hipapi.default_primary_opt(**opt)
        lib.t_primary(hipapi._p(regs), hipapi._p(reg_off), C.c_int64(n), C.c_int64(int(id_base)), C.byref(o), hipapi._p(out), hipapi._p(n_pri), hipapi._p(mapq), hipapi._p(status))
        return {"regs": out, "n_pri": n_pri, "mapq": mapq, "status": status, "orders": int(lib.t_primary_orders())}

    def mapq(reg, **opt):
        assert reg.dtype == hipapi.ALNREG and reg.shape == (1,)
        beyond = C.c_int(-1)
        o = hipapi.default_primary_opt(**opt)
        q = lib.t_primary_mapq(hipapi._p(reg), C.byref(o), C.byref(beyond))
        return int(q), bool(beyond.value)
    run.mapq = mapq
    return run
