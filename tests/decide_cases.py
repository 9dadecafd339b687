"""What the pairing-decision tests share beside tests/decide_gen.py: the scalar host driver of bwa-meme_amd/csrc/meme_decide_rules.h (tests/decide_rules_driver.h)
compiled with g++, the stage's inputs of a batch as the models leave them, and the workload with the model's results as one binary file for the driver as a program of
its own (scripts/decide_rules_main.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

import decide_gen as DG
from pymeme import hipapi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "tests")]
PAIR_IN = ("score", "sub", "n_sub", "z", "status")


def stage_inputs():
    """every batch of the workload and of direct() as the decide stage takes it: dict(name, regs (post-primary), reg_off, n_pri, pair, pes, opt) and the model's result"""
    out = []
    for B, m in zip(DG.workload(), DG.modelled()[0]):
        out.append(({"name": B["name"], "regs": m["primary"]["regs"], "reg_off": B["reg_off"], "n_pri": m["primary"]["n_pri"], "pair": {f: m["pair"][f] for f in PAIR_IN}, "pes": B["pes"],
                     "opt": B["opt"]}, m["decide"]))
    return out + list(zip(DG.direct(), DG.direct_modelled()))


def decide_opt(opt):
    return hipapi.default_decide_opt(**DG.stage_opts(DG.default_opt(**opt))[2])


def same(got, want):
    """OUT and every field of the records; None or the first difference"""
    d = DG.same(got, want)
    if d is None:
        for f in hipapi.ALNREG.names:                # (field by field: numpy does not carry a record type's padding through a copy)
            bad = np.nonzero(got["regs"][f] != want["regs"][f])[0]
            if bad.size:
                return "%s of record %d: %r, expected %r" % (f, bad[0], got["regs"][f][bad[0]], want["regs"][f][bad[0]])
    return d


def build_driver(tmpdir):
    """tests/decide_rules_driver.h as a shared object (g++, contraction off) -> run(stage input) = dict(OUT..., regs), or None where the driver refuses"""
    src = os.path.join(str(tmpdir), "t_decide_rules.cpp")
    with open(src, "w") as f:
        f.write('#include "decide_rules_driver.h"\n')
    so = os.path.join(str(tmpdir), "libt_decide_rules.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC"] + INCLUDES + [src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.t_decide.restype = C.c_int

    def run(S):
        regs, reg_off, n_pri = S["regs"].copy(), np.ascontiguousarray(S["reg_off"], np.int64), np.ascontiguousarray(S["n_pri"], np.int32)
        n = reg_off.shape[0] - 1
        m = n // 2
        cols = [np.ascontiguousarray(S["pair"][f], np.int32) for f in ("score", "sub", "n_sub", "z")] + [np.ascontiguousarray(S["pair"]["status"], np.uint8)]
        out = {"path": np.full(m, -7, np.int32), "sel": np.full((m, 2), -7, np.int32), "q_se": np.full((m, 2), -7, np.int32), "q_pe": np.full(m, -7, np.int32), "flag": np.full(m, -7, np.int32),
               "alt": np.full((m, 2), -7, np.int32), "status": np.full(m, 9, np.uint8)}
        o = decide_opt(S["opt"])
        rc = lib.t_decide(hipapi._p(regs), hipapi._p(reg_off), hipapi._p(n_pri), C.c_int64(n), *[hipapi._p(c) for c in cols], C.c_int64(DG.L_PAC), hipapi.pair_pes(S["pes"]), C.byref(o),
                          *[hipapi._p(out[f]) for f in ("path", "sel", "q_se", "q_pe", "flag", "alt", "status")])
        out["regs"] = regs
        return out if rc == 0 else None
    return run


def dump(path):
    """the stage inputs and the model's results for scripts/decide_rules_main.cpp: int64 batches; per batch int64 nreads, nregs; meme_decide_opt; the four orientations
    (meme_pair_pes); reg_off, n_pri, score, sub, n_sub, z, the pair status, the records; then path, sel, q_se, q_pe, flag, alt, status and the records as the model leaves them"""
    with open(path, "wb") as f:
        S = stage_inputs()
        clean = lambda r: DG.PG.FG.take(r, np.arange(r.shape[0]))       # (zero padding: the program compares records byte by byte)
        f.write(np.array([len(S)], np.int64).tobytes())
        for s, m in S:
            f.write(np.array([s["reg_off"].shape[0] - 1, s["regs"].shape[0]], np.int64).tobytes())
            f.write(bytes(decide_opt(s["opt"])))
            f.write(bytes(hipapi.pair_pes(s["pes"])))
            for a, t in ((s["reg_off"], np.int64), (s["n_pri"], np.int32), (s["pair"]["score"], np.int32), (s["pair"]["sub"], np.int32), (s["pair"]["n_sub"], np.int32), (s["pair"]["z"], np.int32),
                         (s["pair"]["status"], np.uint8), (clean(s["regs"]), None), (m["path"], np.int32), (m["sel"], np.int32), (m["q_se"], np.int32), (m["q_pe"], np.int32), (m["flag"], np.int32),
                         (m["alt"], np.int32), (m["status"], np.uint8), (clean(m["regs"]), None)):
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())


def build_program(tmpdir, sanitize=True):
    """scripts/decide_rules_main.cpp as a program (with -fsanitize=address,undefined unless told otherwise) -> its path"""
    exe = os.path.join(str(tmpdir), "decide_rules_main")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror"] + flags + INCLUDES + [os.path.join(REPO, "scripts", "decide_rules_main.cpp"), "-o", exe], check=True)
    return exe
