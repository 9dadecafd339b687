"""What the record-finishing tests share beside tests/finish_gen.py: the three zero-slack merges the fixture lacks, batches cut out of the workload, and the
scalar host driver of bwa-meme_amd/csrc/meme_finish_rules.h (tests/finish_rules_driver.h) compiled with g++."""
import ctypes as C
import os
import subprocess

import numpy as np

import finish_gen as FG
from pymeme import hipapi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alt_of(W):
    return [c[2] for c in W["contigs"]]


def subset(W, idx):
    """the reads idx of the workload as a batch of their own: dict(reads, read_off, regs, reg_off)"""
    idx = np.asarray(idx, np.int64)
    reads = [W["reads"][W["read_off"][r]:W["read_off"][r + 1]] for r in idx]
    rows = [np.arange(W["reg_off"][r], W["reg_off"][r + 1]) for r in idx]
    return {"reads": np.concatenate(reads) if reads else np.zeros(0, np.uint8), "read_off": np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.int64),
            "regs": FG.take(W["regs"], np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)),
            "reg_off": np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)}


def batch_of(reads, recs):
    """reads: list of code arrays; recs: per read a list of dicts of record fields -> a batch like subset()'s"""
    rows = [x for r in recs for x in r]
    regs = np.zeros(len(rows), hipapi.ALNREG)
    regs["secondary"], regs["seedlen0"], regs["frac_rep"] = -1, 19, 0.25
    regs["c"] = np.arange(len(rows))
    for k, x in enumerate(rows):
        for f, v in x.items():
            regs[f][k] = v
    return {"reads": np.concatenate(reads).astype(np.uint8), "read_off": np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.int64), "regs": regs,
            "reg_off": np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)}


def zero_slack_batch(W, p=5000):
    """Two abutting 100-base pieces of one read, no slack between them on the read or on the reference: with w = 0 on both the band is 0 and the lengths are equal
    (bwa_gen_cigar2's gap-free shortcut: merged to score 200, w 0), the same on the reverse strand, and with w = 1 on both (through the DP: merged with w 2).
    -> (batch of three reads, [(score, w)] expected of the one record each keeps)"""
    g, L = W["genome"], W["l_pac"]
    fwd = g[p:p + 200]
    rc = np.where(fwd > 3, fwd, 3 - fwd)[::-1].astype(np.uint8)

    def pair(rev, w):
        out = []
        for rb, re, qb, qe in ((p, p + 100, 0, 100), (p + 100, p + 200, 100, 200)):
            if rev:
                rb, re, qb, qe = 2 * L - re, 2 * L - rb, 200 - qe, 200 - qb
            out.append(dict(rb=rb, re=re, qb=qb, qe=qe, rid=0, score=100, truesc=100, seedcov=50, w=w))
        return out
    return batch_of([fwd, rc, fwd], [pair(False, 0), pair(True, 0), pair(False, 1)]), [(200, 0), (200, 0), (200, 2)]


def model(W, B, **opt):
    """FG.model of a batch on the workload's genome -> (regs, reg_off, use_mate_sort, counters)"""
    return FG.model(B["regs"], B["reg_off"], B["reads"], B["read_off"], W["text"], W["l_pac"], alt_of(W), FG.default_opt(**opt) if opt else None)


def alt_flipped(W, B):
    """W with is_alt flipped on the contig of the first record the model keeps of the batch B: a contig table the records of B notice"""
    rid = int(model(W, B)[0]["rid"][0])
    return dict(W, contigs=[(o, l, a ^ 1 if k == rid else a) for k, (o, l, a) in enumerate(W["contigs"])])


def finish_opt(**kw):
    return hipapi.default_finish_opt(**{k: (float(np.float32(v)) if k == "mask_level_redun" else v) for k, v in kw.items()})


def build_driver(tmpdir):
    """tests/finish_rules_driver.h as a shared object (g++, contraction off) -> run(W, B, **opt) = dict(regs, reg_off, use_mate_sort, status, n_patch_jobs, n_patched), with
    run.score(text, l_pac, read, qb, qe, rb, re, w_, **opt) = (score, ok)"""
    src = os.path.join(str(tmpdir), "t_finish_rules.cpp")
    with open(src, "w") as f:
        f.write('#include "finish_rules_driver.h"\n')
    so = os.path.join(str(tmpdir), "libt_finish_rules.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"),
                    "-I" + os.path.join(REPO, "tests"), src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.t_finish.restype = C.c_int64

    def run(W, B, **opt):
        regs, reg_off = B["regs"], np.ascontiguousarray(B["reg_off"], np.int64)
        assert regs.dtype == hipapi.ALNREG and regs.flags.c_contiguous
        n = reg_off.shape[0] - 1
        reads, read_off, text = np.ascontiguousarray(B["reads"], np.uint8), np.ascontiguousarray(B["read_off"], np.int64), np.ascontiguousarray(W["text"], np.uint8)
        alt = np.array(alt_of(W), np.uint8)
        out = np.zeros(regs.shape[0], hipapi.ALNREG)
        off, ums, status, ctr = np.zeros(n + 1, np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(2, np.int64)
        o = finish_opt(**opt)
        left = lib.t_finish(hipapi._p(regs), hipapi._p(reg_off), C.c_int64(n), hipapi._p(reads), hipapi._p(read_off), hipapi._p(text), C.c_int64(int(W["l_pac"])), hipapi._p(alt),
                            C.c_int(alt.shape[0]), C.byref(o), hipapi._p(out), hipapi._p(off), hipapi._p(ums), hipapi._p(status), hipapi._p(ctr))
        return {"regs": FG.take(out, np.arange(left)), "reg_off": off, "use_mate_sort": ums, "status": status, "n_patch_jobs": int(ctr[0]), "n_patched": int(ctr[1])}

    def score(text, l_pac, read, qb, qe, rb, re, w_, **opt):
        text, read = np.ascontiguousarray(text, np.uint8), np.ascontiguousarray(read, np.uint8)
        ok = C.c_int(0)
        o = finish_opt(**opt)
        sc = lib.t_patch_score(hipapi._p(text), C.c_int64(int(l_pac)), hipapi._p(read), C.c_int(read.shape[0]), C.c_int(int(qb)), C.c_int(int(qe)), C.c_int64(int(rb)), C.c_int64(int(re)),
                               C.c_int(int(w_)), C.byref(o), C.byref(ok))
        return sc, bool(ok.value)
    run.score = score
    return run


def same(got, want):
    """FG.same_records of a result dict against the model's / the golden's (regs, reg_off, use_mate_sort[, counters])"""
    return FG.same_records(got["regs"], got["reg_off"], got["use_mate_sort"], want[0], want[1], want[2])
