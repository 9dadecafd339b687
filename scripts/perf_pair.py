"""Times of the pair-scoring stage (meme_pair_batch_host) and of the compiled reference's own mem_pair on the same pairs.

    python scripts/perf_pair.py [out.json]        the driver: every step below in a fresh process under `timeout -k 10`, stopping at the first that fails
    python scripts/perf_pair.py --step NAME OUT   one step, its result as a JSON file

Steps:
  fixture       the workload of tests/pair_gen.py (19 batches, 2 951 pairs, up to 520 keys per pair): kernel_ms of five calls per batch, summed; both tiers and the heavy tier alone
  production    the production-shaped batch of scripts/perf_primary.py -- 2 M reads whose records are those the extension stage leaves (tuning ext_live_only) for the 6 000 reads of
                tests/test_gpu_repeat_dense.py's workload, repeated -- marked by the primary stage and paired as the reads come (1 M pairs); kernel_ms of five calls, the middle
                one reported.  The 3 000 distinct pairs are kept for the next step.
  reference     mem_pair of the compiled reference (tests/ref_pair.py, oracle/_ref) on the fixture workload and on the 3 000 distinct pairs of the production batch (scaled to its
                1 M pairs), one thread, timed inside one native loop over the pairs (best of five), and the same divided by 16 CPUs (what kt_for over 16 threads could at best
                make of it)."""
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "bwa-meme_amd")]
KEEP = os.path.join(tempfile.gettempdir(), "perf_pair_records.npz")
STEPS = (("fixture", 120), ("production", 560), ("reference", 300))
PRODUCTION_READS = 2_000_000
L_PAC = 64_000_000
CONTIGS = [(L_PAC * i // 4, L_PAC * (i + 1) // 4 - L_PAC * i // 4, 0) for i in range(4)]
PES = [(0, 3000, 0, 500.0, 300.0), (50, 650, 0, 350.0, 50.0), (0, 2000, 0, 300.0, 150.0), (20, 1500, 0, 250.0, 70.0)]      # the fixture's first batch: all four orientations alive


def call_times(ctx, B, contigs, l_pac, calls=5):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        res = ctx.pair_batch_host(B["regs"], B["reg_off"], B["n_pri"], contigs, l_pac, B["pes"], B["id_base"])
        out.append({"kernel_ms": round(res["kernel_ms"], 4), "call_ms": round(1e3 * (time.perf_counter() - t0), 2), "n_heavy": res["n_heavy"], "pairs_with_candidates": int((res["n_cand"] > 0).sum()),
                    "candidates": int(res["n_cand"].sum())})
    return out


def middle(calls):
    return sorted(c["kernel_ms"] for c in calls)[len(calls) // 2]


def step_fixture():
    import pair_gen as QG
    from pymeme import hipapi
    W, G = QG.workload(), QG.golden()
    ctx = hipapi.Context(0)
    res = {"batches": len(W), "pairs": sum((B["reg_off"].shape[0] - 1) // 2 for B in W), "records": sum(int(B["regs"].shape[0]) for B in W)}
    for name, split in (("tiers", 8), ("heavy_alone", 0)):
        ctx.set_tuning("pair_split", split)
        total, heavy = 0.0, 0
        for B, g in zip(W, G):
            got = ctx.pair_batch_host(B["regs"], B["reg_off"], B["n_pri"], QG.CONTIGS, QG.L_PAC, B["pes"], B["id_base"])
            assert QG.same(got, g) is None
            calls = call_times(ctx, B, QG.CONTIGS, QG.L_PAC)
            total += middle(calls)
            heavy += calls[0]["n_heavy"]
        res[name] = {"kernel_ms_sum": round(total, 4), "n_heavy": heavy}
    ctx.close()
    return res


def step_production():
    import numpy as np
    import torch
    import finish_gen as FG
    from pymeme import hipapi, workload
    n = 2 * L_PAC
    g = workload.repeat_dense_genome(L_PAC)
    text = hipapi.fwd_rc_text(g)
    ctx = hipapi.Context(0)
    d_text, d_sa = hipapi.build_sa_device(ctx, text)
    d_pos5 = hipapi.pos5_from_sa_torch(ctx, d_sa, n)
    del d_sa
    torch.cuda.empty_cache()
    d_pac, d_ent = hipapi.stage_entries_torch(ctx, n, d_text, d_pos5)
    d_l2, n_l2, d_l1, n_l1 = hipapi.train_prmi_device(ctx, d_ent, n, 24)
    keep = (d_pac, d_ent) + hipapi.attach_index_torch(ctx, n, d_pac, d_ent, d_l2, n_l2, d_l1, n_l1)
    nreads, L = 6000, 150
    reads = workload.make_reads_fast(g, nreads, L, seed=79)
    off = np.arange(0, (nreads + 1) * L, L, dtype=np.int64)
    ctx.seed_batch_host(reads.reshape(-1), off)
    ctx.set_tuning("ext_live_only", 1)
    E = ctx.extend_last_batch_host(CONTIGS, hipapi.default_chain_opt(L_PAC))
    P = ctx.primary_batch_host(E["regs"], E["reg_off"].astype(np.int64), 0)                    # the records in their final order, and n_pri
    regs1, off1, n_pri1 = FG.take(P["regs"], np.arange(P["regs"].shape[0])), E["reg_off"].astype(np.int64), P["n_pri"].astype(np.int32)
    np.savez(KEEP, regs=regs1.view(np.uint8).reshape(-1, 112), reg_off=off1, n_pri=n_pri1)
    counts = np.diff(off1)
    reps = -(-PRODUCTION_READS // nreads)
    regs = FG.take(regs1, np.tile(np.arange(regs1.shape[0]), reps))
    reg_off = np.concatenate([[0], np.cumsum(np.tile(counts, reps))])[:PRODUCTION_READS + 1]
    B = {"regs": regs[:int(reg_off[-1])], "reg_off": reg_off, "n_pri": np.tile(n_pri1, reps)[:PRODUCTION_READS], "pes": PES, "id_base": 0}
    keys = np.where((B["n_pri"][0::2] > 0) & (B["n_pri"][1::2] > 0), B["n_pri"][0::2] + B["n_pri"][1::2], 0)
    calls = call_times(ctx, B, CONTIGS, L_PAC)
    res = {"pairs": PRODUCTION_READS // 2, "records": int(reg_off[-1]), "distinct_pairs": nreads // 2, "keys_per_pair": round(float(keys.mean()), 3), "most_keys": int(keys.max()),
           "pairs_without_keys": round(float((keys == 0).mean()), 4), "pairs_with_2_to_8": round(float(((keys >= 2) & (keys <= 8)).mean()), 4), "pairs_above_8": round(float((keys > 8).mean()), 4),
           "kernel_ms": middle(calls), "calls": calls}
    del keep
    ctx.close()
    return res


# the reference's function over a batch through its address, timed inside one native call (a loop in Python would time ctypes): compiled when the step runs
LOOP_SRC = r"""
#include <chrono>
#include <cstddef>
#include <cstdint>
struct V { size_t n, m; void* a; size_t pad[4]; bool use_mate_sort; };      // mem_alnreg_v as the reference is built (MATE_SORT=1)
typedef int (*pair_fn)(const void*, const void*, const uint8_t*, const void*, void*, V*, int, int*, int*, int*, int*);
extern "C" double ref_loop(void* fn, const void* opt, const void* bns, const void* pes, char* regs, const int64_t* off, const int* n_pri, int64_t npairs, int64_t id_base,
                           int* score, int* sub, int* n_sub, int* z) {
    auto t0 = std::chrono::steady_clock::now();
    for (int64_t p = 0; p < npairs; ++p) {
        score[p] = sub[p] = n_sub[p] = 0; z[2 * p] = z[2 * p + 1] = -1;
        if (n_pri[2 * p] == 0 || n_pri[2 * p + 1] == 0) continue;
        V a[2] = {};
        int np[2];
        for (int r = 0; r < 2; ++r) { a[r].n = a[r].m = (size_t)(off[2 * p + r + 1] - off[2 * p + r]); a[r].a = regs + 112 * off[2 * p + r]; np[r] = n_pri[2 * p + r]; }
        score[p] = ((pair_fn)fn)(opt, bns, nullptr, pes, nullptr, a, (int)(id_base + p), &sub[p], &n_sub[p], &z[2 * p], np);
    }
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
"""


def step_reference():
    import ctypes as C
    import numpy as np
    import finish_gen as FG
    import pair_gen as QG
    import ref_pair
    from pymeme import hipapi
    d = tempfile.mkdtemp(prefix="perf_pair_")
    open(os.path.join(d, "loop.cpp"), "w").write(LOOP_SRC)
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", os.path.join(d, "loop.cpp"), "-o", os.path.join(d, "loop.so")], check=True)
    loop = C.CDLL(os.path.join(d, "loop.so")).ref_loop
    loop.restype = C.c_double
    loop.argtypes = [C.c_void_p] * 7 + [C.c_int64, C.c_int64] + [C.c_void_p] * 4

    def run(ref, B, scale, check=None):
        reg_off, n_pri = np.ascontiguousarray(B["reg_off"], dtype=np.int64), np.ascontiguousarray(B["n_pri"], dtype=np.int32)
        npairs = (reg_off.shape[0] - 1) // 2
        pes = (ref_pair.PeStat * 4)(*[ref_pair.PeStat(lo, hi, f, avg, std) for lo, hi, f, avg, std in B["pes"]])
        best = None
        for _ in range(5):
            out = {k: np.zeros(npairs, np.int32) for k in ("score", "sub", "n_sub")}
            out["z"] = np.zeros((npairs, 2), np.int32)
            t = loop(C.cast(ref.fn, C.c_void_p), C.cast(ref.opt, C.c_void_p), C.addressof(ref.bns), C.addressof(pes), B["regs"].ctypes.data, reg_off.ctypes.data, n_pri.ctypes.data, npairs,
                     B["id_base"], out["score"].ctypes.data, out["sub"].ctypes.data, out["n_sub"].ctypes.data, out["z"].ctypes.data)
            best = t if best is None else min(best, t)
        if check is not None:
            assert QG.same(out, check) is None
        return best * scale
    ref = ref_pair.Reference(QG.CONTIGS, QG.L_PAC)
    fixture = sum(run(ref, B, 1.0, g) for B, g in zip(QG.workload(), QG.golden()))
    res = {"fixture": {"one_thread_ms": round(1e3 * fixture, 3), "sixteen_cpus_ms": round(1e3 * fixture / 16, 3)}}
    if os.path.exists(KEEP):
        K = np.load(KEEP)
        regs = FG.take(K["regs"].reshape(-1).view(hipapi.ALNREG), np.arange(K["regs"].shape[0]))
        B = {"regs": regs, "reg_off": K["reg_off"], "n_pri": K["n_pri"], "pes": PES, "id_base": 0}
        t = run(ref_pair.Reference(CONTIGS, L_PAC), B, (PRODUCTION_READS // 2) / ((K["reg_off"].shape[0] - 1) // 2))
        res["production"] = {"one_thread_ms": round(1e3 * t, 3), "sixteen_cpus_ms": round(1e3 * t / 16, 3)}
    return res


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        res = {"fixture": step_fixture, "production": step_production, "reference": step_reference}[sys.argv[2]]()
        json.dump(res, open(sys.argv[3], "w"))
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else "perf_pair.json"
    all_res = {}
    for name, limit in STEPS:
        part = "%s.%s" % (out, name)
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, part]).returncode
        if rc != 0:
            print("step %s ended with status %d: nothing further is started" % (name, rc))
            return rc
        all_res[name] = json.load(open(part))
        os.remove(part)
        print(name, json.dumps(all_res[name]))
        json.dump(all_res, open(out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
