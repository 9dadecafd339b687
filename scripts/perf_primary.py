"""Times of the primary-marking / mapping-quality stage (meme_primary_batch_host) and of the compiled reference's own functions on the same records.

    python scripts/perf_primary.py [out.json]        the driver: every step below in a fresh process under `timeout -k 10`, stopping at the first that fails
    python scripts/perf_primary.py --step NAME OUT   one step, its result as a JSON file

Steps:
  fixture       the workload of tests/primary_gen.py (3 968 reads, 12 618 records, up to 273 per read): kernel_ms of five calls, both tiers and the heavy tier alone
  production    a production-shaped batch: 2 M reads whose records are those the extension stage leaves (tuning ext_live_only) for the 6 000 reads of
                tests/test_gpu_repeat_dense.py's workload, repeated -- its record counts per read; kernel_ms of five calls.  The records are kept for the next step.
  reference     mem_mark_primary_se + mem_approx_mapq_se of the compiled reference (tests/ref_primary.py, oracle/_ref) on the fixture workload and on the 6 000 distinct
                reads of the production batch (scaled to its 2 M reads), one thread, timed inside one native loop over the reads (best of five),
                and the same divided by 16 CPUs (what kt_for over 16 threads could at best make of it)."""
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "bwa-meme_amd")]
KEEP = os.path.join(tempfile.gettempdir(), "perf_primary_records.npz")
STEPS = (("fixture", 120), ("production", 560), ("reference", 300))
PRODUCTION_READS = 2_000_000


def call_times(ctx, regs, reg_off, id_base, calls=5):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        res = ctx.primary_batch_host(regs, reg_off, id_base)
        out.append({"kernel_ms": round(res["kernel_ms"], 4), "call_ms": round(1e3 * (time.perf_counter() - t0), 2), "n_heavy": res["n_heavy"]})
    return out


def step_fixture():
    import numpy as np
    import primary_gen as PG
    from pymeme import hipapi
    W, G = PG.workload(), PG.golden()
    ctx = hipapi.Context(0)
    got = ctx.primary_batch_host(W["regs"], W["reg_off"], PG.ID_BASE)
    assert PG.same(got, G, W["reg_off"], skip_mapq_of=[W["status_read"]]) is None
    res = {"reads": int(W["reg_off"].shape[0] - 1), "records": int(W["regs"].shape[0]), "most_per_read": int(np.diff(W["reg_off"]).max()), "tiers": call_times(ctx, W["regs"], W["reg_off"], PG.ID_BASE)}
    ctx.set_tuning("primary_split", 0)
    res["heavy_alone"] = call_times(ctx, W["regs"], W["reg_off"], PG.ID_BASE)
    ctx.close()
    return res


def step_production():
    import numpy as np
    import torch
    import finish_gen as FG
    from pymeme import hipapi, workload
    l_pac = 64_000_000
    n = 2 * l_pac
    g = workload.repeat_dense_genome(l_pac)
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
    contigs = [(l_pac * i // 4, l_pac * (i + 1) // 4 - l_pac * i // 4, 0) for i in range(4)]
    ctx.set_tuning("ext_live_only", 1)
    E = ctx.extend_last_batch_host(contigs, hipapi.default_chain_opt(l_pac))
    regs1, off1 = E["regs"], E["reg_off"].astype(np.int64)
    assert (regs1["qe"] > regs1["qb"]).all() and (regs1["re"] > regs1["rb"]).all()
    np.savez(KEEP, regs=regs1.view(np.uint8).reshape(-1, 112), reg_off=off1)
    counts = np.diff(off1)
    reps = -(-PRODUCTION_READS // nreads)
    regs = FG.take(regs1, np.tile(np.arange(regs1.shape[0]), reps))
    reg_off = np.concatenate([[0], np.cumsum(np.tile(counts, reps))])[:PRODUCTION_READS + 1]
    regs = regs[:int(reg_off[-1])]
    res = {"reads": PRODUCTION_READS, "records": int(reg_off[-1]), "distinct_reads": nreads, "records_per_read": round(float(counts.mean()), 3), "most_per_read": int(counts.max()),
           "reads_with_1_to_3": round(float(((counts >= 1) & (counts <= 3)).mean()), 4), "reads_above_8": round(float((counts > 8).mean()), 4),
           "calls": call_times(ctx, regs, reg_off, 0)}
    del keep
    ctx.close()
    return res


# the reference's two functions over a batch through their addresses, timed inside one native call (a loop in Python would time ctypes): compiled when the step runs
LOOP_SRC = r"""
#include <chrono>
#include <cstdint>
typedef int (*mark_fn)(const void*, int, void*, int64_t);
typedef int (*mapq_fn)(const void*, const void*);
extern "C" double ref_loop(void* mark, void* mapq, const void* opt, char* regs, const int64_t* off, int64_t n, int64_t id_base, int* n_pri, int* q) {
    auto t0 = std::chrono::steady_clock::now();
    for (int64_t r = 0; r < n; ++r) {
        n_pri[r] = ((mark_fn)mark)(opt, (int)(off[r + 1] - off[r]), regs + 112 * off[r], id_base + r);
        for (int64_t k = off[r]; k < off[r + 1]; ++k) q[k] = ((mapq_fn)mapq)(opt, regs + 112 * k);
    }
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
"""


def step_reference():
    import ctypes as C
    import numpy as np
    import finish_gen as FG
    import primary_gen as PG
    import ref_primary
    from pymeme import hipapi
    ref = ref_primary.Reference()
    d = tempfile.mkdtemp(prefix="perf_primary_")
    open(os.path.join(d, "loop.cpp"), "w").write(LOOP_SRC)
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", os.path.join(d, "loop.cpp"), "-o", os.path.join(d, "loop.so")], check=True)
    loop = C.CDLL(os.path.join(d, "loop.so")).ref_loop
    loop.restype = C.c_double
    loop.argtypes = [C.c_void_p] * 5 + [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]

    def run(regs, reg_off, id_base, scale, check=None):
        reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
        best = None
        for _ in range(5):
            a = regs.copy()
            n_pri, q = np.zeros(reg_off.shape[0] - 1, np.int32), np.zeros(max(a.shape[0], 1), np.int32)
            t = loop(C.cast(ref.mark, C.c_void_p), C.cast(ref.mapq, C.c_void_p), C.cast(ref.opt, C.c_void_p), a.ctypes.data, reg_off.ctypes.data, reg_off.shape[0] - 1, id_base,
                     n_pri.ctypes.data, q.ctypes.data)
            best = t if best is None else min(best, t)
        if check is not None:
            assert PG.same({"regs": a, "n_pri": n_pri, "mapq": q[:a.shape[0]].astype(np.uint8)}, check, reg_off) is None
        return {"one_thread_ms": round(1e3 * best * scale, 3), "sixteen_cpus_ms": round(1e3 * best * scale / 16, 3)}
    W = PG.workload()
    res = {"fixture": run(W["regs"], W["reg_off"], PG.ID_BASE, 1.0, PG.golden())}
    if os.path.exists(KEEP):
        K = np.load(KEEP)
        regs = FG.take(K["regs"].reshape(-1).view(hipapi.ALNREG), np.arange(K["regs"].shape[0]))
        n = K["reg_off"].shape[0] - 1
        res["production"] = run(regs, K["reg_off"], 0, PRODUCTION_READS / n)
    return res


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        res = {"fixture": step_fixture, "production": step_production, "reference": step_reference}[sys.argv[2]]()
        json.dump(res, open(sys.argv[3], "w"))
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else "perf_primary.json"
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
