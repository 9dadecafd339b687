"""Times of the pairing-decision stage (meme_pair_decide_batch_host) next to the pair-scoring stage (meme_pair_batch_host) on the same batch, in the same run.

    python scripts/perf_decide.py [out.json]        the driver: the step below in a fresh process under `timeout -k 10`
    python scripts/perf_decide.py --step NAME OUT   one step, its result as a JSON file

Steps:
  production    the production-shaped batch of scripts/perf_pair.py (1 M pairs, the records the extension stage leaves for 6 000 reads of tests/test_gpu_repeat_dense.py's workload,
                repeated, marked by the primary stage and paired as the reads come): kernel_ms of the pair stage (HIP events, the middle of five calls), then, on that call's
                outputs, kernel_ms of the decision (the middle of five calls) for decide_split 0, 8, 16, 32 and 64, with the pairs each tier took and the paths decided."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "bwa-meme_amd"), os.path.join(REPO, "scripts")]
STEPS = (("production", 900),)
SPLITS = (0, 8, 16, 32, 64)


def production_batch(ctx):
    """scripts/perf_pair.py: step_production's batch"""
    import numpy as np
    import torch
    import finish_gen as FG
    import perf_pair as PP
    from pymeme import hipapi, workload
    n = 2 * PP.L_PAC
    g = workload.repeat_dense_genome(PP.L_PAC)
    d_text, d_sa = hipapi.build_sa_device(ctx, hipapi.fwd_rc_text(g))
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
    E = ctx.extend_last_batch_host(PP.CONTIGS, hipapi.default_chain_opt(PP.L_PAC))
    P = ctx.primary_batch_host(E["regs"], E["reg_off"].astype(np.int64), 0)
    regs1, off1, n_pri1 = FG.take(P["regs"], np.arange(P["regs"].shape[0])), E["reg_off"].astype(np.int64), P["n_pri"].astype(np.int32)
    reps = -(-PP.PRODUCTION_READS // nreads)
    regs = FG.take(regs1, np.tile(np.arange(regs1.shape[0]), reps))
    reg_off = np.concatenate([[0], np.cumsum(np.tile(np.diff(off1), reps))])[:PP.PRODUCTION_READS + 1]
    return keep, {"regs": regs[:int(reg_off[-1])], "reg_off": reg_off, "n_pri": np.tile(n_pri1, reps)[:PP.PRODUCTION_READS], "pes": PP.PES, "id_base": 0}


def step_production():
    import numpy as np
    import perf_pair as PP
    from pymeme import hipapi
    ctx = hipapi.Context(0)
    keep, B = production_batch(ctx)         # (keep: the index arrays the ctx is attached to)
    pair_calls = PP.call_times(ctx, B, PP.CONTIGS, PP.L_PAC)
    pair = ctx.pair_batch_host(B["regs"], B["reg_off"], B["n_pri"], PP.CONTIGS, PP.L_PAC, B["pes"], B["id_base"])
    pair = {f: pair[f].copy() for f in ("score", "sub", "n_sub", "z", "status")}
    recs = np.diff(B["reg_off"]).reshape(-1, 2).sum(axis=1)
    res = {"pairs": int(recs.shape[0]), "records": int(B["reg_off"][-1]), "records_per_pair": round(float(recs.mean()), 3), "most_records": int(recs.max()),
           "pair_kernel_ms": PP.middle(pair_calls), "pair_calls": [c["kernel_ms"] for c in pair_calls], "splits": {}}
    for split in SPLITS:
        ctx.set_tuning("decide_split", split)
        calls = []
        for _ in range(5):
            got = ctx.pair_decide_batch_host(B["regs"], B["reg_off"], B["n_pri"], pair, PP.L_PAC, B["pes"])
            calls.append(round(got["kernel_ms"], 4))
        assert not got["status"].any()
        res["splits"][str(split)] = {"kernel_ms": sorted(calls)[2], "calls": calls, "n_heavy": got["n_heavy"], "pairs_above_split": int((recs > split).sum()),
                                     "paths": np.bincount(got["path"], minlength=4).tolist()}
    del keep
    ctx.close()
    return res


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        json.dump({"production": step_production}[sys.argv[2]](), open(sys.argv[3], "w"))
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else "perf_decide.json"
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
