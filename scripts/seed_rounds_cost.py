#!/usr/bin/env python3
"""What the third seeding round costs inside the search stage, and what the second launch does about it: one process, the benchmark's
index (device build) and reads (bench.sample_reads), every configuration timed in turn, several times round.

    python scripts/seed_rounds_cost.py [--genome bench|repeat_dense] [--mbp 3100] [--reads 10000000] [--steps 5] [--turns 3] [--configs r2,r3s0,r3s1]

A configuration is r<rounds>[s<seed_r3_split>]: r2 = default_seed_opt(rounds=2); r3s0 = three rounds in one k_seed launch; r3s1 = the
third round in a launch of its own, key-only compares first (the default; a library built with -DSEED_R3_CAP=0, chosen with MEME_HIP_LIB,
compares in full there).  A library without the tuning key (the parent's) runs the configurations without an s part only.
--genome repeat_dense: the genome and reads of bench.py's repeat-dense leg (--mbp 128 --reads 1000000 are that leg's sizes).  One JSON line per configuration and
turn, then one summary line per configuration (min / mean / max of the turns' means)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bwa-meme_amd"))
import numpy as np
import torch

import bench
from pymeme import hipapi, synth, workload


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", choices=("bench", "repeat_dense"), default="bench")
    ap.add_argument("--mbp", type=float, default=3100)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--configs", default="r2,r3s0,r3s1")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    l_pac = int(a.mbp * 1e6) & ~1
    n = 2 * l_pac
    t0 = time.time()
    ctx = hipapi.Context(0)
    fwd = synth.make_genome(l_pac, seed=11) if a.genome == "bench" else workload.repeat_dense_genome(l_pac)
    text = hipapi.fwd_rc_text(fwd)
    d_text, d_s = hipapi.build_sa_device(ctx, text)
    d_pos5 = hipapi.pos5_from_sa_torch(ctx, d_s, n)
    del d_s
    torch.cuda.empty_cache()
    d_pac, d_ent = hipapi.stage_entries_torch(ctx, n, d_text, d_pos5)
    bits = 28 if 8.0 * n + 8 > 8.0e9 else 26 if 8.0 * n + 8 > 1.0e9 else 24
    d_l2, n_l2, d_l1, n_l1 = hipapi.train_prmi_device(ctx, d_ent, n, bits)
    keep = (d_pac, d_ent) + hipapi.attach_index_torch(ctx, n, d_pac, d_ent, d_l2, n_l2, d_l1, n_l1)
    del d_text, d_pos5
    torch.cuda.empty_cache()
    print("[cost] index of %.0f Mbp in %.0f s" % (l_pac / 1e6, time.time() - t0), file=sys.stderr, flush=True)
    reads = bench.sample_reads(fwd, a.reads, bench.READ_LEN, 1000) if a.genome == "bench" else workload.make_reads_fast(fwd, a.reads, bench.READ_LEN, seed=78)
    d_reads = torch.from_numpy(reads.reshape(-1)).to(dev)
    d_off = torch.arange(0, (a.reads + 1) * bench.READ_LEN, bench.READ_LEN, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    print("[cost] reads after %.0f s" % (time.time() - t0), file=sys.stderr, flush=True)

    configs = []
    for c in a.configs.split(","):
        rounds, _, split = c[1:].partition("s")
        if split:
            try:
                ctx.set_tuning("seed_r3_split", int(split))
            except hipapi.MemeError:
                print("[cost] %s skipped: this library has no seed_r3_split" % c, file=sys.stderr, flush=True)
                continue
        configs.append((c, int(rounds), int(split) if split else None))
    means = {c[0]: [] for c in configs}
    for turn in range(a.turns):
        for name, rounds, split in configs:
            if split is not None:
                ctx.set_tuning("seed_r3_split", split)
            opt = hipapi.default_seed_opt(rounds=rounds)
            step = lambda: ctx.seed_batch_device(d_reads.data_ptr(), d_off.data_ptr(), a.reads, a.reads * bench.READ_LEN, opt)
            res = step()                                  # warm-up
            ctx.sync()
            stage, reseed, other = [], [], []
            t1 = time.perf_counter()
            for _ in range(a.steps):
                res = step()
                tm = ctx.timings()
                stage.append(tm.seed_kernel_ms); reseed.append(tm.seed_reseed_ms); other.append(tm.seed_gather_ms + tm.seed_pack_ms)
            ctx.sync()
            wall = (time.perf_counter() - t1) / a.steps * 1e3
            line = {"config": name, "turn": turn, "ms_per_step": wall, "search_stage_ms": float(np.mean(stage)), "search_stage_ms_steps": [round(x, 3) for x in stage],
                    "of_which_reseed_kernels_ms": float(np.mean(reseed)), "pack_gather_ms": float(np.mean(other)), "smems": int(res.total_smems),
                    "hits": int(res.total_hits), "searches": int(res.searches), "windows": int(tm.seed_windows), "launches": int(tm.seed_launches)}
            if split:
                line["r3"] = ctx.debug_seed_r3_counts()
                line["repeats_per_read"] = line["r3"]["repeats"] / a.reads
            means[name].append((wall, line["search_stage_ms"]))
            print(json.dumps(line), flush=True)
    for name, v in means.items():
        w, s = [x[0] for x in v], [x[1] for x in v]
        print(json.dumps({"config": name, "ms_per_step": [min(w), float(np.mean(w)), max(w)], "search_stage_ms": [min(s), float(np.mean(s)), max(s)]}), flush=True)
    del keep
    ctx.close()


if __name__ == "__main__":
    main()
