"""Times of the stage of mate rescue's record updates (meme_rescue_batch_host) next to the Smith-Waterman launches of the mate stage on a batch with the same number of
jobs, in the same run.

    python scripts/perf_rescue.py [out.json]        the driver: the step below in a fresh process under `timeout -k 10`
    python scripts/perf_rescue.py --step NAME OUT   one step, its result as a JSON file

Steps:
  production    1 M pairs of TRUE MATES made from synthetic records (read_len is an argument of the stage: no index, no bases): 150-base reads on one 3 Gbp sequence, only
                the FR orientation alive in the statistics; in most pairs both ends are placed and explain each other (every orientation skipped: four gar entries of -1 per
                record looked at), in one pair of nine or so one end is placed and the other has no record or a decoy far away: one job, posed where the walk asks for
                it, a synthetic result at the mate's true place -- about one job per 18 reads, the rate DESIGN 3.10 reports for a chunk.  kernel_ms of the stage (HIP events, the middle of
                five calls) for rescue_lds_recs 128, 32 and 16; then kernel_ms of meme_kswv_batch_host (the mate stage's Smith-Waterman launches) on as many jobs of the
                same shape (150-base queries against windows of the statistics' width, random bases)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "bwa-meme_amd"), os.path.join(REPO, "scripts")]
STEPS = (("production", 600),)
PAIRS = int(os.environ.get("PERF_RESCUE_PAIRS", 1 << 20))
L_PAC = 3_000_000_000
CONTIGS = [(0, 2_000_000_000, 0), (2_000_000_000, 1_000_000_000, 0)]
PES = [(0, 0, 1), (100, 700, 0), (0, 0, 1), (0, 0, 1)]
READ_LEN = 150
LDS = (128, 32, 16)


def production_batch(seed=97):
    """-> the stage's arguments as numpy arrays (batch_reads 512, the reference's)"""
    import numpy as np
    from pymeme import hipapi
    rng = np.random.default_rng(seed)
    kind = rng.random(PAIRS)                         # < 0.08: the mate is to be rescued (0.03 of them with a decoy on the other end, which asks for a job too)
    x = rng.integers(10_000, 1_900_000_000, PAIRS)
    dist = rng.integers(150, 500, PAIRS)
    rescue = kind < 0.08
    decoy = kind < 0.03
    n0 = np.ones(PAIRS, np.int64)
    n1 = np.where(rescue & ~decoy, 0, 1).astype(np.int64)
    counts = np.stack([n0, n1], 1).reshape(-1)
    reg_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    regs = np.zeros(int(reg_off[-1]), hipapi.ALNREG)
    i0 = reg_off[0:-1:2]
    regs["rb"][i0] = x
    has1 = n1 > 0
    i1 = reg_off[1::2][has1]
    # end 1 on the reverse strand `dist` behind end 0 (FR), or a decoy 50 Mbp away
    f1 = np.where(decoy, x + 50_000_000, x + dist)[has1]
    regs["rb"][i1] = 2 * L_PAC - (f1 + READ_LEN)
    regs["re"] = regs["rb"] + READ_LEN
    regs["qe"] = READ_LEN
    regs["score"] = regs["truesc"] = READ_LEN - 5
    regs["score"][i1] = np.where(decoy[has1], 40, READ_LEN - 5)
    regs["seedcov"] = READ_LEN // 2
    regs["secondary"] = regs["secondary_all"] = -1
    regs["n_comp_is_alt"] = 1
    regs["w"] = 100
    # gar: one quad per record (every record is looked at: one per end); a job in orientation 1 where the walk asks for one -- the placed end of a pair to be rescued,
    # and the decoy's own look at end 0's list, which its true record does not explain
    nreads = 2 * PAIRS
    quads = np.full((int(reg_off[-1]), 4), -1, np.int32)
    asks = np.zeros(int(reg_off[-1]), bool)
    asks[i0[rescue]] = True
    i1d = reg_off[1::2][decoy]
    asks[i1d] = True
    batch = np.repeat(np.arange(nreads), counts) // 512
    nb = (nreads + 511) // 512
    job_off = np.concatenate([[0], np.cumsum(np.bincount(batch[asks], minlength=nb))]).astype(np.int64)
    idx = np.arange(int(asks.sum())) - job_off[batch[asks]]
    quads[asks, 1] = idx
    gar_off = np.concatenate([[0], 4 * np.cumsum(np.bincount(batch, minlength=nb))]).astype(np.int64)
    # orientation 1 from a forward record: the mate reversed, the window [rb + low - l_ms, rb + high); the hit where the true mate lies.  The decoy's window holds
    # nothing: a score below min_seed_len
    per_rec = np.zeros(int(reg_off[-1]), hipapi.KSWR)
    per_rec["score"], per_rec["te"], per_rec["qe"], per_rec["te2"] = 10, 9, 9, -1
    d = dist[rescue]
    wrb = x[rescue] + PES[1][0] - READ_LEN
    new_rb = 2 * L_PAC - (x[rescue] + d + READ_LEN)
    hit = np.zeros(int(rescue.sum()), hipapi.KSWR)
    hit["score"], hit["score2"], hit["te2"] = READ_LEN - 8, 0, -1
    hit["qb"], hit["qe"] = 0, READ_LEN - 1
    hit["te"] = 2 * L_PAC - new_rb - 1 - wrb
    hit["tb"] = 2 * L_PAC - (new_rb + READ_LEN) - wrb
    per_rec[i0[rescue]] = hit
    res = per_rec[asks]
    return {"regs": regs, "reg_off": reg_off, "ums": np.ones(nreads, np.uint8), "read_len": np.full(nreads, READ_LEN, np.int32), "n_rescued": int(rescue.sum()),
            "jobs": {"gar": quads.reshape(-1), "gar_off": gar_off, "job_off": job_off, "res": res}}


def step_production():
    import numpy as np
    from pymeme import hipapi
    B = production_batch()
    ctx = hipapi.Context(0)
    njobs = int(B["jobs"]["res"].shape[0])
    out = {"pairs": PAIRS, "records": int(B["reg_off"][-1]), "jobs": njobs, "reads_per_job": round(2 * PAIRS / njobs, 2), "lds": {}}
    for lds in LDS:
        ctx.set_tuning("rescue_lds_recs", lds)
        calls = []
        for _ in range(5):
            R = ctx.rescue_batch_host(B["regs"], B["reg_off"], B["ums"], B["read_len"], B["jobs"], PES, CONTIGS, L_PAC)
            calls.append(round(R["kernel_ms"], 4))
        assert not R["status"].any(), "a walk asks for a result the batch does not pose"
        assert R["n_pushed"] == B["n_rescued"] and R["regs"].shape[0] == B["regs"].shape[0] + B["n_rescued"]
        out["lds"][str(lds)] = {"kernel_ms": sorted(calls)[2], "calls": calls, "n_wave": R["n_wave"], "n_tested": R["n_tested"], "n_pushed": R["n_pushed"], "n_removed": R["n_removed"]}
    # the step the stage sits behind: as many Smith-Waterman jobs of the same shape
    rng = np.random.default_rng(5)
    len1 = PES[1][1] - PES[1][0] + READ_LEN
    jobs = np.zeros(njobs, hipapi.KSWV_JOB)
    jobs["idr"] = np.arange(njobs, dtype=np.int64) * len1
    jobs["idq"] = np.arange(njobs, dtype=np.int64) * READ_LEN
    jobs["len1"], jobs["len2"] = len1, READ_LEN
    jobs["xtra"] = 0x40000 | 0x80000 | 0x10000 | 19
    ref = rng.integers(0, 4, njobs * len1).astype(np.uint8)
    qer = rng.integers(0, 4, njobs * READ_LEN).astype(np.uint8)
    at = rng.integers(0, len1 - READ_LEN, njobs)
    rows = (jobs["idr"] + at)[:, None] + np.arange(READ_LEN)[None, :]
    qer.reshape(njobs, READ_LEN)[:] = ref[rows]      # (the mate lies in its window, as a true mate does)
    calls = []
    for _ in range(5):
        _, ms = ctx.kswv_batch_host(jobs, ref, qer)
        calls.append(round(ms, 4))
    out["kswv"] = {"kernel_ms": sorted(calls)[2], "calls": calls, "jobs": njobs, "len1": len1, "len2": READ_LEN}
    ctx.close()
    return out


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        json.dump({"production": step_production}[sys.argv[2]](), open(sys.argv[3], "w"))
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else "perf_rescue.json"
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
