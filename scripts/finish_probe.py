"""Times of the record-finishing stage (meme_finish_batch_host) beside the extension stage that feeds it, and of the compiled reference's own function on the same reads.

    python scripts/finish_probe.py [out.json] [reads]     the driver: every step below in a fresh process under `timeout -k 10`, stopping at the first that fails
    python scripts/finish_probe.py --step NAME OUT READS  one step, its result as a JSON file

Steps:
  device     the `real` part of tests/finish_gen.py's workload (the extension fixture's reads and records), tiled to about 2 M reads on the fixture genome's index:
             kernel_ms of three calls over the whole batch, over its reads with at most one live record alone (the lane-per-read tier) and over the others alone (the
             wavefront tier), with the reads, records and patch alignments of each; and ext_ms of meme_extend_last_batch_host over the same resident reads.
  reference  mem_sort_dedup_patch_mate_sort of the compiled reference (tests/ref_finish.py, oracle/_ref) over the distinct reads of that batch, one thread: the time of
             Reference.finish, and of the native calls alone inside the same kind of loop (the rest is the Python loop's), scaled to the batch."""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "bwa-meme_amd")]
STEPS = (("device", 560), ("reference", 300))


def real_part():
    import numpy as np
    import finish_cases as FC
    import finish_gen as FG
    W = FG.workload()
    return W, FC.subset(W, np.nonzero(np.array(W["part"]) == "real")[0])


def tiled(B, keep, nreads):
    """the reads `keep` of the batch B repeated to nreads reads"""
    import numpy as np
    import finish_gen as FG
    rl, rc = np.diff(B["read_off"])[keep], np.diff(B["reg_off"])[keep]
    reps = -(-nreads // keep.shape[0])
    bases = np.concatenate([B["reads"][B["read_off"][r]:B["read_off"][r + 1]] for r in keep])
    rows = np.concatenate([np.arange(B["reg_off"][r], B["reg_off"][r + 1]) for r in keep]).astype(np.int64)
    read_off = np.concatenate([[0], np.cumsum(np.tile(rl, reps))])[:nreads + 1]
    reg_off = np.concatenate([[0], np.cumsum(np.tile(rc, reps))])[:nreads + 1]
    return {"reads": np.tile(bases, reps)[:int(read_off[-1])], "read_off": read_off.astype(np.int64), "regs": FG.take(B["regs"], np.tile(rows, reps)[:int(reg_off[-1])]), "reg_off": reg_off.astype(np.int64)}


def step_device(nreads):
    import numpy as np
    from pymeme import hipapi
    W, B = real_part()
    g = W["genome"]
    n = 2 * g.shape[0]
    ctx = hipapi.Context(0)
    d_text, d_sa = hipapi.build_sa_device(ctx, hipapi.fwd_rc_text(g))
    d_pos5 = hipapi.pos5_from_sa_torch(ctx, d_sa, n)
    del d_sa
    d_pac, d_ent = hipapi.stage_entries_torch(ctx, n, d_text, d_pos5)
    d_l2, n_l2, d_l1, n_l1 = hipapi.train_prmi_device(ctx, d_ent, n, 12)
    keep = (d_pac, d_ent) + hipapi.attach_index_torch(ctx, n, d_pac, d_ent, d_l2, n_l2, d_l1, n_l1)
    live = (B["regs"]["qe"] > B["regs"]["qb"]).astype(np.int64)
    live = np.diff(np.concatenate([[0], np.cumsum(live)])[B["reg_off"]])
    every = np.arange(live.shape[0])
    res = {"distinct_reads": int(every.shape[0]), "share_of_reads_with_at_most_one_live_record": round(float((live <= 1).mean()), 4)}
    for name, sel in (("whole", every), ("light_alone", every[live <= 1]), ("wave_alone", every[live > 1])):
        T = tiled(B, sel, max(1, int(round(nreads * sel.shape[0] / every.shape[0]))))
        ctx.seed_batch_host(T["reads"], T["read_off"])
        calls = []
        for _ in range(3):
            t0 = time.perf_counter()
            R = ctx.finish_batch_host(T["regs"], T["reg_off"], W["contigs"], W["l_pac"])
            calls.append({"kernel_ms": round(R["kernel_ms"], 3), "call_ms": round(1e3 * (time.perf_counter() - t0), 1)})
        assert not R["status"].any()
        res[name] = {"reads": int(T["reg_off"].shape[0] - 1), "records_in": int(T["regs"].shape[0]), "records_left": int(R["regs"].shape[0]), "n_wave": R["n_wave"], "patch_jobs": R["n_patch_jobs"],
                     "merges": R["n_patched"], "calls": calls}
        if name == "whole":
            E = ctx.extend_last_batch_host(W["contigs"], hipapi.default_chain_opt(W["l_pac"]))
            res["extension_of_the_same_reads"] = {"ext_ms": round(E["ext_ms"], 3), "chain_ms": round(E["chain_ms"], 3), "bsw_ms": round(E["bsw_ms"], 3), "records": int(E["regs"].shape[0])}
            del E
        del T, R
    del keep
    ctx.close()
    return res


def step_reference(nreads):
    import ctypes as C
    import tempfile
    import numpy as np
    import finish_gen as FG
    import ref_finish
    import ref_py
    from common import build_index
    from pymeme import synth
    if not (ref_py.have("libstage_ref.so") and ref_py.have("libbwa_pic.so") and ref_py.cpu_can_run()):
        return {"skipped": "no compiled reference here"}
    W, B = real_part()
    fa = os.path.join(tempfile.mkdtemp(prefix="fin_probe_"), "c.fa")
    synth.write_fasta(fa, W["genome"], name="cg", contigs=3)
    ref = ref_finish.Reference(build_index(fa, bits=14), alt=(FG.ALT_CONTIG,))
    n = B["reg_off"].shape[0] - 1
    t0 = time.perf_counter()
    ref.finish(B["regs"], B["reg_off"], B["reads"], B["read_off"])
    whole = time.perf_counter() - t0
    fn = getattr(ref_finish.lib(), ref_finish.SORT_DEDUP_PATCH)
    native = 0.0
    for r in range(n):
        a = B["regs"][B["reg_off"][r]:B["reg_off"][r + 1]]
        a = ref_finish.take(a, np.nonzero(a["qe"] > a["qb"])[0])
        if not a.shape[0]:
            continue
        q = np.ascontiguousarray(B["reads"][B["read_off"][r]:B["read_off"][r + 1]], dtype=np.uint8).copy()
        flag = C.c_bool(True)
        t0 = time.perf_counter()
        fn(ref.opt, ref.bns, C.c_void_p(ref.pac.ctypes.data), C.c_void_p(q.ctypes.data), C.c_int(a.shape[0]), C.c_void_p(a.ctypes.data), C.byref(flag))
        native += time.perf_counter() - t0
    scale = nreads / n
    return {"distinct_reads": n, "reference_finish_ms": round(1e3 * whole, 2), "native_calls_ms": round(1e3 * native, 2), "python_loop_share": round(1 - native / whole, 3),
            "native_calls_scaled_to_the_batch_ms": round(1e3 * native * scale, 1), "the_same_over_16_cpus_ms": round(1e3 * native * scale / 16, 1)}


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--step":
        res = {"device": step_device, "reference": step_reference}[sys.argv[2]](int(sys.argv[4]))
        json.dump(res, open(sys.argv[3], "w"))
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else "finish_probe.json"
    nreads = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
    all_res = {"reads": nreads}
    for name, limit in STEPS:
        part = "%s.%s" % (out, name)
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, part, str(nreads)]).returncode
        if rc != 0:
            print("step %s ended with status %d: nothing further is started" % (name, rc))
            return rc
        all_res[name] = json.load(open(part))
        os.remove(part)
        print(name, json.dumps(all_res[name]), flush=True)
        json.dump(all_res, open(out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
