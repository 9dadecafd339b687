"""Writes tests/golden/rescue_golden.npz from the COMPILED REFERENCE (oracle/_ref: `make -f oracle/Makefile.ref`).  Run from the repository root:

    PYTHONPATH=bwa-meme_amd:tests python tests/golden/make_rescue_golden.py

Family A's gar is posed by the reference's own mem_sam_pe_batch_pre and its kswr_t records are computed by its kswv; tests/rescue_gen.py's pose() has to give the same
gar, job for job.  Then the reference runs two ways (tests/ref_rescue.py): its post functions piecewise on every batch of families A and B, and mem_sam_pe_batch_post whole
on family A.  The file is written ONLY if the model of tests/rescue_gen.py equals the piecewise run on every field of every record, the chain rescue model -> primary ->
pair -> decide models equals the whole call on every record and every observable of family A, and the workload meets its floors.  The fixture holds family A's results and kept pairs (the
workload is regenerated from its seed around them), every batch's gar / gar_off / job_off / res, every field of every record behind rescue, and for family A the
records and the SAM observables (tests/decide_gen.py: OBS) behind the whole call.  About 400 KB: the issue foresaw tens of KB, on the scale of decide_golden.npz; the
records of 1 400 pairs with twenty fields each, twice for family A, take more (the chaining and extension fixtures beside it are of this size)."""
import os
import sys

import numpy as np

import ref_rescue
import rescue_gen as RG


def main():
    def genuine_res(B):
        gar, gar_off, job_off, parts = ref_rescue.pose(B)
        assert np.array_equal(gar, B["gar"]) and np.array_equal(gar_off, B["gar_off"]) and np.array_equal(job_off, B["job_off"]), "posing differs from the reference's (%s)" % B["name"]
        kj, ref, qer = RG.job_sequences(B, B["jobs"])
        jobs = np.concatenate([p[0] for p in parts]) if parts else kj
        assert np.array_equal(jobs["len1"], kj["len1"]) and np.array_equal(jobs["len2"], kj["len2"]) and np.array_equal(jobs["xtra"], kj["xtra"]), "jobs differ from the reference's"
        assert np.array_equal(np.concatenate([p[1] for p in parts]), ref) and np.array_equal(np.concatenate([p[2] for p in parts]), qer), "job sequences differ from the reference's"
        return ref_rescue.kswv(parts)

    W = RG.build(genuine_res)
    C = RG.counters()
    R = ref_rescue.Reference()
    out = {"seed": np.array([271828], np.int64)}
    cols, offs, a_res = [], [], []
    w_cols, w_offs, w_frac, w_obs = [], [], [], {f: [] for f in RG.DG.OBS}
    for B in W:
        m = RG.model(B, C)
        assert not m["status"].any(), B["name"]
        want = R.run(B)
        d = RG.same(m, want)
        if d is not None:
            sys.exit("REFUSED: the model differs from the reference's post functions on %s: %s" % (B["name"], d))
        if B["name"] in RG.FAMILY_A:
            obs, whole = R.run_whole(B)
            d = RG.whole_agrees(B, m, obs, whole)
            if d is not None:
                sys.exit("REFUSED: the chained models differ from the reference's whole call on %s: %s" % (B["name"], d))
            w_cols.append(np.stack([whole["regs"][f].astype(np.int64) for f in RG.FIELDS], 1))
            w_offs.append(whole["reg_off"])
            w_frac.append(whole["regs"]["frac_rep"].view(np.uint32).copy())
            for f in RG.DG.OBS:
                w_obs[f].append(obs[f])
        cols.append(np.stack([want["regs"][f].astype(np.int64) for f in RG.FIELDS], 1))
        offs.append(want["reg_off"])
        for f in ("gar", "gar_off", "job_off"):
            out["%s_%s" % (f, B["name"])] = B[f]
        out["res_" + B["name"]] = np.stack([B["res"][f] for f in RG.KSWR.names], 1).astype(np.int32)
        if B["name"] in RG.FAMILY_A:
            a_res.append(out["res_" + B["name"]])
            out["a_keep_" + B["name"]] = np.array(B["keep"], np.int64)
        print("%-16s %5d pairs %6d records in, %6d behind rescue, %5d jobs" % (B["name"], (B["reg_off"].shape[0] - 1) // 2, B["regs"].shape[0], want["regs"].shape[0], len(B["jobs"])))
    missed = RG.floors(C, W)
    if missed:
        sys.exit("REFUSED: the workload misses its floors: " + "; ".join(missed))
    out["a_res"] = np.concatenate(a_res)
    out["cols"] = np.concatenate(cols)
    out["reg_off"] = np.concatenate(offs)
    out["whole_cols"] = np.concatenate(w_cols)
    out["whole_reg_off"] = np.concatenate(w_offs)
    out["whole_frac_rep_bits"] = np.concatenate(w_frac)
    for f in RG.DG.OBS:
        out["whole_" + f] = np.concatenate(w_obs[f])
    out["counters"] = np.array([C[k] for k in sorted(C)], np.int64)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "rescue_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); counters %r" % (path, os.path.getsize(path), C))


if __name__ == "__main__":
    main()
