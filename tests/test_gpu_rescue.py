"""Mate rescue's record updates on the device (meme_rescue_batch_host / _device, bwa-meme_amd/csrc/meme_rescue.hip: what mem_sam_pe_batch_post does with the kswr_t
results before it marks primaries, reference src/bwamem_pair.cpp:851-921) against the model of tests/rescue_gen.py and, through it, the fixture the compiled
reference's post functions wrote (tests/golden/rescue_golden.npz; tests/test_rescue_model.py holds the model against the fixture): every field of every record,
reg_off_out, status and counters, under every value of rescue_lds_recs and rescue_blocks, in small batches, chained in front of the primary, pair and decide stages on
device arrays, and from the real front: meme_matesw_batch_host, meme_matesw_last_device, meme_rescue_batch_device."""
import numpy as np
import pytest

import decide_gen as DG
import pair_gen as QG
import primary_gen as PG
import rescue_cases as RC
import rescue_gen as RG
from finish_gen import take
from pymeme import hipapi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hipapi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def S():
    return RC.stage_inputs()


@pytest.fixture(autouse=True)
def _defaults(ctx):
    ctx.set_tuning("rescue_lds_recs", 0)
    ctx.set_tuning("rescue_blocks", 0)


def host_form(ctx, B):
    regs = take(B["regs"], np.arange(B["regs"].shape[0]))
    before = [regs.tobytes(), B["gar"].tobytes(), B["res"].tobytes()]
    R = ctx.rescue_batch_host(regs, B["reg_off"], B["ums"], B["read_len"], RC.jobs_of(B), B["pes"], RG.CONTIGS, RG.L_PAC, RC.rescue_opt(B["opt"]))
    assert [regs.tobytes(), B["gar"].tobytes(), B["res"].tobytes()] == before
    return {"regs": take(R["regs"], np.arange(R["regs"].shape[0])), "reg_off": R["reg_off"].copy(), "status": R["status"].copy(),
            "counters": {k: R[k] for k in ("n_wave", "n_tested", "n_pushed", "n_removed")}, "kernel_ms": R["kernel_ms"]}


def upload(B):
    import torch
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1).copy()).to(dev)
    T = {"regs": t(take(B["regs"], np.arange(B["regs"].shape[0])).view(np.uint8), np.uint8), "reg_off": t(B["reg_off"], np.int64), "ums": t(B["ums"], np.uint8), "rlen": t(B["read_len"], np.int32),
         "gar": t(B["gar"], np.int32), "gar_off": t(B["gar_off"], np.int64), "job_off": t(B["job_off"], np.int64), "res": t(np.ascontiguousarray(B["res"], hipapi.KSWR).view(np.uint8), np.uint8)}
    return T


def jobs_view(T, B):
    return {"gar": T["gar"].data_ptr(), "gar_off": T["gar_off"].data_ptr(), "job_off": T["job_off"].data_ptr(), "nbatches": B["gar_off"].shape[0] - 1, "res": T["res"].data_ptr(),
            "njobs": B["res"].shape[0]}


def device_form(ctx, B, T=None, total=None, jobs=None):
    import torch
    dev = torch.device("cuda:0")
    T = T or upload(B)
    n = B["reg_off"].shape[0] - 1
    total = B["regs"].shape[0] if total is None else total
    jobs = jobs or jobs_view(T, B)
    room = total + jobs["njobs"]
    O = {"out": torch.full((max(room, 1) * 112,), 0xA5, dtype=torch.uint8, device=dev), "off": torch.full((n + 1,), -7, dtype=torch.int64, device=dev),
         "status": torch.full((max(n, 1),), 9, dtype=torch.uint8, device=dev), "ctr": torch.full((8,), -1, dtype=torch.int64, device=dev)}
    before = {k: v.clone() for k, v in T.items()}
    torch.cuda.synchronize()
    ctx.rescue_batch_device(T["regs"].data_ptr(), T["reg_off"].data_ptr(), T["ums"].data_ptr(), T["rlen"].data_ptr(), n, total, jobs, B["pes"], RG.CONTIGS, RG.L_PAC, RC.rescue_opt(B["opt"]),
                            O["out"].data_ptr(), O["off"].data_ptr(), O["status"].data_ptr(), O["ctr"].data_ptr())
    ctx.sync()
    for k in T:
        assert torch.equal(T[k], before[k]), "input %s changed" % k
    off = O["off"].cpu().numpy()
    left = int(off[n])
    ctr = O["ctr"].cpu().numpy()
    regs = np.frombuffer(O["out"].cpu().numpy()[:left * 112].tobytes(), dtype=hipapi.ALNREG)
    assert (O["out"].cpu().numpy()[left * 112:] == 0xA5).all(), "records written behind the compact output"
    return {"regs": take(regs, np.arange(left)), "reg_off": off, "status": O["status"].cpu().numpy()[:n], "counters": dict(zip(("n_wave", "n_tested", "n_pushed", "n_removed"), [int(x) for x in ctr[:4]])),
            "tensors": O}


def agrees(got, m, name):
    d = RG.same(got, m)
    assert d is None, (name, d)
    assert got["counters"] == RC.counters_of(m), name


def test_whole_workload_host_form_equals_the_model_and_the_fixture(ctx, S):
    for B, m in S:
        agrees(host_form(ctx, B), m, B["name"])


def test_whole_workload_device_form(ctx, S):
    for B, m in S:
        agrees(device_form(ctx, B), m, B["name"])


@pytest.mark.parametrize("lds", [16, 1])
def test_columns_in_hbm(ctx, S, lds):
    ctx.set_tuning("rescue_lds_recs", lds)
    for B, m in S[:4] + S[-2:]:
        agrees(host_form(ctx, B), m, B["name"])


def test_one_workgroup_goes_round_every_loop(ctx, S):
    ctx.set_tuning("rescue_blocks", 1)
    ctx.set_tuning("rescue_lds_recs", 16)
    for B, m in (S[0], S[3]):
        agrees(device_form(ctx, B), m, B["name"])


def test_old_records_keep_their_bytes_and_new_ones_are_zero_elsewhere(ctx, S):
    B, m = S[3]
    got = host_form(ctx, B)
    src = {int(c): k for k, c in enumerate(B["regs"]["c"])}
    old = take(B["regs"], np.arange(B["regs"].shape[0]))
    n_new = 0
    for k in range(got["regs"].shape[0]):
        r = got["regs"][k:k + 1]
        if int(r["c"][0]) in src:                    # an old record: what went in but for flg, n_comp, qe
            j = src[int(r["c"][0])]
            for f in hipapi.ALNREG.names:            # (field by field: numpy does not keep a padded record's padding through a copy)
                if f not in ("flg", "n_comp_is_alt", "qe"):
                    assert r[f][0].tobytes() == old[f][j].tobytes(), (k, f)
            assert int(r["flg"][0]) == 0 and (int(r["n_comp_is_alt"][0]) >> 30) == (int(old["n_comp_is_alt"][j]) >> 30)
        else:
            n_new += 1
            for f in ("c", "truesc", "sub", "alt_sc", "sub_n", "w", "secondary_all", "seedlen0", "hash", "flg"):
                assert int(r[f][0]) == 0, (k, f)
            assert int(r["secondary"][0]) == -1 and float(r["frac_rep"][0]) == 0.0
    assert 100 < n_new <= m["stage"]["n_pushed"]


@pytest.mark.parametrize("name", ["B-one", "B-two", "B-three", "B-matesw-0", "B-all-failed"])
def test_small_batches_and_batches_without_jobs(ctx, S, name):
    B, m = next((B, m) for B, m in S if B["name"] == name)
    agrees(host_form(ctx, B), m, name)
    agrees(device_form(ctx, B), m, name)


def test_empty_batch(ctx):
    import torch
    R = ctx.rescue_batch_host(np.zeros(0, hipapi.ALNREG), np.zeros(1, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.int32),
                              {"gar": np.zeros(0, np.int32), "gar_off": np.zeros(1, np.int64), "job_off": np.zeros(1, np.int64), "res": np.zeros(0, hipapi.KSWR)}, RG.PES, RG.CONTIGS, RG.L_PAC)
    assert R["reg_off"].tolist() == [0] and R["regs"].shape[0] == 0 and R["n_wave"] == 0
    off = torch.full((1,), -7, dtype=torch.int64, device="cuda:0")
    ctr = torch.full((8,), -1, dtype=torch.int64, device="cuda:0")
    ctx.rescue_batch_device(0, 0, 0, 0, 0, 0, {"gar": 0, "gar_off": 0, "job_off": 0, "nbatches": 0, "res": 0, "njobs": 0}, RG.PES, RG.CONTIGS, RG.L_PAC, None, 0, off.data_ptr(), 0, ctr.data_ptr())
    ctx.sync()
    assert off.cpu().tolist() == [0] and ctr.cpu().tolist() == [0] * 8


def test_pairs_with_an_empty_end_and_without_jobs(ctx, S):
    """a batch whose mate stage posed nothing (njobs == 0, every gar entry -1 taken away with its records looked at: max_matesw 0) and pairs with an empty end"""
    B, m = next((B, m) for B, m in S if B["name"] == "B-matesw-0")
    assert B["res"].shape[0] == 0 and (np.diff(B["reg_off"]) == 0).any()
    got = device_form(ctx, B)
    agrees(got, m, B["name"])
    assert got["counters"]["n_pushed"] == 0 and got["counters"]["n_wave"] > 0        # (the mate-sort path sorts twice with nothing pushed)


def test_status_1_keeps_the_list_and_its_neighbours_exact(ctx, S):
    B, m = S[-1]
    assert B["name"] == "status1" and (m["status"] == 1).sum() >= 3
    for lds in (0, 16):
        ctx.set_tuning("rescue_lds_recs", lds)
        agrees(host_form(ctx, B), m, B["name"])
        agrees(device_form(ctx, B), m, B["name"])


def test_status_2_of_the_device_form(ctx, S):
    import torch
    B, m = S[0]
    n = B["reg_off"].shape[0] - 1
    total = B["regs"].shape[0]
    # (a) a read whose span is not inside the array: both lists of its pair report 2; the read itself keeps nothing, its mate keeps its input
    T = upload(B)
    r = 40
    off = B["reg_off"].copy()
    bad = off.copy()
    bad[r + 1] = total + 5                           # read r ends beyond the array; read r + 1 then starts beyond it too
    T["reg_off"] = torch.from_numpy(bad).to("cuda:0")
    got = device_form(ctx, B, T=T)
    st = got["status"]
    assert st[r] == 2 and st[r ^ 1] == 2 and st[r + 1] == 2 and st[(r + 1) ^ 1] == 2
    assert got["reg_off"][r + 1] == got["reg_off"][r]
    fine = [q for q in range(n) if q // 2 not in (r // 2, (r + 1) // 2)]
    # the pairs around keep the model's records (their gar cursors do not move only if the bad reads' records looked at stay what they were: compare lists, not offsets)
    for q in fine[:60] + fine[-60:]:
        if q // RG.default_opt(**B["opt"])["batch_reads"] == r // RG.default_opt(**B["opt"])["batch_reads"] and q > r:
            continue                                 # (behind the bad reads in their worker batch the cursor is the caller's error too)
        a = got["regs"][int(got["reg_off"][q]):int(got["reg_off"][q + 1])]
        w = m["regs"][int(m["reg_off"][q]):int(m["reg_off"][q + 1])]
        assert a.tobytes() == w.tobytes() and st[q] == m["status"][q], q
    # (b) a worker batch whose gar is two quads short (the later batches' entries are theirs, their offsets moved up with them): the lists of that batch whose mate's quads
    # reach beyond its end report 2 and keep their input, flg included; every other list of every batch is the model's
    B2, m2 = next((B, m) for B, m in S if B["name"] == "B-batches-6")
    o2 = RG.default_opt(**B2["opt"])
    cur = RG.cursors(B2, o2)
    g1, g2 = int(B2["gar_off"][1]), int(B2["gar_off"][2])
    short = dict(B2, gar=np.concatenate([B2["gar"][:g2 - 8], B2["gar"][g2:]]), gar_off=np.concatenate([B2["gar_off"][:2], B2["gar_off"][2:] - 8]))
    want2 = {q for q in range(6, 12) if cur[q ^ 1][1] + 4 * cur[q ^ 1][2] > g2 - 8 - g1}
    assert want2
    got = device_form(ctx, short)
    assert set(np.nonzero(got["status"] == 2)[0].tolist()) == want2
    for q in range(B2["reg_off"].shape[0] - 1):
        a = got["regs"][int(got["reg_off"][q]):int(got["reg_off"][q + 1])]
        if q in want2:
            b, e = int(B2["reg_off"][q]), int(B2["reg_off"][q + 1])
            assert a.tobytes() == take(B2["regs"], np.arange(b, e)).tobytes(), q
        else:
            assert a.tobytes() == m2["regs"][int(m2["reg_off"][q]):int(m2["reg_off"][q + 1])].tobytes() and got["status"][q] == m2["status"][q], q


def test_a_null_gar_where_the_offsets_say_it_holds_entries_is_status_2(ctx, S):
    """the offsets are device memory, so the call cannot refuse it: every list whose mate has a record looked at reports 2 and keeps its input, nothing is read through the null"""
    B, m = S[0]
    cur = RG.cursors(B, RG.default_opt(**B["opt"]))
    T = upload(B)
    got = device_form(ctx, B, T=T, jobs=dict(jobs_view(T, B), gar=0))
    n = B["reg_off"].shape[0] - 1
    want = np.array([2 if cur[q ^ 1][2] > 0 else 0 for q in range(n)], np.uint8)
    assert np.array_equal(got["status"], want) and (want == 2).sum() > 100
    assert np.array_equal(got["reg_off"], B["reg_off"])
    keep = take(B["regs"], np.arange(B["regs"].shape[0]))
    keep["flg"] = np.where(np.repeat(want, np.diff(B["reg_off"])) == 2, keep["flg"], 0)
    assert got["regs"].tobytes() == keep.tobytes()


def test_arguments_the_stage_refuses(ctx, S):
    B, _ = S[0]
    regs = take(B["regs"], np.arange(B["regs"].shape[0]))
    J = RC.jobs_of(B)

    def host(reg_off=B["reg_off"], ums=B["ums"], jobs=J, **opt):
        ctx.rescue_batch_host(regs, reg_off, ums if reg_off is B["reg_off"] else ums[:reg_off.shape[0] - 1], B["read_len"][:reg_off.shape[0] - 1], jobs, B["pes"], RG.CONTIGS, RG.L_PAC,
                              RC.rescue_opt(dict(B["opt"], **opt)))
    host()
    for bad in (dict(max_matesw=-1), dict(batch_reads=3), dict(batch_reads=0)):
        with pytest.raises(hipapi.MemeError):
            host(**bad)
    with pytest.raises(hipapi.MemeError):
        host(reg_off=B["reg_off"][:-1])              # an odd number of reads
    with pytest.raises(hipapi.MemeError):
        host(jobs=dict(J, gar_off=J["gar_off"][:-1], job_off=J["job_off"][:-1]))     # worker batches that do not cover the reads
    T = upload(B)
    n, total = B["reg_off"].shape[0] - 1, B["regs"].shape[0]
    import torch
    out = torch.zeros((total + B["res"].shape[0] + 2) * 112, dtype=torch.uint8, device="cuda:0")
    aux = torch.zeros(n + 8, dtype=torch.int64, device="cuda:0")

    def dev(regs_ptr=T["regs"].data_ptr(), out_ptr=out.data_ptr(), n=n, off_ptr=aux.data_ptr()):
        ctx.rescue_batch_device(regs_ptr, T["reg_off"].data_ptr(), T["ums"].data_ptr(), T["rlen"].data_ptr(), n, total, jobs_view(T, B), B["pes"], RG.CONTIGS, RG.L_PAC, RC.rescue_opt(B["opt"]),
                                out_ptr, off_ptr, aux.data_ptr(), aux.data_ptr())
    for bad in (dict(regs_ptr=T["regs"].data_ptr() + 8), dict(out_ptr=out.data_ptr() + 8), dict(out_ptr=T["regs"].data_ptr()), dict(n=n - 1), dict(off_ptr=0), dict(regs_ptr=0)):
        with pytest.raises(hipapi.MemeError):
            dev(**bad)
    ctx.sync()


def test_rescue_primary_pair_and_decide_chained_on_device_arrays(ctx):
    """family A through the four stages without a host copy, one synchronisation at the end = the reference's WHOLE mem_sam_pe_batch_post of the fixture: every field of every
    record behind it and every SAM observable (tests/decide_gen.py: observables_agree, with the stages' outputs where the models' stand)"""
    import torch
    dev = torch.device("cuda:0")
    GW = RG.golden_whole()
    for B, m in zip(RG.workload(), RG.modelled()[0]):
        if B["name"] not in RG.FAMILY_A:
            continue
        o = DG.default_opt(pen_unpaired=RG.default_opt(**B["opt"])["pen_unpaired"])
        pri, pair, dec = DG.stage_opts(o)
        n = B["reg_off"].shape[0] - 1
        id_base = RG.WHOLE_ID_BASE
        obs, whole = GW[B["name"]]
        T = upload(B)
        total = B["regs"].shape[0]
        room = total + B["res"].shape[0]
        R = {"out": torch.zeros(room * 112, dtype=torch.uint8, device=dev), "off": torch.full((n + 1,), -7, dtype=torch.int64, device=dev), "status": torch.zeros(n, dtype=torch.uint8, device=dev),
             "ctr": torch.zeros(8, dtype=torch.int64, device=dev)}
        P = {"out": torch.zeros(room * 112, dtype=torch.uint8, device=dev), "n_pri": torch.full((n,), -7, dtype=torch.int32, device=dev), "mapq": torch.zeros(room, dtype=torch.uint8, device=dev),
             "status": torch.zeros(n, dtype=torch.uint8, device=dev), "heavy": torch.zeros(1, dtype=torch.int64, device=dev)}
        Q = {k: torch.full((n // 2,), -7, dtype=torch.int32, device=dev) for k in ("score", "sub", "n_sub", "n_cand")}
        Q["z"] = torch.full((n,), -7, dtype=torch.int32, device=dev)
        Q["status"] = torch.full((n // 2,), 9, dtype=torch.uint8, device=dev)
        Q["heavy"] = torch.zeros(1, dtype=torch.int64, device=dev)
        D = {k: torch.full((n // 2,), -7, dtype=torch.int32, device=dev) for k in ("path", "q_pe", "flag")}
        D.update({k: torch.full((n,), -7, dtype=torch.int32, device=dev) for k in ("sel", "q_se", "alt")})
        D["status"] = torch.full((n // 2,), 9, dtype=torch.uint8, device=dev)
        D["heavy"] = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ctx.rescue_batch_device(T["regs"].data_ptr(), T["reg_off"].data_ptr(), T["ums"].data_ptr(), T["rlen"].data_ptr(), n, total, jobs_view(T, B), B["pes"], RG.CONTIGS, RG.L_PAC,
                                RC.rescue_opt(B["opt"]), R["out"].data_ptr(), R["off"].data_ptr(), R["status"].data_ptr(), R["ctr"].data_ptr())
        ctx.primary_batch_device(R["out"].data_ptr(), R["off"].data_ptr(), n, room, 2 * id_base, hipapi.default_primary_opt(**pri), P["out"].data_ptr(), P["n_pri"].data_ptr(), P["mapq"].data_ptr(),
                                 P["status"].data_ptr(), P["heavy"].data_ptr())
        ctx.pair_batch_device(P["out"].data_ptr(), R["off"].data_ptr(), P["n_pri"].data_ptr(), n, room, RG.CONTIGS, RG.L_PAC, B["pes"], id_base, hipapi.default_pair_opt(**pair),
                              Q["score"].data_ptr(), Q["sub"].data_ptr(), Q["n_sub"].data_ptr(), Q["n_cand"].data_ptr(), Q["z"].data_ptr(), Q["status"].data_ptr(), Q["heavy"].data_ptr())
        ctx.pair_decide_batch_device(P["out"].data_ptr(), R["off"].data_ptr(), P["n_pri"].data_ptr(), n, room, Q["score"].data_ptr(), Q["sub"].data_ptr(), Q["n_sub"].data_ptr(), Q["z"].data_ptr(),
                                     Q["status"].data_ptr(), RG.L_PAC, B["pes"], hipapi.default_decide_opt(**dec), D["path"].data_ptr(), D["sel"].data_ptr(), D["q_se"].data_ptr(), D["q_pe"].data_ptr(),
                                     D["flag"].data_ptr(), D["alt"].data_ptr(), D["status"].data_ptr(), D["heavy"].data_ptr())
        ctx.sync()                                   # the one wait of the chain
        left = int(whole["reg_off"][n])
        assert np.array_equal(R["off"].cpu().numpy(), whole["reg_off"]), B["name"]
        assert not R["status"].cpu().numpy().any() and not P["status"].cpu().numpy().any() and not Q["status"].cpu().numpy().any() and not D["status"].cpu().numpy().any()
        regs = take(np.frombuffer(P["out"].cpu().numpy()[:left * 112].tobytes(), dtype=hipapi.ALNREG), np.arange(left))
        got = {"regs": regs, "reg_off": whole["reg_off"], "status": whole["status"]}
        assert RG.same(got, whole) is None, (B["name"], RG.same(got, whole))
        dec_out = {"regs": regs, "path": D["path"].cpu().numpy(), "q_pe": D["q_pe"].cpu().numpy(), "flag": D["flag"].cpu().numpy(), "status": D["status"].cpu().numpy(),
                   "sel": D["sel"].cpu().numpy().reshape(-1, 2), "q_se": D["q_se"].cpu().numpy().reshape(-1, 2), "alt": D["alt"].cpu().numpy().reshape(-1, 2)}
        d = DG.observables_agree(B, {"decide": dec_out}, obs, {f: whole["regs"][f] for f in DG.MARKS})
        assert d is None, (B["name"], d)
        assert (dec_out["path"] >= 2).sum() > n // 16, "few pairs of true mates take the paired branch"


def test_matesw_last_device_without_a_mate_call_is_a_state_error():
    c = hipapi.Context(0)
    try:
        with pytest.raises(hipapi.MemeError, match="-5"):
            c.matesw_last_device()
    finally:
        c.close()


def test_from_the_real_front_the_device_pointers_of_the_mate_stage():
    """a small index and a resident batch: meme_matesw_batch_host, then meme_matesw_last_device and meme_rescue_batch_device on its device arrays = the host form fed
    from the pinned results; the pose and the results are the fixture's (family A: the compiled reference's own)"""
    import torch
    B, m = next((B, m) for B, m in zip(RG.workload(), RG.modelled()[0]) if B["name"] == "A-small-batches")
    o = RG.default_opt(**B["opt"])
    g = DG.genome()[0]
    c = hipapi.Context(0)
    try:
        n2 = 2 * RG.L_PAC
        d_text, d_sa = hipapi.build_sa_device(c, hipapi.fwd_rc_text(g))
        d_pos5 = hipapi.pos5_from_sa_torch(c, d_sa, n2)
        del d_sa
        d_pac, d_ent = hipapi.stage_entries_torch(c, n2, d_text, d_pos5)
        d_l2, n_l2, d_l1, n_l1 = hipapi.train_prmi_device(c, d_ent, n2, 12)
        keep = (d_pac, d_ent) + hipapi.attach_index_torch(c, n2, d_pac, d_ent, d_l2, n_l2, d_l1, n_l1)
        c.seed_batch_host(B["reads"], B["read_off"])
        mr = np.zeros(B["regs"].shape[0], hipapi.MATE_REG)
        for f in ("rb", "rid", "score"):
            mr[f] = B["regs"][f]
        R = c.matesw_batch_host(mr, B["reg_off"], [p[:3] for p in B["pes"]], RG.CONTIGS, RG.L_PAC, pen_unpaired=o["pen_unpaired"], max_matesw=o["max_matesw"], min_seed_len=o["min_seed_len"],
                                batch_reads=o["batch_reads"])
        assert np.array_equal(R["gar"], B["gar"]) and np.array_equal(R["gar_off"], B["gar_off"]) and np.array_equal(R["job_off"], B["job_off"])
        assert hipapi.records_equal(R["res"], B["res"])
        pinned = {k: np.array(R[k]) for k in ("gar", "gar_off", "job_off", "res")}
        V = c.matesw_last_device()
        assert V["nbatches"] == B["gar_off"].shape[0] - 1 and V["njobs"] == B["res"].shape[0]
        T = upload(B)
        got = device_form(c, B, T=T, jobs=V)
        agrees(got, m, B["name"])
        want = host_form(c, dict(B, **pinned))
        assert RG.same(got, want) is None and got["counters"] == want["counters"]
        R2 = c.matesw_batch_host(mr, B["reg_off"], [p[:3] for p in B["pes"]], RG.CONTIGS, RG.L_PAC, pen_unpaired=o["pen_unpaired"], max_matesw=o["max_matesw"], min_seed_len=o["min_seed_len"],
                                 batch_reads=o["batch_reads"])
        assert np.array_equal(R2["gar"], pinned["gar"]) and hipapi.records_equal(R2["res"], pinned["res"])      # (the view changes nothing of what the call returns)
        del keep
    finally:
        c.close()
