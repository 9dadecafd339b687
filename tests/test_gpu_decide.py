"""The pairing decision on the device (meme_pair_decide_batch_host / _device, bwa-meme_amd/csrc/meme_decide.hip) against the model of tests/decide_gen.py, which reproduces the
compiled reference's mem_sam_pe on the whole workload, and against that reference's observables in tests/golden/decide_golden.npz: path, sel, q_se, q_pe, flag, alt and status
of every pair and every field of every record, exactly, under every tuning, in small batches, chained behind the stages in front of it, with both status values and every
refused argument."""
import ctypes as C

import numpy as np
import pytest

import decide_cases as DC
import decide_gen as DG
from pymeme import hipapi

pytestmark = pytest.mark.gpu
DEFAULT_SPLIT = 64                # tuning key decide_split: its default
SPLIT_MAX = 1 << 20               # tuning key decide_split: at most this
SENTINEL = -7
MARK_BYTES = np.r_[48:52, 72:80]  # sub, secondary, secondary_all within a record


@pytest.fixture(scope="module")
def ctx():
    c = hipapi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def S():
    return DC.stage_inputs()


@pytest.fixture(autouse=True)
def _default_tuning(ctx):
    yield
    ctx.set_tuning("decide_split", DEFAULT_SPLIT)
    ctx.set_tuning("decide_blocks", 0)


def records_of(s):
    return np.diff(s["reg_off"]).reshape(-1, 2).sum(axis=1)


def run(ctx, s, **opt):
    return ctx.pair_decide_batch_host(s["regs"], s["reg_off"], s["n_pri"], s["pair"], DG.L_PAC, s["pes"], DC.decide_opt(dict(s["opt"], **opt)))


def piece(s, p0, p1):
    off = s["reg_off"]
    b, e = int(off[2 * p0]), int(off[2 * p1])
    return dict(s, regs=DG.PG.FG.take(s["regs"], np.arange(b, e)), reg_off=off[2 * p0:2 * p1 + 1] - b, n_pri=s["n_pri"][2 * p0:2 * p1], pair={f: s["pair"][f][p0:p1] for f in DC.PAIR_IN})


def part(m, s, p0, p1):
    b, e = int(s["reg_off"][2 * p0]), int(s["reg_off"][2 * p1])
    out = {f: m[f][p0:p1] for f in DG.OUT}
    out["regs"] = DG.PG.FG.take(m["regs"], np.arange(b, e))
    return out


def check_whole(ctx, S, split=DEFAULT_SPLIT, golden=None):
    for k, (s, m) in enumerate(S):
        got = run(ctx, s)
        assert DC.same(got, m) is None, s["name"]
        assert got["n_heavy"] == int((records_of(s) > split).sum()), s["name"]
        assert got["kernel_ms"] > 0
        if golden is not None and k < len(golden):
            obs, marks = golden[k]
            assert DG.observables_agree(DG.workload()[k], {"decide": got}, obs, marks) is None, s["name"]


def test_whole_workload_host_form_equals_the_model_and_the_fixture(ctx, S):
    check_whole(ctx, S, golden=DG.golden())
    heavy = sum(int((records_of(s) > DEFAULT_SPLIT).sum()) for s, _ in S)
    assert heavy > 10 and sum(records_of(s).shape[0] for s, _ in S) - heavy > 800


def to_device(s):
    import torch
    dev = torch.device("cuda:0")
    T = {"regs": torch.from_numpy(DG.PG.FG.take(s["regs"], np.arange(s["regs"].shape[0])).view(np.uint8).reshape(-1).copy()).to(dev),
         "reg_off": torch.from_numpy(np.ascontiguousarray(s["reg_off"], np.int64)).to(dev), "n_pri": torch.from_numpy(np.ascontiguousarray(s["n_pri"], np.int32)).to(dev)}
    for f in ("score", "sub", "n_sub"):
        T[f] = torch.from_numpy(np.ascontiguousarray(s["pair"][f], np.int32)).to(dev)
    T["z"] = torch.from_numpy(np.ascontiguousarray(s["pair"]["z"], np.int32).reshape(-1)).to(dev)
    T["status"] = torch.from_numpy(np.ascontiguousarray(s["pair"]["status"], np.uint8)).to(dev)
    return T


def device_form(ctx, s, T, total):
    """the device form on torch tensors, every output prefilled with a sentinel -> the result on the host (after a synchronisation); T["regs"] changes in place"""
    import torch
    dev = torch.device("cuda:0")
    n = s["reg_off"].shape[0] - 1
    m = n // 2
    O = {k: torch.full((m,), SENTINEL, dtype=torch.int32, device=dev) for k in ("path", "q_pe", "flag")}
    O.update({k: torch.full((2 * m,), SENTINEL, dtype=torch.int32, device=dev) for k in ("sel", "q_se", "alt")})
    O["status"] = torch.full((m,), 9, dtype=torch.uint8, device=dev)
    O["heavy"] = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.pair_decide_batch_device(T["regs"].data_ptr(), T["reg_off"].data_ptr(), T["n_pri"].data_ptr(), n, total, T["score"].data_ptr(), T["sub"].data_ptr(), T["n_sub"].data_ptr(),
                                 T["z"].data_ptr(), T["status"].data_ptr(), DG.L_PAC, s["pes"], DC.decide_opt(s["opt"]), O["path"].data_ptr(), O["sel"].data_ptr(), O["q_se"].data_ptr(),
                                 O["q_pe"].data_ptr(), O["flag"].data_ptr(), O["alt"].data_ptr(), O["status"].data_ptr(), O["heavy"].data_ptr())
    ctx.sync()
    got = {k: O[k].cpu().numpy() for k in ("path", "q_pe", "flag", "status")}
    got.update({k: O[k].cpu().numpy().reshape(m, 2) for k in ("sel", "q_se", "alt")})
    got["n_heavy"] = int(O["heavy"].cpu()[0])
    got["regs"] = T["regs"].cpu().numpy().view(hipapi.ALNREG)
    return got


def test_whole_workload_device_form_in_place(ctx, S):
    """every output is overwritten (none keeps its sentinel), the records change in place, and outside sub, secondary and secondary_all every byte of every record is what went in"""
    for s, m in S:
        T = to_device(s)
        before = T["regs"].cpu().numpy().reshape(-1, 112).copy()
        got = device_form(ctx, s, T, s["regs"].shape[0])
        assert DC.same(got, m) is None, s["name"]
        assert got["n_heavy"] == int((records_of(s) > DEFAULT_SPLIT).sum())
        after = got["regs"].view(np.uint8).reshape(-1, 112)
        keep = np.setdiff1d(np.arange(112), MARK_BYTES)
        assert np.array_equal(after[:, keep], before[:, keep]), s["name"]
        for f in ("path", "q_pe", "flag", "sel", "q_se", "alt"):
            if f != "q_se":                                                # (q_se is the reference's int and may be negative; none of the others can be the sentinel)
                assert not (got[f] == SENTINEL).any(), (s["name"], f)
        assert (got["status"] <= 1).all()
    changed = sum(int((m["regs"]["secondary_all"] != s["regs"]["secondary_all"]).sum()) for s, m in S)
    assert changed > 100                                                   # (the swap is taken often enough for "in place" to mean something)


@pytest.mark.parametrize("split", [0, 8, 16, SPLIT_MAX, SPLIT_MAX * 4], ids=["wavefront", "8", "16", "most", "above"])
def test_tier_by_tier(ctx, S, split):
    """decide_split 0: every pair with a record through the wavefront tier; the most (and anything above it, clamped): every pair, the reads of 520 records too, by eight lanes"""
    ctx.set_tuning("decide_split", split)
    check_whole(ctx, S, split=min(split, SPLIT_MAX))


def test_one_workgroup_goes_round_every_loop(ctx, S):
    ctx.set_tuning("decide_blocks", 1)
    check_whole(ctx, S)
    ctx.set_tuning("decide_split", 0)
    check_whole(ctx, S, split=0)


@pytest.mark.parametrize("count", [1, 2, 3])
def test_small_batches(ctx, S, count):
    for s, m in S:
        n = (s["reg_off"].shape[0] - 1) // 2
        for p0 in sorted({0, n // 2, max(n - count, 0)}):
            p1 = min(p0 + count, n)
            assert DC.same(run(ctx, piece(s, p0, p1)), part(m, s, p0, p1)) is None, (s["name"], p0)


def test_empty_batch(ctx, S):
    s, _ = S[0]
    none = run(ctx, dict(s, regs=s["regs"][:0], reg_off=np.zeros(1, np.int64), n_pri=np.zeros(0, np.int32), pair={f: s["pair"][f][:0] for f in DC.PAIR_IN}))
    assert none["path"].shape[0] == 0 and none["regs"].shape[0] == 0 and none["n_heavy"] == 0
    import torch
    e = dict(s, regs=s["regs"][:0], reg_off=np.zeros(1, np.int64), n_pri=np.zeros(0, np.int32), pair={f: s["pair"][f][:0] for f in DC.PAIR_IN})
    T = to_device(e)
    heavy = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    ctx.pair_decide_batch_device(0, T["reg_off"].data_ptr(), 0, 0, 0, 0, 0, 0, 0, 0, DG.L_PAC, s["pes"], None, 0, 0, 0, 0, 0, 0, 0, heavy.data_ptr())
    ctx.sync()
    assert int(heavy.cpu()[0]) == 0
    # pairs without records in front of, between and behind the others
    s, m = S[1]
    n = (s["reg_off"].shape[0] - 1) // 2
    counts = np.zeros((2 * n + 1, 2), np.int64)
    counts[1::2] = np.diff(s["reg_off"]).reshape(-1, 2)
    n_pri = np.zeros((2 * n + 1, 2), np.int32)
    n_pri[1::2] = s["n_pri"].reshape(-1, 2)
    pair = {f: np.zeros((2 * n + 1,) + s["pair"][f].shape[1:], s["pair"][f].dtype) for f in DC.PAIR_IN}
    pair["z"][:] = -1
    for f in DC.PAIR_IN:
        pair[f][1::2] = s["pair"][f]
    got = run(ctx, dict(s, reg_off=np.concatenate([[0], np.cumsum(counts.reshape(-1))]).astype(np.int64), n_pri=n_pri.reshape(-1), pair=pair))
    assert DC.same({f: (got[f][1::2] if f != "regs" else got[f]) for f in DG.OUT + ("regs",)}, m) is None
    assert not got["path"][0::2].any() and (got["sel"][0::2] == -1).all() and (got["flag"][0::2] == 1).all() and not got["status"].any()


def test_primary_pair_and_decide_stages_chained_on_the_workload(ctx):
    """meme_primary_batch_device -> meme_pair_batch_device -> meme_pair_decide_batch_device on the PRE-primary records of every batch, ids 2 P + r and P + p as the reference
    passes them, each stage taking the arrays the one before left in HBM, one synchronisation at the end: the three models chained"""
    import torch
    dev = torch.device("cuda:0")
    for B, m in zip(DG.workload(), DG.modelled()[0]):
        o = DG.default_opt(**B["opt"])
        pri, pair, dec = DG.stage_opts(o)
        n, total = B["reg_off"].shape[0] - 1, B["regs"].shape[0]
        d_in = torch.from_numpy(DG.PG.FG.take(B["regs"], np.arange(total)).view(np.uint8).reshape(-1).copy()).to(dev)
        d_off = torch.from_numpy(B["reg_off"].astype(np.int64)).to(dev)
        P = {"out": torch.zeros(max(total, 1) * 112, dtype=torch.uint8, device=dev), "n_pri": torch.full((n,), -7, dtype=torch.int32, device=dev), "mapq": torch.zeros(max(total, 1), dtype=torch.uint8, device=dev),
             "status": torch.zeros(n, dtype=torch.uint8, device=dev), "heavy": torch.zeros(1, dtype=torch.int64, device=dev)}
        Q = {k: torch.full((n // 2,), -7, dtype=torch.int32, device=dev) for k in ("score", "sub", "n_sub", "n_cand")}
        Q["z"] = torch.full((n,), -7, dtype=torch.int32, device=dev)
        Q["status"] = torch.full((n // 2,), 9, dtype=torch.uint8, device=dev)
        Q["heavy"] = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ctx.primary_batch_device(d_in.data_ptr(), d_off.data_ptr(), n, total, 2 * B["id_base"], hipapi.default_primary_opt(**pri), P["out"].data_ptr(), P["n_pri"].data_ptr(), P["mapq"].data_ptr(),
                                 P["status"].data_ptr(), P["heavy"].data_ptr())
        ctx.pair_batch_device(P["out"].data_ptr(), d_off.data_ptr(), P["n_pri"].data_ptr(), n, total, DG.CONTIGS, DG.L_PAC, B["pes"], B["id_base"], hipapi.default_pair_opt(**pair),
                              Q["score"].data_ptr(), Q["sub"].data_ptr(), Q["n_sub"].data_ptr(), Q["n_cand"].data_ptr(), Q["z"].data_ptr(), Q["status"].data_ptr(), Q["heavy"].data_ptr())
        T = {"regs": P["out"], "reg_off": d_off, "n_pri": P["n_pri"], "score": Q["score"], "sub": Q["sub"], "n_sub": Q["n_sub"], "z": Q["z"], "status": Q["status"]}
        got = device_form(ctx, {"reg_off": B["reg_off"], "pes": B["pes"], "opt": B["opt"]}, T, total)          # (its ctx.sync() is the first wait of the chain)
        got["regs"] = got["regs"][:total]
        assert np.array_equal(P["n_pri"].cpu().numpy(), m["primary"]["n_pri"]) and np.array_equal(Q["score"].cpu().numpy(), m["pair"]["score"]), B["name"]
        assert DC.same(got, m["decide"]) is None, B["name"]


def test_finish_primary_pair_and_decide_stages_chained_without_a_host_copy():
    """meme_finish_batch_device -> meme_primary_batch_device -> meme_pair_batch_device -> meme_pair_decide_batch_device on finish_golden.npz's reads, each taking the arrays the
    stage before it left in HBM: the decision's model on the pair model's result on primary_golden.npz's records (the first batch of the pair workload, which begins with them)"""
    import torch
    import finish_gen as FG
    import pair_gen as QG
    import primary_gen as PG
    dev = torch.device("cuda:0")
    FW, PW, W0, M0 = FG.workload(), PG.workload(), QG.workload()[0], QG.modelled()[0][0]
    c = hipapi.Context(0)
    try:
        g = FW["genome"]
        n2 = 2 * g.shape[0]
        d_text, d_sa = hipapi.build_sa_device(c, hipapi.fwd_rc_text(g))
        d_pos5 = hipapi.pos5_from_sa_torch(c, d_sa, n2)
        del d_sa
        d_pac, d_ent = hipapi.stage_entries_torch(c, n2, d_text, d_pos5)
        d_l2, n_l2, d_l1, n_l1 = hipapi.train_prmi_device(c, d_ent, n2, 12)
        keep = (d_pac, d_ent) + hipapi.attach_index_torch(c, n2, d_pac, d_ent, d_l2, n_l2, d_l1, n_l1)
        n, total = FW["reg_off"].shape[0] - 1, FW["regs"].shape[0]
        assert n == PW["n_fixture"] and n % 2 == 0 and FW["contigs"] == QG.CONTIGS and FW["l_pac"] == QG.L_PAC
        c.seed_batch_host(FW["reads"], FW["read_off"])
        d_regs = torch.from_numpy(FW["regs"].view(np.uint8).reshape(-1).copy()).to(dev)
        d_off = torch.from_numpy(FW["reg_off"].astype(np.int64)).to(dev)
        F = {"out": torch.zeros(total * 112, dtype=torch.uint8, device=dev), "off": torch.full((n + 1,), -7, dtype=torch.int64, device=dev), "ums": torch.zeros(n, dtype=torch.uint8, device=dev),
             "status": torch.zeros(n, dtype=torch.uint8, device=dev), "ctr": torch.zeros(8, dtype=torch.int64, device=dev)}
        P = {"out": torch.zeros(total * 112, dtype=torch.uint8, device=dev), "n_pri": torch.full((n,), -7, dtype=torch.int32, device=dev), "mapq": torch.zeros(total, dtype=torch.uint8, device=dev),
             "status": torch.zeros(n, dtype=torch.uint8, device=dev), "heavy": torch.zeros(1, dtype=torch.int64, device=dev)}
        Q = {k: torch.full((n // 2,), -7, dtype=torch.int32, device=dev) for k in ("score", "sub", "n_sub", "n_cand")}
        Q["z"] = torch.full((n,), -7, dtype=torch.int32, device=dev)
        Q["status"] = torch.full((n // 2,), 9, dtype=torch.uint8, device=dev)
        Q["heavy"] = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        c.finish_batch_device(d_regs.data_ptr(), d_off.data_ptr(), n, total, FW["contigs"], FW["l_pac"], None, F["out"].data_ptr(), F["off"].data_ptr(), F["ums"].data_ptr(), F["status"].data_ptr(),
                              F["ctr"].data_ptr())
        c.primary_batch_device(F["out"].data_ptr(), F["off"].data_ptr(), n, total, PG.ID_BASE, None, P["out"].data_ptr(), P["n_pri"].data_ptr(), P["mapq"].data_ptr(), P["status"].data_ptr(),
                               P["heavy"].data_ptr())
        B = QG.piece(W0, 0, n // 2)
        c.pair_batch_device(P["out"].data_ptr(), F["off"].data_ptr(), P["n_pri"].data_ptr(), n, total, QG.CONTIGS, QG.L_PAC, B["pes"], B["id_base"], None, Q["score"].data_ptr(), Q["sub"].data_ptr(),
                            Q["n_sub"].data_ptr(), Q["n_cand"].data_ptr(), Q["z"].data_ptr(), Q["status"].data_ptr(), Q["heavy"].data_ptr())
        T = {"regs": P["out"], "reg_off": F["off"], "n_pri": P["n_pri"], "score": Q["score"], "sub": Q["sub"], "n_sub": Q["n_sub"], "z": Q["z"], "status": Q["status"]}
        got = device_form(c, {"reg_off": B["reg_off"], "pes": B["pes"], "opt": {}}, T, total)                   # (its ctx.sync() is the first wait of the chain)
        kept = int(B["reg_off"][-1])
        got["regs"] = got["regs"][:kept]
        assert np.array_equal(F["off"].cpu().numpy(), B["reg_off"]) and np.array_equal(P["n_pri"].cpu().numpy(), B["n_pri"])
        pm = QG.part(M0, 0, n // 2)
        want = DG.decide(B["regs"], B["reg_off"], B["n_pri"], pm, B["pes"])
        assert DC.same(got, want) is None
        assert int((want["path"] >= 2).sum()) > 20 and int((want["path"] == 1).sum()) > 0
        del keep
    finally:
        c.close()


def test_status_1_leaves_the_pair_at_its_defaults_and_its_neighbours_exact(ctx, S):
    """a pair-stage status, n_sub + 1 = 65536, sub_n + 1 = 65536 of a record whose quality is asked for: defaults and untouched records; n_sub + 1 = 65535 is inside the table"""
    s, m = next((s, m) for s, m in S if s["name"] == "status")
    for split in (DEFAULT_SPLIT, 0):
        ctx.set_tuning("decide_split", split)
        got = run(ctx, s)
        assert np.nonzero(got["status"])[0].tolist() == s["expect_status1"] and (got["status"][s["expect_status1"]] == 1).all()
        assert DC.same(got, m) is None
        for p in s["expect_status1"]:
            b, e = int(s["reg_off"][2 * p]), int(s["reg_off"][2 * p + 2])
            assert (got["path"][p], got["q_pe"][p], got["flag"][p]) == (0, 0, 1) and got["sel"][p].tolist() == [-1, -1] and got["alt"][p].tolist() == [-1, -1] and got["q_se"][p].tolist() == [0, 0]
            for f in DG.MARKS:
                assert np.array_equal(got["regs"][f][b:e], s["regs"][f][b:e])
    assert int((m["path"] == 3).sum()) > 10                                  # (the defaults are not all there is to compare)


def test_status_2_of_the_device_form(ctx, S):
    """what the device form cannot check on the host: offsets that are no span of the record array, an n_pri that is negative or larger than the span, z outside [0, n_pri)
    on a pair with score > 0, a parent index beyond the read: status 2, defaults, records untouched, the neighbours done; the host form refuses the same arrays"""
    s0, _ = next((s, m) for s, m in S if s["name"] == "secondary")
    s = piece(s0, 0, 12)
    want = DG.decide(s["regs"], s["reg_off"], s["n_pri"], s["pair"], s["pes"])
    assert (s["pair"]["score"][[2, 4, 6, 8, 10]] > 0).all()
    total = s["regs"].shape[0]
    off, n_pri, z, regs = s["reg_off"].astype(np.int64).copy(), s["n_pri"].copy(), s["pair"]["z"].copy(), s["regs"].copy()
    off[5] = total + 5                                   # read 4 ends and read 5 starts beyond the array: pair 2
    n_pri[8] = int(off[9] - off[8]) + 1                  # more than the read has: pair 4
    n_pri[13] = -1                                       # pair 6
    z[8][1] = n_pri[17]                                  # z = n_pri: pair 8
    z[10][0] = -1                                        # pair 10
    bad = dict(s, reg_off=off, n_pri=n_pri, pair=dict(s["pair"], z=z), regs=regs)
    T = to_device(bad)
    got = device_form(ctx, bad, T, total)
    assert got["status"].tolist() == [0, 0, 2, 0, 2, 0, 2, 0, 2, 0, 2, 0]
    for p in (2, 4, 6, 8, 10):
        assert (got["path"][p], got["q_pe"][p], got["flag"][p]) == (0, 0, 1) and got["sel"][p].tolist() == [-1, -1] and got["alt"][p].tolist() == [-1, -1] and got["q_se"][p].tolist() == [0, 0]
    keep = np.array([0, 1, 3, 5, 7, 9, 11])
    assert DG.same({f: got[f][keep] for f in DG.OUT}, {f: want[f][keep] for f in DG.OUT}) is None
    rows = np.concatenate([np.arange(s["reg_off"][2 * p], s["reg_off"][2 * p + 2]) for p in (6, 8, 10)])      # (pairs whose spans are sound: their records are where they were)
    for f in hipapi.ALNREG.names:
        assert np.array_equal(got["regs"][f][rows], s["regs"][f][rows]), f
    rows = np.concatenate([np.arange(s["reg_off"][2 * p], s["reg_off"][2 * p + 2]) for p in (0, 1, 7, 9, 11)])
    for f in hipapi.ALNREG.names:
        assert np.array_equal(got["regs"][f][rows], want["regs"][f][rows]), f
    for field, value in (("n_pri", n_pri), ("z", z)):    # the host form sees the same arrays and refuses the call
        with pytest.raises(hipapi.MemeError):
            run(ctx, dict(s, n_pri=value) if field == "n_pri" else dict(s, pair=dict(s["pair"], z=value)))
    # a parent index beyond the read, on the record z names
    p, i = next((p, i) for p in range(12) for i in range(2) if p not in (2, 4, 6, 8, 10) and s["regs"]["secondary"][int(s["reg_off"][2 * p + i]) + int(s["pair"]["z"][p][i])] >= 0)
    regs["secondary"][int(s["reg_off"][2 * p + i]) + int(s["pair"]["z"][p][i])] = int(s["reg_off"][2 * p + i + 1] - s["reg_off"][2 * p + i])
    worse = dict(s, regs=regs)
    got = device_form(ctx, worse, to_device(worse), total)
    assert got["status"][p] == 2 and got["status"].sum() == 2 and got["path"][p] == 0
    with pytest.raises(hipapi.MemeError):
        run(ctx, worse)


def test_arguments_the_stage_refuses(ctx, S):
    s = piece(S[0][0], 0, 4)
    assert DC.same(run(ctx, s), part(S[0][1], S[0][0], 0, 4)) is None
    with pytest.raises(hipapi.MemeError):                # an odd number of reads
        run(ctx, dict(s, reg_off=s["reg_off"][:-1], n_pri=s["n_pri"][:-1], pair={f: s["pair"][f][:3] for f in DC.PAIR_IN}))
    for kw in (dict(a=0), dict(a=1, b=-1), dict(mapQ_coef_len=0.0, mapQ_coef_fac=3), dict(mapQ_coef_len=-1.0, mapQ_coef_fac=3)):
        with pytest.raises(hipapi.MemeError):
            run(ctx, s, **kw)
    down = s["reg_off"].copy()
    down[3] = down[2] - 1
    with pytest.raises(hipapi.MemeError):
        run(ctx, dict(s, reg_off=down))
    # a record array that is not 16-byte aligned: host form and device form
    raw = np.zeros(s["regs"].shape[0] * 112 + 64, np.uint8)
    at = (-raw.ctypes.data) % 16 + 8
    odd = raw[at:at + s["regs"].shape[0] * 112].view(hipapi.ALNREG)
    for f in hipapi.ALNREG.names:
        odd[f] = s["regs"][f]
    assert odd.ctypes.data % 16 == 8
    with pytest.raises(hipapi.MemeError, match="16-byte"):
        run(ctx, dict(s, regs=odd))
    T = to_device(s)
    n, total = s["reg_off"].shape[0] - 1, s["regs"].shape[0]
    out = [T["score"].data_ptr()] * 8                    # (never written: the call is refused before any launch)

    def dev(regs_ptr=T["regs"].data_ptr(), n=n, score=T["score"].data_ptr(), outs=out, opt=DC.decide_opt({})):
        ctx.pair_decide_batch_device(regs_ptr, T["reg_off"].data_ptr(), T["n_pri"].data_ptr(), n, total, score, T["sub"].data_ptr(), T["n_sub"].data_ptr(), T["z"].data_ptr(), T["status"].data_ptr(),
                                     DG.L_PAC, s["pes"], opt, *outs)
    with pytest.raises(hipapi.MemeError, match="16-byte"):
        dev(regs_ptr=T["regs"].data_ptr() + 8)
    with pytest.raises(hipapi.MemeError):
        dev(n=n - 1)
    with pytest.raises(hipapi.MemeError):
        dev(regs_ptr=0)
    with pytest.raises(hipapi.MemeError):
        dev(score=0)
    with pytest.raises(hipapi.MemeError):
        dev(outs=[0] + out[1:])
    with pytest.raises(hipapi.MemeError):
        dev(outs=out[:7] + [0])
    with pytest.raises(hipapi.MemeError):
        dev(opt=DC.decide_opt(dict(a=0)))
    L = hipapi.lib()                                     # null ctx, options, orientations, result
    cols = [np.ascontiguousarray(s["pair"][f], np.int32) for f in ("score", "sub", "n_sub", "z")] + [np.ascontiguousarray(s["pair"]["status"], np.uint8)]
    res, pin, o = hipapi.DecideHost(), hipapi.DecidePairIn(*[hipapi._p(c) for c in cols]), DC.decide_opt({})
    args = [C.c_void_p(ctx.h), hipapi._p(s["regs"]), hipapi._p(np.ascontiguousarray(s["reg_off"], np.int64)), hipapi._p(np.ascontiguousarray(s["n_pri"], np.int32)), C.c_int64(n), C.byref(pin),
            C.c_int64(DG.L_PAC), hipapi.pair_pes(s["pes"]), C.byref(o), C.byref(res)]
    for k in (0, 2, 3, 5, 7, 8, 9):
        a = list(args)
        a[k] = None
        assert L.meme_pair_decide_batch_host(*a) < 0
    assert L.meme_pair_decide_batch_host(*args) == 0
    for f in ("score", "sub", "n_sub", "z", "status"):   # a column of the pair stage's outputs missing
        pin2 = hipapi.DecidePairIn(*[hipapi._p(c) for c in cols])
        setattr(pin2, f, None)
        a = list(args)
        a[5] = C.byref(pin2)
        assert L.meme_pair_decide_batch_host(*a) < 0
    ctx.sync()
    assert DC.same(run(ctx, s), part(S[0][1], S[0][0], 0, 4)) is None      # the ctx is none the worse
