"""Pair scoring on the device (meme_pair_batch_host / _device, bwa-meme_amd/csrc/meme_pair.hip) against the compiled reference's outputs in
tests/golden/pair_golden.npz and, for n_cand, other options, tunings and batches, against the model of tests/pair_gen.py that reproduces them: score,
sub, n_sub, n_cand, z and status of every pair, exactly."""
import numpy as np
import pytest

import pair_gen as QG
from pymeme import hipapi

pytestmark = pytest.mark.gpu
LIGHT_MAX = 8                     # keys of a pair the eight-lane tier takes (tuning key pair_split: at most this)
ALL = QG.RESULT + ("n_cand", "status")


@pytest.fixture(scope="module")
def ctx():
    c = hipapi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def W():
    return QG.workload()


@pytest.fixture(scope="module")
def golden():
    return QG.golden()


@pytest.fixture(scope="module")
def modelled():
    return QG.modelled()[0]


@pytest.fixture(autouse=True)
def _default_tuning(ctx):
    yield
    ctx.set_tuning("pair_split", LIGHT_MAX)
    ctx.set_tuning("pair_blocks", 0)
    ctx.set_tuning("pair_lds_keys", 0)


def keys_of(B):
    n0, n1 = B["n_pri"][0::2], B["n_pri"][1::2]
    return np.where((n0 > 0) & (n1 > 0), n0 + n1, 0)


def run(ctx, B, **opt):
    return ctx.pair_batch_host(B["regs"], B["reg_off"], B["n_pri"], B.get("contigs", QG.CONTIGS), QG.L_PAC, B["pes"], B["id_base"], hipapi.default_pair_opt(**opt))


def check_whole(ctx, W, golden, modelled, split=LIGHT_MAX):
    for B, g, m in zip(W, golden, modelled):
        got = run(ctx, B)
        assert QG.same(got, g) is None, B["name"]
        assert QG.same(got, m, ALL) is None, B["name"]
        assert got["n_heavy"] == int((keys_of(B) > split).sum()), B["name"]
        assert got["kernel_ms"] > 0


def test_whole_workload_host_form(ctx, W, golden, modelled):
    check_whole(ctx, W, golden, modelled)
    assert sum(int((keys_of(B) > LIGHT_MAX).sum()) for B in W) > 100 and sum(int(((keys_of(B) > 0) & (keys_of(B) <= LIGHT_MAX)).sum()) for B in W) > 1500


def device_form(ctx, B, d_regs, d_off, d_n_pri, total, **opt):
    """the device form on torch tensors -> the result on the host (after a synchronisation)"""
    import torch
    dev = torch.device("cuda:0")
    n = B["reg_off"].shape[0] - 1
    m = n // 2
    T = {k: torch.full((m,), -7, dtype=torch.int32, device=dev) for k in ("score", "sub", "n_sub", "n_cand")}
    T["z"] = torch.full((2 * m,), -7, dtype=torch.int32, device=dev)
    T["status"] = torch.full((m,), 9, dtype=torch.uint8, device=dev)
    T["heavy"] = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.pair_batch_device(d_regs.data_ptr(), d_off.data_ptr(), d_n_pri.data_ptr(), n, total, B.get("contigs", QG.CONTIGS), QG.L_PAC, B["pes"], B["id_base"], hipapi.default_pair_opt(**opt),
                          T["score"].data_ptr(), T["sub"].data_ptr(), T["n_sub"].data_ptr(), T["n_cand"].data_ptr(), T["z"].data_ptr(), T["status"].data_ptr(), T["heavy"].data_ptr())
    ctx.sync()
    got = {k: T[k].cpu().numpy() for k in ("score", "sub", "n_sub", "n_cand", "status")}
    got["z"] = T["z"].cpu().numpy().reshape(m, 2)
    got["n_heavy"] = int(T["heavy"].cpu()[0])
    return got


def to_device(B):
    import torch
    dev = torch.device("cuda:0")
    return (torch.from_numpy(B["regs"].view(np.uint8).reshape(-1).copy()).to(dev), torch.from_numpy(B["reg_off"].astype(np.int64)).to(dev), torch.from_numpy(B["n_pri"].astype(np.int32)).to(dev))


def test_whole_workload_device_form(ctx, W, golden, modelled):
    for B, g, m in zip(W, golden, modelled):
        d_regs, d_off, d_n_pri = to_device(B)
        got = device_form(ctx, B, d_regs, d_off, d_n_pri, B["regs"].shape[0])
        assert QG.same(got, g) is None, B["name"]
        assert QG.same(got, m, ALL) is None, B["name"]
        assert got["n_heavy"] == int((keys_of(B) > LIGHT_MAX).sum())
        assert np.array_equal(d_regs.cpu().numpy(), B["regs"].view(np.uint8).reshape(-1))          # the input is left alone


def test_finish_primary_and_pair_stages_chained_without_a_host_copy(W, modelled):
    """meme_finish_batch_device -> meme_primary_batch_device -> meme_pair_batch_device on finish_golden.npz's reads, each taking the arrays the stage before it left in HBM:
    the model's result on primary_golden.npz's records (the first batch of the workload, which begins with them)"""
    import torch
    import finish_cases as FC
    import finish_gen as FG
    import primary_gen as PG
    dev = torch.device("cuda:0")
    FW, PW = FG.workload(), PG.workload()
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
        torch.cuda.synchronize()
        c.finish_batch_device(d_regs.data_ptr(), d_off.data_ptr(), n, total, FW["contigs"], FW["l_pac"], None, F["out"].data_ptr(), F["off"].data_ptr(), F["ums"].data_ptr(), F["status"].data_ptr(),
                              F["ctr"].data_ptr())
        c.primary_batch_device(F["out"].data_ptr(), F["off"].data_ptr(), n, total, PG.ID_BASE, None, P["out"].data_ptr(), P["n_pri"].data_ptr(), P["mapq"].data_ptr(), P["status"].data_ptr(),
                               P["heavy"].data_ptr())
        B = QG.piece(W[0], 0, n // 2)
        got = device_form(c, B, P["out"], F["off"], P["n_pri"], total)                                # (its ctx.sync() is the first wait of the chain)
        assert np.array_equal(F["off"].cpu().numpy(), B["reg_off"]) and np.array_equal(P["n_pri"].cpu().numpy(), B["n_pri"])
        want = QG.part(modelled[0], 0, n // 2)
        assert QG.same(got, want, ALL) is None
        assert int(got["n_cand"].sum()) == int(want["n_cand"].sum()) > 50          # (the fixture's reads are paired as they come, not mates: few pairs have candidates)
        assert got["n_heavy"] == int((keys_of(B) > LIGHT_MAX).sum()) > 50
        # record finishing twice more, with the table it has used and at once, no host synchronisation in between, with another: the ctx's one contig table has to wait
        # for the kernels that read it before it is overwritten
        FWB = FC.alt_flipped(FW, FC.subset(FW, np.arange(10)))
        want_a, want_b = FC.model(FW, FW), FC.model(FWB, FW)
        assert FG.same_records(*want_a[:3], *want_b[:3]) is not None
        F2 = {k: torch.zeros_like(v) for k, v in F.items()}
        torch.cuda.synchronize()
        for w, T in ((FW, F), (FWB, F2)):
            c.finish_batch_device(d_regs.data_ptr(), d_off.data_ptr(), n, total, w["contigs"], w["l_pac"], None, T["out"].data_ptr(), T["off"].data_ptr(), T["ums"].data_ptr(),
                                  T["status"].data_ptr(), T["ctr"].data_ptr())
        c.sync()
        for T, want in ((F, want_a), (F2, want_b)):
            off = T["off"].cpu().numpy()
            left = {"regs": FG.take(T["out"].cpu().numpy().view(hipapi.ALNREG), np.arange(off[-1])), "reg_off": off, "use_mate_sort": T["ums"].cpu().numpy()}
            assert FC.same(left, want) is None and not T["status"].cpu().numpy().any()
        del keep
    finally:
        c.close()


@pytest.mark.parametrize("split", [0, LIGHT_MAX])
def test_tier_by_tier(ctx, W, golden, modelled, split):
    """pair_split 0: every non-empty pair through the wavefront tier, the pairs of 2 to 8 keys too; 8: the pairs of 2 to 8 keys alone, nothing for the wavefront tier"""
    if split == 0:
        ctx.set_tuning("pair_split", 0)
        check_whole(ctx, W, golden, modelled, split=0)
        return
    for B, m in zip(W, modelled):
        k = keys_of(B)
        keep = np.nonzero(k <= LIGHT_MAX)[0]
        rows = np.concatenate([np.arange(B["reg_off"][2 * p], B["reg_off"][2 * p + 2]) for p in keep] + [np.zeros(0, np.int64)]).astype(np.int64)
        counts = np.diff(B["reg_off"]).reshape(-1, 2)[keep].reshape(-1)
        n_pri = B["n_pri"].reshape(-1, 2)[keep].reshape(-1)
        # (the ids move with the pairs: the model runs on the batch as it is called)
        sub = dict(B, regs=QG.PG.FG.take(B["regs"], rows), reg_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), n_pri=n_pri)
        got = run(ctx, sub)
        assert got["n_heavy"] == 0
        assert QG.same(got, QG.model(sub), ALL) is None, B["name"]


def test_split_in_between_and_above_the_group(ctx, W, golden, modelled):
    for split, counts_as in ((3, 3), (1000, LIGHT_MAX)):
        ctx.set_tuning("pair_split", split)
        check_whole(ctx, W[1:], golden[1:], modelled[1:], split=counts_as)


def test_sorted_keys_behind_the_lds_cap_run_from_hbm(ctx, W, golden, modelled):
    """pair_lds_keys 16: the pairs of 64, 65, 257 and 520 keys keep all but 16 sorted keys in the workspace (by default only the last of them does, past 512); 1: all but one"""
    sizes = [B for B in W if B["name"] == "sizes"]
    assert len(sizes) == 1 and {64, 65, 257, 520} <= set(keys_of(sizes[0]).tolist())
    for cap in (16, 1):
        ctx.set_tuning("pair_lds_keys", cap)
        check_whole(ctx, W[1:], golden[1:], modelled[1:])
    ctx.set_tuning("pair_lds_keys", 16)
    ctx.set_tuning("pair_split", 0)
    check_whole(ctx, W[:1], golden[:1], modelled[:1], split=0)


def test_one_workgroup_goes_round_every_loop(ctx, W, golden, modelled):
    ctx.set_tuning("pair_blocks", 1)
    check_whole(ctx, W, golden, modelled)
    ctx.set_tuning("pair_split", 0)
    check_whole(ctx, W[1:], golden[1:], modelled[1:], split=0)


@pytest.mark.parametrize("count", [1, 2, 3])
def test_small_batches(ctx, W, modelled, count):
    for B, m in zip(W, modelled):
        n = (B["reg_off"].shape[0] - 1) // 2
        for p0 in sorted({0, n // 2, n - count}):
            got = run(ctx, QG.piece(B, p0, p0 + count))
            assert QG.same(got, QG.part(m, p0, p0 + count), ALL) is None, (B["name"], p0)


def test_empty_pairs_at_both_ends_of_a_batch(ctx, W):
    """pairs without records, and pairs one of whose ends has none that takes part, in front of, between and behind the others; a batch of nothing else; no pairs at all"""
    B = next(b for b in W if b["name"] == "scores")
    n = (B["reg_off"].shape[0] - 1) // 2
    counts = np.zeros((2 * n + 3, 2), np.int64)
    n_pri = np.zeros((2 * n + 3, 2), np.int32)
    counts[2:-1:2] = np.diff(B["reg_off"]).reshape(-1, 2)               # empty, empty, pair, empty, pair, ..., empty
    n_pri[2:-1:2] = B["n_pri"].reshape(-1, 2)
    n_pri[2:-1:8, 1] = 0                                                # every fourth pair: the second end has records, none takes part
    E = dict(B, reg_off=np.concatenate([[0], np.cumsum(counts.reshape(-1))]).astype(np.int64), n_pri=n_pri.reshape(-1), id_base=(1 << 23) - n)
    want = QG.model(E)
    got = run(ctx, E)
    assert QG.same(got, want, ALL) is None
    dead = (n_pri == 0).any(axis=1)
    assert int(dead.sum()) >= n + 3 + n // 4 and not got["n_cand"][dead].any() and (got["z"][dead] == -1).all() and int(got["n_cand"].sum()) > 100
    none = run(ctx, dict(B, regs=B["regs"][:0], reg_off=np.zeros(7, np.int64), n_pri=np.zeros(6, np.int32)))
    assert none["score"].tolist() == [0, 0, 0] and none["z"].tolist() == [[-1, -1]] * 3 and none["status"].tolist() == [0, 0, 0] and none["n_heavy"] == 0
    assert run(ctx, dict(B, regs=B["regs"][:0], reg_off=np.zeros(1, np.int64), n_pri=np.zeros(0, np.int32)))["score"].shape[0] == 0


@pytest.mark.parametrize("split", [LIGHT_MAX, 0], ids=["tiers", "heavy"])
def test_status_1_skips_the_pair_and_leaves_its_neighbours_exact(ctx, W, split):
    """a record that takes part with rid outside the contigs or a negative score; the same record behind n_pri is nobody's business"""
    ctx.set_tuning("pair_split", split)
    for name, p in (("scores", 2), ("sizes", 9)):                       # a pair of the light tier, and one of 64 keys
        B = next(b for b in W if b["name"] == name)
        P = QG.piece(B, p - 2, p + 3)
        want = QG.model(P)
        assert want["n_cand"][1:4].all()
        k = int(P["reg_off"][5]) - 1                                    # the last record of the pair's first end
        for field, value in (("rid", 3), ("rid", -1), ("score", -5)):
            regs = P["regs"].copy()
            regs[field][k] = value
            got = run(ctx, dict(P, regs=regs))
            assert got["status"].tolist() == [0, 0, 1, 0, 0]
            assert (got["score"][2], got["sub"][2], got["n_sub"][2], got["n_cand"][2]) == (0, 0, 0, 0) and got["z"][2].tolist() == [-1, -1]
            keep = np.array([0, 1, 3, 4])
            assert QG.same({f: got[f][keep] for f in ALL}, {f: want[f][keep] for f in ALL}, ALL) is None
            n_pri = P["n_pri"].copy()
            n_pri[4] -= 1                                               # the record no longer takes part
            if n_pri[4] > 0:
                Q = dict(P, regs=regs, n_pri=n_pri)
                good = dict(Q, regs=P["regs"])
                assert QG.same(run(ctx, Q), QG.model(good), ALL) is None


def test_status_2_of_the_device_form(ctx, W):
    """reg_off and n_pri of the device form cannot be checked on the host: a pair one of whose reads has offsets that are no span of the record array, or an n_pri that
    is negative or larger than the span, is skipped with status 2; its neighbours are done"""
    B = next(b for b in W if b["name"] == "scores")
    P = QG.piece(B, 0, 8)
    want = QG.model(P)
    total = P["regs"].shape[0]
    off, n_pri = P["reg_off"].astype(np.int64).copy(), P["n_pri"].copy()
    off[5] = total + 5                                   # read 4 ends and read 5 starts beyond the array: pair 2
    n_pri[8] = int(off[9] - off[8]) + 1                  # more than the read has: pair 4
    n_pri[13] = -1                                       # pair 6
    bad = dict(P, reg_off=off, n_pri=n_pri)
    d_regs, d_off, d_n_pri = to_device(bad)
    got = device_form(ctx, bad, d_regs, d_off, d_n_pri, total)
    assert got["status"].tolist() == [0, 0, 2, 0, 2, 0, 2, 0]
    for p in (2, 4, 6):
        assert (got["score"][p], got["sub"][p], got["n_sub"][p], got["n_cand"][p]) == (0, 0, 0, 0) and got["z"][p].tolist() == [-1, -1]
    keep = np.array([0, 1, 3, 5, 7])
    assert QG.same({f: got[f][keep] for f in ALL}, {f: want[f][keep] for f in ALL}, ALL) is None
    with pytest.raises(hipapi.MemeError):                # the host form sees the same n_pri and refuses the call
        run(ctx, dict(P, n_pri=n_pri))


@pytest.mark.parametrize("name", list(QG.OTHER), ids=list(QG.OTHER))
@pytest.mark.parametrize("split", [LIGHT_MAX, 0], ids=["tiers", "heavy"])
def test_other_options_equal_the_model(ctx, W, name, split):
    kw = QG.OTHER[name]
    ctx.set_tuning("pair_split", split)
    for B in W[1:] if split == 0 else W:
        assert QG.same(run(ctx, B, **kw), QG.model(B, QG.default_opt(**kw)), ALL) is None, B["name"]


def test_the_id_decides_where_q_ties(ctx, W):
    B = next(b for b in W if b["name"] == "scores")
    a, b = run(ctx, B), run(ctx, dict(B, id_base=B["id_base"] + 1))
    assert QG.same(b, QG.model(dict(B, id_base=B["id_base"] + 1)), ALL) is None
    assert np.array_equal(a["score"], b["score"]) and np.array_equal(a["n_sub"], b["n_sub"]) and (a["z"] != b["z"]).any()


def test_arguments_the_stage_refuses(ctx, W):
    B = QG.piece(W[1], 0, 4)
    with pytest.raises(hipapi.MemeError):                # an odd number of reads
        run(ctx, dict(B, reg_off=B["reg_off"][:-1], n_pri=B["n_pri"][:-1]))
    wide = [(0, 1 << 20, 0, 300.0, 50.0)] + list(QG.PES[1:])
    with pytest.raises(hipapi.MemeError, match="penalty table"):       # 2^20 + 1 distances of a live orientation
        run(ctx, dict(B, pes=wide))
    wide[0] = (0, (1 << 20) - 1, 0, 300.0, 50.0)                       # 2^20: the most
    assert QG.same(run(ctx, dict(B, pes=wide)), QG.model(dict(B, pes=wide)), ALL) is None
    wide[0] = (0, 1 << 30, 1, 300.0, 50.0)                             # a failed orientation has no table
    assert QG.same(run(ctx, dict(B, pes=wide)), QG.model(dict(B, pes=wide)), ALL) is None
    with pytest.raises(hipapi.MemeError):
        run(ctx, B, a=0)
    down = B["reg_off"].copy()
    down[3] = down[2] - 1
    with pytest.raises(hipapi.MemeError):
        run(ctx, dict(B, reg_off=down))
    with pytest.raises(hipapi.MemeError):                # contigs that are no reference sequences of the genome
        run(ctx, dict(B, contigs=[(0, 100000, 0), (50000, 100000, 0), (200000, 100000, 0)]))


def test_a_refused_contig_table_is_not_remembered(ctx, W):
    """the ctx keeps one contig table: a table it refuses leaves nothing behind, and a table that differs in is_alt alone (which pair scoring does not read) is staged
    like any other"""
    B = QG.piece(W[1], 0, 4)
    want = QG.model(B)
    with pytest.raises(hipapi.MemeError):
        run(ctx, dict(B, contigs=[(0, 100000, 0), (50000, 100000, 0), (200000, 100000, 0)]))
    assert QG.same(run(ctx, B), want, ALL) is None
    alt = [(o, l, a ^ 1) for o, l, a in QG.CONTIGS]
    assert alt != list(QG.CONTIGS) and [c[:2] for c in alt] == [c[:2] for c in QG.CONTIGS]
    assert QG.same(run(ctx, dict(B, contigs=alt)), want, ALL) is None
