"""Record finishing on the device (meme_finish_batch_host / _device, bwa-meme_amd/csrc/meme_finish.hip: the compaction to the live records,
mem_sort_dedup_patch_mate_sort with mem_patch_reg and its alignment, the is_alt flag) against the compiled reference's records in
tests/golden/finish_golden.npz and, for other options and hand-made reads, against the model of tests/finish_gen.py that reproduces them: every field
of every record in the final order, the compact offsets and the useMateSort flag, exactly.  The index of the fixture genome is built on the device; a
batch's reads are made resident by a seeding call (read r of a finishing call is read r of that batch)."""
import numpy as np
import pytest

import finish_cases as FC
import finish_gen as FG
import primary_gen as PG
from pymeme import hipapi
from test_finish_model import OTHER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def W():
    return FG.workload()


@pytest.fixture(scope="module")
def gold():
    return FG.golden()


@pytest.fixture(scope="module")
def ctx(W):
    """a ctx with the index of the workload's genome, built on the device (as tests/test_gpu_mate.py stages it)"""
    c = hipapi.Context(0)
    g = W["genome"]
    n = 2 * g.shape[0]
    d_text, d_sa = hipapi.build_sa_device(c, hipapi.fwd_rc_text(g))
    d_pos5 = hipapi.pos5_from_sa_torch(c, d_sa, n)
    del d_sa
    d_pac, d_ent = hipapi.stage_entries_torch(c, n, d_text, d_pos5)
    d_l2, n_l2, d_l1, n_l1 = hipapi.train_prmi_device(c, d_ent, n, 12)
    keep = (d_pac, d_ent) + hipapi.attach_index_torch(c, n, d_pac, d_ent, d_l2, n_l2, d_l1, n_l1)
    yield c
    c.close()
    del keep


@pytest.fixture(autouse=True)
def _default_tuning(ctx):
    yield
    ctx.set_tuning("finish_blocks", 0)
    ctx.set_tuning("finish_lds_recs", 0)


def run(ctx, W, B, **opt):
    ctx.seed_batch_host(B["reads"], B["read_off"])
    return ctx.finish_batch_host(B["regs"], B["reg_off"], W["contigs"], W["l_pac"], FC.finish_opt(**opt))


def gold_of(gold, idx):
    """the golden records of the reads idx as a batch's result: (regs, reg_off, use_mate_sort)"""
    regs, off, ums = gold
    rows = [np.arange(off[r], off[r + 1]) for r in idx]
    return (FG.take(regs, np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)), np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64),
            ums[np.asarray(idx, np.int64)])


def live_counts(W):
    live = (W["regs"]["qe"] > W["regs"]["qb"]).astype(np.int64)
    return np.diff(np.concatenate([[0], np.cumsum(live)])[W["reg_off"]])


def check_whole(got, W, gold):
    assert FC.same(got, gold) is None
    assert not got["status"].any()                                         # the cap is zero: the model runs the whole workload without meeting a rejected call
    assert (got["n_patch_jobs"], got["n_patched"]) == (404, 236)
    assert got["n_wave"] == int((live_counts(W) > 1).sum()) == 3624 - 2220


def test_whole_workload_host_form(ctx, W, gold):
    got = run(ctx, W, W)
    check_whole(got, W, gold)
    assert got["kernel_ms"] > 0


def _device_form(ctx, W, B):
    """the device form on torch tensors -> (output tensors by name, the input tensors: the call is asynchronous, so the caller keeps them until it has synchronised)"""
    import torch
    dev = torch.device("cuda:0")
    n, total = B["reg_off"].shape[0] - 1, B["regs"].shape[0]
    ctx.seed_batch_host(B["reads"], B["read_off"])
    d_regs = torch.from_numpy(B["regs"].view(np.uint8).reshape(-1).copy()).to(dev)
    d_off = torch.from_numpy(B["reg_off"].astype(np.int64)).to(dev)
    T = {"out": torch.zeros(total * 112, dtype=torch.uint8, device=dev), "off": torch.full((n + 1,), -7, dtype=torch.int64, device=dev),
         "ums": torch.full((n,), 9, dtype=torch.uint8, device=dev), "status": torch.full((n,), 9, dtype=torch.uint8, device=dev), "ctr": torch.full((8,), -1, dtype=torch.int64, device=dev)}
    torch.cuda.synchronize()
    ctx.finish_batch_device(d_regs.data_ptr(), d_off.data_ptr(), n, total, W["contigs"], W["l_pac"], None, T["out"].data_ptr(), T["off"].data_ptr(), T["ums"].data_ptr(),
                            T["status"].data_ptr(), T["ctr"].data_ptr())
    return T, (d_regs, d_off)


def test_whole_workload_device_form(ctx, W, gold):
    T, (d_regs, _) = _device_form(ctx, W, W)
    ctx.sync()
    off = T["off"].cpu().numpy()
    ctr = T["ctr"].cpu().numpy()
    got = {"regs": FG.take(T["out"].cpu().numpy().view(hipapi.ALNREG), np.arange(off[-1])), "reg_off": off, "use_mate_sort": T["ums"].cpu().numpy(), "status": T["status"].cpu().numpy(),
           "n_wave": int(ctr[0]), "n_patch_jobs": int(ctr[1]), "n_patched": int(ctr[2])}
    check_whole(got, W, gold)
    assert np.array_equal(d_regs.cpu().numpy(), W["regs"].view(np.uint8).reshape(-1))          # the input is left alone


def test_device_outputs_feed_the_primary_stage_without_a_host_copy(ctx, W):
    import torch
    dev = torch.device("cuda:0")
    T, inputs = _device_form(ctx, W, W)
    n, total = W["reg_off"].shape[0] - 1, W["regs"].shape[0]
    d_out = torch.zeros(total * 112, dtype=torch.uint8, device=dev)
    d_n_pri = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_mapq = torch.full((total,), 99, dtype=torch.uint8, device=dev)
    d_status = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    d_heavy = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.primary_batch_device(T["out"].data_ptr(), T["off"].data_ptr(), n, total, PG.ID_BASE, None, d_out.data_ptr(), d_n_pri.data_ptr(), d_mapq.data_ptr(), d_status.data_ptr(), d_heavy.data_ptr())
    ctx.sync()
    PW, want = PG.workload(), PG.golden()
    assert PW["n_fixture"] == n
    off = PW["reg_off"][:n + 1]
    left = int(off[-1])
    assert np.array_equal(T["off"].cpu().numpy(), off)
    got = {"regs": FG.take(d_out.cpu().numpy().view(hipapi.ALNREG), np.arange(left)), "n_pri": d_n_pri.cpu().numpy(), "mapq": d_mapq.cpu().numpy()[:left]}
    want = {"regs": FG.take(want["regs"], np.arange(left)), "n_pri": want["n_pri"][:n], "mapq": want["mapq"][:left]}
    assert PG.same(got, want, off) is None
    assert not d_status.cpu().numpy().any()
    del inputs


@pytest.mark.parametrize("part", ["sort", "redundant", "patch", "real"])
def test_each_part_alone(ctx, W, gold, part):
    idx = np.nonzero(np.array(W["part"]) == part)[0]
    assert idx.shape[0] > 50
    got = run(ctx, W, FC.subset(W, idx))
    assert FC.same(got, gold_of(gold, idx)) is None and not got["status"].any()


def test_zero_slack_merges(ctx, W):
    B, expected = FC.zero_slack_batch(W)
    got = run(ctx, W, B)
    assert FC.same(got, FC.model(W, B)) is None and not got["status"].any()
    assert list(zip(got["regs"]["score"].tolist(), got["regs"]["w"].tolist())) == expected
    assert (got["n_wave"], got["n_patch_jobs"], got["n_patched"]) == (3, 3, 3)


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_small_batches(ctx, W, gold, count):
    for r0 in (0, 200, W["first_real"] - 20, W["first_real"] + 700):       # the sort part; the patch part; across the seam; extension records
        idx = np.arange(r0, r0 + count)
        got = run(ctx, W, FC.subset(W, idx))
        assert FC.same(got, gold_of(gold, idx)) is None and not got["status"].any(), r0


def test_reads_without_records_and_only_dead_records(ctx, W):
    idx = np.arange(W["first_real"], W["first_real"] + 70)
    B = FC.subset(W, idx)
    empty = dict(B, regs=B["regs"][:0].copy(), reg_off=np.zeros(71, np.int64))
    got = run(ctx, W, empty)
    assert got["regs"].shape[0] == 0 and not got["reg_off"].any() and got["use_mate_sort"].tolist() == [1] * 70 and not got["status"].any() and got["n_wave"] == 0
    dead = dict(B, regs=B["regs"].copy())
    dead["regs"]["qb"] = dead["regs"]["qe"] = -1
    got = run(ctx, W, dead)
    assert got["regs"].shape[0] == 0 and not got["reg_off"].any() and got["use_mate_sort"].tolist() == [1] * 70 and got["n_wave"] == 0
    none = run(ctx, W, dict(B, regs=B["regs"][:0].copy(), reg_off=np.zeros(1, np.int64)))
    assert none["regs"].shape[0] == 0 and none["reg_off"].tolist() == [0] and none["status"].shape[0] == 0


def test_live_counts_at_the_edges_of_the_introsort_one_read_per_call(ctx, W, gold):
    live = live_counts(W)
    sort_part = np.array(W["part"]) == "sort"
    for n in FG.SORT_COUNTS:
        r = int(np.nonzero(sort_part & (live == n))[0][-1])                # (the last one: a `dups` read)
        got = run(ctx, W, FC.subset(W, [r]))
        assert FC.same(got, gold_of(gold, [r])) is None and got["n_wave"] == (n > 1), n


def test_one_workgroup_goes_round_every_loop(ctx, W, gold):
    ctx.set_tuning("finish_blocks", 1)
    check_whole(run(ctx, W, W), W, gold)


def test_records_in_hbm(ctx, W, gold):
    """finish_lds_recs 4: the wavefront tier walks every read handed over with more than four records in its HBM workspace"""
    ctx.set_tuning("finish_lds_recs", 4)
    assert int((np.diff(W["reg_off"]) > 4).sum()) > 500
    check_whole(run(ctx, W, W), W, gold)


@pytest.fixture(scope="module")
def synthetic(W):
    return FC.subset(W, np.arange(W["first_real"]))


@pytest.mark.parametrize("name", list(OTHER), ids=list(OTHER))
def test_other_options_equal_the_model(ctx, W, synthetic, name):
    want = FC.model(W, synthetic, **OTHER[name])
    got = run(ctx, W, synthetic, **OTHER[name])
    assert FC.same(got, want) is None and not got["status"].any()
    assert (got["n_patch_jobs"], got["n_patched"]) == (want[3]["n_patch_jobs"], want[3]["n_patched"])


def test_a_9000_base_target_streams_through_the_rows(ctx, W, gold):
    """the patch part's records around the bar w == opt.w << 1: targets of 9 000 bases against 400-base queries, the band as wide as the matrix"""
    off = W["reg_off"]
    idx = [r for r in np.nonzero(np.array(W["part"]) == "patch")[0] if off[r + 1] - off[r] == 2 and
           int(W["regs"]["re"][off[r]:off[r + 1]].max() - W["regs"]["rb"][off[r]:off[r + 1]].min()) == 9000]
    assert len(idx) == 6
    B = FC.subset(W, idx)
    got = run(ctx, W, B)
    assert got["n_patch_jobs"] == FC.model(W, B)[3]["n_patch_jobs"] == 4
    assert FC.same(got, gold_of(gold, idx)) is None and not got["status"].any()


def test_a_patch_that_bridges_the_strands_sets_status(ctx, W, gold):
    g, L = W["genome"], W["l_pac"]
    idx = np.arange(W["first_real"] - 30, W["first_real"] + 30)
    B = FC.subset(W, idx)
    bridge = FC.batch_of([g[L - 300:L - 100]], [[dict(rb=L - 300, re=L - 200, qb=0, qe=100, rid=2, score=100, truesc=100, w=0),
                                                 dict(rb=L - 200, re=L + 100, qb=100, qe=200, rid=2, score=100, truesc=100, w=0)]])
    both = {"reads": np.concatenate([B["reads"], bridge["reads"]]), "read_off": np.concatenate([B["read_off"], B["read_off"][-1] + bridge["read_off"][1:]]),
            "regs": FG.take(np.concatenate([B["regs"], bridge["regs"]]), np.arange(B["regs"].shape[0] + 2)), "reg_off": np.concatenate([B["reg_off"], B["reg_off"][-1] + bridge["reg_off"][1:]])}
    got = run(ctx, W, both)
    assert got["status"].tolist() == [0] * 60 + [1]
    want = gold_of(gold, idx)
    left = int(want[1][-1])
    others = {"regs": FG.take(got["regs"], np.arange(left)), "reg_off": got["reg_off"][:61], "use_mate_sort": got["use_mate_sort"][:60]}
    assert FC.same(others, want) is None


def test_the_contig_table_follows_the_call(ctx, W):
    """one ctx, the tables A, B, A in turn: the ctx keeps one contig table and restages it when a call brings another"""
    B = FC.subset(W, np.arange(10))
    WB = FC.alt_flipped(W, B)
    want = {"A": FC.model(W, B), "B": FC.model(WB, B)}
    assert FG.same_records(*want["A"][:3], *want["B"][:3]) is not None        # the two tables give different records: the test cannot pass on a stale table
    for name, w in (("A", W), ("B", WB), ("A", W)):
        got = run(ctx, w, B)
        assert FC.same(got, want[name]) is None and not got["status"].any(), name


def test_arguments_the_stage_refuses(ctx, W):
    B = FC.subset(W, np.arange(10))
    fresh = hipapi.Context(0)
    try:
        with pytest.raises(hipapi.MemeError):                                # no resident batch
            fresh.finish_batch_host(B["regs"], B["reg_off"], W["contigs"], W["l_pac"])
    finally:
        fresh.close()
    ctx.seed_batch_host(B["reads"][:B["read_off"][5]], B["read_off"][:6])
    with pytest.raises(hipapi.MemeError):                                    # ten reads, five resident
        ctx.finish_batch_host(B["regs"], B["reg_off"], W["contigs"], W["l_pac"])
    ctx.seed_batch_host(B["reads"], B["read_off"])
    for bad in (dict(w=-1), dict(e_del=0), dict(e_ins=0), dict(e_del=-1), dict(e_ins=-2)):
        with pytest.raises(hipapi.MemeError):
            ctx.finish_batch_host(B["regs"], B["reg_off"], W["contigs"], W["l_pac"], hipapi.default_finish_opt(**bad))
    with pytest.raises(hipapi.MemeError):                                    # not the index's l_pac
        ctx.finish_batch_host(B["regs"], B["reg_off"], W["contigs"], W["l_pac"] - 1)
    assert FC.same(ctx.finish_batch_host(B["regs"], B["reg_off"], W["contigs"], W["l_pac"]), gold_of(FG.golden(), np.arange(10))) is None
