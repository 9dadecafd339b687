"""Primary marking and mapping quality on the device (meme_primary_batch_host / _device, bwa-meme_amd/csrc/meme_primary.hip) against the compiled
reference's outputs in tests/golden/primary_golden.npz and, for other options, ids and batches, against the model of tests/primary_gen.py that
reproduces them: every field of every record in the final order, n_pri and every quality, exactly."""
import numpy as np
import pytest

import primary_gen as PG
from pymeme import hipapi

pytestmark = pytest.mark.gpu
OTHER, split_other = PG.OTHER, PG.split_other
LIGHT_MAX = 8                     # records of a read the eight-lane tier takes (tuning key primary_split: at most this)


@pytest.fixture(scope="module")
def ctx():
    c = hipapi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def W():
    return PG.workload()


@pytest.fixture(scope="module")
def golden():
    return PG.golden()


@pytest.fixture(autouse=True)
def _default_tuning(ctx):
    yield
    ctx.set_tuning("primary_split", LIGHT_MAX)
    ctx.set_tuning("primary_blocks", 0)


def piece(W, res, r0, r1):
    """reads [r0, r1) of the workload as a batch of their own -> (regs, reg_off), and the same reads of a result over the whole workload"""
    off = W["reg_off"]
    b, e = int(off[r0]), int(off[r1])
    regs = PG.FG.take(W["regs"], np.arange(b, e))
    part = {"regs": PG.FG.take(res["regs"], np.arange(b, e)), "n_pri": res["n_pri"][r0:r1], "mapq": res["mapq"][b:e]}
    return regs, off[r0:r1 + 1] - b, part


def check(got, want, reg_off, status_reads=()):
    assert PG.same(got, want, reg_off, skip_mapq_of=status_reads) is None
    status = np.zeros(reg_off.shape[0] - 1, np.uint8)
    status[list(status_reads)] = 1
    assert np.array_equal(got["status"], status)


def test_whole_workload_host_form(ctx, W, golden):
    got = ctx.primary_batch_host(W["regs"], W["reg_off"], PG.ID_BASE)
    check(got, golden, W["reg_off"], [W["status_read"]])
    assert got["n_heavy"] == int((np.diff(W["reg_off"]) > LIGHT_MAX).sum()) > 100 and got["kernel_ms"] > 0


def test_whole_workload_device_form(ctx, W, golden):
    import torch
    dev = torch.device("cuda:0")
    n, total = W["reg_off"].shape[0] - 1, W["regs"].shape[0]
    d_regs = torch.from_numpy(W["regs"].view(np.uint8).reshape(-1).copy()).to(dev)
    d_off = torch.from_numpy(W["reg_off"].astype(np.int64)).to(dev)
    d_out = torch.zeros(total * 112, dtype=torch.uint8, device=dev)
    d_n_pri = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_mapq = torch.full((total,), 99, dtype=torch.uint8, device=dev)
    d_status = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    d_heavy = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.primary_batch_device(d_regs.data_ptr(), d_off.data_ptr(), n, total, PG.ID_BASE, None, d_out.data_ptr(), d_n_pri.data_ptr(), d_mapq.data_ptr(), d_status.data_ptr(), d_heavy.data_ptr())
    ctx.sync()
    got = {"regs": d_out.cpu().numpy().view(hipapi.ALNREG), "n_pri": d_n_pri.cpu().numpy(), "mapq": d_mapq.cpu().numpy(), "status": d_status.cpu().numpy()}
    check(got, golden, W["reg_off"], [W["status_read"]])
    assert int(d_heavy.cpu()[0]) == int((np.diff(W["reg_off"]) > LIGHT_MAX).sum())
    assert np.array_equal(d_regs.cpu().numpy(), W["regs"].view(np.uint8).reshape(-1))          # the input is left alone


def test_device_form_marks_offsets_that_are_no_span(ctx, W, golden):
    """reg_off of the device form cannot be checked on the host: a read whose offsets decrease or leave the record array is skipped with status 2, its neighbours are done"""
    import torch
    dev = torch.device("cuda:0")
    regs, off, want = piece(W, golden, W["n_fixture"], W["n_fixture"] + 6)
    total = regs.shape[0]
    bad = off.astype(np.int64).copy()
    bad[3] = total + 5                                   # read 2 ends and read 3 starts beyond the array
    d_regs = torch.from_numpy(regs.view(np.uint8).reshape(-1).copy()).to(dev)
    d_off = torch.from_numpy(bad).to(dev)
    d_out = torch.zeros(total * 112, dtype=torch.uint8, device=dev)
    d_n_pri = torch.zeros(6, dtype=torch.int32, device=dev)
    d_mapq = torch.zeros(total, dtype=torch.uint8, device=dev)
    d_status = torch.zeros(6, dtype=torch.uint8, device=dev)
    d_heavy = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.primary_batch_device(d_regs.data_ptr(), d_off.data_ptr(), 6, total, PG.ID_BASE + W["n_fixture"], None, d_out.data_ptr(), d_n_pri.data_ptr(), d_mapq.data_ptr(), d_status.data_ptr(), d_heavy.data_ptr())
    ctx.sync()
    assert d_status.cpu().numpy().tolist() == [0, 0, 2, 2, 0, 0]
    out = d_out.cpu().numpy().view(hipapi.ALNREG)
    for r in (0, 1, 4, 5):
        b, e = int(off[r]), int(off[r + 1])
        assert hipapi.records_equal(PG.FG.take(out, np.arange(b, e)), PG.FG.take(want["regs"], np.arange(b, e)))
    b, e = int(off[2]), int(off[4])
    assert not out[b:e].view(np.uint8).any()             # nothing written for the skipped reads


def test_light_tier_alone(ctx, W, golden):
    """a batch of the reads with at most eight records: nothing goes to the wavefront tier"""
    n = np.diff(W["reg_off"])
    keep = np.nonzero(n <= LIGHT_MAX)[0]
    assert keep.shape[0] > 3000 and set(range(LIGHT_MAX + 1)) <= set(n[keep].tolist())
    idx = np.concatenate([np.arange(W["reg_off"][r], W["reg_off"][r + 1]) for r in keep])
    regs = PG.FG.take(W["regs"], idx)
    off = np.concatenate([[0], np.cumsum(n[keep])]).astype(np.int64)
    want = PG.model(regs, off, PG.ID_BASE + np.arange(keep.shape[0]))
    got = ctx.primary_batch_host(regs, off, PG.ID_BASE)
    assert got["n_heavy"] == 0
    check(got, want, off, np.nonzero(want["status"])[0].tolist())


@pytest.mark.parametrize("split", [0, 2])
def test_heavy_tier_takes_what_the_split_sends(ctx, W, golden, split):
    """primary_split 0: every non-empty read through the wavefront tier, the reads of 1 to 8 records too; 2: both tiers meet inside the light tier's range"""
    ctx.set_tuning("primary_split", split)
    got = ctx.primary_batch_host(W["regs"], W["reg_off"], PG.ID_BASE)
    assert got["n_heavy"] == int((np.diff(W["reg_off"]) > split).sum())
    check(got, golden, W["reg_off"], [W["status_read"]])


def test_split_above_the_light_tiers_group_counts_as_eight(ctx, W, golden):
    ctx.set_tuning("primary_split", 1000)
    got = ctx.primary_batch_host(W["regs"], W["reg_off"], PG.ID_BASE)
    assert got["n_heavy"] == int((np.diff(W["reg_off"]) > LIGHT_MAX).sum())
    check(got, golden, W["reg_off"], [W["status_read"]])


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_small_batches(ctx, W, golden, count):
    for r0 in (0, W["n_fixture"] - 20, W["n_fixture"] + 5):          # fixture reads; across the seam; synthetic lists
        regs, off, want = piece(W, golden, r0, r0 + count)
        got = ctx.primary_batch_host(regs, off, PG.ID_BASE + r0)
        check(got, want, off)


def test_reads_without_records(ctx, W):
    """empty reads between the others, at both ends and alone"""
    n = np.diff(W["reg_off"])
    assert int((n == 0).sum()) > 50                                     # the workload has its own
    r0 = W["n_fixture"] - 40
    regs, off, _ = piece(W, PG.golden(), r0, r0 + 80)
    counts = np.zeros(2 * 80 + 3, np.int64)
    counts[2:-1:2] = np.diff(off)                                      # empty, empty, read, empty, read, ..., empty
    off2 = np.concatenate([[0], np.cumsum(counts)])
    want = PG.model(regs, off2, 5000 + np.arange(counts.shape[0]))
    got = ctx.primary_batch_host(regs, off2, 5000)
    check(got, want, off2)
    assert np.array_equal(got["n_pri"][counts == 0], np.zeros(int((counts == 0).sum()), np.int32))
    none = ctx.primary_batch_host(regs[:0], np.zeros(4, np.int64), 1)
    assert none["regs"].shape[0] == 0 and none["n_pri"].tolist() == [0, 0, 0] and none["status"].tolist() == [0, 0, 0] and none["n_heavy"] == 0
    assert ctx.primary_batch_host(regs[:0], np.zeros(1, np.int64), 1)["n_pri"].shape[0] == 0


def test_one_workgroup_goes_round_every_loop(ctx, W, golden):
    ctx.set_tuning("primary_blocks", 1)
    got = ctx.primary_batch_host(W["regs"], W["reg_off"], PG.ID_BASE)
    check(got, golden, W["reg_off"], [W["status_read"]])


@pytest.mark.parametrize("name", list(OTHER), ids=list(OTHER))
@pytest.mark.parametrize("split", [LIGHT_MAX, 0], ids=["tiers", "heavy"])
def test_other_options_equal_the_model(ctx, W, name, split):
    kw, id_base = split_other(name)
    ids = np.arange(W["reg_off"].shape[0] - 1, dtype=np.int64) + id_base
    want = PG.model(W["regs"], W["reg_off"], ids, PG.default_opt(**kw))
    if name == "primary5":
        assert want["counters"]["n_reordered"] >= 50
    ctx.set_tuning("primary_split", split)
    got = ctx.primary_batch_host(W["regs"], W["reg_off"], id_base, hipapi.default_primary_opt(**kw))
    check(got, want, W["reg_off"], np.nonzero(want["status"])[0].tolist())


def test_the_id_decides_where_scores_tie(ctx, W, golden):
    got = {}
    for id_base in (PG.ID_BASE, PG.ID_BASE + 1):
        got[id_base] = ctx.primary_batch_host(W["regs"], W["reg_off"], id_base)
    check(got[PG.ID_BASE], golden, W["reg_off"], [W["status_read"]])
    ids = np.arange(W["reg_off"].shape[0] - 1, dtype=np.int64) + PG.ID_BASE + 1
    check(got[PG.ID_BASE + 1], PG.model(W["regs"], W["reg_off"], ids), W["reg_off"], [W["status_read"]])
    a, b = got[PG.ID_BASE]["regs"], got[PG.ID_BASE + 1]["regs"]
    moved = (a["rb"] != b["rb"]) | (a["qb"] != b["qb"]) | (a["c"] != b["c"])
    assert moved.any()
    # records move only inside reads that have equal (score, is_alt) pairs
    off = W["reg_off"]
    for r in np.unique(np.searchsorted(off, np.nonzero(moved)[0], "right") - 1):
        x = W["regs"][off[r]:off[r + 1]]
        keys = list(zip(x["score"].tolist(), (x["n_comp_is_alt"] >> 30).tolist()))
        assert len(set(keys)) < len(keys), r


def test_a_span_beyond_the_log_table_sets_status(ctx, W, golden):
    r = W["status_read"]
    regs, off, want = piece(W, golden, r, r + 1)
    assert int((regs["re"] - regs["rb"]).max()) == 70000
    got = ctx.primary_batch_host(regs, off, PG.ID_BASE + r)
    assert got["status"].tolist() == [1]
    assert hipapi.records_equal(got["regs"], want["regs"]) and np.array_equal(got["n_pri"], want["n_pri"])      # the marking is done
    # inside the table the same read is fine
    regs["re"] = np.minimum(regs["re"], regs["rb"] + 65535)
    got = ctx.primary_batch_host(regs, off, PG.ID_BASE + r)
    check(got, PG.model(regs, off, [PG.ID_BASE + r]), off)


def test_arguments_the_stage_refuses(ctx, W):
    regs, off, _ = piece(W, PG.golden(), 0, 10)
    for bad in (dict(mapQ_coef_len=0.0), dict(mapQ_coef_len=-1.0), dict(a=0)):
        with pytest.raises(hipapi.MemeError):
            ctx.primary_batch_host(regs, off, 0, hipapi.default_primary_opt(**bad))
    down = off.copy()
    down[3] = down[2] - 1
    with pytest.raises(hipapi.MemeError):
        ctx.primary_batch_host(regs, down, 0)
