"""Parity of the HIP banded-SW kernel (through the C ABI) against the golden reference outputs and the oracle."""
import os

import numpy as np
import pytest

import bsw_gen
import oracle_py as O
from common import GOLDEN
from pymeme import hipapi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[0, 1 << 30], ids=["lane-per-pair", "lanes-per-pair"])
def ctx(request):
    # big batches take the lane-per-pair kernel, small ones the lanes-per-pair kernel: force each for every test
    c = hipapi.Context(0)
    c.set_tuning("bsw_lane_min_pairs", request.param)
    yield c
    c.close()


def _opt(eb):
    return hipapi.default_bsw_opt(end_bonus=eb)


@pytest.mark.parametrize("w,eb", [(100, 5), (100, 0), (200, 5), (200, 0)])
def test_hip_bsw_equals_reference_golden(ctx, w, eb):
    z = np.load(os.path.join(GOLDEN, "bsw_golden.npz"))
    pairs = z["pairs"].astype(hipapi.SEQPAIR).copy()
    ctx.bsw_batch(pairs, z["ref"], z["qer"], w, _opt(eb))
    assert np.array_equal(bsw_gen.outputs(pairs), z["scalar_w%d_eb%d" % (w, eb)])


@pytest.mark.parametrize("kw", [dict(), dict(max_q=300, sub=0.06, indel=0.02), dict(max_q=40), dict(max_q=500, h0_max=400),
                                dict(max_q=150, sub=0.3, unrelated_frac=0.5), dict(max_q=1000, min_q=600, h0_max=50)])
def test_hip_bsw_equals_oracle_random(ctx, kw):
    pairs, ref, qer = bsw_gen.make_pairs(1500, seed=11, **kw)
    for w in (100, 200, 7):
        want = pairs.copy()
        O.bsw_batch(want, ref, qer, w, O.default_bsw_params(5), threads=0)
        got = pairs.copy()
        ctx.bsw_batch(got, ref, qer, w, _opt(5))
        assert np.array_equal(bsw_gen.outputs(got), bsw_gen.outputs(want)), (kw, w)


def test_hip_bsw_other_scoring(ctx):
    pairs, ref, qer = bsw_gen.make_pairs(1500, seed=5, max_q=200)
    o = hipapi.BswOpt(4, 2, 8, 1, 50, 7, 2, 5)
    po = O.OrcBswParams(4, 2, 8, 1, 50, 7, 2, 5)
    want = pairs.copy(); O.bsw_batch(want, ref, qer, 60, po)
    got = pairs.copy(); ctx.bsw_batch(got, ref, qer, 60, o)
    assert np.array_equal(bsw_gen.outputs(got), bsw_gen.outputs(want))


def test_hip_bsw_edge_cases(ctx):
    # empty query / empty target / single bases / all-N / zero h0
    pairs = np.zeros(6, dtype=hipapi.SEQPAIR)
    ref = np.array([0, 1, 2, 3, 4, 4, 4, 0, 0, 0, 0, 0], np.uint8)
    qer = np.array([0, 1, 2, 3, 4, 4, 4, 0, 0, 0, 0, 0], np.uint8)
    spec = [(0, 0, 4, 0, 10), (0, 0, 0, 4, 10), (0, 0, 1, 1, 1), (4, 4, 3, 3, 20), (7, 7, 5, 5, 0), (0, 7, 4, 5, 3)]
    for i, (idr, idq, l1, l2, h0) in enumerate(spec):
        pairs[i]["idr"], pairs[i]["idq"], pairs[i]["len1"], pairs[i]["len2"], pairs[i]["h0"] = idr, idq, l1, l2, h0
    want = pairs.copy(); O.bsw_batch(want, ref, qer, 100, O.default_bsw_params(5))
    got = pairs.copy(); ctx.bsw_batch(got, ref, qer, 100, _opt(5))
    assert np.array_equal(bsw_gen.outputs(got), bsw_gen.outputs(want))
    assert ctx.bsw_batch(np.zeros(0, hipapi.SEQPAIR), ref, qer, 100).shape[0] == 0


@pytest.mark.parametrize("q", [1, 30, 31, 62, 63, 94, 95, 126, 127, 158, 159, 222, 223, 318, 319, 600, 601])
def test_hip_bsw_length_class_boundaries(ctx, q):
    # the lane-per-pair kernel is launched per LDS size class (query <= 30 / 62 / 94 / 126 / 158 / 222 / 318 / 600); longer queries and scores
    # beyond 14 bits take the lanes-per-pair kernel: every boundary, with a wavefront that is not full
    pairs, ref, qer = bsw_gen.make_pairs(130, seed=100 + q, min_q=q, max_q=q, h0_max=60)
    want = pairs.copy()
    O.bsw_batch(want, ref, qer, 100, O.default_bsw_params(5), threads=0)
    got = pairs.copy()
    ctx.bsw_batch(got, ref, qer, 100, _opt(5))
    assert np.array_equal(bsw_gen.outputs(got), bsw_gen.outputs(want))


def test_hip_bsw_scores_beyond_14_bits_and_mixed_lengths(ctx):
    a, ra, qa = bsw_gen.make_pairs(300, seed=21, max_q=120, h0_max=30000)      # h0 + qlen >= 2^14 for most pairs
    b, rb, qb = bsw_gen.make_pairs(300, seed=22, max_q=700)                     # both kernels in one batch
    b = b.copy(); b["idr"] += ra.shape[0]; b["idq"] += qa.shape[0]
    pairs = np.concatenate([a, b]); ref = np.concatenate([ra, rb]); qer = np.concatenate([qa, qb])
    order = np.random.default_rng(3).permutation(pairs.shape[0])
    pairs = pairs[order].copy()
    want = pairs.copy()
    O.bsw_batch(want, ref, qer, 100, O.default_bsw_params(5), threads=0)
    got = pairs.copy()
    ctx.bsw_batch(got, ref, qer, 100, _opt(5))
    assert np.array_equal(bsw_gen.outputs(got), bsw_gen.outputs(want))


def test_hip_bsw_queries_beyond_the_lds_resident_limit(ctx):
    """getScores16's class reaches 32 k bases (src/bandedSWA.h:47-86): queries of 5-9 k bases keep their DP rows in an HBM
    workspace instead of LDS; a mixed batch (short pairs alongside) exercises both storage modes of one launch sequence."""
    a, ra, qa = bsw_gen.make_pairs(6, seed=31, min_q=5000, max_q=9000, h0_max=100)
    b, rb, qb = bsw_gen.make_pairs(200, seed=32, max_q=300)
    b = b.copy(); b["idr"] += ra.shape[0]; b["idq"] += qa.shape[0]
    pairs = np.concatenate([a, b]); ref = np.concatenate([ra, rb]); qer = np.concatenate([qa, qb])
    for w in (100, 500):
        want = pairs.copy()
        O.bsw_batch(want, ref, qer, w, O.default_bsw_params(5), threads=0)
        got = pairs.copy()
        ctx.bsw_batch(got, ref, qer, w, _opt(5))
        assert np.array_equal(bsw_gen.outputs(got), bsw_gen.outputs(want)), w


@pytest.mark.parametrize("w", [100, 40, 200, 7])
def test_ring_of_band_columns_equals_a_word_per_query_column(w):
    """Round 6: queries longer than the band is wide keep 2w + 2 columns in a ring (k_bsw_lane_circ, tuning "bsw_circ", the default) instead of one LDS word
    per query column: same six outputs as the oracle and as the linear kernel, for every class the ring replaces -- long targets (the band slides the
    whole query length), large h0 (first-row values beyond the ring's first fill), gaps that re-grow the band, unrelated pairs (early exits)."""
    c = hipapi.Context(0)
    try:
        c.set_tuning("bsw_lane_min_pairs", 0)
        for kw in (dict(max_q=600, min_q=150), dict(max_q=600, min_q=230, sub=0.06, indel=0.03), dict(max_q=420, min_q=200, h0_max=900),
                   dict(max_q=320, min_q=100, sub=0.3, unrelated_frac=0.5), dict(max_q=600, min_q=1, h0_max=60)):
            pairs, ref, qer = bsw_gen.make_pairs(3000, seed=61 + w, **kw)
            want = pairs.copy()
            O.bsw_batch(want, ref, qer, w, O.default_bsw_params(5), threads=0)
            for circ in (1, 0):
                c.set_tuning("bsw_circ", circ)
                got = pairs.copy()
                c.bsw_batch(got, ref, qer, w, _opt(5))
                assert np.array_equal(bsw_gen.outputs(got), bsw_gen.outputs(want)), (kw, w, circ)
    finally:
        c.close()


# ---- the launch shapes only production-sized batches select: the device entry (class ranges read back, every class launched), one launch per LDS class from the
# ---- host entry, and grids of one and three workgroups, where a lane / group handles dozens of pairs in sequence -------------------------------------------
_oracle_cache = {}


def _oracle(key, make, w, eb=5):
    """(pairs, ref, qer, the oracle's six outputs) of a generated batch, computed once per module run"""
    if (key, w, eb) not in _oracle_cache:
        if key not in _oracle_cache:
            _oracle_cache[key] = make()
        pairs, ref, qer = _oracle_cache[key]
        want = pairs.copy()
        O.bsw_batch(want, ref, qer, w, O.default_bsw_params(eb), threads=0)
        _oracle_cache[(key, w, eb)] = bsw_gen.outputs(want)
    return _oracle_cache[key] + (_oracle_cache[(key, w, eb)],)


def _concat(batches):
    """several make_pairs batches as one (the sequence offsets shifted)"""
    ps, rs, qs, ro, qo = [], [], [], 0, 0
    for p, r, q in batches:
        p = p.copy(); p["idr"] += ro; p["idq"] += qo
        ps.append(p); rs.append(r); qs.append(q)
        ro += r.shape[0]; qo += q.shape[0]
    return np.concatenate(ps), np.concatenate(rs), np.concatenate(qs)


_BOUNDARY_Q = (1, 30, 31, 62, 63, 94, 95, 126, 127, 158, 159, 222, 223, 318, 319, 600, 601)


def _boundary_batch():
    return _concat([bsw_gen.make_pairs(130, seed=100 + q, min_q=q, max_q=q, h0_max=60) for q in _BOUNDARY_Q])


def _mixed_batch():
    a = bsw_gen.make_pairs(300, seed=21, max_q=120, h0_max=30000)
    b = bsw_gen.make_pairs(300, seed=22, max_q=700)
    pairs, ref, qer = _concat([a, b])
    return pairs[np.random.default_rng(3).permutation(pairs.shape[0])].copy(), ref, qer


def _on_device(ctx, pairs, ref, qer, w, opt):
    """meme_bsw_batch_device on torch tensors, as bench.py's BSW leg calls it; the six outputs back"""
    import torch
    d_pairs = torch.from_numpy(pairs.copy().view(np.uint8)).cuda()
    d_ref = torch.from_numpy(np.concatenate([ref, np.zeros(16, np.uint8)])).cuda()        # (the host entry's buffers have 16 bytes beyond the sequences too)
    d_qer = torch.from_numpy(np.concatenate([qer, np.zeros(16, np.uint8)])).cuda()
    torch.cuda.synchronize()
    ctx.bsw_batch_device(d_pairs.data_ptr(), d_ref.data_ptr(), d_qer.data_ptr(), pairs.shape[0], w, opt)
    ctx.sync()
    return bsw_gen.outputs(d_pairs.cpu().numpy().view(hipapi.SEQPAIR))


@pytest.mark.parametrize("circ", [1, 0])
def test_device_entry_equals_golden_and_oracle(ctx, circ):
    """meme_bsw_batch_device does not know the longest query: it reads it back and launches EVERY length class, each finding its range on the device and
    leaving when it is empty -- bench.py's and the extension stage's entry, which no other test calls."""
    ctx.set_tuning("bsw_circ", circ)
    try:
        z = np.load(os.path.join(GOLDEN, "bsw_golden.npz"))
        pairs = z["pairs"].astype(hipapi.SEQPAIR).copy()
        for w in (100, 200):
            for eb in (5, 0):
                assert np.array_equal(_on_device(ctx, pairs, z["ref"], z["qer"], w, _opt(eb)), z["scalar_w%d_eb%d" % (w, eb)]), (w, eb)
        # every class boundary in ONE batch: several classes have a range, the others are empty, in the same call
        pairs, ref, qer, want = _oracle("boundaries", _boundary_batch, 100)
        lens = set(pairs["len2"].tolist())
        assert lens == set(_BOUNDARY_Q) and pairs.shape[0] == 17 * 130
        assert np.array_equal(_on_device(ctx, pairs, ref, qer, 100, _opt(5)), want)
        pairs, ref, qer, want = _oracle("mixed", _mixed_batch, 100)
        assert np.array_equal(_on_device(ctx, pairs, ref, qer, 100, _opt(5)), want)
    finally:
        ctx.set_tuning("bsw_circ", 1)


@pytest.mark.parametrize("h0_max", [60, 900])
@pytest.mark.parametrize("w", [7, 100])
def test_ring_seam_at_exact_query_lengths(w, h0_max):
    """The ring of k_bsw_lane_circ has C = ((2w + 4 + 3) / 4) * 4 columns (20 for w = 7, 204 for w = 100).  Query lengths around its seam, 130 pairs of each:
    C - 1 is the last length without a top-up, at C the first topped-up column is `end` itself, 2C is the second lap; h0 up to 900 keeps first-row values
    positive beyond the first fill.  All six outputs of every pair equal the oracle's, with the ring and with a word per query column."""
    ring = ((2 * w + 4 + 3) // 4) * 4
    assert ring == {7: 20, 100: 204}[w]
    lens = (ring - 2, ring - 1, ring, ring + 1, 2 * ring - 1, 2 * ring, 2 * ring + 1)
    pairs, ref, qer, want = _oracle(("seam", w, h0_max), lambda: _concat([bsw_gen.make_pairs(130, seed=300 + q + h0_max, min_q=q, max_q=q, h0_max=h0_max) for q in lens]), w)
    assert pairs.shape[0] == 7 * 130 and set(pairs["len2"].tolist()) == set(lens)
    c = hipapi.Context(0)
    try:
        c.set_tuning("bsw_lane_min_pairs", 0)
        for circ in (1, 0):
            c.set_tuning("bsw_circ", circ)
            got = pairs.copy()
            c.bsw_batch(got, ref, qer, w, _opt(5))
            assert np.array_equal(bsw_gen.outputs(got), want), (w, h0_max, circ)
    finally:
        c.close()


@pytest.mark.parametrize("max_q", [600, 120])
def test_host_entry_launches_per_class_beyond_the_one_launch_bound(max_q):
    """launch_bsw sends a batch of fewer than n_cus * 64 * 16 pairs out as ONE launch of the longest query's class; production's 2 M-read chunks are beyond
    that and get one launch per LDS class.  3 000 oracle-checked pairs, named n_cus * 1024 + 1000 times over (the replicas share the sequence bytes).
    max_q = 120: the classes above the longest query are skipped by the host."""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    base, ref, qer, want = _oracle(("classes", max_q), lambda: bsw_gen.make_pairs(3000, seed=71 + max_q, max_q=max_q, min_q=1), 100)
    n = n_cus * 1024 + 1000
    assert n > n_cus * 64 * 16
    idx = np.arange(n) % base.shape[0]
    pairs = base[idx].copy()
    c = hipapi.Context(0)
    try:
        c.set_tuning("bsw_lane_min_pairs", 0)
        for circ in (1, 0):
            c.set_tuning("bsw_circ", circ)
            got = pairs.copy()
            c.bsw_batch(got, ref, qer, 100, _opt(5))
            bad = np.nonzero((bsw_gen.outputs(got) != want[idx]).any(axis=1))[0]
            assert bad.size == 0, (circ, bad.size, int(bad[0]), int(idx[bad[0]]))
    finally:
        c.close()


@pytest.mark.parametrize("blocks", [1, 3])
def test_one_and_three_workgroups_take_the_whole_batch(blocks):
    """Tuning "bsw_blocks": the persistent grids draw pairs by ticket; with the default grid and a test-sized batch a lane or group sees one pair, at most two.
    One and three workgroups: a lane of k_bsw_lane / k_bsw_lane_circ takes ~24 pairs in turn (state left in the LDS ring or the registers by pair n would show
    in pair n + 1), a group of k_bsw<LP> ~25, HBM-workspace rows included."""
    c = hipapi.Context(0)
    try:
        c.set_tuning("bsw_blocks", blocks)
        c.set_tuning("bsw_lane_min_pairs", 0)
        for w in (100, 7):
            pairs, ref, qer, want = _oracle("lanes", lambda: bsw_gen.make_pairs(1500, seed=81, max_q=320, min_q=100, h0_max=900), w)
            assert pairs.shape[0] // (64 * blocks) >= 7 and (blocks > 1 or pairs.shape[0] // 64 >= 20)
            for circ in (1, 0):
                c.set_tuning("bsw_circ", circ)
                got = pairs.copy()
                c.bsw_batch(got, ref, qer, w, _opt(5))
                assert np.array_equal(bsw_gen.outputs(got), want), (w, circ)
        c.set_tuning("bsw_circ", 1)
        c.set_tuning("bsw_lane_min_pairs", 1 << 30)
        pairs, ref, qer, want = _oracle("groups", lambda: bsw_gen.make_pairs(400, seed=82, max_q=700), 100)
        got = pairs.copy()
        c.bsw_batch(got, ref, qer, 100, _opt(5))
        assert np.array_equal(bsw_gen.outputs(got), want)
        pairs, ref, qer, want = _oracle("hbm rows", lambda: _concat([bsw_gen.make_pairs(6, seed=31, min_q=5000, max_q=9000, h0_max=100), bsw_gen.make_pairs(200, seed=32, max_q=300)]), 100)
        got = pairs.copy()
        c.bsw_batch(got, ref, qer, 100, _opt(5))
        assert np.array_equal(bsw_gen.outputs(got), want)
    finally:
        c.close()
