"""The case texts of tests/index_cases.py (CPU only): the host builder gives the suffix array of the definition for each, the set of cases reaches the branches
it names -- conditions on the inputs, computed from the definition, not measurements of a build -- and the host trainer's models of the P-RMI cases cover
every key."""
import numpy as np
import pytest

import index_cases as IC
from common import entry_keys, prmi_bounds_cover
from pymeme import hostapi


@pytest.mark.parametrize("name", IC.NAMES)
def test_host_builder_equals_the_definition(name):
    c = IC.case(name)
    text, sa = hostapi.build_sa(c.fwd)
    assert np.array_equal(text, c.text)
    assert c.n >= 64 and c.n <= 5000 and sorted(c.sa.tolist()) == list(range(c.n))
    assert np.array_equal(sa, c.sa), "first differing slot %d" % np.nonzero(sa != c.sa)[0][:1]


def test_cases_reach_the_refinement_edges():
    cs = [IC.case(n) for n in IC.NAMES]
    assert IC.case("no_ties_2000").tied == 0 and IC.case("no_ties_2000").round_floor() == 0          # a build with an empty refinement
    assert IC.case("all_A_600").round_floor() == 6 and IC.case("period_AGT_700").round_floor() == 7
    assert any(int(c.hist.max()) * 2 > c.N for c in cs)                                               # one bucket with more than half of everything
    c = IC.case("copies_3x700")
    assert c.N - c.tied < 100                                                                         # all but a few dozen suffixes tied
    assert {64, 66, 74} <= {c.n for c in cs} and min(c.n for c in cs) == 64
    for name in ("all_A_40", "all_A_600", "all_T_33"):
        assert IC.case(name).k_pad == IC.case(name).n // 2 + 1
    # a real suffix whose key equals a padding suffix's zero-filled key, for every length of the T run
    c = IC.case("padding_key_ties")
    assert c.k_pad == 32
    for m in range(1, 32):
        same = np.nonzero(c.keys == c.keys[c.N - m])[0]                                               # the padding suffix T^m
        assert (same < c.n).any(), m


def test_cases_reach_the_group_and_piece_paths():
    """with the sa_chunk / sa_piece values the GPU test uses (Case.builds)"""
    three_groups = oversize = skipped = two_pad_pieces = empty_piece = crowded_piece = later_tied_group = 0
    for name in IC.NAMES:
        c = IC.case(name)
        for chunk, piece in c.builds():
            groups = c.bucket_groups(chunk)
            live = [g for g in groups if g[2] > 0]
            assert sum(g[2] for g in groups) == c.N and groups[0][0] == 0 and groups[-1][1] == 256
            three_groups += len(live) >= 3
            oversize += any(e == b + 1 and tot > chunk for b, e, tot in groups)
            skipped += any(tot == 0 for _, _, tot in groups)
            per_piece = c.pieces(piece)
            assert sum(per_piece) == c.k_pad
            two_pad_pieces += sum(1 for p in per_piece if p) >= 2
            empty_piece += len(per_piece) > 1 and 0 in per_piece
            crowded_piece += len(per_piece) > 1 and max(per_piece) >= 2
            # tied suffixes in a group behind the first: their slots are offset and collected as a second part
            cnt = dict(zip(*np.unique(c.keys, return_counts=True)))
            tied_bucket = {int(k) >> 56 for k, v in cnt.items() if v > 1}
            later_tied_group += sum(1 for b, e, tot in live if any(b <= t < e for t in tied_bucket)) >= 2
        d = c.stats()
        assert d["groups"] == 1 and d["pieces"] == 1 and d["pad_pieces"] == 1 and d["largest_group"] == c.N       # the defaults: one group, one piece
    assert min(three_groups, oversize, skipped, two_pad_pieces, empty_piece, crowded_piece, later_tied_group) >= 1, \
        (three_groups, oversize, skipped, two_pad_pieces, empty_piece, crowded_piece, later_tied_group)


# ---- the P-RMI cases of tests/test_gpu_prmi.py ---------------------------------------------------------------------------------------------------
def _counts(name):
    fwd, bits, _ = IC.PRMI[name]
    text, sa = hostapi.build_sa(fwd)
    return text, sa, bits, IC.leaf_counts(entry_keys(text, sa), bits)


def test_prmi_small_counts_case_has_its_counts():
    _, _, _, c = _counts("small_counts")
    assert c.min() >= 4 and c.max() == 30 and (c == 10).any() and ((c > 1) & (c <= 9)).any()
    assert IC.third_layer_records(c, 1)[c <= 9].sum() == 0 and set(IC.third_layer_records(c, 1)[c == 10]) == {1} and set(IC.third_layer_records(c, 9)[c == 30]) == {2}
    assert IC.third_layer_records(c, 10)[c == 10].sum() == 0                                          # at the threshold: a plain leaf


def test_prmi_sparse_case_skips_empty_leaves_between_routed_ones():
    _, _, bits, c = _counts("more_leaves_than_keys")
    assert c.sum() == 128 and (c == 0).mean() > 0.99
    routed = np.nonzero(IC.third_layer_records(c, 9))[0]
    assert routed.size >= 2 and (c[routed[0] + 1:routed[1]] == 0).any()


def test_third_layer_record_rule_rounds_half_away_from_zero():
    assert IC.third_layer_records([9, 10, 29, 30, 49, 50, 1000, 1001], 1).tolist() == [0, 1, 1, 2, 2, 3, 50, 50]
    assert IC.third_layer_records([1000, 1001], 1000).tolist() == [0, 50]


@pytest.mark.parametrize("name", list(IC.PRMI))
def test_host_trainer_bounds_cover_every_key(name):
    text, sa, bits, c = _counts(name)
    thresholds = IC.PRMI[name][2] or IC.thresholds_at_a_count(c)
    for t in thresholds:
        l1, l2 = hostapi.train_prmi(text, sa, bits=bits, partial_threshold=t)
        routed = (l2["err"] >> np.uint64(63)).astype(bool)
        assert np.array_equal(routed, IC.third_layer_records(c, t) > 0), (name, t)
        assert l1.shape[0] == IC.third_layer_records(c, t).sum()
        n = sa.shape[0]
        prmi_bounds_cover(text, sa, l1, l2, range(n) if n <= 1000 else np.random.default_rng(t).integers(0, n, size=1000))
