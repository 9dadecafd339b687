"""P-RMI training on the device (meme_prmi_train_device) against the host trainer: the two parameter tables must be equal
bit for bit (same double arithmetic), for models without and with a partial third layer."""
import numpy as np
import pytest
import torch

import index_cases as IC
from common import entry_keys
from pymeme import hipapi, hostapi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hipapi.Context(0)
    yield c
    c.close()


def _first_difference(name, got, want):
    same = got.view(np.uint64).reshape(-1, 3) == want.view(np.uint64).reshape(-1, 3)
    if not same.all():
        bad = np.nonzero(~same.all(axis=1))[0]
        raise AssertionError("%s: %d of %d records differ, first %d: %r vs %r" % (name, bad.size, want.shape[0], bad[0], got[bad[0]], want[bad[0]]))


def _stage(ctx, fwd):
    """host text and suffix array of the strand, their 32-base keys, and the staged entries on the device"""
    text, sa = hostapi.build_sa(fwd)
    n = int(text.shape[0])
    dev = torch.device("cuda", 0)
    d_text = torch.from_numpy(text).to(dev)
    d_sa = torch.from_numpy(sa.view(np.int64)).to(dev)
    d_pos5 = hipapi.pos5_from_sa_torch(ctx, d_sa, n)
    d_pac, d_ent = hipapi.stage_entries_torch(ctx, n, d_text, d_pos5)
    return text, sa, entry_keys(text, sa), d_ent


def _train_both(ctx, staged, bits, threshold):
    """both trainers; the device's tables (second layer, third layer) once they equal the host's bit for bit"""
    text, sa, _, d_ent = staged
    n = int(text.shape[0])
    l1, l2 = hostapi.train_prmi(text, sa, bits=bits, partial_threshold=threshold)
    d_l2, n_l2, d_l1, n_l1 = hipapi.train_prmi_device(ctx, d_ent, n, bits, threshold)
    g2 = d_l2.cpu().numpy().view(hostapi.RMI_DTYPE)
    g1 = d_l1.cpu().numpy().view(hostapi.RMI_DTYPE)[:n_l1]
    if n_l1 == 0 and l1.shape[0] == 1:
        assert not l1.view(np.uint64).any()                   # the host trainer pads an empty third layer with one zero record
        l1 = l1[:0]
    assert n_l2 == l2.shape[0] and n_l1 == l1.shape[0], (n_l2, l2.shape, n_l1, l1.shape)
    _first_difference("second layer", g2, l2)
    _first_difference("third layer", g1, l1)
    return g2, g1


def _compare(ctx, fwd, bits, threshold=1000):
    return _train_both(ctx, _stage(ctx, fwd), bits, threshold)[1].shape[0]


def _routed(l2):
    return (l2["err"] >> np.uint64(63)).astype(bool)


def test_plain_leaves(ctx):
    assert _compare(ctx, synth.make_genome(300_000, seed=5, repeat_frac=0.05), bits=16) == 0


def test_partial_third_layer_everywhere(ctx):
    # 2^8 leaves over 800 k keys: every leaf is beyond the threshold and routes into third-layer records
    assert _compare(ctx, synth.make_genome(400_000, seed=6, repeat_frac=0.1, n_dups=6, dup_len=2000), bits=8) > 30000


def test_mixed_and_equal_key_runs(ctx):
    # homopolymers and exact duplicates: long runs of equal 32-base keys, leaves whose keys are all identical, empty leaves
    fwd = synth.make_genome(500_000, seed=7, repeat_frac=0.2, repeat_len=300, n_families=3, divergence=0.0, n_dups=12, dup_len=4000, poly_runs=10)
    fwd[1000:9000] = 0                                          # 8 000 A in a row (and as many T on the other strand)
    assert _compare(ctx, fwd, bits=14, threshold=200) > 0
    # That genome has runs of equal keys inside leaves, but at 2^14 leaves no routed leaf whose keys are ALL equal (every run of T inside the text ends, and the
    # suffixes T^j X of its end share the leaf) and no empty leaf: 68 routed leaves, none empty.  A text that has both, asserted from the host keys: 300 A at
    # the start of the strand are 300 T at the end of the text, whose suffixes all have the key T^32.
    fwd, bits, (threshold,) = IC.PRMI["equal_key_leaf"]
    staged = _stage(ctx, fwd)
    keys = staged[2]
    counts = IC.leaf_counts(keys, bits)
    routed = IC.third_layer_records(counts, threshold) > 0
    start = np.concatenate([[0], np.cumsum(counts)])
    assert any(keys[start[m]] == keys[start[m + 1] - 1] for m in np.nonzero(routed)[0])     # a routed leaf whose keys are all equal
    empty = counts == 0
    assert (empty[1:] & routed[:-1]).any() or (empty[:-1] & routed[1:]).any()               # an empty leaf next to a routed one
    l2, l1 = _train_both(ctx, staged, bits, threshold)
    assert np.array_equal(_routed(l2), routed) and l1.shape[0] > 0


def test_low_threshold_small_text(ctx):
    rng = np.random.default_rng(8)
    assert _compare(ctx, rng.integers(0, 4, size=5000).astype(np.uint8), bits=4, threshold=50) > 0


# ---- the count edges (tests/index_cases.py; the counts themselves are asserted without a GPU by tests/test_index_cases.py) -----------------------------
def test_threshold_at_a_leafs_count(ctx):
    """c > threshold at c == threshold: the leaf stays plain with its own count as the threshold and routes with one less, bit 63 of its record says which"""
    fwd, bits, _ = IC.PRMI["threshold_at_count"]
    staged = _stage(ctx, fwd)
    counts = IC.leaf_counts(staged[2], bits)
    m = IC.leaf_at_the_threshold(counts)
    at, below = IC.thresholds_at_a_count(counts)
    assert at == counts[m] and below == at - 1
    plain, _ = _train_both(ctx, staged, bits, at)
    routes, l1 = _train_both(ctx, staged, bits, below)
    assert not _routed(plain)[m] and _routed(routes)[m]
    assert np.array_equal(_routed(plain), counts > at) and np.array_equal(_routed(routes), counts >= at)
    assert l1.shape[0] == IC.third_layer_records(counts, below).sum()


@pytest.mark.parametrize("threshold", IC.PRMI["small_counts"][2])
def test_small_counts_beyond_the_threshold(ctx, threshold):
    """count / 20 rounds to no record for up to 9 keys (the leaf is fitted as a plain one although it is beyond the threshold), to one for 10, to two for 30"""
    fwd, bits, _ = IC.PRMI["small_counts"]
    staged = _stage(ctx, fwd)
    counts = IC.leaf_counts(staged[2], bits)
    recs = IC.third_layer_records(counts, threshold)
    if threshold == 1:
        assert ((counts > threshold) & (counts <= 9)).any() and recs[counts <= 9].sum() == 0
    assert (counts == 10).any() and (counts == 30).any() and set(recs[counts == 30]) == {2}
    assert set(recs[counts == 10]) == ({1} if threshold < 10 else {0})
    l2, l1 = _train_both(ctx, staged, bits, threshold)
    assert np.array_equal(_routed(l2), recs > 0) and l1.shape[0] == recs.sum()
    err = l2["err"][recs > 0]
    assert np.array_equal(err & np.uint64(0xffffffff), recs[recs > 0].astype(np.uint64))                       # records of each routed leaf ...
    assert np.array_equal((err >> np.uint64(32)) & np.uint64(0x7fffffff), (np.cumsum(recs) - recs)[recs > 0].astype(np.uint64))   # ... and where they start


def test_one_bit(ctx):
    fwd, bits, (threshold,) = IC.PRMI["one_bit"]
    l2, l1 = _train_both(ctx, _stage(ctx, fwd), bits, threshold)
    assert l2.shape[0] == 2 and _routed(l2).all() and l1.shape[0] == 250


def test_more_leaves_than_keys(ctx):
    """2^14 leaves over 128 keys: nearly every leaf is empty, and the search of a third-layer record for its leaf has to pass empty and plain leaves"""
    fwd, bits, (threshold,) = IC.PRMI["more_leaves_than_keys"]
    staged = _stage(ctx, fwd)
    counts = IC.leaf_counts(staged[2], bits)
    assert counts.sum() == 128 and (counts == 0).mean() > 0.99
    recs = IC.third_layer_records(counts, threshold)
    routed = np.nonzero(recs)[0]
    assert routed.size >= 2 and (counts[routed[0] + 1:routed[1]] == 0).any()
    l2, l1 = _train_both(ctx, staged, bits, threshold)
    assert np.array_equal(np.nonzero(_routed(l2))[0], routed) and l1.shape[0] == recs.sum()


def test_capacity_protocol(ctx):
    """room for one record less than needed: MEME_E_CAPACITY and the number needed; the retry with that room gives the host's tables"""
    import ctypes as C
    fwd, bits, _ = IC.PRMI["small_counts"]
    staged = _stage(ctx, fwd)
    text, sa, keys, d_ent = staged
    n = int(text.shape[0])
    total = int(IC.third_layer_records(IC.leaf_counts(keys, bits), 9).sum())
    assert total >= 2
    l1, l2 = hostapi.train_prmi(text, sa, bits=bits, partial_threshold=9)
    dev = d_ent.device
    d_l2 = torch.zeros((1 << bits) * 24, dtype=torch.uint8, device=dev)
    d_l1 = torch.zeros(total * 24, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    cnt = C.c_int64(-1)
    args = (C.c_void_p(ctx.h), C.c_void_p(d_ent.data_ptr()), C.c_int64(n), C.c_int(bits), C.c_int(9), C.c_void_p(d_l2.data_ptr()), C.c_void_p(d_l1.data_ptr()))
    E_CAPACITY = -4
    assert hipapi.lib().meme_prmi_train_device(*args, C.c_int64(total - 1), C.byref(cnt)) == E_CAPACITY and cnt.value == total
    ctx.sync()
    assert not d_l1.any() and not d_l2.any()                  # nothing is written by the refused call
    cnt = C.c_int64(-1)
    assert hipapi.lib().meme_prmi_train_device(*args, C.c_int64(total), C.byref(cnt)) == 0 and cnt.value == total
    ctx.sync()
    _first_difference("second layer", d_l2.cpu().numpy().view(hostapi.RMI_DTYPE), l2)
    _first_difference("third layer", d_l1.cpu().numpy().view(hostapi.RMI_DTYPE), l1)
