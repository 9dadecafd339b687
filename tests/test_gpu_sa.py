"""Device-side suffix-array construction (meme_sa_build_device) against the host builder, whose output is verified
byte-identical to `bwa-meme index -a meme` (tests/test_ref_live.py, where the compiled reference is available)."""
import numpy as np
import pytest

import index_cases as IC
from pymeme import hipapi, hostapi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hipapi.Context(0)
    yield c
    c.close()


def _check(ctx, fwd):
    text, sa = hostapi.build_sa(fwd)
    t2 = hipapi.fwd_rc_text(fwd)
    assert np.array_equal(text, t2)
    _, d_sa = hipapi.build_sa_device(ctx, t2)
    got = d_sa.cpu().numpy().view(np.uint64)
    if not np.array_equal(got, sa):
        bad = np.nonzero(got != sa)[0]
        raise AssertionError("suffix arrays differ at %d of %d slots, first at %d: %d vs %d" % (bad.size, sa.size, bad[0], got[bad[0]], sa[bad[0]]))


def test_random_genome(ctx):
    _check(ctx, synth.make_genome(200_000, seed=3, repeat_frac=0.0, n_dups=0, poly_runs=0))


def test_repeat_rich_genome(ctx):
    # long exact duplicates and homopolymer runs: many rounds of prefix doubling, ties that end at the end of the text
    _check(ctx, synth.make_genome(600_000, seed=31, repeat_frac=0.2, repeat_len=300, n_families=4, divergence=0.02, n_dups=10,
                                  dup_len=3000, poly_runs=8))


@pytest.mark.parametrize("tail", ["A", "T", "ACGT"])
def test_text_ends_in_a_run(ctx, tail):
    # the suffixes of a homopolymer at the very end of the text differ only in their length: shorter sorts first
    rng = np.random.default_rng(5)
    body = rng.integers(0, 4, size=4000).astype(np.uint8)
    codes = {"A": 0, "C": 1, "G": 2, "T": 3}
    t = np.array([codes[c] for c in tail] * (120 // len(tail)), np.uint8)
    # fwd + rc ends with the reverse complement of the START of the forward strand: put the run there too
    rc_t = (3 - t[::-1]).astype(np.uint8)
    _check(ctx, np.concatenate([rc_t, body, t]))


def test_smallest_text(ctx):
    _check(ctx, np.array([0, 1, 2, 3] * 8, np.uint8))           # 64 suffixes


def test_midsize_genome_equals_host_builder(ctx):
    _check(ctx, synth.make_genome(16_000_000, seed=91, repeat_frac=0.05, repeat_len=400, n_families=8, divergence=0.03,
                                  n_dups=20, dup_len=5000, poly_runs=6))


# ---- the case texts of tests/index_cases.py: the definition of the array, and the paths only big texts take forced with sa_chunk / sa_piece -------------
def _build(ctx, c, chunk, piece):
    """one build of case c with these tuning keys: the array against the definition and the host builder, the build's own account against the prediction"""
    import torch
    ctx.set_tuning("sa_chunk", chunk)
    ctx.set_tuning("sa_piece", piece)
    d_text, d_sa = hipapi.build_sa_device(ctx, c.text)
    got = d_sa.cpu().numpy().view(np.uint64)
    what = "%s, sa_chunk %d, sa_piece %d" % (c.name, chunk, piece)
    assert torch.equal(d_text.cpu(), torch.from_numpy(c.text)), "%s: the text on the device changed" % what
    stats = ctx.debug_sa_stats()
    print(what, stats, "round floor", c.round_floor())
    for name, want in (("definition", c.sa), ("host builder", hostapi.build_sa(c.fwd)[1])):
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError("%s: differs from the %s at %d of %d slots, first at %d: %d vs %d; %r" % (what, name, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]], stats))
    rounds = stats.pop("rounds")
    assert stats == c.stats(chunk, piece), what
    assert rounds >= c.round_floor() and (rounds == 0) == (c.tied == 0), (what, rounds, c.round_floor())
    return got


@pytest.mark.parametrize("name", IC.NAMES)
def test_case_text_at_every_group_and_piece_size(name):
    c = IC.case(name)
    ctx = hipapi.Context(0)                                   # a ctx of its own: the keys do not leak into the other tests
    try:
        for chunk, piece in c.builds():
            _build(ctx, c, chunk, piece)
    finally:
        ctx.close()


def test_same_array_whatever_the_keys_between_two_builds():
    c = IC.case("ends_in_T")
    ctx = hipapi.Context(0)
    try:
        first = _build(ctx, c, IC.DEFAULT_CHUNK, IC.DEFAULT_PIECE)
        assert np.array_equal(_build(ctx, c, 1, 64), first)
        assert np.array_equal(_build(ctx, c, IC.DEFAULT_CHUNK, IC.DEFAULT_PIECE), first)
        ctx.set_tuning("sa_chunk", 0)                         # clamped to 1
        ctx.set_tuning("sa_piece", -5)
        hipapi.build_sa_device(ctx, c.text)
        assert ctx.debug_sa_stats()["groups"] == c.stats(1, 1)["groups"] and ctx.debug_sa_stats()["pieces"] == c.N
    finally:
        ctx.close()


def test_bad_arguments_are_refused_and_the_ctx_builds_on():
    import ctypes as C
    import torch
    c = IC.case("smallest")
    ctx = hipapi.Context(0)
    try:
        with pytest.raises(hipapi.MemeError, match="-5"):     # MEME_E_STATE: nothing built yet
            ctx.debug_sa_stats()
        dev = torch.device("cuda", 0)
        d_text = torch.from_numpy(c.text).to(dev)
        d_sa = torch.full((c.n,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        L, h = hipapi.lib(), C.c_void_p(ctx.h)
        E_ARG = -2
        assert L.meme_sa_build_device(h, C.c_void_p(d_text.data_ptr()), C.c_int64(63), C.c_void_p(d_sa.data_ptr())) == E_ARG
        assert L.meme_sa_build_device(h, C.c_void_p(0), C.c_int64(c.n), C.c_void_p(d_sa.data_ptr())) == E_ARG
        assert L.meme_sa_build_device(h, C.c_void_p(d_text.data_ptr()), C.c_int64(c.n), C.c_void_p(0)) == E_ARG
        assert L.meme_sa_build_device(C.c_void_p(0), C.c_void_p(d_text.data_ptr()), C.c_int64(c.n), C.c_void_p(d_sa.data_ptr())) == E_ARG
        ctx.sync()
        assert bool((d_sa == -1).all())                       # a refused call writes nothing
        with pytest.raises(hipapi.MemeError, match="-5"):
            ctx.debug_sa_stats()
        _build(ctx, c, IC.DEFAULT_CHUNK, IC.DEFAULT_PIECE)
    finally:
        ctx.close()
