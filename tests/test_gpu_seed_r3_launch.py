"""Tier 0 of seeding with the third round in a k_seed launch of its own (tuning seed_r3_split, default 1), its searches first compared on the
64-bit keys alone: every case against the oracle SMEM by SMEM and hit by hit, and against the single launch (seed_r3_split = 0) -- same
SMEMs, same hits, same number of searches."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle_py as O
from common import build_index
from pymeme import hipapi, synth

pytestmark = pytest.mark.gpu

MAX_INTV = 20          # default max_mem_intv: a third-round interval of this many suffixes is not emitted


def _rc(x):
    return (3 - x[::-1]).astype(np.uint8)


def _batch(reads):
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in reads])
    return np.concatenate(reads).astype(np.uint8), off


def _d2h(ptr, count, dtype):
    """`count` items of a seeding result's device array"""
    out = np.empty(count, dtype=dtype)
    if count:
        cp = hipapi.lib().hipMemcpy                    # the HIP runtime the library runs on
        cp.restype, cp.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert cp(out.ctypes.data, ptr, out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


def _fixed(reads, L):
    return reads.reshape(-1), np.arange(0, (reads.shape[0] + 1) * L, L, dtype=np.int64)


class Case:
    """A genome with its index on disk, the oracle's view of it and a ctx that holds it."""

    def __init__(self, tmp, g, name):
        fa = os.path.join(str(tmp), name + ".fa")
        synth.write_fasta(fa, g, contigs=2)
        self.g = g
        self.prefix = build_index(fa, bits=12)
        self.idx = O.load_index_files(self.prefix)
        self.ctx = hipapi.Context(0)
        self.ctx.load_index_files(self.prefix)

    def close(self):
        self.ctx.close()

    def run(self, reads, off, opt, split):
        c = self.ctx
        """(seed dump, the round-3 launch's counts + the call's searches and windows, k_seed launches) of one device-resident seeding call"""
        c.set_tuning("seed_r3_split", split)
        n = off.shape[0] - 1
        d_reads = torch.from_numpy(np.ascontiguousarray(reads, dtype=np.uint8)).cuda()
        d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).cuda()
        torch.cuda.synchronize()
        res = c.seed_batch_device(d_reads.data_ptr(), d_off.data_ptr(), n, int(off[-1]), opt)
        c.sync()
        smems, hits = _d2h(res.d_smems, res.total_smems, hipapi.MEM_TL), _d2h(res.d_hits, res.total_hits, np.uint64)
        smem_off, hit_off = _d2h(res.d_smem_off, n + 1, np.int64), _d2h(res.d_hit_off, n + 1, np.int64)
        slots, counts, hl = hipapi.smems_to_slots(smems, smem_off, hits, hit_off)
        tm = c.timings()
        r = dict(c.debug_seed_r3_counts(), searches=int(res.searches), windows=int(tm.seed_windows))
        return O.format_seed_dump(slots, counts, hl), r, int(tm.seed_launches)

    def check(self, reads, off, min_seed_len=19, max_mem_intv=MAX_INTV, rounds=3, tag=None):
        """oracle == single launch == two launches; returns the counts of the two-launch call"""
        p = O.default_seed_params(rounds)
        opt = hipapi.default_seed_opt(rounds=rounds)
        p.min_seed_len = opt.min_seed_len = min_seed_len
        p.split_len = opt.split_len = int(min_seed_len * 1.5 + .499)
        p.max_mem_intv = opt.max_mem_intv = max_mem_intv
        sm, ns, hits, nh, _ = O.seed_batch(self.idx, reads, off, params=p, smem_cap=1024, hit_cap=1 << 16, threads=0)
        want = O.format_seed_dump(sm, ns, hits)
        d0, r0, l0 = self.run(reads, off, opt, 0)
        d1, r1, l1 = self.run(reads, off, opt, 1)
        assert not r0["split"] and r0["repeats"] == 0, tag
        assert d0 == want, tag
        assert d1 == want, tag
        assert r1["searches"] == r0["searches"], tag
        r1["launches"], r1["launches_single"], r1["windows_single"] = l1, l0, r0["windows"]
        return r1


# ---- genomes ---------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("c19", "c20", "c21", "k31", "k32", "k33", "k64")


def _family_genome(seed=5):
    """300 kbp of random bases holding families of a repeated unit.  c19 / c20 / c21: that many identical copies of a 200-base unit (either
    side of max_mem_intv).  k31 / k32 / k33 / k64: 25 copies that agree over exactly that many bases -- random flanks, the shared piece, then
    a base that copy 0 alone has -- so a query cut from copy 0 at the piece's start shares exactly k bases with 24 other suffixes.
    Returns (genome, {family: (start of copy 0's unit or shared piece, its length)})."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, 300_000, dtype=np.uint8)
    where = {}
    slot = iter(range(2000, 298_000, 1000))       # planting sites, 1000 bases apart
    for fam, copies in (("c19", 19), ("c20", 20), ("c21", 21)):
        unit = rng.integers(0, 4, 200, dtype=np.uint8)
        for i in range(copies):
            at = next(slot)
            g[at:at + 200] = unit
            if i == 0:
                where[fam] = (at, 200)
    for fam, k in (("k31", 31), ("k32", 32), ("k33", 33), ("k64", 64)):
        piece = rng.integers(0, 4, k, dtype=np.uint8)
        for i in range(25):
            at = next(slot) + 200
            g[at:at + k] = piece
            g[at + k] = 0 if i == 0 else 1 + i % 3                         # copy 0 continues with A, no other does
            if i == 0:
                where[fam] = (at, k)
    return g, where


def _cuts(g, at, span, L, lo=-45, hi=5, rcs=True):
    """reads of L bases starting at at + d for d in [lo, hi): the piece at `at` lies at every offset a third-round pivot can take"""
    out = []
    for d in range(lo, hi):
        r = g[at + d:at + d + L].copy()
        out.append(r)
        if rcs and d % 5 == 0:
            out.append(_rc(r))
    return out


@pytest.fixture(scope="module")
def fam(tmp_path_factory):
    g, where = _family_genome()
    c = Case(tmp_path_factory.mktemp("fam"), g, "fam")
    c.where = where
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    g = np.random.default_rng(23).integers(0, 4, 200_000, dtype=np.uint8)      # repeat-free
    c = Case(tmp_path_factory.mktemp("plain"), g, "plain")
    yield c
    c.close()


@pytest.fixture(scope="module")
def ends(tmp_path_factory):
    """100 kbp whose last 200 bases are a unit U and whose first 200 are rc(U) -- so the fwd+rc text begins with rc(U) and ENDS with U -- with
    22 more copies of U inside: the suffixes of fewer than 32 bases, and of 32 bases up to a read length, at the text's end sort into the runs and
    windows of the queries cut from the copies; the same at the text's start for their reverse complements."""
    rng = np.random.default_rng(41)
    g = rng.integers(0, 4, 100_000, dtype=np.uint8)
    unit = rng.integers(0, 4, 200, dtype=np.uint8)
    for i in range(22):
        g[3000 + 4000 * i:3200 + 4000 * i] = unit
    g[:200] = _rc(unit)
    g[-200:] = unit
    c = Case(tmp_path_factory.mktemp("ends"), g, "ends")
    yield c
    c.close()


# ---- random reads ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [4, 32])
@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("L", [150, 250])
def test_random_reads(fam, L, defer, lanes):
    """seed_blocks = 1: one workgroup, every group takes many reads in both launches"""
    reads, _, _ = synth.make_reads(fam.g, 1500, L, seed=300 + L, n_frac=0.05, exact_frac=0.2)
    c = fam.ctx
    try:
        c.set_tuning("group_lanes", lanes); c.set_tuning("seed_defer", defer); c.set_tuning("seed_blocks", 1)
        r = fam.check(*_fixed(reads, L), tag=(L, defer, lanes))
        assert r["split"]
    finally:
        c.set_tuning("group_lanes", 4); c.set_tuning("seed_defer", 1); c.set_tuning("seed_blocks", 0)


# ---- the cap's boundaries --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_cap_boundaries(fam, family):
    """Reads cut from copy 0 of a family, its unit or shared piece at every offset from 45 bases into the read to 5 before it, both strands.
    Where at least max_mem_intv suffixes share 32 bases with a query and the query is longer (c20: exactly max_mem_intv; c21; k33 and k64: 25)
    the keys cannot decide the search and it runs again in full: the counter says so.  k32: 25 suffixes share exactly 32 bases -- the run at the
    capped level 32 reaches max_mem_intv, the search runs again and finds the same.  c19: 19 suffixes, and k31: 25 suffixes sharing 31 bases,
    are decided by the keys, and nothing else in the random genome around them comes near 20 suffixes sharing 32 bases: no search runs twice."""
    at, span = fam.where[family]
    r = fam.check(*_batch(_cuts(fam.g, at, span, 150) + _cuts(fam.g, at, span, 60, rcs=False)), tag=family)
    assert r["split"]
    if family in ("c19", "k31"):
        assert r["repeats"] == 0
    else:                                                          # the boundary itself: cnt >= max_mem_intv at L >= 32
        assert r["repeats"] > 0


def test_no_repeat_without_repeats(plain):
    reads, _, _ = synth.make_reads(plain.g, 2000, 150, seed=9, n_frac=0.02, exact_frac=0.3)
    r = plain.check(*_fixed(reads, 150))
    assert r["split"] and r["repeats"] == 0


# ---- text ends -------------------------------------------------------------------------------------------------------------------------
def test_text_ends(ends):
    g = ends.g
    text = ends.idx.text
    n = text.shape[0]
    reads = []
    for at in (3000, 7000, 87000):                                 # copies of the unit inside, with their flanks
        reads += _cuts(g, at, 200, 150, lo=-120, hi=180)
    for L in (150, 100, 64, 40, 33, 32, 31, 25):                   # the text's own ends and the fwd/rc junction
        reads += [text[n - L:].copy(), text[:L].copy(), text[n // 2 - L // 2:n // 2 - L // 2 + L].copy()]
    for d in range(0, 170, 3):                                     # reads running up to, and starting at, both ends
        reads += [text[n - 150 - d:n - d].copy(), text[d:d + 150].copy()]
    r = ends.check(*_batch(reads))
    assert r["split"] and r["repeats"] > 0


# ---- pivots and lengths ----------------------------------------------------------------------------------------------------------------
def test_n_at_pivots_and_short_reads(fam):
    g = fam.g
    rng = np.random.default_rng(3)
    reads = [np.full(150, 4, np.uint8), np.full(19, 4, np.uint8), np.full(41, 4, np.uint8)]     # all N
    sites = [int(x) for x in rng.integers(1000, 290_000, 40)] + [fam.where[f][0] - 10 for f in FAMILIES]
    for at in sites:
        for npos in (0, 19, 20, 21):
            r = g[at:at + 150].copy(); r[npos] = 4; reads.append(r)
        r = g[at:at + 150].copy(); r[[0, 19, 20, 21]] = 4; reads.append(r)
        for L in (19, 20, 21, 39, 40, 41):
            reads.append(g[at + 10:at + 10 + L].copy())
            reads.append(_rc(g[at + 10:at + 10 + L]))
    r = fam.check(*_batch(reads))
    assert r["split"]


# ---- options ---------------------------------------------------------------------------------------------------------------------------
def _family_reads(fam):
    reads = []
    for f in FAMILIES:
        at, span = fam.where[f]
        reads += _cuts(fam.g, at, span, 150, lo=-40, hi=2)
    return _batch(reads)


def test_msl_32_keeps_the_cap_and_33_drops_it(fam):
    """min_seed_len 31: the third round's msl is 32, the last value for which the keys decide every level the walk can stop at; 32: msl 33,
    the round compares in full and nothing is run twice"""
    reads, off = _family_reads(fam)
    r = fam.check(reads, off, min_seed_len=31)
    assert r["split"] and r["repeats"] > 0
    r = fam.check(reads, off, min_seed_len=32)
    assert r["split"] and r["repeats"] == 0


def test_all_families_default_options(fam):
    """the batch of the option tests under the default options; the repeats' windows are counted (the single launch runs no search twice)"""
    reads, off = _family_reads(fam)
    r = fam.check(reads, off)
    assert r["split"] and r["repeats"] > 0
    assert r["windows"] > r["windows_single"]


@pytest.mark.parametrize("kw", [dict(max_mem_intv=0), dict(rounds=2)])
def test_no_second_launch_without_a_third_round(fam, kw):
    reads, off = _family_reads(fam)
    r = fam.check(reads, off, **kw)
    assert not r["split"] and r["repeats"] == 0


# ---- overflow --------------------------------------------------------------------------------------------------------------------------
def test_overflow_in_the_first_launch(tmp_path_factory):
    """A 150-A read against a genome with a 400-A run, and 250-base mosaics of 20-base pieces from 12 loci, with 8 SMEM slots per read: rounds 1-2
    alone overflow them (two rounds, re-seeding inside k_seed: a second launch of the overflow tier), so with three rounds the first launch
    sends them to the overflow list, the second leaves them alone and tier 1 seeds them: same seeds and searches as the single launch."""
    rng = np.random.default_rng(77)
    g = rng.integers(0, 4, 150_000, dtype=np.uint8)
    g[50_000:50_400] = 0
    c = Case(tmp_path_factory.mktemp("ovf"), g, "ovf")
    try:
        reads = [np.zeros(150, np.uint8)]
        for k in range(30):
            reads.append(np.concatenate([g[s:s + 20] for s in rng.integers(1000, 140_000, 12)] + [g[200 + k:210 + k]]))
        reads += [g[s:s + 150].copy() for s in rng.integers(1000, 140_000, 200)]       # and reads that do not overflow, around them
        reads, off = _batch(reads)
        c.ctx.set_tuning("smem_cap", 8)
        c.ctx.set_tuning("seed_defer", 0)
        _, _, launches = c.run(reads, off, hipapi.default_seed_opt(rounds=2), 1)
        assert launches >= 2                                        # k_seed's rounds 1-2 overflow by themselves
        for defer in (0, 1):
            c.ctx.set_tuning("seed_defer", defer)
            r = c.check(reads, off, tag=defer)
            assert r["split"] and r["launches"] >= 2
    finally:
        c.close()


def test_overflow_in_the_second_launch(plain):
    """8 SMEM slots per read: rounds 1-2 of these reads fit (two rounds: no overflow tier runs), the third round's SMEMs do not -- the second launch
    sends the read to the overflow list, and its searches are counted once, by the tier that seeds it"""
    reads, _, _ = synth.make_reads(plain.g, 1500, 150, seed=19, sub_rate=0.005, n_frac=0.0)
    reads, off = _fixed(reads, 150)
    c = plain.ctx
    try:
        c.set_tuning("smem_cap", 8)
        for defer in (0, 1):
            c.set_tuning("seed_defer", defer)
            _, _, l2 = plain.run(reads, off, hipapi.default_seed_opt(rounds=2), 1)
            assert l2 == 1                                          # (at most one SMEM per error and a few re-seeded ones: rounds 1-2 fit)
            r = plain.check(reads, off, tag=defer)
            assert r["split"] and r["launches"] >= 2
    finally:
        c.set_tuning("smem_cap", 128); c.set_tuning("seed_defer", 1)
