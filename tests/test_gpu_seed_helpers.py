"""The helper kernels of a seeding call -- the read packer, the offsets scan and the hit gather -- on the small g1 index: the packed image word for
word against a numpy restatement of its layout, and the seeds against the oracle with the helpers' grids capped (helper_blocks), so that their loops go
round several times on test-sized batches."""
import os

import numpy as np
import pytest

import oracle_py as O
from common import GOLDEN, build_index
from pymeme import hipapi
from test_gpu_seed import _mixed_length_batch

gpu = pytest.mark.gpu


# ---- the packed layout, restated -------------------------------------------------------------------------------------------------------------------------
def pack_image(reads, off):
    """Per read fw[W] rc[W] nfw[MW] nrc[MW] len | hasN << 31: 2 bits per base, first base in the top bits of a word, a byte above 3 is an N and packed
    as A on both strands; mask bit j of word m = base 64 m + j of that strand is an N; W = ceil(maxlen / 32) + 2, MW = ceil(maxlen / 64)."""
    n = off.shape[0] - 1
    lens = np.diff(off)
    maxlen = max(int(lens.max()) if n else 1, 1)
    W, MW = (maxlen + 31) // 32 + 2, (maxlen + 63) // 64
    out = np.zeros((n, 2 * W + 2 * MW + 1), np.uint64)
    csh = (np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64))[None, :]
    msh = np.arange(64, dtype=np.uint64)[None, :]
    for r in range(n):
        b = reads[off[r]:off[r + 1]]
        isn = b > 3
        strands = ((np.where(isn, 0, b), isn), (np.where(isn[::-1], 0, 3 - np.minimum(b[::-1], 3)), isn[::-1]))
        for s, (codes, mask) in enumerate(strands):
            c = np.zeros(32 * W, np.uint64)
            c[:codes.shape[0]] = codes
            out[r, s * W:(s + 1) * W] = np.bitwise_or.reduce(c.reshape(W, 32) << csh, axis=1)
            m = np.zeros(64 * MW, np.uint64)
            m[:mask.shape[0]] = mask
            out[r, 2 * W + s * MW:2 * W + (s + 1) * MW] = np.bitwise_or.reduce(m.reshape(MW, 64) << msh, axis=1)
        out[r, -1] = b.shape[0] | (int(isn.any()) << 31)
    return out, W, MW


def _pack_batch(nreads, tail, seed=5):
    """`nreads` reads for the packer.  The first ones are the listed cases -- every word count 1..16 with lengths 32 c - 31 and 32 c, lengths 1..18, an
    empty read, N at base 0 / 31 / 32 / 63 / 64 / the last base, a read that is all N, bytes above 4 -- the rest random lengths 1..500 with an N in one
    of 20; the order is shuffled, so read starts fall on all four byte phases, and the last read is sized so that the buffer has `tail` = total % 4."""
    rng = np.random.default_rng(seed)
    lens = [32 * c - 31 for c in range(1, 17)] + [min(500, 32 * c) for c in range(1, 17)] + list(range(1, 19)) + [0]
    cases = [rng.integers(0, 4, size=l).astype(np.uint8) for l in lens]
    for pos in (0, 31, 32, 63, 64, 149):
        r = rng.integers(0, 4, size=150).astype(np.uint8)
        r[pos] = 4
        cases.append(r)
    for l in (1, 33, 64, 65, 129, 500):                     # N at the last base of reads that end at and beside word boundaries
        r = rng.integers(0, 4, size=l).astype(np.uint8)
        r[-1] = 4
        cases.append(r)
    cases.append(np.full(150, 4, np.uint8))
    cases.append(np.full(77, 4, np.uint8))
    r = rng.integers(0, 4, size=200).astype(np.uint8)
    r[[3, 70, 199]] = [5, 255, 128]                         # any byte above 3 is an N
    cases.append(r)
    if nreads <= len(cases):
        pick = rng.choice(len(cases), size=nreads, replace=False)
        reads = [cases[k] for k in pick]
        if nreads > 1:
            reads[0] = cases[31]                            # the 500-base read stays in: the layout has its 16 + 2 words
    else:
        reads = list(cases)
        while len(reads) < nreads:
            r = rng.integers(0, 4, size=int(rng.integers(1, 501))).astype(np.uint8)
            if rng.random() < 0.05:
                r[rng.integers(0, r.shape[0], size=int(rng.integers(1, 4)))] = 4
            reads.append(r)
    order = rng.permutation(len(reads))
    reads = [reads[k] for k in order]
    total = sum(r.shape[0] for r in reads)
    grow = (tail - total) % 4                               # the last read ends at the buffer's last byte
    reads[-1] = np.concatenate([reads[-1], rng.integers(0, 4, size=grow).astype(np.uint8)])[:500] if reads[-1].shape[0] + grow <= 500 \
        else reads[-1][:reads[-1].shape[0] - (4 - grow)]
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in reads])
    flat = np.concatenate(reads) if off[-1] else np.zeros(0, np.uint8)
    return flat, off


def test_pack_batch_holds_the_listed_cases():
    reads, off = _pack_batch(1600, 1)
    lens = np.diff(off)
    assert off.shape[0] - 1 == 1600 and off[-1] % 4 == 1 and lens.max() == 500
    assert set(range(0, 19)) <= set(lens.tolist())
    assert all(32 * c - 31 in lens and min(500, 32 * c) in lens for c in range(1, 17))
    assert set((off[:-1] % 4).tolist()) == {0, 1, 2, 3}
    first = [set(), set()]
    for r in range(1600):
        b = reads[off[r]:off[r + 1]]
        pos = np.flatnonzero(b > 3)
        first[0] |= set(pos.tolist())
        first[1] |= set((b.shape[0] - 1 - pos).tolist())
    assert {0, 31, 32, 63, 64} <= first[0] and 0 in first[1]
    assert any(lens[r] > 0 and (reads[off[r]:off[r + 1]] > 3).all() for r in range(1600))
    for tail in (1, 2, 3):
        for n in (1, 31, 32, 33):
            _, o = _pack_batch(n, tail)
            assert o.shape[0] - 1 == n and o[-1] % 4 == tail and np.diff(o).max() <= 500


def test_restated_layout_rc_strand_is_fw_strand_of_reverse_complement():
    reads, off = _pack_batch(300, 2)
    n = off.shape[0] - 1
    rc = np.concatenate([np.where(reads[off[r]:off[r + 1]] > 3, reads[off[r]:off[r + 1]], 3 - np.minimum(reads[off[r]:off[r + 1]], 3))[::-1] for r in range(n)])
    a, W, MW = pack_image(reads, off)
    b, _, _ = pack_image(rc, off)
    assert np.array_equal(a[:, W:2 * W], b[:, :W]) and np.array_equal(a[:, :W], b[:, W:2 * W])
    assert np.array_equal(a[:, 2 * W + MW:2 * W + 2 * MW], b[:, 2 * W:2 * W + MW]) and np.array_equal(a[:, -1], b[:, -1])
    # and one read by hand: ACGTN -> fw 00 01 10 11 00, rc of it N A C G T -> 00 00 01 10 11; N masks bit 4 / bit 0
    img, W, MW = pack_image(np.array([0, 1, 2, 3, 4], np.uint8), np.array([0, 5], np.int64))
    assert (W, MW) == (3, 1) and img.shape == (1, 9)
    assert int(img[0, 0]) == 0b0001101100 << 54 and int(img[0, 3]) == 0b0000011011 << 54
    assert int(img[0, 6]) == 1 << 4 and int(img[0, 7]) == 1 and int(img[0, 8]) == 5 | 1 << 31
    assert not img[0, [1, 2, 4, 5]].any()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1():
    return build_index(os.path.join(GOLDEN, "g1.fa"))


@pytest.fixture(scope="module")
def ctx(g1):
    c = hipapi.Context(0)
    c.load_index_files(g1)
    yield c
    c.close()


@gpu
@pytest.mark.parametrize("helper_blocks", [1, 3, 0])
@pytest.mark.parametrize("nreads,tail", [(1, 1), (31, 2), (32, 3), (33, 1), (1600, 2), (1600, 3)])
def test_packed_image_equals_restated_layout(ctx, nreads, tail, helper_blocks):
    reads, off = _pack_batch(nreads, tail)
    want, W, MW = pack_image(reads, off)
    ctx.set_tuning("helper_blocks", helper_blocks)
    try:
        ctx.seed_batch(reads, off)
        got, gW, gMW = ctx.debug_packed_reads()
    finally:
        ctx.set_tuning("helper_blocks", 0)
    assert (gW, gMW) == (W, MW) and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, "first differing (read, word): %s of %d; got %x want %x" % (bad[0], bad.shape[0], got[tuple(bad[0])], want[tuple(bad[0])])


@gpu
def test_packed_image_of_uniform_150_base_reads(ctx):
    """The benchmark's shape: every read 150 bases (32 reads of a wavefront's chunk span 4 800 bytes), one in 50 with an N."""
    rng = np.random.default_rng(11)
    n = 1111
    reads = rng.integers(0, 4, size=150 * n).astype(np.uint8)
    reads[rng.integers(0, reads.shape[0], size=n // 50)] = 4
    off = np.arange(n + 1, dtype=np.int64) * 150
    want, _, _ = pack_image(reads, off)
    for hb in (0, 2):
        ctx.set_tuning("helper_blocks", hb)
        try:
            ctx.seed_batch(reads, off)
            got, _, _ = ctx.debug_packed_reads()
        finally:
            ctx.set_tuning("helper_blocks", 0)
        assert np.array_equal(got, want), hb


_seeds = {}
SMEM_CAP, HIT_CAP = 1024, 1 << 13              # the oracle's room per read of the mixed batch ...
X_SMEM_CAP, X_HIT_CAP = 8192, 1 << 15          # ... and of the reads added here (the 150-A read has thousands of SMEMs)
N_EXTRA = 16


def _seed_batch_and_oracle(g1):
    """The mixed-length batch of test_gpu_seed.py + a 150-A read + reads stitched from short pieces of the genome (more than 16 SMEMs each, hit lists
    longer than 4) + three tandem repeats the genome does not hold (no SMEM at all); the oracle's seeds of it per read, once per module run."""
    if not _seeds:
        reads, off, _ = _mixed_length_batch(g1)
        idx = O.load_index_files(g1)
        g = idx.text[:idx.text.shape[0] // 2]
        extra = [np.zeros(150, np.uint8)]
        rng = np.random.default_rng(77)
        for _ in range(12):
            pos = rng.integers(0, g.shape[0] - 40, size=12)
            extra.append(np.concatenate([g[p:p + int(rng.integers(20, 40))] for p in pos])[:500])
        for rep in (np.array([0, 1], np.uint8), np.array([0, 0, 1], np.uint8), np.array([2, 3, 3, 0], np.uint8)):
            extra.append(np.tile(rep, 60)[:150])
        assert len(extra) == N_EXTRA
        xoff = np.concatenate([[0], np.cumsum([e.shape[0] for e in extra])]).astype(np.int64)
        sm, ns, hits, nh, _ = O.seed_batch(idx, reads, off, smem_cap=SMEM_CAP, hit_cap=HIT_CAP, threads=0)
        xsm, xns, xhits, xnh, _ = O.seed_batch(idx, np.concatenate(extra), xoff, smem_cap=X_SMEM_CAP, hit_cap=X_HIT_CAP, threads=0)
        _seeds.update(reads=np.concatenate([reads] + extra), off=np.concatenate([off, off[-1] + xoff[1:]]),
                      sm=[sm[r, :ns[r]] for r in range(ns.shape[0])] + [xsm[r, :xns[r]] for r in range(N_EXTRA)],
                      hits=[hits[r, :nh[r]] for r in range(ns.shape[0])] + [xhits[r, :xnh[r]] for r in range(N_EXTRA)],
                      caps=(int(ns.max()), int(nh.max()), int(xns.max()), int(xnh.max())))
    return _seeds


def _oracle_dump(S, first, n, hps):
    """The oracle's dump of reads first .. first + n - 1 with at most hps hits kept per SMEM (0: all): the hit list of an SMEM holds its first
    min(count, hps) positions."""
    rows = S["sm"][first:first + n]
    ns = np.array([row.shape[0] for row in rows], np.int32)
    sm = np.zeros((n, max(1, int(ns.max()))), O.MEM_TL_DTYPE)
    hits = []
    for r, row in enumerate(rows):
        sm[r, :ns[r]] = row
        kept, beg = [], 0
        for i in range(int(ns[r])):
            hb, hc = int(row[i]["hitbeg"]), int(row[i]["hitcount"])
            keep = hc if hps == 0 else min(hc, hps)
            kept.append(S["hits"][first + r][hb:hb + keep])
            sm[r, i]["hitbeg"], sm[r, i]["hitcount"] = beg, keep
            beg += keep
        hits.append(np.concatenate(kept) if kept else np.zeros(0, np.uint64))
    return O.format_seed_dump(sm, ns, hits)


def _gpu_dump(c, reads, off, hps):
    smems, smem_off, hits, hit_off = c.seed_batch(reads, off, hipapi.default_seed_opt(hits_per_smem=hps))
    smems = smems.copy()
    if hps:
        smems["hitcount"] = np.minimum(smems["hitcount"], hps)      # (the dump prints hits[hitbeg : hitbeg + hitcount])
    slots, counts, hl = hipapi.smems_to_slots(smems, smem_off, hits, hit_off)
    return O.format_seed_dump(slots, counts, hl)


def test_oracle_handles_the_seed_batch_within_its_caps(g1):
    S = _seed_batch_and_oracle(g1)
    n = S["off"].shape[0] - 1
    ns, nh, xns, xnh = S["caps"]
    assert ns < SMEM_CAP and nh < HIT_CAP and xns < X_SMEM_CAP and xnh < X_HIT_CAP
    counts = np.array([row.shape[0] for row in S["sm"]])
    assert (counts > 16).sum() >= 8 and counts[n - N_EXTRA] > 2048     # several 16-SMEM rounds of a gather group; the 150-A read needs the last tier
    assert sum(int((row["hitcount"] > 4).sum()) for row in S["sm"]) >= 8 and max(int(row["hitcount"].max()) for row in S["sm"] if row.shape[0]) > 16
    assert counts[-3:].sum() == 0                                      # reads without an SMEM at the batch's end
    r = n - N_EXTRA
    assert S["off"][r + 1] - S["off"][r] == 150 and not S["reads"][S["off"][r]:S["off"][r + 1]].any()   # the 150-A read


@gpu
@pytest.mark.parametrize("helper_blocks", [1, 3, 0])
@pytest.mark.parametrize("smem_cap,defer", [(128, 1), (128, 0), (8, 1)])
def test_seeds_equal_oracle_with_small_helper_grids(g1, helper_blocks, smem_cap, defer):
    S = _seed_batch_and_oracle(g1)
    n = S["off"].shape[0] - 1
    c = hipapi.Context(0)
    try:
        c.load_index_files(g1)
        c.set_tuning("helper_blocks", helper_blocks)
        c.set_tuning("smem_cap", smem_cap)
        c.set_tuning("seed_defer", defer)
        for hps in (0, 1, 3, 5):
            assert _gpu_dump(c, S["reads"], S["off"], hps) == _oracle_dump(S, 0, n, hps), hps
        assert c.timings().seed_launches >= 2                          # several tiers' slots in one gather (the 150-A read overflows 128 slots too)
    finally:
        c.close()


@gpu
@pytest.mark.parametrize("nreads", [1, 15, 16, 17])
def test_seeds_equal_oracle_for_few_reads(ctx, g1, nreads):
    """Fewer reads than a gather workgroup has 16-lane groups, as many, and one more."""
    S = _seed_batch_and_oracle(g1)
    n = S["off"].shape[0] - 1
    first = n - N_EXTRA - 1                                             # the batch's tail: a mixed read, the 150-A read, the stitched reads, the repeats
    off = S["off"][first:first + nreads + 1] - S["off"][first]
    reads = S["reads"][S["off"][first]:S["off"][first + nreads]]
    for hb in (1, 0):
        ctx.set_tuning("helper_blocks", hb)
        try:
            for hps in (0, 3):
                assert _gpu_dump(ctx, reads, off, hps) == _oracle_dump(S, first, nreads, hps), (hb, hps)
        finally:
            ctx.set_tuning("helper_blocks", 0)
