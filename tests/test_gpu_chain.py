"""Chaining on the device (meme_chain_last_batch_host = mem_chain_Learned + mem_chain_flt for the batch just seeded), through
the C ABI, against the chains the compiled reference made of the same reads (tests/golden/chain_golden.npz) and against the
oracle's restatement on every read."""
import os

import numpy as np
import pytest

import oracle_py as O
from common import GOLDEN, build_index, chain_golden_workload
from pymeme import hipapi, synth

pytestmark = pytest.mark.gpu


def _run(ctx, prefix, reads, wave_tiers=1, tuning=()):
    ctx.set_tuning("chain_wave_tiers", wave_tiers)
    for key, value in tuning:
        ctx.set_tuning(key, value)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    flat = np.concatenate(reads)
    ctx.load_index_files(prefix)
    smems, smem_off, hits, hit_off = ctx.seed_batch_host(flat, off)
    ann = [l.split() for l in open(prefix + ".ann")]
    l_pac = int(ann[0][0])
    contigs = [(int(ann[2 + 2 * k][0]), int(ann[2 + 2 * k][1]), 0) for k in range(int(ann[0][1]))]
    res = ctx.chain_last_batch_host(contigs, hipapi.default_chain_opt(l_pac))
    return (smems, smem_off, hits, hit_off), res, l_pac, contigs


@pytest.mark.parametrize("wave_tiers", [1, 0])
def test_device_chains_equal_reference_golden_and_oracle(tmp_path, wave_tiers):
    """wave_tiers 1: repeat-rich reads go through the LDS tier (one wavefront per read, chains in LDS), the B-tree tier takes what that
    leaves; 0: everything beyond the lane-per-read tier goes through the B-tree tier."""
    _golden_body(tmp_path, wave_tiers)


def test_golden_reads_with_nothing_routed_past_the_lane_tier(tmp_path):
    """The fixture's reads are the ones the lane tier normally finishes or never sees (more than chain_light_hits hits: LDS tier at once).  With
    chain_light_hits out of reach the lane tier starts on every read with at most 256 hits and hands what it cannot hold to the LDS tier of 256 chains."""
    G = np.load(os.path.join(GOLDEN, "chain_golden.npz"))
    sm = np.zeros(G["smems"].shape[0], hipapi.MEM_TL)
    sm["start"], sm["end"], sm["hitbeg"], sm["hitcount"] = G["smems"].T
    work = _work(sm, G["smem_off"], G["read_len"])
    assert ((work > 32) & (work <= 256)).sum() >= 20 and (work > 256).sum() == 0       # by default routed to the LDS tier at once; with the key all of them are the lane tier's
    _golden_body(tmp_path, 1, (("chain_light_hits", 1 << 30),), every=6)


def _golden_body(tmp_path, wave_tiers, tuning=(), every=1):
    """every: the stride of the read-by-read comparisons with the fixture (Python loops, 13 s for all reads); the counts and tree sizes of every read, and the
    oracle on every read, are compared whatever it is"""
    g, reads = chain_golden_workload()
    fa = str(tmp_path / "c.fa")
    synth.write_fasta(fa, g, name="cg", contigs=3)
    prefix = build_index(fa, bits=14)
    G = np.load(os.path.join(GOLDEN, "chain_golden.npz"))
    ctx = hipapi.Context(0)
    try:
        (smems, smem_off, hits, hit_off), R, l_pac, contigs = _run(ctx, prefix, reads, wave_tiers, tuning)
    finally:
        ctx.close()
    n = len(reads)
    assert n == G["read_len"].shape[0] and l_pac == int(G["l_pac"])
    # the seeds are the fixture's inputs (the fixture was dumped from the same backend; the seeds themselves are pinned by test_gpu_seed).
    # The ORDER of a read's SMEMs is not part of the contract -- the consumer sorts them by (start, end), src/bwamem.cpp:1397, and equal
    # keys carry equal hit lists -- so the comparison is per read on the sorted (start, end, hits) triples.
    assert np.array_equal(smem_off, G["smem_off"]) and np.array_equal(hit_off, G["hit_off"])

    def canon(sm_start, sm_end, sm_hb, sm_hc, hv):
        return sorted((int(a), int(b), tuple(int(x) for x in hv[int(hb):int(hb) + int(hc)])) for a, b, hb, hc in zip(sm_start, sm_end, sm_hb, sm_hc))
    for r in range(0, n, every):
        s0, s1, h0, h1 = int(smem_off[r]), int(smem_off[r + 1]), int(hit_off[r]), int(hit_off[r + 1])
        mine = canon(smems["start"][s0:s1], smems["end"][s0:s1], smems["hitbeg"][s0:s1], smems["hitcount"][s0:s1], hits[h0:h1])
        gs = G["smems"][s0:s1]
        assert mine == canon(gs[:, 0], gs[:, 1], gs[:, 2], gs[:, 3], G["hits"][h0:h1]), r
    opt = O.default_chain_opt(l_pac)
    contig_off = np.array([c[0] for c in contigs], np.int64)
    contig_alt = np.zeros(len(contigs), np.uint8)
    assert R["n_fallback"] == 0 and not R["fallback"].any()                 # every read is chained on the device
    assert np.array_equal(R["chain_off"], G["chain_off"]) and np.array_equal(R["tree_size"], G["tree_size"])
    for r in range(0, n, every):
        c0, c1 = int(G["chain_off"][r]), int(G["chain_off"][r + 1])
        d0, d1 = int(R["chain_off"][r]), int(R["chain_off"][r + 1])
        assert d1 - d0 == c1 - c0 and int(R["tree_size"][r]) == int(G["tree_size"][r]), r
        if d1 > d0:
            assert R["frac_rep"][r:r + 1].view(np.uint32)[0] == G["frac_rep_bits"][r], r
        sd = R["seeds"][int(R["seed_off"][r]):int(R["seed_off"][r + 1])]
        for k in range(d1 - d0):
            ch = R["chains"][d0 + k]
            want = G["chains"][c0 + k]
            got = [int(ch[f]) for f in ("pos", "rid", "n_seeds", "w", "kept", "first", "is_alt")]
            assert got == [int(x) for x in want[:7]], (r, k, got, want)
            gs = sd[int(ch["seed_beg"]):int(ch["seed_beg"]) + int(ch["n_seeds"])]
            ws = G["seeds"][int(want[7]):int(want[7]) + int(want[2])]
            assert np.array_equal(np.stack([gs["rbeg"], gs["qbeg"], gs["len"]], 1), ws), (r, k)
    # and the oracle agrees with the device on the same seeds, read by read, field by field
    read_len = np.array([len(r) for r in reads], np.int32)
    assert O.chain_compare_batch(smems, smem_off, hits, hit_off, read_len, contig_off, contig_alt, opt, R) == (0, -1)
    assert R["n_tier2"] > 0                                                   # the fixture's repeat reads went through the wavefront-per-read tier


def _contigs3():
    return [(0, 70_000, 0), (70_000, 80_000, 0), (150_000, 50_000, 1)]


def test_device_chains_equal_reference_on_equal_positions_and_big_trees():
    """tests/golden/chain_dup_golden.npz through meme_chain_batch_host: made-up seed sets with up to 1 300 chains per read, most with
    several chains at EQUAL positions, against the chains the compiled reference (its B-tree, its introsort) made of them."""
    import chain_gen  # noqa: F401  (the fixture's generator; here only the fixture is used)
    G = np.load(os.path.join(GOLDEN, "chain_dup_golden.npz"))
    sm = np.zeros(G["smems"].shape[0], hipapi.MEM_TL)
    sm["start"], sm["end"], sm["hitbeg"], sm["hitcount"] = G["smems"].T
    ctx = hipapi.Context(0)
    try:
        R = ctx.chain_batch_host(sm, G["smem_off"], G["hits"], G["hit_off"], G["read_len"], _contigs3(), hipapi.default_chain_opt(int(G["l_pac"])))
    finally:
        ctx.close()
    _assert_dup_golden(R, G)


def _assert_dup_golden(R, G):
    assert R["n_fallback"] == 0
    assert np.array_equal(R["chain_off"], G["chain_off"]) and np.array_equal(R["seed_off"], G["seed_off"])
    assert np.array_equal(R["tree_size"], G["tree_size"])
    for k, f in enumerate(("pos", "rid", "n_seeds", "w", "kept", "first", "is_alt", "seed_beg")):
        assert np.array_equal(R["chains"][f].astype(np.int64), G["chains"][:, k]), f
    assert np.array_equal(np.stack([R["seeds"]["rbeg"], R["seeds"]["qbeg"], R["seeds"]["len"]], 1), G["seeds"])
    has = np.diff(G["chain_off"]) > 0
    assert np.array_equal(R["frac_rep"].view(np.uint32)[has], G["frac_rep_bits"][has])


def _one_hit_chains(weights, spacing, dup):
    """A read of len(weights) SMEMs of one hit each: SMEM i starts at query base i (2 i for 40 and fewer), is 19 + weights[i] long and hits position
    1 000 + i * spacing, so that every hit opens a chain of its own and the chains in tree order weigh 19 + weights.  dup: one more SMEM far
    behind them in the query whose hit lies ON chain 0's position and opens a second chain there."""
    n, k = len(weights), 2 if len(weights) <= 40 else 1
    sm = np.zeros(n + (1 if dup else 0), hipapi.MEM_TL)
    sm["start"][:n] = k * np.arange(n); sm["end"][:n] = sm["start"][:n] + 19 + np.asarray(weights)
    hits = (1000 + spacing * np.arange(n)).astype(np.uint64)
    if dup:
        sm["start"][n] = n + 65; sm["end"][n] = n + 90          # (chain 0's seed starts at 0: more than the band w = 100 behind it, so it cannot be appended)
        hits = np.append(hits, hits[0])
    sm["hitbeg"] = np.arange(sm.shape[0]); sm["hitcount"] = 1
    return sm, hits


def _tied_batch():
    """two pairs of reads of one-hit chains with monotone weights full of ties (test_tied_monotone_weights_...): -> (reads, smems, smem_off, hits, hit_off, read_len, pairs)"""
    pairs = [([(40 - i) // 2 for i in range(40)], 1000, 150), ([i // 2 for i in range(100)], 600, 250)]
    reads = [_one_hit_chains(w, spacing, dup) for w, spacing, _ in pairs for dup in (False, True)]
    read_len = np.array([rl for _, _, rl in pairs for _ in (0, 1)], np.int32)
    smem_off = np.zeros(5, np.int64); hit_off = np.zeros(5, np.int64)
    smem_off[1:] = np.cumsum([sm.shape[0] for sm, _ in reads]); hit_off[1:] = np.cumsum([h.shape[0] for _, h in reads])
    smems = np.concatenate([sm for sm, _ in reads]); hits = np.concatenate([h for _, h in reads])
    return reads, smems, smem_off, hits, hit_off, read_len, pairs


def test_tied_monotone_weights_take_the_sort_fallback_in_both_wavefront_tiers():
    """The comb-sort branch of the shared sort (bwa-meme_amd/csrc/meme_ksort.h) on the device: monotone chain weights full of ties spend klib's depth
    budget, and where its comb sort leaves equal weights differs from a stable sort.  Read A of each pair has more chains than the lane tier
    holds and is sorted by the LDS tier (wave_introsort_lds); read B also puts two chains on one position and is sorted by the B-tree tier
    (k_chain_wave).  The lane tier never has more than 16 chains: the sort is one partition pass there, which the goldens cover."""
    import test_introsort_model as M
    reads, smems, smem_off, hits, hit_off, read_len, pairs = _tied_batch()
    for weights, _, _ in pairs:                                  # what the model makes of these weights (ids in tree order)
        arr = [(19 + w, i) for i, w in enumerate(weights)]
        M.COMB_CALLS[0] = 0
        assert M.klib(arr) != M.stable(arr) and M.COMB_CALLS[0] > 0, len(weights)
    assert int(smems["end"].max()) <= 250 and int(smems["end"][:smem_off[2]].max()) <= 150
    contig_off, contig_alt, oo = np.array([0, 70_000, 150_000], np.int64), np.array([0, 0, 1], np.uint8), O.default_chain_opt(200_000)
    trees = [O.chain_read(sm, h, rl, contig_off, contig_alt, oo)[3] for (sm, h), rl in zip(reads, read_len)]
    assert trees == [40, 41, 100, 101]
    assert O.chain_read(reads[0][0], reads[0][1], 150, contig_off, contig_alt, oo)[0] == 40          # default options drop none of read A's chains
    ctx = hipapi.Context(0)
    try:
        R = ctx.chain_batch_host(smems, smem_off, hits, hit_off, read_len, _contigs3(), hipapi.default_chain_opt(200_000))
        tier3 = int(ctx.timings().chain_tier3_reads)
    finally:
        ctx.close()
    assert R["n_fallback"] == 0 and list(R["tree_size"]) == trees
    assert tier3 == 2 and R["n_tier2"] == 4                      # both B reads reached the B-tree tier, through the LDS tier that sorts the A reads
    assert O.chain_compare_batch(smems, smem_off, hits, hit_off, read_len, contig_off, contig_alt, oo, R) == (0, -1)


def test_the_contig_table_follows_the_call():
    """one ctx, the tables A, B, A in turn (B: the first boundary moved into the reads' hits): the ctx keeps one contig table and restages it when a call brings another"""
    reads, smems, smem_off, hits, hit_off, read_len, _ = _tied_batch()
    tables = {"A": _contigs3(), "B": [(0, 30_000, 0), (30_000, 120_000, 0), (150_000, 50_000, 1)]}
    oo = O.default_chain_opt(200_000)
    cols = {k: (np.array([c[0] for c in t], np.int64), np.array([c[2] for c in t], np.uint8)) for k, t in tables.items()}
    rids = {k: [int(ch["rid"]) for ch in O.chain_read(reads[0][0], reads[0][1], int(read_len[0]), off, alt, oo)[1]] for k, (off, alt) in cols.items()}
    assert rids["A"] != rids["B"] and len(rids["A"]) == len(rids["B"]) == 40      # the two tables give different chains: the test cannot pass on a stale table
    ctx = hipapi.Context(0)
    try:
        for name in ("A", "B", "A"):
            R = ctx.chain_batch_host(smems, smem_off, hits, hit_off, read_len, tables[name], hipapi.default_chain_opt(200_000))
            assert R["n_fallback"] == 0
            assert O.chain_compare_batch(smems, smem_off, hits, hit_off, read_len, cols[name][0], cols[name][1], oo, R) == (0, -1), name
    finally:
        ctx.close()


def _adversarial(n, seed):
    import chain_gen
    reads = chain_gen.workload(seed, n, l_pac=200_000)
    smem_off = np.zeros(len(reads) + 1, np.int64); hit_off = np.zeros(len(reads) + 1, np.int64)
    for r, (sm, h) in enumerate(reads):
        smem_off[r + 1] = smem_off[r] + sm.shape[0]; hit_off[r + 1] = hit_off[r] + h.shape[0]
    smems = np.concatenate([sm for sm, _ in reads]).astype(hipapi.MEM_TL)
    hits = np.concatenate([h for _, h in reads])
    read_len = np.array([250 if r % 5 == 2 else 150 for r in range(len(reads))], np.int32)
    return smems, smem_off, hits, hit_off, read_len


def test_device_chains_equal_oracle_on_adversarial_batch():
    """5 000 made-up reads (tests/chain_gen.py) chained on the device and compared with the oracle by the batched checker."""
    smems, smem_off, hits, hit_off, read_len = _adversarial(5000, 991)
    ctx = hipapi.Context(0)
    try:
        R = ctx.chain_batch_host(smems, smem_off, hits, hit_off, read_len, _contigs3(), hipapi.default_chain_opt(200_000))
    finally:
        ctx.close()
    assert R["n_fallback"] == 0 and R["n_tier2"] > 1000
    bad = O.chain_compare_batch(smems, smem_off, hits, hit_off, read_len, np.array([0, 70_000, 150_000], np.int64), np.array([0, 0, 1], np.uint8),
                                O.default_chain_opt(200_000), R)
    assert bad == (0, -1), bad


@pytest.mark.parametrize("name,change", [("narrow_band", dict(w=3)), ("wide_band", dict(w=2000)), ("short_gap", dict(max_chain_gap=40)),
                                         ("few_hits", dict(max_occ=37)), ("strict_filter", dict(drop_ratio=0.9, mask_level=0.1)),
                                         ("few_extended", dict(max_chain_extend=3)), ("weight_floor", dict(min_chain_weight=40))])
def test_device_chains_equal_oracle_under_other_options(name, change):
    """The same kind of batch under other chaining options: the band and gap limits enter test_and_merge and with it the rule by which the
    wavefront tier commits a batch of hits at once; max_occ the sampling of the hits; the rest the filter."""
    smems, smem_off, hits, hit_off, read_len = _adversarial(2500, 1200 + len(name))
    do, oo = hipapi.default_chain_opt(200_000), O.default_chain_opt(200_000)
    for k, v in change.items():
        setattr(do, k, v); setattr(oo, k, v)
    ctx = hipapi.Context(0)
    try:
        R = ctx.chain_batch_host(smems, smem_off, hits, hit_off, read_len, _contigs3(), do)
    finally:
        ctx.close()
    assert R["n_fallback"] == 0
    bad = O.chain_compare_batch(smems, smem_off, hits, hit_off, read_len, np.array([0, 70_000, 150_000], np.int64), np.array([0, 0, 1], np.uint8), oo, R)
    assert bad == (0, -1), (name, bad)


def test_chain_call_needs_a_seeded_batch_and_sane_options(tmp_path):
    g = synth.make_genome(60_000, seed=9)
    fa = str(tmp_path / "e.fa")
    synth.write_fasta(fa, g, contigs=1)
    prefix = build_index(fa, bits=12)
    ctx = hipapi.Context(0)
    try:
        ctx.load_index_files(prefix)
        with pytest.raises(hipapi.MemeError, match="no seeded batch"):
            ctx.chain_last_batch_host([(0, 60_000, 0)], hipapi.default_chain_opt(60_000))
        r, _, _ = synth.make_reads(g, 50, 100, seed=10)
        ctx.seed_batch_host(r.reshape(-1), np.arange(0, 51 * 100, 100, dtype=np.int64))
        bad = hipapi.default_chain_opt(60_000)
        bad.max_occ = 0
        with pytest.raises(hipapi.MemeError, match="bad options"):
            ctx.chain_last_batch_host([(0, 60_000, 0)], bad)
        with pytest.raises(hipapi.MemeError, match="not a valid reference sequence"):          # a bntann1_t length is positive and inside the genome
            ctx.chain_last_batch_host([(0, 70_000, 0)], hipapi.default_chain_opt(60_000))
        res = ctx.chain_last_batch_host([(0, 60_000, 0)], hipapi.default_chain_opt(60_000))
        assert res["chain_off"].shape[0] == 51 and res["chain_off"][-1] == res["chains"].shape[0] >= 40
        w = res["chains"]["w"]
        for i in range(50):                                     # the filter's output is ordered by weight
            c = w[int(res["chain_off"][i]):int(res["chain_off"][i + 1])]
            assert np.all(c[:-1] >= c[1:])
    finally:
        ctx.close()


# ---- the routes between the tiers: k_chain_route's thresholds and the lane tier's give-up limit moved through the tuning keys, so that every hand-over
# ---- (lane -> LDS256 -> B-tree, LDS-N -> B-tree) is taken by reads the default thresholds send elsewhere ------------------------------------------------
_ROUTES = [(0, 256), (1 << 30, 256), (1 << 30, 0), (1 << 30, 1 << 30), (32, 31), (32, 32), (32, 33)]          # (chain_light_hits, chain_lane_hits)
_route_inputs = {}


def _work(smems, smem_off, read_len, max_occ=500, min_seed_len=19):
    """k_chain_route's measure: the hits a read has to walk, sum over its SMEMs of min(hitcount, max_occ); 0 for reads below min_seed_len"""
    h = np.minimum(smems["hitcount"].astype(np.int64), max_occ)
    cs = np.concatenate([[0], np.cumsum(h)])
    return np.where(np.asarray(read_len) >= min_seed_len, cs[smem_off[1:]] - cs[smem_off[:-1]], 0)


def _route_model(work, n_smems, light, lane_hits):
    """(class k_chain_route gives a read: 0 lane tier, 1 / 2 / 3 LDS tier of 256 / 512 / 1 024 chains; reads certain to pass through a wavefront tier; chains the
    last LDS tier on a read's way holds)"""
    cls = np.where(work > 512, 3, np.where(work > 256, 2, np.where(work > light, 1, 0)))
    gives_up = (cls == 0) & (work > 0) & ((work > lane_hits) | (n_smems > 48))            # (SMEM_CAP1 = 48; the 16-chain / 8-seed limits give up more)
    return cls, (cls > 0) | gives_up, np.where(cls == 3, 1024, np.where(cls == 2, 512, 256))


def _inputs(name):
    if name not in _route_inputs:
        if name == "dup":
            G = np.load(os.path.join(GOLDEN, "chain_dup_golden.npz"))
            sm = np.zeros(G["smems"].shape[0], hipapi.MEM_TL)
            sm["start"], sm["end"], sm["hitbeg"], sm["hitcount"] = G["smems"].T
            _route_inputs[name] = (sm, G["smem_off"], G["hits"], G["hit_off"], G["read_len"], int(G["l_pac"]), G)
        else:
            _route_inputs[name] = _with_boundary_reads(*_adversarial(1500, 1300)) + (200_000, None)
    return _route_inputs[name]


def _with_boundary_reads(smems, smem_off, hits, hit_off, read_len):
    """+ 30 reads with exactly 31, 32 and 33 hits to walk (made-up reads cut off at that many hits): the two sides of chain_light_hits = 32 and of the
    chain_lane_hits values next to it"""
    import chain_gen
    rng = np.random.default_rng(77)
    sm_l, h_l, so, ho = [smems], [hits], list(smem_off), list(hit_off)
    for k in range(30):
        want = 31 + k % 3
        while True:
            sm, h = chain_gen.make_read(rng, n_smems=6, max_hits=40)
            if int(sm["hitcount"].sum()) >= want:
                break
        keep = int(np.searchsorted(np.cumsum(sm["hitcount"]), want))               # the SMEM the cut falls into
        sm = sm[:keep + 1].copy()
        sm["hitcount"][keep] = want - int(sm["hitcount"][:keep].sum())
        sm_l.append(sm.astype(hipapi.MEM_TL)); h_l.append(h[:want])
        so.append(so[-1] + sm.shape[0]); ho.append(ho[-1] + want)
    return np.concatenate(sm_l), np.array(so, np.int64), np.concatenate(h_l), np.array(ho, np.int64), np.concatenate([read_len, np.full(30, 150, np.int32)])


@pytest.mark.parametrize("light,lane_hits", _ROUTES)
def test_every_route_between_the_tiers_gives_the_same_chains(light, lane_hits):
    """light = 0: every read with hits is routed to an LDS tier at once; 1 << 30: none by chain_light_hits (reads beyond 256 / 512 hits still go to the tiers of
    512 / 1 024 chains: those thresholds are fixed), the lane tier starts on the rest -- and gives every one up (lane_hits = 0), or walks until its 16 chains or
    8 seeds per chain are full (1 << 30); 31 / 32 / 33: either side of the default."""
    for name, change in (("dup", {}), ("adversarial", {}), ("adversarial", dict(w=3))):
        smems, smem_off, hits, hit_off, read_len, l_pac, G = _inputs(name)
        do, oo = hipapi.default_chain_opt(l_pac), O.default_chain_opt(l_pac)
        for k, v in change.items():
            setattr(do, k, v); setattr(oo, k, v)
        work = _work(smems, smem_off, read_len)
        cls, waved, cap = _route_model(work, np.diff(smem_off), light, lane_hits)
        assert (work > 0).sum() > 0.9 * work.shape[0] and (work > 256).sum() > 0 and (work > 512).sum() > 0
        if light == 0:
            assert (cls[work > 0] > 0).all()
        elif light == 1 << 30:
            assert ((cls == 0) & (work > 32)).sum() > 100                # reads the default sends to an LDS tier at once, now the lane tier's
        elif G is None:
            assert all((work == v).sum() >= 10 for v in (31, 32, 33))    # 32 hits: the lane tier's, given up at lane_hits = 31; 33: routed
        ctx = hipapi.Context(0)
        try:
            ctx.set_tuning("chain_light_hits", light)
            ctx.set_tuning("chain_lane_hits", lane_hits)
            R = ctx.chain_batch_host(smems, smem_off, hits, hit_off, read_len, _contigs3(), do)
            tier3 = int(ctx.timings().chain_tier3_reads)
        finally:
            ctx.close()
        print("%s %s light=%d lane_hits=%d: n_tier2 %d (model: at least %d), chain_tier3_reads %d" % (name, change, light, lane_hits, R["n_tier2"], int(waved.sum()), tier3))
        assert R["n_fallback"] == 0
        assert R["n_tier2"] >= int(waved.sum())
        if light == 0 or lane_hits == 0:
            assert R["n_tier2"] >= int((work > 0).sum())
        if G is not None:
            _assert_dup_golden(R, G)
            # a read with more chains than the last LDS tier on its way holds ends in the B-tree tier (k_chain_lds<N> gives up beyond N chains)
            over = int((G["tree_size"] > cap).sum())
            assert over >= 4 and tier3 >= over, (over, tier3)
        else:
            bad = O.chain_compare_batch(smems, smem_off, hits, hit_off, read_len, np.array([0, 70_000, 150_000], np.int64), np.array([0, 0, 1], np.uint8), oo, R)
            assert bad == (0, -1), (name, change, bad)
            assert tier3 >= int((R["tree_size"] > cap).sum())
