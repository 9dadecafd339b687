"""The reads at sequence ends of tests/edge_gen.py without a GPU: that the workload reaches the edges it was written for (conditions the oracle alone has to
meet, so a generator that drifted is caught before the device tests compare anything), that the oracle equals the COMPILED REFERENCE there (the committed
records in tests/golden/edge_golden.npz; live against oracle/_ref where it is built, under other options too, like tests/test_ref_live.py), and that the
scalar mem_chain2aln tests/test_ext_rules_model.py compiles from bwa-meme_amd/csrc/meme_ext_rules.h gives the oracle's records on it.  The device runs the same
workload in tests/test_gpu_edges.py."""
import numpy as np
import pytest

import edge_gen as EG
import oracle_py as O
import ref_py
from test_ext_rules_model import _assert_fields, _extend, _flat, driver  # noqa: F401  (driver: the module-scoped fixture)
from test_ref_live import _same_chains, needs_stage


@pytest.fixture(scope="module")
def W():
    return EG.workload()


def _live(regs):
    return regs["qe"] > regs["qb"]


# ---- what the workload is for ------------------------------------------------------------------------------------------------------------
def test_genome_and_reads_are_the_ones_described(W):
    lens = sorted(int(l) for l in W["contig_len"])
    assert lens[:5] == [19, 40, 150, 260, 700] and all(l >= 4000 for l in lens[5:]) and len(lens) == 8
    assert [int(a) for a in W["contig_alt"]].count(1) == 1 and int(W["contig_len"][np.argmax(W["contig_alt"])]) >= 4000
    assert 14_000 <= W["l_pac"] <= 16_000 and int(W["contig_off"][-1] + W["contig_len"][-1]) == W["l_pac"]
    assert sorted(set(np.diff(W["read_off"]).tolist())) == [60, 150, 250]
    assert set(W["kind"].tolist()) == {"perfect", "clipped", "gap", "island", "junction"}
    # both strands of everything: read 2 i + 1 is the reverse complement of read 2 i
    for r in range(0, len(W["reads_list"]), 2):
        assert np.array_equal(W["reads_list"][r + 1], (3 - W["reads_list"][r][::-1]))
    # the junction reads are the text's own bases across l_pac
    L = W["l_pac"]
    junction = [r for r in np.nonzero(W["kind"] == "junction")[0] if r % 2 == 0]
    want = [(n, k) for n in EG.READ_LENS for k in EG.junction_offsets(n)]
    assert len(junction) == len(want)
    for r, (n, k) in zip(junction, want):
        assert np.array_equal(W["reads_list"][r], W["text"][L - k:L - k + n])


def test_seeds_sit_on_first_and_last_bases_and_leave_short_targets(W):
    left, right = EG.seed_targets(W)
    n_left0, n_right0 = int((left == 0).sum()), int((right == 0).sum())
    short = {v: int((left == v).sum() + (right == v).sum()) for v in (1, 5, 18, 19, 20)}
    print("zero-length targets left / right: %d / %d; targets of 1, 5, 18, 19, 20 bases: %s" % (n_left0, n_right0, short))
    assert n_left0 >= 100 and n_right0 >= 100
    assert all(v >= 10 for v in short.values()), short
    # a zero-length target is a seed ON the sequence's first / last base (on its strand), with a flank of the read beyond it
    S, L = W["seeds"], W["l_pac"]
    rid = np.repeat(W["chains"]["rid"], W["chains"]["n_seeds"])            # (a read's seeds lie chain by chain)
    assert np.array_equal(EG.chain_seeds(W["chain_off"], W["chains"], W["seed_off"], S)[:, 0], S["rbeg"])
    beg, end = W["contig_off"][rid], W["contig_off"][rid] + W["contig_len"][rid]
    rev = S["rbeg"] >= L
    lo, hi = np.where(rev, 2 * L - end, beg), np.where(rev, 2 * L - beg, end)
    assert np.array_equal(left == 0, (S["rbeg"] == lo) & (S["qbeg"] > 0))
    assert np.array_equal(right == 0, (S["rbeg"] + S["len"] == hi) & (right >= 0))
    assert ((left == 0) & rev).sum() >= 50 and ((left == 0) & ~rev).sum() >= 50         # both strands
    assert ((left == 0) & (right == 0)).any()                                          # a seed from a sequence's first base to its last


def test_records_reach_both_ends_of_the_text_and_the_strand_junction(W):
    regs, (jobs, retried) = EG.oracle_records(W)
    live, L = _live(regs), W["l_pac"]
    counts = {"rb == 0": int((live & (regs["rb"] == 0)).sum()), "re == 2 l_pac": int((live & (regs["re"] == 2 * L)).sum()),
              "re == l_pac": int((live & (regs["re"] == L)).sum()), "rb == l_pac": int((live & (regs["rb"] == L)).sum())}
    print("live records %d of %d, %s; jobs %d" % (int(live.sum()), regs.shape[0], counts, jobs))
    assert all(v >= 50 for v in counts.values()), counts
    assert not (live & (regs["rb"] < L) & (regs["re"] > L)).any()                      # no record bridges the strands
    # ... and every record lies inside its sequence
    beg, end = W["contig_off"][regs["rid"]], W["contig_off"][regs["rid"]] + W["contig_len"][regs["rid"]]
    rev = regs["rb"] >= L
    frb, fre = np.where(rev, 2 * L - regs["re"], regs["rb"]), np.where(rev, 2 * L - regs["rb"], regs["re"])
    assert (~live | ((frb >= beg) & (fre <= end))).all()


def test_every_sequence_that_can_hold_a_seed_has_chains_and_the_alt_one_has_alt_chains(W):
    per = np.bincount(W["chains"]["rid"], minlength=W["contig_off"].shape[0])
    alt = int((W["chains"]["is_alt"] != 0).sum())
    print("chains per sequence %s, ALT chains %d" % (per.tolist(), alt))
    for c, n in enumerate(W["contig_len"]):
        assert (per[c] > 0) == (n >= 40), (c, int(n), int(per[c]))
    assert per[int(np.nonzero(W["contig_len"] == 19)[0][0])] == 0
    assert alt >= 100 and np.array_equal(W["chains"]["is_alt"] != 0, W["contig_alt"][W["chains"]["rid"]] != 0)


def test_a_band_of_three_retries_jobs(W):
    _, (jobs, retried) = EG.oracle_records(W, 3, 5, 100)
    print("w = 3: %d jobs, %d retried" % (jobs, retried))
    assert retried >= 100


# ---- the oracle equals the compiled reference here -----------------------------------------------------------------------------------------
def test_oracle_chains_and_records_equal_the_reference_golden(W):
    G = EG.golden()
    assert np.array_equal(W["chain_off"], G["chain_off"]) and np.array_equal(W["tree_size"], G["tree_size"]) and np.array_equal(W["seed_off"], G["reg_off"])
    for k, f in enumerate(EG.CHAIN_FIELDS):
        assert np.array_equal(W["chains"][f].astype(np.int64), G["chains"][:, k]), f
    assert np.array_equal(EG.chain_seeds(W["chain_off"], W["chains"], W["seed_off"], W["seeds"]), G["seeds"])
    has = np.diff(W["chain_off"]) > 0                                      # (frac_rep of a read without chains is not defined)
    assert np.array_equal(W["frac_rep"].view(np.uint32)[has], G["frac_rep_bits"][has])
    regs, _ = EG.oracle_records(W)
    for k, f in enumerate(O.ALNREG_FIELDS):
        bad = np.nonzero(regs[f].astype(np.int64) != G["regs"][:, k])[0]
        assert bad.size == 0, (f, int(bad[0]), int(regs[f][bad[0]]), int(G["regs"][bad[0], k]))
    assert np.array_equal(regs["frac_rep"].view(np.uint32), G["reg_frac_bits"])


@needs_stage
def test_chain_oracle_equals_reference_live(W):
    copt = O.default_chain_opt(W["l_pac"])
    for r in range(W["read_off"].shape[0] - 1):
        sm, hits, n = W["smems"][r, :W["n_smems"][r]], W["hits"][r, :W["n_hits"][r]], int(W["read_off"][r + 1] - W["read_off"][r])
        want = ref_py.chain_read(sm, hits, n, W["contig_off"], W["contig_len"], W["contig_alt"], copt)
        got = O.chain_read(sm, hits, n, W["contig_off"], W["contig_alt"], copt)
        assert _same_chains(got, want), (r, W["kind"][r], got[0], want[0], got[3], want[3])


@needs_stage
@pytest.mark.parametrize("w,clip,zdrop", EG.EXT_OPTIONS)
def test_ext_oracle_equals_reference_live(W, w, clip, zdrop):
    want = ref_py.extend_reads(W["reads"], W["read_off"], W["chain_off"], W["chains"], W["seed_off"], W["seeds"], W["frac_rep"], W["text"], W["l_pac"],
                               W["contig_off"], W["contig_len"], W["contig_alt"], EG.ext_opt(O, w, clip, zdrop))
    got, _ = EG.oracle_records(W, w, clip, zdrop)
    for f in O.ALNREG_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, (f, int(bad[0]), int(got[f][bad[0]]), int(want[f][bad[0]]))
    assert np.array_equal(got["frac_rep"].view(np.uint32), want["frac_rep"].view(np.uint32))


@needs_stage
def test_gen_cigar2_oracle_equals_reference_live_on_every_live_record(W):
    regs, _ = EG.oracle_records(W)
    read = np.repeat(np.arange(W["read_off"].shape[0] - 1), np.diff(W["seed_off"]))
    n = 0
    for k in np.nonzero(_live(regs))[0]:
        a = regs[k]
        q = W["reads_list"][read[k]][int(a["qb"]):int(a["qe"])]
        want = ref_py.gen_cigar2(W["genome"], q, int(a["rb"]), int(a["re"]), int(a["w"]))
        got = O.gen_cigar2(W["text"], W["l_pac"], q, int(a["rb"]), int(a["re"]), int(a["w"]))
        assert want is not None and got is not None, k
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:] == want[2:], (k, a, got[0], want[0], got[2:], want[2:])
        n += 1
    assert n > 1500


# ---- the shared rules header on the workload ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,clip,zdrop", EG.EXT_OPTIONS)
def test_rules_header_gives_the_oracle_records_in_both_orders(driver, W, w, clip, zdrop):  # noqa: F811
    oo = EG.ext_opt(O, w, clip, zdrop)
    want, _ = EG.oracle_records(W, w, clip, zdrop)
    F = _flat(W)
    regs, tally = _extend(driver, W, F, oo, 0)
    _assert_fields(regs, want, want["frac_rep"].view(np.uint32), "batch")
    assert not regs["n_comp_is_alt"].any() and not regs["hash"].any() and not regs["flg"].any()
    # job and byte counts of the geometry == the SeqPairs posed, zero-length targets among them (a pose whose query would overlap its target shows here)
    assert tally[4] == 0 and tally[0] == tally[2] and tally[1] == tally[3] and tally[0] > 0, tally
    keep = _live(want)
    regs, tally = _extend(driver, W, F, oo, 1)
    assert np.array_equal(_live(regs), keep)
    _assert_fields(regs[keep], want[keep], want["frac_rep"].view(np.uint32)[keep], "rounds")
    assert tally[4] == 0 and tally[0] == tally[2] and tally[1] == tally[3], tally
