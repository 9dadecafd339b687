"""Reads at the ends of reference sequences through every device stage (the workload of tests/edge_gen.py: sequences of 19 to 5 500 bases from explicit
(offset, len, is_alt) tuples, one of them ALT; reads that start before a sequence's first base, end behind its last, carry a gap 14 bases from it, or cross
the strand junction).  Seeding, chaining, extension, CIGAR generation and record finishing against the compiled reference's chains and records of the workload
(tests/golden/edge_golden.npz) and against the oracle (pinned on the reference on this workload in tests/test_edge_workload.py), exactly.  That the workload
reaches zero-length targets, the text's first and last base and l_pac is asserted there, without a GPU.

One index of the workload's genome is built on the device for the module; every test takes a ctx of its own on it, so MEME_TUNING is applied as the ctx is
made and nothing has to be set back."""
import numpy as np
import pytest

import edge_gen as EG
import finish_cases as FC
import oracle_py as O
from pymeme import hipapi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def W():
    return EG.workload()


@pytest.fixture(scope="module")
def home(W):
    """a ctx with the index of the workload's genome, built on the device (as tests/test_gpu_mate.py stages it)"""
    c = hipapi.Context(0)
    n = 2 * W["l_pac"]
    d_text, d_sa = hipapi.build_sa_device(c, W["text"])
    d_pos5 = hipapi.pos5_from_sa_torch(c, d_sa, n)
    del d_sa
    d_pac, d_ent = hipapi.stage_entries_torch(c, n, d_text, d_pos5)
    d_l2, n_l2, d_l1, n_l1 = hipapi.train_prmi_device(c, d_ent, n, 12)
    keep = (d_pac, d_ent) + hipapi.attach_index_torch(c, n, d_pac, d_ent, d_l2, n_l2, d_l1, n_l1)
    yield c
    c.close()
    del keep


@pytest.fixture
def make_ctx(home, monkeypatch):
    """make_ctx(tuning): a fresh ctx on the module's index, made under MEME_TUNING = tuning"""
    made = []

    def make(tuning=""):
        monkeypatch.setenv("MEME_TUNING", tuning)
        c = hipapi.Context(0)
        made.append(c)
        c.attach_index(home.describe_index())
        return c
    yield make
    for c in made:
        c.close()


def _fields_equal(regs, want, frac_bits):
    """regs: ALNREG records of the device; want: the fixture's int64 columns or the oracle's records"""
    assert regs.shape[0] == want.shape[0]
    for k, f in enumerate(O.ALNREG_FIELDS):
        w = want[:, k] if want.dtype == np.int64 else want[f].astype(np.int64)
        bad = np.nonzero(regs[f].astype(np.int64) != w)[0]
        assert bad.size == 0, (f, int(bad[0]), int(regs[f][bad[0]]), int(w[bad[0]]))
    assert np.array_equal(regs["frac_rep"].view(np.uint32), frac_bits)
    assert not regs["n_comp_is_alt"].any() and not regs["hash"].any() and not regs["flg"].any()


# ---- seeding -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 4, 32])
def test_seeds_equal_the_oracle(W, make_ctx, lanes):
    ctx = make_ctx("group_lanes=%d" % lanes)
    smems, smem_off, hits, hit_off = ctx.seed_batch_host(W["reads"], W["read_off"])
    slots, counts, hl = hipapi.smems_to_slots(smems, smem_off, hits, hit_off)
    assert O.format_seed_dump(slots, counts, hl) == O.format_seed_dump(W["smems"], W["n_smems"], W["hits"])


# ---- chaining ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", ["", "chain_light_hits=0"], ids=["default", "no-lane-tier"])
def test_chains_equal_the_reference_golden_and_the_oracle(W, make_ctx, tuning):
    G = EG.golden()
    ctx = make_ctx(tuning)
    smems, smem_off, hits, hit_off = ctx.seed_batch_host(W["reads"], W["read_off"])
    R = ctx.chain_last_batch_host(W["contigs"], hipapi.default_chain_opt(W["l_pac"]))
    assert R["n_fallback"] == 0 and not R["fallback"].any()
    read_len = np.diff(W["read_off"]).astype(np.int32)
    assert O.chain_compare_batch(smems, smem_off, hits, hit_off, read_len, W["contig_off"], W["contig_alt"], O.default_chain_opt(W["l_pac"]), R) == (0, -1)
    assert np.array_equal(R["chain_off"], G["chain_off"]) and np.array_equal(R["tree_size"], G["tree_size"]) and np.array_equal(R["seed_off"], G["reg_off"])
    for k, f in enumerate(EG.CHAIN_FIELDS):
        assert np.array_equal(R["chains"][f].astype(np.int64), G["chains"][:, k]), f
    assert np.array_equal(EG.chain_seeds(R["chain_off"], R["chains"], R["seed_off"], R["seeds"]), G["seeds"])
    has = np.diff(G["chain_off"]) > 0
    assert np.array_equal(R["frac_rep"].view(np.uint32)[has], G["frac_rep_bits"][has])
    assert int((R["chains"]["is_alt"] != 0).sum()) >= 100


# ---- extension -----------------------------------------------------------------------------------------------------------------------------
# every way the stage can be made to run, as MEME_TUNING (and the reads as FASTQ letters): eight lanes per light read / a wavefront per read; the lane-per-pair
# BSW kernel / the lanes-per-pair one for every job, the zero-length targets among them; the survivors only, all seeds extended first / in rounds; a slab per read
WAYS = {"eight-lanes-per-light-read": "ext_split=1", "wavefront-per-read": "ext_split=0", "bsw-lane-per-pair": "bsw_lane_min_pairs=0",
        "bsw-lanes-per-pair": "bsw_lane_min_pairs=%d" % (1 << 30), "live-only-rounds-0": "ext_live_only=1,ext_rounds=0", "live-only-rounds-2": "ext_live_only=1,ext_rounds=2",
        "slab-per-read": "ext_slab_jobs=1", "fastq-letters": ""}


def _letters(W):
    """the reads as FASTQ letters, three in ten in lower case (the workload has no ambiguous bases)"""
    letters = np.frombuffer(b"ACGT", np.uint8)[W["reads"]].copy()
    letters[np.random.default_rng(3).random(letters.shape[0]) < 0.3] |= 0x20
    return letters


@pytest.mark.parametrize("w,clip,zdrop", EG.EXT_OPTIONS)
@pytest.mark.parametrize("way", list(WAYS))
def test_extension_records_equal_the_reference_golden_and_the_oracle(W, make_ctx, way, w, clip, zdrop):
    """Under the default options the records are the compiled reference's (the fixture), under the others the oracle's; n_retried is the oracle's count
    wherever every chained seed is extended (in rounds the seeds the purge drops are not, so fewer jobs run: at most the oracle's count)."""
    ctx = make_ctx(WAYS[way])
    if way == "fastq-letters":
        ctx.seed_batch_resident_ascii(_letters(W), W["read_off"])
    else:
        ctx.seed_batch_resident(W["reads"], W["read_off"])
    R = ctx.extend_last_batch_host(W["contigs"], hipapi.default_chain_opt(W["l_pac"]), EG.ext_opt(hipapi, w, clip, zdrop))
    want, (_, retried) = EG.oracle_records(W, w, clip, zdrop)
    if (w, clip, zdrop) == EG.EXT_OPTIONS[0]:
        G = EG.golden()
        cols, bits, off = G["regs"], G["reg_frac_bits"], G["reg_off"]
        keep = cols[:, 3] > cols[:, 2]
    else:
        cols, bits, off = want, want["frac_rep"].view(np.uint32), W["seed_off"]
        keep = want["qe"] > want["qb"]
    rounds = 2 if way == "live-only-rounds-2" else 0
    print("%s w=%d clip=%d zdrop=%d: %d records, n_pairs %d, n_retried %d (oracle %d), n_ext_seeds %d" % (way, w, clip, zdrop, R["regs"].shape[0], R["n_pairs"], R["n_retried"], retried,
                                                                                                        R["n_ext_seeds"]))
    assert R["total_seeds"] == keep.shape[0]
    if way.startswith("live-only"):
        assert 0 < int(keep.sum()) < keep.shape[0]
        assert np.array_equal(R["reg_off"], np.concatenate([[0], np.cumsum(keep.astype(np.int64))])[off])
        _fields_equal(R["regs"], cols[keep], bits[keep])
    else:
        assert np.array_equal(R["reg_off"], off)
        _fields_equal(R["regs"], cols, bits)
    if rounds:
        assert int(keep.sum()) <= R["n_ext_seeds"] < keep.shape[0] and R["n_retried"] <= retried
    else:
        assert R["n_ext_seeds"] == keep.shape[0] and R["n_retried"] == retried
    assert R["n_pairs"] > int(keep.sum()) and R["n_flt_jobs"] == 0


# ---- CIGARs --------------------------------------------------------------------------------------------------------------------------------
def test_cigars_of_every_live_record_equal_the_oracle(W, make_ctx):
    """bwa_gen_cigar2 as mem_reg2aln calls it for a record (src/bwamem.cpp:2340-2347, with the record's own band): the records whose rb / re are a sequence's first
    or last base, position 0, l_pac and 2 l_pac among them.  (The records are the oracle's, which the extension test above shows the device makes.)"""
    regs, _ = EG.oracle_records(W)
    read = np.repeat(np.arange(W["read_off"].shape[0] - 1), np.diff(W["seed_off"]))
    live = np.nonzero(regs["qe"] > regs["qb"])[0]
    L = W["l_pac"]
    assert all(int(m.sum()) >= 50 for m in (regs["rb"][live] == 0, regs["re"][live] == 2 * L, regs["re"][live] == L, regs["rb"][live] == L))
    jobs = np.zeros(live.shape[0], hipapi.CJOB)
    jobs["rb"], jobs["read"], jobs["qb"], jobs["qlen"] = regs["rb"][live], read[live], regs["qb"][live], regs["qe"][live] - regs["qb"][live]
    jobs["tlen"], jobs["w_"] = regs["re"][live] - regs["rb"][live], regs["w"][live]
    ctx = make_ctx()
    ctx.seed_batch_resident(W["reads"], W["read_off"])
    res, cig, md, _ = ctx.gen_cigar_batch_host(jobs)
    assert res.shape[0] == jobs.shape[0]
    o = m = n_gapped = 0
    for k, J in enumerate(jobs):
        q = W["reads_list"][int(J["read"])][int(J["qb"]):int(J["qb"]) + int(J["qlen"])]
        want = O.gen_cigar2(W["text"], L, q, int(J["rb"]), int(J["rb"]) + int(J["tlen"]), int(J["w_"]))
        assert want is not None, k
        sc, cg, nm, s = want
        D = res[k]
        assert int(D["cigar_off"]) == o and int(D["md_off"]) == m, k
        assert md[m + int(D["md_len"])] == 0
        assert (int(D["score"]), int(D["nm"]), md[m:m + int(D["md_len"])].tobytes()) == (sc, nm, s) and np.array_equal(cig[o:o + int(D["n_cigar"])], cg), (k, J, D, want)
        o += int(D["n_cigar"]); m += int(D["md_len"]) + 1
        n_gapped += cg.shape[0] > 1
    assert o == cig.shape[0] and m == md.shape[0] and n_gapped >= 50


# ---- finishing -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", ["", "finish_lds_recs=4"], ids=["default", "records-in-hbm"])
def test_finished_records_equal_the_model(W, make_ctx, tuning):
    """mem_sort_dedup_patch_mate_sort and the is_alt flag on the device's own extension records: final order, offsets, useMateSort and the ALT bits against the model
    of tests/finish_gen.py (which reproduces the compiled reference's records in tests/golden/finish_golden.npz); no read left to the host."""
    ctx = make_ctx(tuning)
    ctx.seed_batch_resident(W["reads"], W["read_off"])
    R = ctx.extend_last_batch_host(W["contigs"], hipapi.default_chain_opt(W["l_pac"]))
    B = {"regs": R["regs"], "reg_off": R["reg_off"], "reads": W["reads"], "read_off": W["read_off"]}
    want = FC.model(W, B)
    got = ctx.finish_batch_host(R["regs"], R["reg_off"], W["contigs"], W["l_pac"])
    assert FC.same(got, want) is None
    assert not got["status"].any()
    alt_bit = (got["regs"]["n_comp_is_alt"].view(np.uint32) >> 30) & 1
    assert np.array_equal(alt_bit != 0, W["contig_alt"][got["regs"]["rid"]] != 0) and int(alt_bit.sum()) >= 100
    assert int((np.diff(R["reg_off"]) > 4).sum()) >= 100 and int((np.diff(got["reg_off"]) > 1).sum()) >= 50
