"""The rules of mem_chain2aln_across_reads_V2 (reference src/bwamem.cpp:2573-3497), mem_seed_sw / mem_flt_chained_seeds (:494-598) and bns_fetch_seq
(src/bntseq.cpp:479-570) that the kernels of meme_ext.hip and the posing kernel of meme_mate.hip share, written once in bwa-meme_amd/csrc/meme_ext_rules.h:
spans, the seed filter's window, the job geometry and the SeqPair of a side, the record a seed starts as, the extension order, seedcov, the fold, the two
purge predicates.  The header is compiled here with g++ into a scalar mem_chain2aln for one read -- plain loops, every rule taken from the header, banded SW and
the filter's alignment borrowed from the oracle through function pointers (neither is under test) -- which runs the purge in two orders: the reference's (extend
everything, then purge) and the one of extension in rounds (test a seed against the survivors before it, extend it only if it survives).  Both have to give the
records the compiled reference recorded (tests/golden/ext_golden.npz) and the oracle's under other options, exactly; the job geometry has to equal what the driver
poses.  (The kernels themselves are checked in tests/test_gpu_ext.py and tests/test_gpu_mate.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
from common import GOLDEN, ext_golden_inputs, flt_hsp, flt_workload, seed_sw_window
from pymeme import hipapi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''#include <vector>
#include "meme_ext_rules.h"
struct Chain { int64_t pos; int32_t rid, n_seeds, w, first, kept, is_alt, seed_beg, pad; };       // the oracle's chain record
typedef int (*bsw_fn)(int qlen, const uint8_t* query, int tlen, const uint8_t* target, int w, int h0, const meme_bsw_opt* p, int* qle, int* tle, int* gtle, int* gscore,
                      int* max_off, int64_t* cells);
typedef int (*sw_fn)(int qlen, const uint8_t* query, const uint8_t* text, int64_t l_pac, int64_t rb, int tlen, const meme_ext_opt* o);
struct Ref { const uint8_t* text; int64_t l_pac; const int64_t* contig_off; const int* contig_len; int n_contigs; };

struct ReadExt {
    const uint8_t* read; int l_query; const Chain* chains; int nc; const meme_chain_seed* seeds; const int* score; const Ref& X; const meme_ext_opt& o; bsw_fn bsw;
    meme_alnreg* out; int64_t* tally;        // tally: jobs and bytes by the geometry [0, 1], as posed [2, 3]; seeds whose two disagree [4]
    std::vector<int64_t> rmax; std::vector<int> ord; std::vector<uint8_t> seq;
    meme_bsw_opt side_opt(bool left) const {
        meme_bsw_opt b{o.o_del, o.e_del, o.o_ins, o.e_ins, o.zdrop, left ? o.pen_clip5 : o.pen_clip3, o.a, o.b};
        return b;
    }
    // spans, the extension order, the records (what k_ext_jobs does in its first two parts)
    void records(float frac_rep) {
        int S = 0;
        for (int c = 0; c < nc; ++c) S += chains[c].n_seeds;
        rmax.assign(2 * nc + 2, 0); ord.assign(S + 1, 0);
        for (int c = 0; c < nc; ++c) {
            const Chain& ch = chains[c];
            const meme_chain_seed* sd = seeds + ch.seed_beg;
            if (ch.n_seeds == 0) continue;
            int64_t b = X.l_pac << 1, e = 0;
            for (int i = 0; i < ch.n_seeds; ++i) { const ExtSpan x = ext_seed_reach(sd[i], l_query, o); b = x.b < b ? x.b : b; e = x.e > e ? x.e : e; }
            ext_span_finish(b, e, sd[0].rbeg, X.l_pac);
            bns_clamp(X.l_pac, X.contig_off[ch.rid], X.contig_len[ch.rid], sd[0].rbeg >= X.l_pac, b, e);
            rmax[2 * c] = b; rmax[2 * c + 1] = e;
            for (int il = 0; il < ch.n_seeds; ++il) {
                int rank = 0;
                for (int k = 0; k < ch.n_seeds; ++k) rank += ext_seed_before(sc(ch, k), k, sc(ch, il), il);
                ord[ch.seed_beg + rank] = il;
                const ExtGeom g = ext_geom(sd[il], b, e, l_query);
                out[ch.seed_beg + (ch.n_seeds - 1 - rank)] = ext_record0(sd[il], g.sideL, g.sideR, l_query, o, ch.rid, frac_rep, (uint64_t)c, sd, ch.n_seeds);
            }
        }
    }
    int sc(const Chain& ch, int k) const { return score ? score[ch.seed_beg + k] : seeds[ch.seed_beg + k].len; }
    // one side of a seed: posed behind the jobs so far, aligned with the band doubled once, folded
    template <bool LEFT> void side(meme_alnreg& a, const Chain& ch, const meme_chain_seed& t, const ExtGeom& g, int h0) {
        const meme_chain_seed* sd = seeds + ch.seed_beg;
        meme_seqpair sp = ext_pose(h0, 0, 0, LEFT ? g.l1L : g.l1R, LEFT ? g.l2L : g.l2R, (int)seq.size());
        const bool fits = sp.idr % 4 == 0 && sp.idq % 4 == 0 && sp.idq >= sp.idr + sp.len1;
        seq.resize(((size_t)sp.idq + sp.len2 + 3) / 4 * 4 + (fits ? 0 : 4));        // (a pose that overlaps itself shows as bytes the geometry did not plan)
        for (int k = 0; k < sp.len1; ++k) seq[sp.idr + k] = X.text[LEFT ? t.rbeg - 1 - k : t.rbeg + t.len + k];
        for (int k = 0; k < sp.len2; ++k) seq[sp.idq + k] = read[LEFT ? t.qbeg - 1 - k : t.qbeg + t.len + k];
        ++tally[2];
        const meme_bsw_opt bo = side_opt(LEFT);
        for (int attempt = 0; attempt < EXT_BAND_TRIES; ++attempt) {
            const int w = o.w << attempt;
            sp.score = bsw(sp.len2, &seq[sp.idq], sp.len1, &seq[sp.idr], w, sp.h0, &bo, &sp.qle, &sp.tle, &sp.gtle, &sp.gscore, &sp.max_off, nullptr);
            if (ext_fold<LEFT>(a, sp, w, attempt + 1 == EXT_BAND_TRIES, o, l_query)) { seedcov(a, sd, ch.n_seeds); break; }
        }
    }
    // both sides of the seed whose record is a: left, then right from the left result's score
    void extend(meme_alnreg& a, int c, int il) {
        const Chain& ch = chains[c];
        const meme_chain_seed t = seeds[ch.seed_beg + il];
        const ExtGeom g = ext_geom(t, rmax[2 * c], rmax[2 * c + 1], l_query);
        const size_t before = seq.size();
        const int64_t jobs_before = tally[2];
        if (g.sideL) side<true>(a, ch, t, g, t.len * o.a);
        if (g.sideR) side<false>(a, ch, t, g, a.score);
        tally[0] += g.jobs(); tally[1] += g.bytesL + g.bytesR; tally[3] += (int64_t)(seq.size() - before);
        if (tally[2] - jobs_before != g.jobs() || (int64_t)(seq.size() - before) != g.bytesL + g.bytesR) ++tally[4];
    }
    bool dropped(int cur, const Chain& ch, int k) const {
        const meme_chain_seed* sd = seeds + ch.seed_beg;
        const int* co = &ord[ch.seed_beg];
        const meme_chain_seed s = sd[co[k]];
        bool found = false;
        for (int i = 0; i < cur && !found; ++i) found = ext_covers(out[i].rb, out[i].re, out[i].qb, out[i].qe, out[i].w, out[i].seedlen0, s, l_query, o);
        if (!found) return false;
        for (int u = k + 1; u < ch.n_seeds; ++u) if (co[u] >= 0 && ext_other_diagonal(s, sd[co[u]])) return false;
        return true;
    }
    // the walk in extension order; rounds: a seed is extended when the walk finds it alive, else everything is extended first
    void run(float frac_rep, bool rounds) {
        records(frac_rep);
        if (!rounds) for (int c = 0; c < nc; ++c) for (int k = chains[c].n_seeds - 1; k >= 0; --k) extend(out[chains[c].seed_beg + chains[c].n_seeds - 1 - k], c, ord[chains[c].seed_beg + k]);
        int cur = 0;
        for (int c = 0; c < nc; ++c)
            for (int k = chains[c].n_seeds - 1; k >= 0; --k, ++cur) {
                if (dropped(cur, chains[c], k)) { out[cur].qb = -1; out[cur].qe = -1; ord[chains[c].seed_beg + k] = -1; }
                else if (rounds) extend(out[cur], c, ord[chains[c].seed_beg + k]);
            }
    }
};

extern "C" void t_extend_batch(const uint8_t* reads, const int64_t* read_off, int64_t n, const int64_t* chain_off, const Chain* chains, const int64_t* seed_off,
                               const meme_chain_seed* seeds, const int* score, const float* frac_rep, const uint8_t* text, int64_t l_pac, const int64_t* contig_off,
                               const int* contig_len, int n_contigs, const meme_ext_opt* o, int rounds, bsw_fn bsw, meme_alnreg* out, int64_t* tally) {
    const Ref X{text, l_pac, contig_off, contig_len, n_contigs};
    for (int64_t r = 0; r < n; ++r) {
        ReadExt E{reads + read_off[r], (int)(read_off[r + 1] - read_off[r]), chains + chain_off[r], (int)(chain_off[r + 1] - chain_off[r]), seeds + seed_off[r],
                  score ? score + seed_off[r] : nullptr, X, *o, bsw, out + seed_off[r], tally, {}, {}, {}};
        E.run(frac_rep[r], rounds != 0);
    }
}

// mem_flt_chained_seeds: hsp[r] = the read's bar, -1 where the filter does not run; seeds that stay packed into seeds2 / score2, kept[r] of read r, chains updated
extern "C" int64_t t_flt_batch(const uint8_t* reads, const int64_t* read_off, int64_t n, const int64_t* chain_off, Chain* chains, const int64_t* seed_off,
                               const meme_chain_seed* seeds, const int* hsp, const uint8_t* text, int64_t l_pac, const int64_t* contig_off, const int* contig_len, int n_contigs,
                               const meme_ext_opt* o, sw_fn sw, meme_chain_seed* seeds2, int* score2, int64_t* kept) {
    int64_t n_sw = 0, d = 0;
    for (int64_t r = 0; r < n; ++r) {
        const uint8_t* read = reads + read_off[r];
        const int l_query = (int)(read_off[r + 1] - read_off[r]);
        int k_read = 0;
        for (int64_t c = chain_off[r]; c < chain_off[r + 1]; ++c) {
            int kc = 0;
            for (int j = 0; j < chains[c].n_seeds; ++j) {
                const meme_chain_seed t = seeds[seed_off[r] + chains[c].seed_beg + j];
                int v = FLT_OFF;
                if (hsp[r] >= 0) {
                    v = -1;
                    const FltWindow W = flt_window(t, l_query, l_pac, contig_off, contig_len, n_contigs, 200);
                    if (W.job) { v = sw(W.qe - W.qb, read + W.qb, text, l_pac, W.rb, (int)(W.re - W.rb), o); ++n_sw; }
                }
                if (!flt_keeps(v, hsp[r])) continue;
                seeds2[d] = t; score2[d] = flt_kept_score(v, t.len, o->a);
                ++d; ++kc;
            }
            chains[c].seed_beg = k_read; chains[c].n_seeds = kc;
            k_read += kc;
        }
        kept[r] = k_read;
    }
    return n_sw;
}

// w[5 k ..]: job, rb, re, qb, qe of flt_window for seed k of a read of l_query bases
extern "C" void t_flt_window(int64_t n, const meme_chain_seed* seeds, int l_query, int64_t l_pac, const int64_t* contig_off, const int* contig_len, int n_contigs, int64_t* w) {
    for (int64_t k = 0; k < n; ++k) {
        const FltWindow W = flt_window(seeds[k], l_query, l_pac, contig_off, contig_len, n_contigs, 200);
        w[5 * k] = W.job; w[5 * k + 1] = W.rb; w[5 * k + 2] = W.re; w[5 * k + 3] = W.qb; w[5 * k + 4] = W.qe;
    }
}
'''

_p = lambda a: C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("ext_rules")
    src = d / "t_ext_rules.cpp"
    src.write_text(DRIVER)
    so = str(d / "libt_ext_rules.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(REPO, "bwa-meme_amd", "csrc"), "-I" + os.path.join(REPO, "include"),
                    str(src), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.t_flt_batch.restype = C.c_int64
    return lib


def _flat(I, chains=None, seed_off=None, seeds=None):
    return dict(reads=np.ascontiguousarray(I["reads"], np.uint8), read_off=np.ascontiguousarray(I["read_off"], np.int64), chain_off=np.ascontiguousarray(I["chain_off"], np.int64),
                chains=np.array(I["chains"] if chains is None else chains, O.ORC_CHAIN_DTYPE), seed_off=np.ascontiguousarray(I["seed_off"] if seed_off is None else seed_off, np.int64),
                seeds=np.ascontiguousarray(I["seeds"] if seeds is None else seeds, O.ORC_CSEED_DTYPE), frac_rep=np.ascontiguousarray(I["frac_rep"], np.float32),
                text=np.ascontiguousarray(I["text"], np.uint8), contig_off=np.ascontiguousarray(I["contig_off"], np.int64), contig_len=np.ascontiguousarray(I["contig_len"], np.int32))


def _extend(lib, I, F, opt, rounds, score=None):
    """(records, tally) of the driver over a batch; opt: O.OrcExtOpt (the ten fields of meme_ext_opt, same order)"""
    bsw = C.cast(O.lib().orc_bsw_extend, C.c_void_p)
    out = np.zeros(int(F["seed_off"][-1]), hipapi.ALNREG)
    tally = np.zeros(5, np.int64)
    if score is not None:
        score = np.ascontiguousarray(score, np.int32)
    lib.t_extend_batch(_p(F["reads"]), _p(F["read_off"]), C.c_int64(F["read_off"].shape[0] - 1), _p(F["chain_off"]), _p(F["chains"]), _p(F["seed_off"]), _p(F["seeds"]),
                       _p(score) if score is not None else C.c_void_p(0), _p(F["frac_rep"]), _p(F["text"]), C.c_int64(int(I["l_pac"])), _p(F["contig_off"]), _p(F["contig_len"]),
                       C.c_int(F["contig_off"].shape[0]), C.byref(opt), C.c_int(rounds), bsw, _p(out), _p(tally))
    return out, tally


def _assert_fields(regs, want, frac_bits, where):
    """regs: ALNREG records; want: the fixture's int64 columns or the oracle's records"""
    for k, f in enumerate(O.ALNREG_FIELDS):
        w = want[:, k] if want.dtype == np.int64 else want[f].astype(np.int64)
        bad = np.nonzero(regs[f].astype(np.int64) != w)[0]
        assert bad.size == 0, (where, f, int(bad[0]), int(regs[f][bad[0]]), int(w[bad[0]]))
    assert np.array_equal(regs["frac_rep"].view(np.uint32), frac_bits), where


def _assert_plan_equals_pose(tally, n_seeds_extended):
    assert tally[4] == 0 and tally[0] == tally[2] and tally[1] == tally[3] and tally[0] > n_seeds_extended, tally


@pytest.fixture(scope="module")
def golden():
    I = ext_golden_inputs()
    return I, _flat(I), np.load(os.path.join(GOLDEN, "ext_golden.npz"))


def test_golden_fixture_crosses_the_seams_of_the_lane_code(golden):
    I, F, G = golden
    per_read = np.diff(F["seed_off"])
    assert per_read.shape[0] == 3100 and int(F["seed_off"][-1]) == G["regs"].shape[0] == 16802
    assert int((per_read == 8).sum()) == 66 and int((per_read == 9).sum()) == 28 and int(per_read.max()) == 75       # EXT_LIGHT's two sides, one 64-record chunk crossed


def test_batch_order_equals_the_reference_golden_and_the_plan_equals_the_pose(driver, golden):
    I, F, G = golden
    regs, tally = _extend(driver, I, F, O.default_ext_opt(), 0)
    _assert_fields(regs, G["regs"], G["frac_rep_bits"], "batch")
    assert not regs["n_comp_is_alt"].any() and not regs["hash"].any() and not regs["flg"].any()
    _assert_plan_equals_pose(tally, regs.shape[0])          # every seed of the fixture: job and byte counts of the geometry == the SeqPairs posed


def test_rounds_order_gives_the_golden_survivors(driver, golden):
    I, F, G = golden
    regs, tally = _extend(driver, I, F, O.default_ext_opt(), 1)
    keep = G["regs"][:, 3] > G["regs"][:, 2]
    assert 0 < int(keep.sum()) < keep.shape[0]
    assert np.array_equal(regs["qe"] > regs["qb"], keep)
    _assert_fields(regs[keep], G["regs"][keep], G["frac_rep_bits"][keep], "rounds")
    _assert_plan_equals_pose(tally, int(keep.sum()))
    assert tally[0] < _extend(driver, I, F, O.default_ext_opt(), 0)[1][0]       # (the purged seeds were not extended)


@pytest.mark.parametrize("w,clip,zdrop", [(20, 5, 100), (100, 0, 30)])
def test_both_orders_equal_the_oracle_with_other_options(driver, golden, w, clip, zdrop):
    I, F, _ = golden
    oo = O.default_ext_opt(w)
    oo.pen_clip5 = oo.pen_clip3 = clip
    oo.zdrop = zdrop
    want, _ = O.extend_batch(I["reads"], I["read_off"], I["chain_off"], I["chains"], I["seed_off"], I["seeds"], I["frac_rep"], I["text"], I["l_pac"],
                             I["contig_off"], I["contig_len"], oo)
    regs, tally = _extend(driver, I, F, oo, 0)
    _assert_fields(regs, want, want["frac_rep"].view(np.uint32), "batch")
    _assert_plan_equals_pose(tally, regs.shape[0])
    keep = want["qe"] > want["qb"]
    regs, _ = _extend(driver, I, F, oo, 1)
    assert np.array_equal(regs["qe"] > regs["qb"], keep)
    _assert_fields(regs[keep], want[keep], want["frac_rep"].view(np.uint32)[keep], "rounds")


@pytest.mark.parametrize("W,penalties", [(5, None), (10, None), (20, None), (20, (2, 9, 3, 2, 5, 1))])
def test_seed_filter_window_and_the_records_behind_it_equal_the_oracle(driver, W, penalties):
    """flt_window / flt_keeps / flt_kept_score: the seeds that stay, their scores and the number of alignments equal orc_flt_batch's (whose orc_seed_sw poses its own
    window: equal scores on every seed = the same windows aligned); behind it, with those scores as the extension order, both orders equal orc_extend_batch_scored."""
    I = flt_workload(W, lo=420, hi=500)
    oo = O.default_ext_opt()
    if penalties:
        oo.a, oo.b, oo.o_del, oo.e_del, oo.o_ins, oo.e_ins = penalties
    chains, soff, seeds, score, n_sw = O.flt_batch(I["reads"], I["read_off"], I["chain_off"], I["chains"], I["seed_off"], I["seeds"], I["text"], I["l_pac"],
                                                   I["contig_off"], I["contig_len"], oo, W)
    F = _flat(I)
    n = F["read_off"].shape[0] - 1
    hsp = np.array([flt_hsp(int(l), W, oo.a) for l in np.diff(F["read_off"])], np.int32)
    assert (hsp >= 0).any() and ((hsp < 0).any() or W == 5)          # (-W 5: every read; -W 20: the reads of 440 bases and more)
    seeds2 = np.zeros(F["seeds"].shape[0], O.ORC_CSEED_DTYPE); score2 = np.zeros(F["seeds"].shape[0], np.int32); kept = np.zeros(n, np.int64)
    got_sw = driver.t_flt_batch(_p(F["reads"]), _p(F["read_off"]), C.c_int64(n), _p(F["chain_off"]), _p(F["chains"]), _p(F["seed_off"]), _p(F["seeds"]), _p(hsp), _p(F["text"]),
                                C.c_int64(int(I["l_pac"])), _p(F["contig_off"]), _p(F["contig_len"]), C.c_int(F["contig_off"].shape[0]), C.byref(oo),
                                C.cast(O.lib().orc_seed_sw_window, C.c_void_p), _p(seeds2), _p(score2), _p(kept))
    assert got_sw == n_sw > 500
    assert np.array_equal(np.concatenate([[0], np.cumsum(kept)]), soff)
    assert np.array_equal(seeds2[:soff[-1]], seeds) and np.array_equal(score2[:soff[-1]], score)
    assert all(np.array_equal(F["chains"][f], chains[f]) for f in ("seed_beg", "n_seeds"))
    assert W < 20 or int(I["seed_off"][-1] - soff[-1]) > 0
    want, _ = O.extend_batch(I["reads"], I["read_off"], I["chain_off"], chains, soff, seeds, I["frac_rep"], I["text"], I["l_pac"], I["contig_off"], I["contig_len"],
                             oo, seed_score=score)
    F2 = _flat(I, chains=F["chains"], seed_off=soff, seeds=seeds2[:soff[-1]])
    regs, tally = _extend(driver, I, F2, oo, 0, score=score2)
    _assert_fields(regs, want, want["frac_rep"].view(np.uint32), "batch")
    _assert_plan_equals_pose(tally, regs.shape[0])
    keep = want["qe"] > want["qb"]
    regs, _ = _extend(driver, I, F2, oo, 1, score=score2)
    assert np.array_equal(regs["qe"] > regs["qb"], keep)
    _assert_fields(regs[keep], want[keep], want["frac_rep"].view(np.uint32)[keep], "rounds")


def test_window_clamp_and_contig_search_at_the_strand_boundary_and_contig_edges(driver):
    """flt_window with the shared pieces under it (ext_span_finish, bns_contig_of, bns_clamp: what k_ext_jobs, k_flt_pose and k_mate_plan call) against the plain
    restatement of mem_seed_sw's window and bns_fetch_seq in common.seed_sw_window, on seeds placed where the pieces matter: across l_pac, within SEEDSW_EXT bases of
    a sequence's first and last base on both strands, at the ends of the text, too long for a job."""
    rng = np.random.default_rng(811)
    l_pac, l_query, ext = 90_000, 250, 50
    contig_off = np.array([0, 20_011, 20_050, 61_003], np.int64)           # (a 39-base sequence: shorter than a window)
    contig_len = np.diff(np.concatenate([contig_off, [l_pac]])).astype(np.int32)
    edges = np.concatenate([contig_off, [l_pac]])
    edges = np.concatenate([edges, 2 * l_pac - edges])                     # every sequence end on either strand, l_pac and the ends of the text among them
    rows = []
    for e in edges:
        for d in range(-ext - 40, ext + 41, 3):
            ln = int(rng.integers(19, 120))
            rows.append((e + d, int(rng.integers(0, l_query - ln + 1)), ln))           # starts near the edge
            rows.append((e + d - ln, int(rng.integers(0, l_query - ln + 1)), ln))      # ends near it
    rows += [(int(rng.integers(0, 2 * l_pac - 240)), int(rng.integers(0, 10)), ln) for ln in (150, 199, 200, 201, 240) for _ in range(20)]
    rows += [(int(rng.integers(0, 2 * l_pac - 120)), int(rng.integers(0, l_query - 119)), int(rng.integers(19, 120))) for _ in range(2000)]
    rows = [(rb, qb, ln) for rb, qb, ln in rows if rb >= 0 and rb + ln <= 2 * l_pac]
    seeds = np.zeros(len(rows), O.ORC_CSEED_DTYPE)
    seeds["rbeg"], seeds["qbeg"], seeds["len"] = np.array(rows, np.int64).T
    got = np.zeros((seeds.shape[0], 5), np.int64)
    driver.t_flt_window(C.c_int64(seeds.shape[0]), _p(seeds), C.c_int(l_query), C.c_int64(l_pac), _p(contig_off), _p(contig_len), C.c_int(contig_off.shape[0]), _p(got))
    kinds = {"straddles": 0, "fwd_first": 0, "fwd_last": 0, "rev_first": 0, "rev_last": 0, "no_job": 0}
    for k, (rb, qb, ln) in enumerate(rows):
        want = seed_sw_window(rb, qb, ln, l_query, l_pac, contig_off, contig_len)
        assert (want is None) == (got[k, 0] == 0), (k, rows[k])
        if want is None:
            kinds["no_job"] += 1
            continue
        assert tuple(int(x) for x in got[k, 1:]) == want, (k, rows[k], want)
        mid = (rb + rb + ln) >> 1
        rev = mid >= l_pac
        fpos = 2 * l_pac - 1 - mid if rev else mid
        rid = int(np.searchsorted(contig_off, fpos, side="right") - 1)
        beg, end = int(contig_off[rid]), int(contig_off[rid] + contig_len[rid])
        f_rb, f_re = (2 * l_pac - (rb + ln), 2 * l_pac - rb) if rev else (rb, rb + ln)      # the seed on the forward strand
        kinds["straddles"] += rb < l_pac < rb + ln
        kinds[("rev_" if rev else "fwd_") + "first"] += 0 <= f_rb - beg < ext
        kinds[("rev_" if rev else "fwd_") + "last"] += 0 <= end - f_re < ext
    assert all(v > 0 for v in kinds.values()), kinds
