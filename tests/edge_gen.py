"""Reads at the ends of reference sequences, for every device stage (tests/test_edge_workload.py on the CPU, tests/test_gpu_edges.py on the device,
tests/golden/edge_golden.npz: the compiled reference's chains and records of this workload).

The genome is 15 169 random bases cut by explicit (offset, len, is_alt) tuples into eight sequences: 150 bases (exactly a read; the genome's first), 4 500, 19
(min_seed_len: too short to hold a seed and a flank), 700, 40, an ALT sequence of 4 000, 5 500 and 260 (just above a 250-base read; the genome's last, so its end is the strand junction
l_pac).  Reads of 60, 150 and 250 bases, each kind on both strands, for every sequence:

  perfect   the read starts k bases before the sequence's first base, or ends k bases behind its last one, k in OVERHANGS; the overhang is the neighbouring
            sequence's bases (random ones beyond the genome): reads that bridge two sequences, whose long seeds bridge too and are dropped by the chaining
  clipped   the same reads with unrelated bases in that overhang
  gap       a 3-base deletion or insertion GAP_AT bases from the sequence's first or last base: a flank too short to seed, so an extension crosses the gap
            with the sequence's end inside its band
  island    a whole sequence shorter than the read with unrelated bases on both sides of it: a seed from the sequence's first base to its last
  junction  text[l_pac - k : l_pac - k + L] of the fwd + rc text for k in 1, 19, 20, L / 2, L - 20, L - 19: reads across the strand junction

workload() returns the layout of common.ext_golden_inputs() -- seeds and chains from the oracle -- plus what the other stages need."""
import numpy as np

# (len, is_alt) in genome order
CONTIGS = ((150, 0), (4500, 0), (19, 0), (700, 0), (40, 0), (4000, 1), (5500, 0), (260, 0))
READ_LENS = (60, 150, 250)
OVERHANGS = (0, 1, 5, 18, 19, 20, 40)
GAP_AT, GAP_LEN = 14, 3
ISLAND_MIN = 40                 # sequences this long and longer get gap and island reads (the 19-base one is to stay without chains)
# (w, pen_clip5 = pen_clip3, zdrop) of the extension runs: the defaults (what the fixture holds), a band of 3 (most gap jobs retried), no clipping penalty with
# an early z-drop, a band of 1
EXT_OPTIONS = ((100, 5, 100), (3, 5, 100), (100, 0, 30), (1, 5, 100))
CHAIN_FIELDS = ("pos", "rid", "n_seeds", "w", "first", "kept", "is_alt", "seed_beg")       # seed_beg counts from the read's first chained seed
_PAD = 512                      # random bases in front of and behind the genome: what a read that leaves the genome reads there
_CACHE = {}


def _rc(r):
    return (3 - r[::-1]).astype(np.uint8)


def junction_offsets(L):
    return (1, 19, 20, L // 2, L - 20, L - 19)


def contig_table():
    """[(offset, len, is_alt)] of CONTIGS"""
    out, o = [], 0
    for ln, alt in CONTIGS:
        out.append((o, ln, alt))
        o += ln
    return out


def make_reads(seed=4201):
    """(genome, reads as a list of code arrays, kind label per read, sequence per read (-1: junction))"""
    rng = np.random.default_rng(seed)
    contigs = contig_table()
    l_pac = contigs[-1][0] + contigs[-1][1]
    g = rng.integers(0, 4, size=l_pac, dtype=np.uint8)
    wide = np.concatenate([rng.integers(0, 4, size=_PAD, dtype=np.uint8), g, rng.integers(0, 4, size=_PAD, dtype=np.uint8)])
    text = np.concatenate([g, _rc(g)])
    reads, kind, where = [], [], []

    def add(r, label, c):
        for strand in (0, 1):
            reads.append(np.ascontiguousarray(_rc(r) if strand else r, dtype=np.uint8)); kind.append(label); where.append(c)

    for c, (beg, ln, _) in enumerate(contigs):
        end = beg + ln
        for L in READ_LENS:
            for k in OVERHANGS:
                for first, a in ((True, beg - k), (False, end + k - L)):      # the read is wide[_PAD + a : _PAD + a + L]: over the first base, over the last one
                    r = wide[_PAD + a:_PAD + a + L].copy()
                    add(r, "perfect", c)
                    pos = np.arange(a, a + L)
                    out = (pos < beg) if first else (pos >= end)              # the overhang of k bases; the read's other end stays what the genome has there
                    r2 = r.copy()
                    r2[out] = rng.integers(0, 4, size=int(out.sum()), dtype=np.uint8)
                    add(r2, "clipped", c)
            if ln < ISLAND_MIN:
                continue
            if ln < L:                                                        # the whole sequence inside the read, unrelated bases on both sides of it
                for at in (1, (L - ln) // 2):
                    r = rng.integers(0, 4, size=L, dtype=np.uint8)
                    r[at:at + ln] = g[beg:end]
                    add(r, "island", c)
            for first in (True, False):
                for ins in (False, True):
                    # written from the sequence's edge inwards (and on into the neighbour where the read is longer), then turned round for the last base
                    src = wide[_PAD + beg:_PAD + beg + L + GAP_LEN] if first else wide[_PAD + end - L - GAP_LEN:_PAD + end][::-1]
                    mid = rng.integers(0, 4, size=GAP_LEN, dtype=np.uint8) if ins else src[:0]
                    r = np.concatenate([src[:GAP_AT], mid, src[GAP_AT + (0 if ins else GAP_LEN):]])[:L]
                    add(r if first else r[::-1], "gap", c)
    for L in READ_LENS:
        for k in junction_offsets(L):
            add(text[l_pac - k:l_pac - k + L].copy(), "junction", -1)
    return g, reads, np.array(kind), np.array(where, np.int32)


def workload():
    """dict in the layout of common.ext_golden_inputs(): genome, text, l_pac, contigs [(offset, len, is_alt)], contig_off / contig_len / contig_alt, reads,
    read_off, reads_list, the oracle's seeds (smems, n_smems, hits, n_hits of O.seed_batch on hostapi.build_sa's suffix array), the oracle's chains of them under
    the default options with the ALT flags (chain_off, chains, seed_off, seeds, tree_size, frac_rep), kind and sequence per read.  Cached: treat as read-only."""
    if "W" in _CACHE:
        return _CACHE["W"]
    import oracle_py as O
    from pymeme import hipapi, hostapi
    g, reads, kind, where = make_reads()
    contigs = contig_table()
    l_pac = g.shape[0]
    contig_off = np.array([c[0] for c in contigs], np.int64)
    contig_len = np.array([c[1] for c in contigs], np.int32)
    contig_alt = np.array([c[2] for c in contigs], np.uint8)
    text = hipapi.fwd_rc_text(g)
    _, sa = hostapi.build_sa(g)
    idx = O.Index(text, sa)
    read_off = np.zeros(len(reads) + 1, np.int64)
    read_off[1:] = np.cumsum([len(r) for r in reads])
    flat = np.concatenate(reads)
    sm, nsm, hits, nh, _ = O.seed_batch(idx, flat, read_off, smem_cap=512, hit_cap=1 << 14)
    copt = O.default_chain_opt(l_pac)
    ch_list, sd_list, frac, tree, coff, soff = [], [], [], [], [0], [0]
    for r in range(len(reads)):
        rc, ch, sd, tr, fr = O.chain_read(sm[r, :nsm[r]], hits[r, :nh[r]], len(reads[r]), contig_off, contig_alt, copt)
        assert rc >= 0
        ch_list.append(ch); sd_list.append(sd); frac.append(fr); tree.append(tr)
        coff.append(coff[-1] + rc); soff.append(soff[-1] + sd.shape[0])
    W = {"genome": g, "text": text, "l_pac": l_pac, "contigs": contigs, "contig_off": contig_off, "contig_len": contig_len, "contig_alt": contig_alt,
         "reads_list": reads, "reads": flat, "read_off": read_off, "smems": sm, "n_smems": nsm, "hits": hits, "n_hits": nh,
         "chain_off": np.array(coff, np.int64), "chains": np.concatenate(ch_list), "seed_off": np.array(soff, np.int64), "seeds": np.concatenate(sd_list),
         "tree_size": np.array(tree, np.int32), "frac_rep": np.array(frac, np.float32), "kind": kind, "contig_of_read": where}
    _CACHE["W"] = W
    return W


def seed_targets(W, a=1, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100):
    """Per chained seed, the target lengths mem_chain2aln_across_reads_V2 gives its left and right extension (reference src/bwamem.cpp:2648-2690 and 2722 / 2783,
    bns_fetch_seq src/bntseq.cpp:541-570), in Python integers: the chain's span rmax -- over its seeds, rbeg - (qbeg + max_gap(qbeg)) and the mirror image, inside
    the text, cut at l_pac on the first seed's strand, then inside the first seed's sequence -- and from it rbeg - rmax[0] and rmax[1] - (rbeg + len).
    -> (left, right) arrays over W["seeds"]; a side a seed does not have (it starts / ends the read) has length -1."""
    l_pac = W["l_pac"]

    def max_gap(q):
        l = max(int((q * a - o_del) / e_del + 1.), int((q * a - o_ins) / e_ins + 1.), 1)
        return min(l, w << 1)
    S = W["seeds"]
    rbeg, qbeg, ln = S["rbeg"].tolist(), S["qbeg"].tolist(), S["len"].tolist()
    left, right = np.full(len(rbeg), -1, np.int64), np.full(len(rbeg), -1, np.int64)
    for r in range(W["read_off"].shape[0] - 1):
        L = int(W["read_off"][r + 1] - W["read_off"][r])
        s0 = int(W["seed_off"][r])
        for ch in W["chains"][W["chain_off"][r]:W["chain_off"][r + 1]]:
            ks = range(s0 + int(ch["seed_beg"]), s0 + int(ch["seed_beg"]) + int(ch["n_seeds"]))
            if not len(ks):
                continue
            b = min(rbeg[k] - (qbeg[k] + max_gap(qbeg[k])) for k in ks)
            e = max(rbeg[k] + ln[k] + (L - qbeg[k] - ln[k]) + max_gap(L - qbeg[k] - ln[k]) for k in ks)
            b, e = max(b, 0), min(e, 2 * l_pac)
            first = rbeg[ks[0]]
            if b < l_pac < e:
                if first < l_pac:
                    e = l_pac
                else:
                    b = l_pac
            off, clen = int(W["contig_off"][ch["rid"]]), int(W["contig_len"][ch["rid"]])
            lo, hi = (off, off + clen) if first < l_pac else (2 * l_pac - off - clen, 2 * l_pac - off)
            b, e = max(b, lo), min(e, hi)
            for k in ks:
                if qbeg[k] > 0:
                    left[k] = rbeg[k] - b
                if qbeg[k] + ln[k] != L:
                    right[k] = e - (rbeg[k] + ln[k])
    return left, right


def ext_opt(mod, w, clip, zdrop):
    """the extension options of one EXT_OPTIONS row as mod's record (mod: oracle_py or pymeme.hipapi)"""
    o = mod.default_ext_opt(w)
    o.pen_clip5 = o.pen_clip3 = clip
    o.zdrop = zdrop
    return o


def oracle_records(W, w=100, clip=5, zdrop=100):
    """O.extend_batch of the workload's chains under one option set -> (records, (jobs, retried jobs)); cached"""
    import oracle_py as O
    key = ("regs", w, clip, zdrop)
    if key not in _CACHE:
        _CACHE[key] = O.extend_batch(W["reads"], W["read_off"], W["chain_off"], W["chains"], W["seed_off"], W["seeds"], W["frac_rep"], W["text"], W["l_pac"],
                                     W["contig_off"], W["contig_len"], ext_opt(O, w, clip, zdrop))
    return _CACHE[key]


def chain_seeds(chain_off, chains, seed_off, seeds):
    """the seeds of every chain in chain order, whatever the layout inside a read: (rbeg, qbeg, len) rows"""
    per_read = np.diff(np.asarray(chain_off))
    n = np.asarray(chains["n_seeds"], np.int64)
    first = np.repeat(np.asarray(seed_off)[:-1], per_read) + np.asarray(chains["seed_beg"], np.int64)
    idx = np.repeat(first - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))
    return np.stack([seeds["rbeg"][idx].astype(np.int64), seeds["qbeg"][idx].astype(np.int64), seeds["len"][idx].astype(np.int64)], 1)


def golden():
    """tests/golden/edge_golden.npz (tests/golden/make_edge_golden.py): the compiled reference's chains of the workload's seeds and its records of those chains
    under the default options -> dict(chain_off, chains [n, CHAIN_FIELDS], seeds [n, 3] in chain order, tree_size, frac_rep_bits per read, reg_off,
    regs [n, O.ALNREG_FIELDS], reg_frac_bits)"""
    import os
    if "G" not in _CACHE:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_golden.npz"))
        _CACHE["G"] = {k: z[k] for k in z.files}
    return _CACHE["G"]
