"""A blocked region's lane search stops at what the region reads: the match length from the best slot's two neighbours (r_L = max(a, b)), the
interval only in stage 2 with r_L >= min_seed_len.  The inputs are the smallest at which those paths can go wrong: best slots at either end of
the suffix array (a neighbour that does not exist), runs of 17 and 40 suffixes that leave the 16-entry cached window (neighbours and run walks
outside it), SMEMs of two and more occurrences emitted from stage 2, another option set, and batches that leave quads and wavefronts with idle
members while others return early.  Every read of every batch is compared with the oracle, with the re-seeding kernels (seed_defer 1) and
without them (seed_defer 0)."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
from common import build_index
from pymeme import hipapi, synth
from test_gpu_reseed_quads import HIT_CAP, SMEM_CAP, flat_batch, gpu_dump, oracle_dump, tiny_batch, tiny_genome

pytestmark = pytest.mark.gpu

GENOME_BP = 200_000
COPIES = (3, 17, 40)
RAGGED = (1, 3, 63, 65, 257)


def planted_genome(word_len, copies, seed, words_per_family=2):
    """A random genome with families of `copies[k]` copies of a word of word_len[0]..word_len[1] bases inside otherwise unique sequence.  The first
    copy of a family is the one reads are drawn from; the bases next to every other copy differ from the bases next to it, so that the family
    shares the word and not one base more.  Returns (genome, [(position of the first copy, word length, copies)])."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, size=GENOME_BP, dtype=np.uint8)
    n_loci = sum(copies) * words_per_family
    at = 1000 + 900 * rng.permutation((GENOME_BP - 2000) // 900)[:n_loci]        # loci at least 900 bases apart
    fams, k = [], 0
    for c in copies:
        for _ in range(words_per_family):
            m = int(rng.integers(word_len[0], word_len[1] + 1))
            w = rng.integers(0, 4, size=m, dtype=np.uint8)
            first = int(at[k])
            for j in range(c):
                p = int(at[k]); k += 1
                g[p:p + m] = w
                if j:
                    g[p - 1] = (g[first - 1] + 1 + j % 3) % 4
                    g[p + m] = (g[first + m] + 1 + (j // 3) % 3) % 4
            fams.append((first, m, c))
    return g, fams


def planted_reads(g, fams, seed):
    """Reads of 60..150 bases around each family's first copy.  One substitution cuts a read into two SMEMs; the one that holds the word is unique
    and at least split_len bases long, and the word lies to the left of, at, or to the right of its middle, or against either of its ends --
    there the zig-zag's queries run into the substitution, which the plcp table cannot see."""
    rng = np.random.default_rng(seed)
    reads = []
    for first, m, _ in fams:
        for side in (0, 1):                            # the SMEM with the word lies before / behind the substitution
            for place in range(5):                     # word against the SMEM's far end, left of, at, right of the middle, against the substitution
                for rep in range(9 if place in (0, 4) else 3):
                    x = int(rng.integers(m + 12, m + 30)) if place in (0, 4) else int(rng.integers(30, 46)) + m + int(rng.integers(30, 46))
                    room = x - m                       # bases of the SMEM outside the word
                    before = (0, room // 4, room // 2, room - room // 4, room)[place]
                    if side == 0:                      # SMEM = read[0, x), substitution at x
                        s = first - before
                        length = int(np.clip(x + 1 + rng.integers(20, 60), 60, 150))
                        sub = x
                    else:                              # substitution at `lead`, SMEM = read[lead + 1, lead + 1 + x)
                        lead = int(rng.integers(20, 60))
                        s = first - before - lead - 1
                        length = int(np.clip(lead + 1 + x, 60, 150))
                        sub = lead
                    r = g[s:s + length].copy()
                    r[sub] = (r[sub] + 1 + rep % 3) % 4
                    if side == 1 and lead + 1 + x < length:
                        r[lead + 1 + x] = (r[lead + 1 + x] + 1) % 4      # ... and ends at a second substitution
                    reads.append(r)
    order = rng.permutation(len(reads))                # neighbours in a quad are unlike each other
    return [reads[i] for i in order]


class Planted:
    def __init__(self, tmp, name, word_len, copies, seed, words_per_family=2):
        self.g, self.fams = planted_genome(word_len, copies, seed, words_per_family)
        fa = str(tmp / (name + ".fa"))
        synth.write_fasta(fa, self.g)
        self.prefix = build_index(fa, bits=8)
        self.idx = O.load_index_files(self.prefix)
        self.reads = planted_reads(self.g, self.fams, seed + 1)
        self.want = {}

    def oracle(self, key, make):
        if key not in self.want:
            self.want[key] = make()
        return self.want[key]


@pytest.fixture(scope="module")
def short_words(tmp_path_factory):
    """families of 3, 17 and 40 copies of a 14..18-base word: shorter than a seed, runs wider than the cached window"""
    return Planted(tmp_path_factory.mktemp("early_stop_a"), "short_words", (14, 18), COPIES, 701)


@pytest.fixture(scope="module")
def long_words(tmp_path_factory):
    """families of 17 and 40 copies of a 19..27-base word: SMEMs that stage 2 emits, with intervals wider than the cached window"""
    return Planted(tmp_path_factory.mktemp("early_stop_b"), "long_words", (19, 27), (17, 40), 703, words_per_family=3)


def open_ctx(prefix):
    c = hipapi.Context(0)
    c.load_index_files(prefix)
    return c


@pytest.fixture(scope="module")
def ctx_short(short_words):
    c = open_ctx(short_words.prefix)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_long(long_words):
    c = open_ctx(long_words.prefix)
    yield c
    c.close()


def check(c, reads, off, want, opt=None, cap=128):
    """Both ways of re-seeding against the oracle; returns the debug counts of the seed_defer 1 call."""
    c.set_tuning("smem_cap", cap)
    counts = None
    for defer in (1, 0):
        c.set_tuning("seed_defer", defer)
        assert gpu_dump(c, reads, off, opt) == want, "seed_defer %d" % defer
        if defer:
            assert c.timings().seed_reseed_ms > 0
            counts = c.debug_reseed_counts()
            print("reseed counts:", counts)
    return counts


def consistent(counts):
    # every search of the batch rounds is counted once by stage and once by outcome; the last pass adds to both
    assert sum(counts["stage"]) == counts["no_interval"] + counts["walked"]
    assert sum(counts["stage"]) >= sum(counts["rounds"])
    assert all(a >= b for a, b in zip(counts["rounds"], counts["rounds"][1:]))
    assert counts["walked"] <= counts["stage"][2]


def end_reads(g):
    """60-bp windows of the tiny genome with one substitution, made so that a blocked search's best slot is the suffix array's first or last.
    Over an A run (24 bases; six loci on the two strands): f unique bases, the run, and the base behind the run replaced
    by an A.  The first SMEM is [0, f + 24); the table blocks a rightward search from the run's start (plcp there is 24, all that is left of the
    SMEM), and its query A^25... sorts before every suffix: best slot 0, no slot below it.  The same over a T run: the query T^25... sorts behind
    every suffix, best slot n - 1, no slot above it.  f = 24 puts the region's middle on the run's start (stage 0); other f reach it by the
    zig-zag or not at all.  Also windows that end k bases into a T run behind a substitution: the last SMEM's queries are T^j, which every suffix
    that begins with T^j matches in full and sorts before -- best slot n - 1 again."""
    reads = []
    for at in (300, 1500, 3300):
        for run, base in ((at, 0), (at + 200, 3)):
            for f in (20, 22, 24, 26, 28, 30):
                r = g[run - f:run - f + 60].copy()
                assert (r[f:f + 24] == base).all() and r[f + 24] != base
                r[f + 24] = base
                reads.append(r)
        for k in (16, 18, 20, 22):
            for u in (12, 20, 28):
                e = at + 200 + k
                r = g[e - 60:e].copy()
                r[u] = (r[u] + 1) % 4
                reads.append(r)
    return flat_batch(reads)


def blocked_searches(idx, reads, off, msl=19, split_len=28):
    """The re-seeding of unique SMEMs restated on the CPU: the oracle's first-round SMEMs, the plcp table (orc_build_plcp), the region walk
    of DESIGN 3.1b, and for every search the table cannot answer the best slot by the kernels' ordering rule (a suffix that matches all of
    the query sorts before it) and the answer by brute force.  Returns [(stage, best slot, answer, occurrences of the answer counted up to 18)]."""
    text, sa = idx.text, idx.sa.astype(np.int64)
    n = text.shape[0]
    plcp = np.zeros(n, np.uint8)
    O.lib().orc_build_plcp(C.c_void_p(text.ctypes.data), C.c_void_p(idx.sa.ctypes.data), C.c_int64(n), C.c_void_p(plcp.ctypes.data))
    slot_of = np.zeros(n, np.int64)
    slot_of[sa] = np.arange(n)
    tb = bytes(text.tolist())
    p1 = O.default_seed_params(1)
    sm, ns, hits, nh, _ = O.seed_batch(idx, reads, off, params=p1, smem_cap=SMEM_CAP, hit_cap=HIT_CAP, threads=0)

    def lcp(x, y, cap):
        k = 0
        while k < cap and x + k < n and y + k < n and tb[x + k] == tb[y + k]:
            k += 1
        return k

    def compare(q, slot):                               # lane_compare_ent: (capped LCP, sorts before the query)
        pos = int(sa[slot])
        lc = min(len(q), n - pos)
        k = 0
        while k < lc and tb[pos + k] == q[k]:
            k += 1
        return (lc, pos < n - len(q)) if k >= lc else (k, tb[pos + k] < q[k])

    out = []
    for r in range(ns.shape[0]):
        rd = reads[off[r]:off[r + 1]]
        l_seq = rd.shape[0]
        for m in sm[r, :ns[r]]:
            qb, qe = int(m["start"]), int(m["end"])
            if qe - qb < split_len or m["hitcount"] != 1:
                continue
            t = int(hits[r, m["hitbeg"]])
            sl = int(slot_of[t])                        # not deferred when a neighbour shares a seed's length with the SMEM
            if (sl > 0 and lcp(t, int(sa[sl - 1]), qe - qb) >= msl) or (sl < n - 1 and lcp(t, int(sa[sl + 1]), qe - qb) >= msl):
                continue
            t0, pivot, nxt, guard, stage = t - qb, (qb + qe) >> 1, 0, 0, 0
            while stage != 3:
                inside = qb <= pivot < qe
                if stage == 1:
                    guard += 1
                    if pivot >= nxt or guard > 4 * l_seq + 16:
                        break
                    plc, room = (int(plcp[n - 1 - (t0 + pivot)]) if inside else 0), pivot - qb + 1
                else:
                    plc, room = (int(plcp[t0 + pivot]) if inside or stage == 0 else 0), qe - pivot
                searched = plc == 0 or plc == 255 or plc >= room
                if searched:
                    q = bytes(((3 - rd[::-1])[l_seq - 1 - pivot:] if stage == 1 else rd[pivot:]).tolist())
                    lo, hi = 0, len(q)                  # the longest prefix with two occurrences
                    while lo < hi:
                        mid = (lo + hi + 1) // 2
                        i1 = tb.find(q[:mid])
                        if i1 >= 0 and tb.find(q[:mid], i1 + 1) >= 0:
                            lo = mid
                        else:
                            hi = mid - 1
                    plc = lo
                    lo, hi = -1, n                      # partition point, then the better of the two slots around it
                    while hi - lo > 1:
                        mid = (lo + hi) // 2
                        if compare(q, mid)[1]:
                            lo = mid
                        else:
                            hi = mid
                    lm = compare(q, hi - 1)[0] if hi > 0 else -1
                    lp = compare(q, hi)[0] if hi < n else -1
                    occ, at = 0, tb.find(q[:plc])
                    while at >= 0 and occ < 18:
                        occ, at = occ + 1, tb.find(q[:plc], at + 1)
                    out.append((stage, hi - 1 if lm >= lp else hi, plc, occ))
                if stage == 0:
                    nxt, stage = pivot + plc, 1
                elif stage == 1:
                    pivot = pivot - plc + 1
                    stage = 3 if nxt - pivot < msl else 2
                else:
                    pivot, stage = pivot + plc, 1
    return out


def test_best_slot_at_either_end_of_the_suffix_array(tmp_path):
    g = tiny_genome()
    fa = str(tmp_path / "tiny.fa")
    synth.write_fasta(fa, g)
    prefix = build_index(fa, bits=4)
    idx = O.load_index_files(prefix)
    reads, off = end_reads(g)
    # on the CPU first: blocked searches whose best slot is the array's first (no slot below it) and its last (none above)
    n = idx.sa.shape[0]
    found = blocked_searches(idx, reads, off)
    first = [s for s in found if s[1] == 0]
    last = [s for s in found if s[1] == n - 1]
    print("blocked searches: %d, best slot 0: %s, best slot n - 1: %s" % (len(found), first, last))
    assert first and last, found
    assert any(s[0] == 2 and s[2] >= 19 for s in first + last) or any(s[0] == 0 for s in first + last)
    c = open_ctx(prefix)
    try:
        counts = check(c, reads, off, oracle_dump(idx, reads, off))
        consistent(counts)
        assert sum(counts["stage"]) >= len(first) + len(last), (counts, found)
        t2, t3 = tiny_batch(g)                          # ... and the quads' batch over the runs and the duplication's ends
        consistent(check(c, t2, t3, oracle_dump(idx, t2, t3)))
    finally:
        c.close()


def test_runs_that_leave_the_cached_window(short_words, ctx_short):
    reads, off = flat_batch(short_words.reads)
    counts = check(ctx_short, reads, off, short_words.oracle("all", lambda: oracle_dump(short_words.idx, reads, off)))
    consistent(counts)
    assert all(n > 0 for n in counts["stage"]), counts               # blocked searches in stages 0, 1 and 2
    assert counts["no_interval"] > 0 and counts["neighbour_probes"] > 0, counts


def test_appends_that_overflow(short_words, ctx_short):
    reads, off = flat_batch(short_words.reads)
    check(ctx_short, reads, off, short_words.oracle("all", lambda: oracle_dump(short_words.idx, reads, off)), cap=16)


def test_stage_2_that_emits(long_words, ctx_long):
    reads, off = flat_batch(long_words.reads)
    sm, ns, hits, nh, _ = O.seed_batch(long_words.idx, reads, off, smem_cap=SMEM_CAP, hit_cap=HIT_CAP, threads=0)
    # on the CPU first: stage-2 searches of blocked regions that emit (a seed's length or more) an interval wider than the cached window
    wide = [s for s in blocked_searches(long_words.idx, reads, off) if s[0] == 2 and s[2] >= 19 and s[3] > 16]
    print("stage-2 searches that emit more than 16 occurrences:", len(wide))
    assert wide
    counts = check(ctx_long, reads, off, O.format_seed_dump(sm, ns, hits))
    consistent(counts)
    assert counts["walked"] >= len(wide), counts


def test_another_option_set(short_words, ctx_short, long_words, ctx_long):
    opt = hipapi.default_seed_opt(rounds=3)
    opt.min_seed_len, opt.split_len, opt.split_width = 25, 40, 3
    p = O.default_seed_params(3)
    p.min_seed_len, p.split_len, p.split_width = 25, 40, 3
    for case, c in ((short_words, ctx_short), (long_words, ctx_long)):
        reads, off = flat_batch(case.reads)
        consistent(check(c, reads, off, case.oracle("opt", lambda: oracle_dump(case.idx, reads, off, params=p)), opt=opt))


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_batches(short_words, ctx_short, n):
    assert len(short_words.reads) >= max(RAGGED)
    reads, off = flat_batch(short_words.reads[:max(RAGGED)])
    want = short_words.oracle("ragged", lambda: oracle_dump(short_words.idx, reads, off, first=RAGGED))
    consistent(check(ctx_short, reads[:off[n]], off[:n + 1], want[n]))
