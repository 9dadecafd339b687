"""The re-seeding kernels fetch suffix-array and plcp windows four lanes wide: the lanes of a quad serve each other in four sub-rounds, so
every lane of a wavefront has to be inside the cooperative calls whether it has work or not.  These batches leave quads, wavefronts and
workgroups with missing or idle members at every level; the seeds must equal the oracle's with the re-seeding kernels (seed_defer 1) and
without them (seed_defer 0)."""
import numpy as np
import pytest

import oracle_py as O
from common import build_index
from pymeme import hipapi, synth, workload

pytestmark = pytest.mark.gpu

SMEM_CAP, HIT_CAP = 1024, 1 << 16          # the oracle's per-read capacities (it raises when a read exceeds them)


def flat_batch(reads):
    """A list of reads of any lengths -> (codes, offsets)."""
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in reads])
    return np.concatenate(reads).astype(np.uint8), off


def ragged_reads(g):
    reads, _, _ = synth.make_reads(g, 1027, 150, seed=611)
    return reads


def short_reads(g):
    reads, _, _ = synth.make_reads(g, 512, 25, seed=612, indel_rate=0.0)
    return reads


def one_owner_batch(g, j):
    """150-bp reads where index % 4 == j, 25-bp reads (shorter than split_len: never re-seeded) elsewhere."""
    long_, short = ragged_reads(g)[:512], short_reads(g)
    return flat_batch([long_[i] if i % 4 == j else short[i] for i in range(512)])


def unequal_batch(g):
    """Noisy 250-bp reads (many regions, regions that block repeatedly) next to exact 101-bp reads and reads with 5 % N."""
    a, _, _ = synth.make_reads(g, 400, 250, seed=613, sub_rate=0.05, indel_rate=0.0075)
    b, _, _ = synth.make_reads(g, 400, 101, seed=614, exact_frac=1.0)
    c, _, _ = synth.make_reads(g, 400, 150, seed=615, n_frac=0.05)
    return flat_batch([x[i] for i in range(400) for x in (a, b, c)])


def tiny_genome():
    """A few thousand bases with an exact duplication and runs of A and of T: queries that sort first and last in the suffix array."""
    rng = np.random.default_rng(616)
    g = rng.integers(0, 4, size=4000, dtype=np.uint8)
    g[2600:2900] = g[700:1000]                                   # exact duplication
    for k, at in enumerate((300, 1500, 3300)):
        g[at:at + 24] = 0                                        # A runs (T runs on the other strand)
        g[at + 24] = 1 + k % 3
        g[at + 200:at + 224] = 3                                 # T runs
        g[at + 224] = k % 3
    return g


def tiny_batch(g):
    """Every 60-bp window over the runs and over the duplication's ends, exact, and the same windows with one substitution."""
    starts = []
    for at in (300, 1500, 3300):
        starts += list(range(at - 50, at + 20, 3)) + list(range(at + 150, at + 220, 3))
    for edge in (700, 1000, 2600, 2900):
        starts += list(range(edge - 55, edge - 4, 4))
    reads = [g[s:s + 60].copy() for s in starts]
    for r in [x.copy() for x in reads[::2]]:
        r[7] = (r[7] + 1) % 4
        reads.append(r)
    return flat_batch(reads)


def oracle_dump(idx, reads, off, params=None, first=None):
    sm, ns, hits, nh, _ = O.seed_batch(idx, reads, off, params=params, smem_cap=SMEM_CAP, hit_cap=HIT_CAP, threads=0)
    if first is None:
        return O.format_seed_dump(sm, ns, hits)
    return {n: O.format_seed_dump(sm[:n], ns[:n], hits[:n]) for n in first}


def gpu_dump(c, reads, off, opt=None):
    smems, smem_off, hits, hit_off = c.seed_batch(reads, off, opt or hipapi.default_seed_opt(rounds=3))
    slots, counts, hl = hipapi.smems_to_slots(smems, smem_off, hits, hit_off)
    return O.format_seed_dump(slots, counts, hl)


def check(c, reads, off, want, opt=None, cap=128):
    c.set_tuning("smem_cap", cap)
    for defer in (1, 0):
        c.set_tuning("seed_defer", defer)
        assert gpu_dump(c, reads, off, opt) == want, "seed_defer %d" % defer
        if defer:
            assert c.timings().seed_reseed_ms > 0


class Case:
    """The shared index (the repeat-rich recipe of test_reseeding_on_the_plcp_table_equals_searching at 2 Mbp), one context on it, and
    the oracle's answers, each computed once."""

    def __init__(self, workdir):
        self.g = synth.make_genome(2_000_000, seed=17, repeat_frac=0.10, repeat_len=350, n_families=6, divergence=0.02, n_dups=30,
                                   dup_len=3000, poly_runs=8)
        self.prefix = workload.build_index_on_disk(self.g, workdir, bits=0, threads=8)
        self.idx = O.load_index_files(self.prefix)
        self.want = {}

    def oracle(self, key, make):
        if key not in self.want:
            self.want[key] = make()
        return self.want[key]


RAGGED = (1, 3, 5, 63, 65, 257, 1027)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(str(tmp_path_factory.mktemp("reseed_quads")))


@pytest.fixture(scope="module")
def ctx(case):
    c = hipapi.Context(0)
    c.load_index_files(case.prefix)
    yield c
    c.close()


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_batches(case, ctx, n):
    reads = ragged_reads(case.g)
    off = np.arange(0, 1028 * 150, 150, dtype=np.int64)
    want = case.oracle("ragged", lambda: oracle_dump(case.idx, reads, off, first=RAGGED))
    check(ctx, reads[:n], off[:n + 1], want[n])


@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_one_owner_per_quad(case, ctx, j):
    reads, off = one_owner_batch(case.g, j)
    check(ctx, reads, off, case.oracle(("owner", j), lambda: oracle_dump(case.idx, reads, off)))


def test_unequal_work_in_a_quad(case, ctx):
    reads, off = unequal_batch(case.g)
    check(ctx, reads, off, case.oracle("unequal", lambda: oracle_dump(case.idx, reads, off)))


def test_appends_that_overflow(case, ctx):
    """16 SMEM slots per read: SMEMs appended by the re-seeding kernels overflow, and the read goes to the next tier from there."""
    reads, off = unequal_batch(case.g)
    check(ctx, reads, off, case.oracle("unequal", lambda: oracle_dump(case.idx, reads, off)), cap=16)
    assert ctx.timings().seed_launches >= 2


def test_windows_clamped_at_both_ends_of_the_suffix_array(tmp_path):
    g = tiny_genome()
    fa = str(tmp_path / "tiny.fa")
    synth.write_fasta(fa, g)
    prefix = build_index(fa, bits=4)
    idx = O.load_index_files(prefix)
    reads, off = tiny_batch(g)
    sm, ns, hits, nh, _ = O.seed_batch(idx, reads, off, smem_cap=SMEM_CAP, hit_cap=HIT_CAP, threads=0)
    # the batch does hold SMEMs of several occurrences whose suffix-array intervals touch the array's first and last slots
    n = idx.sa.shape[0]
    slot_of = np.zeros(n, np.int64)
    slot_of[idx.sa.astype(np.int64)] = np.arange(n)
    lo, hi = n, -1
    for r in range(ns.shape[0]):
        for m in sm[r, :ns[r]]:
            if m["hitcount"] >= 2:
                s = slot_of[hits[r, m["hitbeg"]:m["hitbeg"] + m["hitcount"]].astype(np.int64)]
                lo, hi = min(lo, int(s.min())), max(hi, int(s.max()))
    assert lo < 4 and hi > n - 5, (lo, hi, n)
    c = hipapi.Context(0)
    try:
        c.load_index_files(prefix)
        check(c, reads, off, O.format_seed_dump(sm, ns, hits))
    finally:
        c.close()


def test_another_option_set(case, ctx):
    reads, off = unequal_batch(case.g)
    opt = hipapi.default_seed_opt(rounds=3)
    opt.min_seed_len, opt.split_len, opt.split_width = 25, 40, 3
    p = O.default_seed_params(3)
    p.min_seed_len, p.split_len, p.split_width = 25, 40, 3
    check(ctx, reads, off, case.oracle("unequal_opt", lambda: oracle_dump(case.idx, reads, off, params=p)), opt=opt)
