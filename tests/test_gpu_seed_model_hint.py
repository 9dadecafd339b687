"""The learned model is a hint: whatever the parameter tables hold, the seeding kernels give the oracle's seeds.

Every index here is loaded from arrays (`Context.load_index_host`), so any RMI_DTYPE tables can stand beside a correct text and suffix array.  The
oracle never sees a model: one expected dump per read set serves every model.  The model families force what an accurate model of a small text
almost never reaches: k_seed's relocation after a first window without the partition point (gallop down / up with the clamps at slot 0 and n - W,
bisection, the final window, the bracket mask), the placement of the first window from any error word, the probe-and-double branch of
lane_search in the re-seeding kernels, and rmi_lookup's third-layer route with pointers out of range, its one-record table and non-finite
predictions.  Besides the dumps the tests check that the number of searches does not depend on the model (where the counter can say so) and,
from `seed_windows`, that the relocation code really ran.  Read-back figures of every case: profiles/tests_model_as_hint.md; each case prints its own."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_py as O
from common import GOLDEN, build_index, entry_keys, pos5_image, read_fastq_codes
from pymeme import hipapi, hostapi, synth
from pymeme.hostapi import RMI_DTYPE

pytestmark = pytest.mark.gpu

U = np.uint64
EDGE = 68                                    # the widest window (64) plus the most a placement rule has moved one (4)
ERR_BELOW_MAX, ERR_ABOVE_MAX = 0x3fffffff, 0x7fffffff
SHIFTS = (11, 12, 13, 16, 17, 64, 65, 1000)


# ---- host restatements ---------------------------------------------------------------------------------------------------------------------
def read_keys(reads, off):
    """The key a search from any base of any read would look up, on both strands: the bases up to the next N or the read's end, at most 32 of
    them, T-padded.  Returns (keys, read index, valid bases capped at 32)."""
    out = []
    for strand in (0, 1):
        parts, rid = [], []
        for r in range(off.shape[0] - 1):
            s = reads[off[r]:off[r + 1]]
            if strand:
                s = np.where(s < 4, 3 - s, 4)[::-1]
            parts += [s, np.full(32, 4, np.uint8)]
            rid += [np.full(s.shape[0], r), np.full(32, -1)]
        p = np.concatenate(parts + [np.full(32, 4, np.uint8)]).astype(np.uint64)
        rid = np.concatenate(rid)
        m = p.shape[0] - 32
        alive = np.ones(m, bool)
        k = np.zeros(m, np.uint64)
        vlen = np.zeros(m, np.int64)
        for j in range(32):
            c = p[j:j + m]
            alive &= c < 4
            vlen += alive
            k = (k << U(2)) | np.where(alive, c, U(3))
        keep = (rid >= 0) & (vlen > 0)
        out.append((k[keep], rid[keep], vlen[keep]))
    return tuple(np.concatenate([o[i] for o in out]) for i in range(3))


def reads_no_first_window_can_serve(ix, reads, off):
    """Per read: True when no key the read can be searched under has a partition point within EDGE slots of either end of the suffix array.
    The partition point of a query lies between the first and the last slot its 32-base key could take (searchsorted left / right on the
    sorted entry keys).  Keys: every base of either strand as a start, with at least as many valid bases as the shortest query the pivot
    logic (the oracle's restatement of it) hands to a search for that read -- a superset of the queries the kernels can pose."""
    v0 = O.shortest_queries(ix.oracle, reads, off)
    k, rid, vlen = read_keys(reads, off)
    lo, hi = np.searchsorted(ix.keys, k, "left"), np.searchsorted(ix.keys, k, "right")
    bad = ~((lo > EDGE) & (hi < ix.n - EDGE)) & (v0[rid] > 0) & (vlen >= np.minimum(v0[rid], 32))
    ok = np.ones(off.shape[0] - 1, bool)
    ok[np.unique(rid[bad])] = False
    return ok


def predict(l2, l1, n, keys):
    """rmi_lookup in numpy for finite tables with well-formed routes: (predicted slot, error word).  A product and a sum where the kernel
    has one FMA: the callers allow two slots for that."""
    n2 = l2.shape[0]
    bits = n2.bit_length() - 1
    assert n2 == 1 << bits
    m = (keys >> U(64 - bits)).astype(np.int64) if bits else np.zeros(keys.shape[0], np.int64)
    x = keys.astype(np.float64)
    rec = l2[m]
    f = rec["slope"] * x + rec["icpt"]
    err = rec["err"].copy()
    routed = (err >> U(63)) != 0
    if routed.any():
        ps = ((err >> U(32)) & U(0x7fffffff)).astype(np.int64)
        pn = (err & U(0xffffffff)).astype(np.float64) - 1.0
        assert (pn[routed] >= 0).all()
        c = np.where(f >= 0.0, np.minimum(f, pn), 0.0)
        j = np.minimum(ps + c.astype(np.int64), max(l1.shape[0] - 1, 0))
        j = np.where(routed, j, 0)
        r1 = l1[j] if l1.shape[0] else np.zeros(keys.shape[0], RMI_DTYPE)
        f = np.where(routed, r1["slope"] * x + r1["icpt"], f)
        err = np.where(routed, r1["err"], err)
    return np.clip(np.floor(f), 0, n - 1).astype(np.int64), err


def first_window(pos, err, W, n):
    """k_seed's placement of the first window from the record's error word"""
    below = ((err >> U(32)) & U(ERR_BELOW_MAX)).astype(np.int64) + 1
    above = (err & U(ERR_ABOVE_MAX)).astype(np.int64)
    span = below + above + 1
    base = np.where(span <= W, pos - below - (W - span) // 2, pos - (below * W) // span)
    return np.clip(base, 0, n - W)


# ---- model families: (ix, rng) -> (l2, l1) -------------------------------------------------------------------------------------------------
def _table(n_rec, icpt=0.0, slope=0.0, err=0):
    t = np.zeros(n_rec, RMI_DTYPE)
    t["icpt"], t["slope"], t["err"] = icpt, slope, err
    return t


NO_L1 = np.zeros(0, RMI_DTYPE)


def _random_table(n_rec, n, rng):
    t = np.zeros(n_rec, RMI_DTYPE)
    t["icpt"] = rng.uniform(-n, 2 * n, n_rec)
    t["slope"] = rng.uniform(-1.0, 1.0, n_rec) * 4.0 * n / 2.0 ** 64
    t["err"] = rng.integers(0, 1 << 63, n_rec, dtype=np.uint64)
    return t


def _global_line(ix):
    """one record for the whole array: the least-squares line of slot over key, with the bounds it really has"""
    x = ix.keys.astype(np.float64)
    slope, icpt = np.polyfit(x, np.arange(ix.n, dtype=np.float64), 1)
    d = np.floor(slope * x + icpt) - np.arange(ix.n)
    below = min(ERR_BELOW_MAX, int(max(d.max(), 0)) + 2)
    above = min(ERR_ABOVE_MAX, int(max(-d.min(), 0)) + 2)
    return _table(1, icpt, slope, (below << 32) | above)


def _with_err(t, word):
    """the error word of every non-routing record replaced; routing records keep bit 63 and their third-layer pointers"""
    t = t.copy()
    plain = (t["err"] >> U(63)) == 0
    t["err"][plain] = word
    return t


def _shifted(t, by):
    t = t.copy()
    plain = (t["err"] >> U(63)) == 0
    t["icpt"][plain] += by
    return t


def _bad_routes(l2, n_l1, rng):
    """every second-layer record claims a route: first record and record count at random, among them firsts beyond the table, counts of 0
    and of 2^32 - 1"""
    t = l2.copy()
    k = t.shape[0]
    ps = np.where(rng.random(k) < 0.5, rng.integers(0, 2 * max(n_l1, 1) + 2, k), rng.integers(0, 1 << 31, k)).astype(np.uint64)
    cnt = rng.integers(0, 1 << 32, k).astype(np.uint64)
    pick = rng.random(k)
    cnt[pick < 0.2] = 0
    cnt[(pick >= 0.2) & (pick < 0.4)] = (1 << 32) - 1
    cnt[(pick >= 0.4) & (pick < 0.6)] = rng.integers(1, 2 * max(n_l1, 1) + 2, int(((pick >= 0.4) & (pick < 0.6)).sum()))
    t["err"] = (U(1) << U(63)) | (ps << U(32)) | cnt
    return t


def _sprinkle_non_finite(t, rng, share=0.3):
    t = t.copy()
    idx = np.nonzero(rng.random(t.shape[0]) < share)[0]
    vals = np.array([np.nan, np.inf, -np.inf])
    for f in ("icpt", "slope"):
        sel = idx[rng.random(idx.shape[0]) < 0.6]
        t[f][sel] = vals[rng.integers(0, 3, sel.shape[0])]
    return t


def _coarse(ix, bits, threshold):
    key = (bits, threshold)
    if key not in ix.coarse:
        l1, l2 = hostapi.train_prmi(ix.text, ix.sa, bits=bits, partial_threshold=threshold)
        ix.coarse[key] = (l2, l1)
    return ix.coarse[key]


MODELS = {
    "honest": lambda ix, rng: (ix.l2, ix.l1),
    "zero": lambda ix, rng: (_table(ix.l2.shape[0]), NO_L1),
    "top": lambda ix, rng: (_table(ix.l2.shape[0], icpt=1e300), NO_L1),
    "middle": lambda ix, rng: (_table(ix.l2.shape[0], icpt=ix.n / 2), NO_L1),
    "reversed": lambda ix, rng: (_table(ix.l2.shape[0], icpt=ix.n - 1, slope=-(ix.n - 1) / 2.0 ** 64), NO_L1),
    "one_record_zero": lambda ix, rng: (_table(1), NO_L1),
    "one_record_line": lambda ix, rng: (_global_line(ix), NO_L1),
    "random": lambda ix, rng: (_random_table(ix.l2.shape[0], ix.n, rng), NO_L1),
    "coarse_bits1_flat": lambda ix, rng: _coarse(ix, 1, 10 ** 9),
    "coarse_bits1_partial": lambda ix, rng: _coarse(ix, 1, 50),
    "coarse_bits4_flat": lambda ix, rng: _coarse(ix, 4, 10 ** 9),
    "coarse_bits4_partial": lambda ix, rng: _coarse(ix, 4, 50),
    "lying_bounds_zero": lambda ix, rng: (_with_err(ix.l2, 0), _with_err(ix.l1, 0)),
    "lying_bounds_max": lambda ix, rng: tuple(_with_err(t, (ERR_BELOW_MAX << 32) | ERR_ABOVE_MAX) for t in (ix.l2, ix.l1)),
    "lying_bounds_below": lambda ix, rng: tuple(_with_err(t, ERR_BELOW_MAX << 32) for t in (ix.l2, ix.l1)),
    "lying_bounds_above": lambda ix, rng: tuple(_with_err(t, ERR_ABOVE_MAX) for t in (ix.l2, ix.l1)),
}
for _s in SHIFTS:
    for _sign in (1, -1):
        MODELS["shifted_%+d" % (_sign * _s)] = (lambda by: lambda ix, rng: (_shifted(ix.l2, by), _shifted(ix.l1, by)))(_sign * _s)
# The families below are safe only with the NaN-safe clamps of rmi_lookup and the zeroed placeholder record of a model without a third layer
AFTER_THE_FIX = {
    "bad_routes_honest_l1": lambda ix, rng: (_bad_routes(ix.l2, _coarse(ix, 4, 50)[1].shape[0], rng), _coarse(ix, 4, 50)[1]),
    "bad_routes_random_l1": lambda ix, rng: (_bad_routes(ix.l2, 777, rng), _random_table(777, ix.n, rng)),
    "bad_routes_empty_l1": lambda ix, rng: (_bad_routes(ix.l2, 0, rng), NO_L1),
    "non_finite_leaves": lambda ix, rng: (_sprinkle_non_finite(ix.l2, rng), NO_L1),
    "non_finite_third_layer": lambda ix, rng: tuple(_sprinkle_non_finite(t, rng) for t in _coarse(ix, 4, 50)),
    "all_nan": lambda ix, rng: (_table(ix.l2.shape[0], icpt=np.nan, slope=np.nan), NO_L1),
    "all_nan_third_layer": lambda ix, rng: (_coarse(ix, 4, 50)[0], _table(_coarse(ix, 4, 50)[1].shape[0], icpt=np.nan, slope=np.nan)),
}
MODELS.update(AFTER_THE_FIX)
MUST_RELOCATE_ALWAYS = ("zero", "top", "one_record_zero")                        # (a one-record table of zeros predicts what `zero` predicts)
# (coarse_bits1_partial is not here: with partial_threshold = 50 each of its two leaves routes to thousands of third-layer records of about 20
# keys each -- a model finer than the honest one's leaves, whose first window holds the partition point just as often; its figures are
# printed with the others)
MORE_WINDOWS_THAN_HONEST = ("middle", "reversed", "random", "coarse_bits1_flat", "shifted_+1000", "shifted_-1000")
# also run with smem_cap = 8: the overflow tiers restart searches, and on R's 150-base reads the re-seeding kernels then pose hundreds of lane searches
# instead of a dozen (`top` as well, so that lane_search doubles down from the last slot as often as up from the first)
SMALL_SLOTS_TOO = ("zero", "top", "random")


def build_model(name, ix):
    rng = np.random.default_rng(sum(name.encode()) * 7919 + ix.n)
    l2, l1 = MODELS[name](ix, rng)
    l2, l1 = np.ascontiguousarray(l2), np.ascontiguousarray(l1)
    assert l2.dtype == RMI_DTYPE and l1.dtype == RMI_DTYPE
    assert l2.shape[0] >= 1 and l2.shape[0] & (l2.shape[0] - 1) == 0, "the loader takes a power-of-two second layer only"
    if name not in AFTER_THE_FIX:
        for t in (l2, l1):
            assert np.isfinite(t["icpt"]).all() and np.isfinite(t["slope"]).all(), name
    return l2, l1


# ---- indexes, read sets, expected dumps (host only) --------------------------------------------------------------------------------------------
class Batch:
    def __init__(self, ix, name, reads, off, smem_cap=512, hit_cap=1 << 14, golden=None):
        self.name = name
        self.reads = np.ascontiguousarray(reads, dtype=np.uint8).reshape(-1)
        self.off = np.ascontiguousarray(off, dtype=np.int64)
        self.n = self.off.shape[0] - 1
        sm, ns, hits, nh, ctr = O.seed_batch(ix.oracle, self.reads, self.off, smem_cap=smem_cap, hit_cap=hit_cap, threads=0)
        self.want = O.format_seed_dump(sm, ns, hits)
        self.oracle_searches = int(ctr.searches)
        self.max_smems = int(ns.max()) if self.n else 0
        if golden is not None:
            assert self.want == golden, "the oracle on the rebuilt index no longer gives the committed dump"

    def subset(self, ix, keep, name):
        lens = np.diff(self.off)[keep]
        off = np.zeros(lens.shape[0] + 1, np.int64)
        off[1:] = np.cumsum(lens)
        reads = np.concatenate([self.reads[self.off[r]:self.off[r + 1]] for r in np.nonzero(keep)[0]])
        return Batch(ix, name, reads, off)


class Index:
    def __init__(self, name, fwd, bits):
        self.name = name
        self.text, self.sa = hostapi.build_sa(fwd)
        self.n = self.text.shape[0]
        self.pos5 = pos5_image(self.sa)
        self.keys = entry_keys(self.text, self.sa)
        assert (self.keys[1:] >= self.keys[:-1]).all()
        self.l1, self.l2 = hostapi.train_prmi(self.text, self.sa, bits=bits)
        self.oracle = O.Index(self.text, self.sa)
        self.coarse = {}
        self.batches = []
        self.safe = {}                       # batch name -> the batch without the reads whose first window could serve them

    def add(self, batch, max_removed):
        """the batch, and beside it the batch `zero` and `top` are measured on"""
        ok = reads_no_first_window_can_serve(self, batch.reads, batch.off)
        removed = np.nonzero(~ok)[0]
        assert removed.shape[0] <= max_removed, (batch.name, removed.tolist())
        self.batches.append(batch)
        self.safe[batch.name] = batch if removed.shape[0] == 0 else batch.subset(self, ok, batch.name + "/filtered")
        return removed


def _has_poly_run_or_n(read, run=7):
    """an N, or `run` A's or T's in a row: what puts one of a read's keys next to an end of the suffix array (with an N, a query of one or two
    bases can be posed, and a lone T is the last key there is)"""
    if (read > 3).any():
        return True
    for base in (0, 3):
        hit = np.convolve((read == base).astype(np.int64), np.ones(run, np.int64), "valid")
        if hit.size and hit.max() == run:
            return True
    return False


_G1_BITS, _R_BITS = 12, 14
_state = {}


def g1_index():
    if "g1" not in _state:
        prefix = build_index(os.path.join(GOLDEN, "g1.fa"))           # (the tool settles the genome's ambiguous bases; the text's first half is the result)
        both = np.fromfile(prefix + ".0123", np.uint8)
        ix = Index("g1", both[:both.shape[0] // 2], _G1_BITS)
        assert np.array_equal(ix.text, both)
        for length in (150, 250, 60, 25):
            reads, off = read_fastq_codes(os.path.join(GOLDEN, "g1_reads_%d.fq" % length))
            b = Batch(ix, "g1_reads_%d" % length, reads, off, golden=open(os.path.join(GOLDEN, "g1_seeds_%d.txt" % length)).read())
            # a golden set loses a read only where it really holds one with an N or a poly-A / poly-T run
            removed = ix.add(b, max_removed=b.n // 10)
            for r in removed:
                assert _has_poly_run_or_n(reads[off[r]:off[r + 1]]), (length, int(r))
        _state["g1"] = ix
    return _state["g1"]


def r_index():
    """300 kbp with repeat families, duplications and poly runs: wide hit intervals, so level walks and edge requests start from partition
    windows that relocations found"""
    if "R" not in _state:
        g = synth.make_genome(300_000, seed=31, repeat_frac=0.2, repeat_len=300, n_families=4, divergence=0.02, n_dups=10, dup_len=3000, poly_runs=8)
        ix = Index("R", g, _R_BITS)
        for L, kw in ((150, dict(exact_frac=0.3, n_frac=0.05)), (250, dict(sub_rate=0.05, indel_rate=0.0075)), (40, dict())):
            reads, _, _ = synth.make_reads(g, 1000, L, seed=100 + L, **kw)
            off = np.arange(0, (reads.shape[0] + 1) * L, L, dtype=np.int64)
            b = Batch(ix, "R_reads_%d" % L, reads, off)
            ix.add(b, max_removed=b.n // 50)                           # at most 2 %
        _state["R"] = ix
    return _state["R"]


INDEXES = {"g1": g1_index, "R": r_index}
# (group_lanes, seed_defer, smem_cap)
SETTINGS = {"g1": [(lanes, defer, 128) for lanes in (1, 4, 32) for defer in (1, 0)], "R": [(4, 1, 128), (32, 1, 128), (4, 0, 128)]}
SMALL_SLOT_SETTINGS = {"g1": [(4, 1, 8), (32, 0, 8)], "R": [(4, 1, 8)]}


# ---- the device side -----------------------------------------------------------------------------------------------------------------------
class Gpu:
    def __init__(self):
        import torch
        self.torch = torch
        self.ctx = hipapi.Context(0)
        self.cp = hipapi.lib().hipMemcpy
        self.cp.restype, self.cp.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.dev = {}
        self.honest = {}                     # (index, batch, setting) -> (searches, windows, lane searches) under the honest model
        self.round1 = {}                     # (index, batch, setting) -> searches of a first-round-only run
        self.broken = None                   # the first error of a device call: nothing more is started on the device after it

    def _guarded(self, call, *args, **kw):
        if self.broken:
            pytest.fail("an earlier device call of this module failed: " + self.broken)
        try:
            return call(*args, **kw)
        except Exception as e:
            self.broken = repr(e)
            raise

    def close(self):
        self.dev.clear()
        self.ctx.close()

    def load(self, ix, l2, l1):
        self._guarded(self.ctx.load_index_host, ix.pos5, ix.text, l1, l2)

    def _d2h(self, ptr, count, dtype):
        out = np.empty(count, dtype=dtype)
        if count:
            assert self.cp(out.ctypes.data, ptr, count * np.dtype(dtype).itemsize, 2) == 0          # hipMemcpyDeviceToHost
        return out

    def run(self, batch, setting, rounds=3, dump=True):
        """one seeding call: (dump, searches, windows loaded by k_seed, searches the re-seeding kernels' lanes did)"""
        return self._guarded(self._run, batch, setting, rounds, dump)

    def _run(self, batch, setting, rounds, dump):
        torch = self.torch
        if batch.name not in self.dev:
            padded = np.concatenate([batch.reads, np.zeros(64, np.uint8)])
            self.dev[batch.name] = (torch.from_numpy(padded).cuda(), torch.from_numpy(batch.off).cuda())
            torch.cuda.synchronize()
        d_reads, d_off = self.dev[batch.name]
        lanes, defer, cap = setting
        for key, value in (("group_lanes", lanes), ("seed_defer", defer), ("smem_cap", cap)):
            self.ctx.set_tuning(key, value)
        res = self.ctx.seed_batch_device(d_reads.data_ptr(), d_off.data_ptr(), batch.n, batch.reads.shape[0], hipapi.default_seed_opt(rounds=rounds))
        tm = self.ctx.timings()
        text = None
        if dump:
            smems = self._d2h(res.d_smems, res.total_smems, hipapi.MEM_TL)
            hits = self._d2h(res.d_hits, res.total_hits, np.uint64)
            so, ho = self._d2h(res.d_smem_off, batch.n + 1, np.int64), self._d2h(res.d_hit_off, batch.n + 1, np.int64)
            text = O.format_seed_dump(*hipapi.smems_to_slots(smems, so, hits, ho))
        return text, int(res.searches), int(tm.seed_windows), int(tm.seed_lane_searches)


@pytest.fixture(scope="module")
def gpu():
    g = Gpu()
    yield g
    g.close()


def _batches_for(ix, model):
    """(batch, is the filtered one) pairs: `zero` and `top` also run on the batch whose every search has to relocate"""
    out = [(b, False) for b in ix.batches]
    if model in MUST_RELOCATE_ALWAYS:
        out += [(ix.safe[b.name], True) for b in ix.batches if ix.safe[b.name] is not b]
    return out


def _honest_baseline(gpu, ix):
    """searches / windows / lane searches of the honest model for every batch and setting of an index (first use; the model stays loaded)"""
    if (ix.name, "done") in gpu.honest:
        return
    gpu.load(ix, ix.l2, ix.l1)
    for setting in SETTINGS[ix.name] + SMALL_SLOT_SETTINGS[ix.name]:
        for b in ix.batches + [s for s in ix.safe.values() if s.name.endswith("/filtered")]:
            text, searches, windows, lane = gpu.run(b, setting)
            assert text == b.want, (ix.name, "honest", b.name, setting)
            gpu.honest[(ix.name, b.name, setting)] = (searches, windows, lane)
            if setting[1] == 1:
                gpu.round1[(ix.name, b.name, setting)] = gpu.run(b, setting, rounds=1, dump=False)[1]
    gpu.honest[(ix.name, "done")] = True


def _shift_precondition(ix, l2, l1, by):
    """A shift by W or W + 1 slots has to leave true slots just outside the first window on the far side, fewer than W slots away: at least
    100 suffix keys of the index, for W = 12 and for W = 64 (two slots are allowed for the rounding of the restated prediction)."""
    for W, shifts in ((12, (12, 13)), (64, (64, 65))):
        if abs(by) not in shifts:
            continue
        pos, err = predict(l2, l1, ix.n, ix.keys)
        base = first_window(pos, err, W, ix.n)
        true = np.searchsorted(ix.keys, ix.keys, "left")
        d = base - true if by > 0 else true - (base + W - 1)          # slots between the true slot and the window's near end
        near = int(((d > 2) & (d < W - 2)).sum())
        assert near >= 100, (ix.name, by, W, near)


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("index", ["g1", "R"])
def test_any_model_gives_the_same_seeds(gpu, index, model):
    """g1: group_lanes 1 / 4 / 32 (W = 12 / 12 / 64), each with seed_defer 1 and 0; R: group_lanes 4 and 32 with seed_defer 1, 4 with seed_defer 0;
    three rounds; `zero`, `top` and `random` also with 8 SMEM slots per read.  Per (model, setting, read set): the dump is the oracle's, the search
    count is the honest model's, and the windows per search are what the family has to cost."""
    ix = INDEXES[index]()
    _honest_baseline(gpu, ix)
    l2, l1 = build_model(model, ix)
    if model.startswith("shifted_"):
        _shift_precondition(ix, l2, l1, int(model.split("_")[1]))
    gpu.load(ix, l2, l1)
    settings = SETTINGS[index] + (SMALL_SLOT_SETTINGS[index] if model in SMALL_SLOTS_TOO else [])
    wrong = []                               # every figure that misses is reported, not only the first
    for setting in settings:
        lanes, defer, cap = setting
        lane_total = 0
        for b, filtered in _batches_for(ix, model):
            text, searches, windows, lane = gpu.run(b, setting)
            h_searches, h_windows, h_lane = gpu.honest[(index, b.name, setting)]
            where = (index, model, b.name, setting)
            print("%s %s %s lanes=%d defer=%d cap=%d: searches %d windows %d (%.3f per search; honest %.3f) lane searches %d (honest %d)" % (
                index, model, b.name, *setting, searches, windows, windows / max(searches, 1), h_windows / max(h_searches, 1), lane, h_lane))
            assert text == b.want, where
            # The pivot logic decides what is searched; the model only decides where a search starts.  One thing the model does decide: whether
            # a unique SMEM's search ends inside its partition window (`have_pos`), and only then is the SMEM's re-seeding region left to
            # k_reseed.  A region costs the same count in either kernel, but a read that overflows its slots in the re-seeding kernels has been
            # counted in tier 0 and is counted again in the tier that re-runs it, while a read that overflows inside k_seed is counted once.
            # So the count is the model's only where no read can overflow behind k_seed; elsewhere it is at least the count without overflow.
            if defer == 0 or b.max_smems <= cap:
                if searches != h_searches:
                    wrong.append(where + ("searches", searches, h_searches))
            else:
                assert b.max_smems <= 128
                if searches < gpu.honest[(index, b.name, (lanes, defer, 128))][0]:
                    wrong.append(where + ("searches below the count without overflow", searches))
            if b.max_smems > cap and gpu.ctx.timings().seed_launches < 2:
                wrong.append(where + ("no overflow tier ran",))
            lane_total += lane
            if model in MUST_RELOCATE_ALWAYS and (filtered or ix.safe[b.name] is b):
                # No first window of this batch holds a partition point (reads_no_first_window_can_serve), so every search of k_seed loads two
                # windows or more.  With seed_defer = 0 every search is k_seed's.  With seed_defer = 1 `searches` also counts the re-seeding
                # kernels' table walks and lane searches, which load no window of k_seed's: there k_seed's share is bounded from below by the
                # first round's searches, all of which stay in k_seed.
                floor = searches if defer == 0 else gpu.round1[(index, b.name, setting)]
                if windows < 2 * floor:
                    wrong.append(where + ("windows < 2 x searches", windows, floor))
            if model in MORE_WINDOWS_THAN_HONEST and windows <= h_windows:
                wrong.append(where + ("no more windows than the honest model", windows, h_windows))
        # The model has to reach lane_search, not only k_seed.  Lane searches are rare by design (a region is left to the re-seeding kernels only
        # where its locus shares fewer than min_seed_len bases with its suffix-array neighbours, and there the plcp table answers nearly
        # everything): of R's read sets only the noisy 250-base one poses any with 128 slots per read, so the count is taken over the three.
        if index == "R" and defer == 1 and lane_total <= 0:
            wrong.append((index, model, setting, "no lane search"))
    assert not wrong, wrong


# ---- tiny indexes: n - W is 0, 2, 16, ... and every clamp is active ------------------------------------------------------------------------------
def _tiny_case(length):
    rng = np.random.default_rng(4000 + length)
    ix = Index("tiny%d" % length, rng.integers(0, 4, length).astype(np.uint8), bits=2)
    reads = []
    for k in range(60):
        L = int(rng.integers(19, min(60, ix.n) + 1))
        p = int(rng.integers(0, ix.n - L + 1))
        reads.append(ix.text[p:p + L].copy())
    for r in list(reads):
        m = r.copy()
        q = int(rng.integers(0, m.shape[0]))
        m[q] = (m[q] + 1 + int(rng.integers(0, 3))) & 3
        reads.append(m)
    reads += [np.zeros(19, np.uint8), np.zeros(60, np.uint8), np.full(19, 3, np.uint8), np.full(60, 3, np.uint8)]
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in reads])
    return ix, Batch(ix, ix.name, np.concatenate(reads), off, smem_cap=1024, hit_cap=1 << 14)


@pytest.mark.parametrize("length", [32, 33, 40, 64, 65])
def test_tiny_indexes(gpu, length):
    """n = 64 (the widest window, and the least the loader takes), 66, 80, 128, 130 suffixes"""
    ix, b = _tiny_case(length)
    assert ix.n == 2 * length
    counts = {}
    for model in ("honest", "zero", "top", "middle"):
        l2, l1 = build_model(model, ix)
        gpu.load(ix, l2, l1)
        for setting in [(lanes, defer, 128) for lanes in (1, 4, 32) for defer in (1, 0)]:
            text, searches, windows, lane = gpu.run(b, setting)
            print("%s %s lanes=%d defer=%d: searches %d windows %d lane searches %d" % (ix.name, model, setting[0], setting[1], searches, windows, lane))
            assert text == b.want, (length, model, setting)
            assert counts.setdefault(setting, searches) == searches, (length, model, setting)
