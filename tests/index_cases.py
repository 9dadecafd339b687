"""Case texts for the index builders, the definition of the suffix array they must produce, and what a build must report about itself.

The suffix array (the reference's `.pos_packed` order, src/Learnedindex.cpp:157-229, 242): let k = (longest run of A or of T in the text) + 1; sort the
suffixes of text + T * k as byte strings, so that a string which is a prefix of another comes first; drop the k suffixes that start in the padding.  That is
`sorted(range(N), key=lambda i: padded[i:])`, and every case is small enough (N of at most a few thousand) for it to take well under a second.

Beside the definition stand the figures `meme_debug_sa_stats` must report for a build of the case (tests/test_gpu_sa.py asserts them, so each branch of the
device builder is known to have run): k, the groups of four-base buckets for a given `sa_chunk`, the suffixes whose 32-base key is shared, the pieces of the
padding drop for a given `sa_piece`, and a floor for the refinement rounds.  tests/test_index_cases.py (no GPU) checks the host builder against the definition
and that the set of cases reaches what it claims.  The P-RMI cases of tests/test_gpu_prmi.py are here too, with the host-side key counts they rest on."""
import functools

import numpy as np

from pymeme.hipapi import fwd_rc_text

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
DEFAULT_CHUNK = DEFAULT_PIECE = 1 << 28


def codes(s):
    return np.array([_CODE[c] for c in s], np.uint8)


def rand(n, seed):
    return np.random.default_rng(seed).integers(0, 4, size=n).astype(np.uint8)


def run_ends(tail, body=2000):
    """the texts of test_gpu_sa.test_text_ends_in_a_run at this module's size: a run of `tail` at both ends of both strands"""
    t = codes(tail * (120 // len(tail)))
    return np.concatenate([(3 - t[::-1]).astype(np.uint8), rand(body, 5), t])


def padding_key_ties():
    """T^m A^(32-m) C for every m: the key of the real suffix T^m A^(32-m) equals the key of the padding suffix T^m, which is filled with zeros = A behind the sentinel"""
    return codes("".join("T" * m + "A" * (32 - m) + "C" for m in range(1, 32)))


# name -> forward strand; the text is fwd_rc_text(fwd)
FORWARD = {
    "smallest": codes("ACGT" * 8),                           # 64 suffixes, the least the call takes
    "odd_33": rand(33, 33),                                  # n = 66 and 74: no multiples of 32
    "odd_37": rand(37, 37),
    "all_A_40": codes("A" * 40),                             # one bucket holds nearly everything, k = n / 2 + 1
    "all_A_600": codes("A" * 600),
    "all_T_33": codes("T" * 33),
    "all_C_500": codes("C" * 500),
    "period_AC_50": codes("AC" * 50),
    "period_AGT_700": codes("AGT" * 700),
    "copies_3x700": np.tile(rand(700, 700), 3),              # all but a few dozen suffixes tied
    "no_ties_2000": rand(2000, 2000),                        # no tied suffix: the refinement is empty
    "padding_key_ties": padding_key_ties(),
    "ends_in_A": run_ends("A"),
    "ends_in_T": run_ends("T"),
    "ends_in_ACGT": run_ends("ACGT"),
}
NAMES = tuple(FORWARD)


def longest_at_run(text):
    best = run = 0
    prev = -1
    for c in text.tolist():
        run = run + 1 if c == prev else 1
        prev = c
        if c in (0, 3) and run > best:
            best = run
    return best


def neighbour_lcps(padded, sa):
    """Kasai: common prefix of every suffix-array neighbour pair of `padded` (a suffix that is a prefix of its neighbour shares its whole length)"""
    n = len(padded)
    rank = [0] * n
    for r, i in enumerate(sa):
        rank[i] = r
    lcp = [0] * n
    h = 0
    for i in range(n):
        if rank[i] == 0:
            h = 0
            continue
        j = sa[rank[i] - 1]
        while i + h < n and j + h < n and padded[i + h] == padded[j + h]:
            h += 1
        lcp[rank[i]] = h
        if h:
            h -= 1
    return lcp


class Case:
    def __init__(self, name):
        self.name = name
        self.fwd = FORWARD[name]
        self.text = fwd_rc_text(self.fwd)
        self.n = int(self.text.shape[0])
        self.k_pad = longest_at_run(self.text) + 1
        self.N = self.n + self.k_pad
        padded = bytes(self.text.tolist()) + b"\x03" * self.k_pad
        # ---- the definition
        self.sa_pad = sorted(range(self.N), key=lambda i: padded[i:])
        self.sa = np.array([i for i in self.sa_pad if i < self.n], np.uint64)
        # ---- what the device builder's first pass sees: the first 32 bases of every suffix of the padded text, zeros behind the sentinel
        z = np.concatenate([np.frombuffer(padded, np.uint8), np.zeros(32, np.uint8)]).astype(np.uint64)
        keys = np.zeros(self.N, np.uint64)
        for j in range(32):
            keys = (keys << np.uint64(2)) | z[j:j + self.N]
        self.keys = keys
        self.hist = np.bincount((keys >> np.uint64(56)).astype(np.int64), minlength=256)
        _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
        self.tied = int((cnt[inv] > 1).sum())                # suffixes that share their key with another one
        self.max_lcp = max(neighbour_lcps(padded, self.sa_pad))
        self.pad_slots = [j for j, i in enumerate(self.sa_pad) if i >= self.n]

    def bucket_groups(self, chunk):
        """The builder's greedy rule: from bucket b on, a group takes consecutive buckets while its total stays within `chunk`; its first bucket is taken
        whatever its size, so a bucket alone may exceed the chunk.  Returns [(first bucket, end bucket, suffixes)], groups without a suffix included."""
        out, b = [], 0
        while b < 256:
            e, tot = b, 0
            while e < 256 and (e == b or tot + int(self.hist[e]) <= chunk):
                tot += int(self.hist[e])
                e += 1
            out.append((b, e, tot))
            b = e
        return out

    def pieces(self, piece):
        """pad entries found in each piece of min(piece, N) slots of the padded array"""
        piece = min(piece, self.N)
        return np.bincount(np.array(self.pad_slots) // piece, minlength=-(-self.N // piece)).tolist()

    def round_floor(self):
        """Round r of the refinement orders by 32 << r bases: neighbours that share max_lcp bases are apart only once 32 << r exceeds it"""
        r = 0
        while (32 << r) <= self.max_lcp:
            r += 1
        return r

    def stats(self, chunk=DEFAULT_CHUNK, piece=DEFAULT_PIECE):
        """what meme_debug_sa_stats must report, but for `rounds`, which has the floor round_floor()"""
        groups = [g for g in self.bucket_groups(chunk) if g[2] > 0]
        per_piece = self.pieces(piece)
        return {"k_pad": self.k_pad, "groups": len(groups), "largest_group": max(g[2] for g in groups), "tied": self.tied, "pieces": len(per_piece),
                "pad_pieces": sum(1 for c in per_piece if c)}

    def builds(self):
        """the (sa_chunk, sa_piece) pairs the GPU test builds the case with: defaults, each key small and at its edges, both small"""
        d = DEFAULT_CHUNK
        return [(d, d), (1, d), (self.N // 3, d), (d, 64), (d, self.N - 1), (d, self.N), (self.N // 3, 64)]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---- P-RMI cases ------------------------------------------------------------------------------------------------------------------------------------
def leaf_counts(keys, bits):
    return np.bincount((keys >> np.uint64(64 - bits)).astype(np.int64), minlength=1 << bits)


def third_layer_records(counts, threshold):
    """records per leaf: a leaf beyond the threshold gets round-half-away(count / 20) of them -- none for 9 keys and fewer, which leaves it a plain leaf"""
    c = np.asarray(counts, np.int64)
    return np.where(c > threshold, (c + 10) // 20, 0)


def leaf_at_the_threshold(counts):
    """a leaf of median size: with its key count as the threshold it stays plain while larger leaves route, with one less it routes too"""
    m = int(np.argsort(counts, kind="stable")[len(counts) // 2])
    assert counts[m] >= 10 and counts.max() > counts[m]
    return m


def thresholds_at_a_count(counts):
    c = int(counts[leaf_at_the_threshold(counts)])
    return (c, c - 1)


# A 112-base strand whose 16 two-base leaves (bits = 4) hold 6 to 30 keys, among them leaves of 6, 8 and 9 (beyond a threshold of 1, yet count / 20 rounds to no
# record: a plain leaf), of exactly 10 (0.5 rounds away from zero: one record) and of exactly 30 keys (1.5: two records).  Found by a search over random strands;
# tests/test_index_cases.py asserts the counts.
SMALL_COUNTS_FWD = "GAACGAAGCGATAAAGGACGACCCGGTACGGGCACAATCCGCTACCGAGGCCACCGCCTCGGGGGCCGTAGTGGCGTCGGACCCCCATGTGCCCCAGGCACGCAGGCAACCC"

# name -> (forward strand, bits, thresholds)
PRMI = {
    "threshold_at_count": (rand(2500, 8), 4, None),          # thresholds c and c - 1 of one leaf, chosen by the test from the counts
    "small_counts": (codes(SMALL_COUNTS_FWD), 4, (1, 9, 10)),
    "one_bit": (rand(2500, 9), 1, (1000,)),
    "more_leaves_than_keys": (codes("A" * 64), 14, (9,)),
    "equal_key_leaf": (np.concatenate([codes("A" * 300), rand(3000, 0)]), 14, (200,)),      # the last leaf holds 300 times the key T^32 and nothing else
}
