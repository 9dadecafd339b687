"""SAM text on the device (meme_sam_format_batch_host = mem_aln2sam for a chunk's plain records), through the C ABI, against the text the compiled
reference's mem_aln2sam wrote for the same records (tests/golden/sam_golden.npz) and against the oracle with other options."""
import os

import numpy as np
import pytest

import oracle_py as O
from common import GOLDEN, SAM_LONG_NAMES, SAM_LONG_READS, SAM_LONG_STRINGS, build_index, sam_long_workload, sam_workload
from pymeme import hipapi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sam")
    recs, blob, names, reads, quals, contigs = sam_workload()
    g = synth.make_genome(120_000, seed=5)
    fa = str(tmp / "g.fa")
    synth.write_fasta(fa, g, contigs=2)
    prefix = build_index(fa, bits=12)
    ctx = hipapi.Context(0)
    ctx.load_index_files(prefix)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    ctx.seed_batch_host(np.concatenate(reads), off)            # stages the reads the records refer to
    yield ctx, recs, blob, names, reads, quals, contigs
    ctx.close()


def test_device_sam_text_equals_reference_golden(staged):
    ctx, recs, blob, names, reads, quals, contigs = staged
    G = np.load(os.path.join(GOLDEN, "sam_golden.npz"))
    # the fixture mixes reads with and without qualities; the device stages qualities per batch: two passes over the two kinds
    have = np.array([q is not None for q in quals])
    for with_q in (True, False):
        sel = np.nonzero(have == with_q)[0]
        qbuf = b"".join(quals[k] if quals[k] is not None else b"!" * len(reads[k]) for k in range(len(reads))) if with_q else None
        ctx.sam_stage_text(names, qbuf)
        for softclip, rg in ((0, b""), (1, b"grp1")):
            want_text, want_off = G["text_%d" % softclip].tobytes(), G["off_%d" % softclip]
            text, off, ms = ctx.sam_format_batch_host(recs[sel], blob, contigs, softclip, rg)
            assert off.shape[0] == sel.shape[0] + 1 and off[0] == 0 and off[-1] == len(text)
            for i, k in enumerate(sel):
                assert text[off[i]:off[i + 1]] == want_text[want_off[k]:want_off[k + 1]], (int(k), softclip, text[off[i]:off[i + 1]], want_text[want_off[k]:want_off[k + 1]])


def test_device_sam_text_errors_and_empty(staged):
    ctx, recs, blob, names, reads, quals, contigs = staged
    ctx.sam_stage_text(names, None)
    text, off, _ = ctx.sam_format_batch_host(recs[:0], blob, contigs)
    assert text == b""
    # empty slots (read = -1) between records: no text for them, the others unchanged
    holes = recs[:6].copy()
    holes["read"][[1, 4]] = -1
    cb0, co0 = O.contig_table(contigs)
    text, off, _ = ctx.sam_format_batch_host(holes, blob, contigs)
    assert off[2] == off[1] and off[5] == off[4]
    for k in (0, 2, 3, 5):
        assert text[off[k]:off[k + 1]] == O.aln2sam(recs[k], blob, names[k], reads[k], None, cb0, co0)
    bad = recs[:4].copy()
    bad["read"][1] = len(reads) + 3
    with pytest.raises(hipapi.MemeError, match="malformed"):
        ctx.sam_format_batch_host(bad, blob, contigs)
    bad = recs[:4].copy()
    k = int(np.nonzero(bad["n_cigar"] > 0)[0][0])
    bad["cigar_off"][k] = blob.shape[0] - 2
    with pytest.raises(hipapi.MemeError, match="malformed"):
        ctx.sam_format_batch_host(bad, blob, contigs)
    # a blob whose last string is not terminated
    cut = recs[-1:].copy()
    if cut["xa_off"][0] < 0:
        cut["xa_off"][0] = 0
    with pytest.raises(hipapi.MemeError, match="does not end inside the blob|malformed"):
        ctx.sam_format_batch_host(cut, np.full(64, 65, np.uint8), contigs)
    # one long name, a one-base read: the oracle's text
    cb, co = O.contig_table(contigs)
    r = recs[:1].copy()
    got, off, _ = ctx.sam_format_batch_host(r, blob, contigs, 0, b"x" * 200)
    assert got == O.aln2sam(r[0], blob, names[0], reads[0], None, cb, co, 0, b"x" * 200)


def _own_blob(rec, blob):
    """The record with a blob of its own in which every offset is 4-byte aligned (what the oracle's orc_aln2sam asks of its caller): the same operations and
    strings, hence the same text."""
    r = rec.copy()
    raw = blob.tobytes()
    b = bytearray()
    if r["n_cigar"] > 0:
        s = int(r["cigar_off"])
        e = raw.index(b"\0", s + 4 * int(r["n_cigar"]))
        r["cigar_off"] = 0
        b += raw[s:e + 1]
    if r["m_n_cigar"] > 0:
        b += b"\0" * (-len(b) % 4)
        s = int(r["m_cigar_off"])
        r["m_cigar_off"] = len(b)
        b += raw[s:s + 4 * int(r["m_n_cigar"])]
    if r["xa_off"] >= 0:
        b += b"\0" * (-len(b) % 4)
        s = int(r["xa_off"])
        r["xa_off"] = len(b)
        b += raw[s:raw.index(b"\0", s) + 1]
    b += b"\0" * 8
    return r, np.frombuffer(bytes(b), np.uint8).copy()


def test_names_md_and_xa_strings_of_64_bytes_and_more(tmp_path):
    """k_sam_format copies names, MD and XA strings with 64-lane loops and finds the strings' ends 64 bytes at a time; sam_workload()'s strings are all shorter
    than 64 bytes, so no such loop takes a second turn there.  Here: every length around one, two and many turns, at every alignment, the last string in the
    blob's final bytes; hard clipping cut off SEQ and QUAL on both strands; and one record with every number at its widest, inside k_sam_bounds' allowance."""
    recs, blob, names, reads, quals, contigs = sam_long_workload()
    # what the record set is for, before the GPU sees it
    raw = blob.tobytes()
    md_at = recs["cigar_off"] + 4 * recs["n_cigar"].astype(np.int64)
    md_len = np.array([raw.index(b"\0", int(p)) - int(p) for p in md_at])
    has_xa = recs["xa_off"] >= 0
    xa_len = np.array([raw.index(b"\0", int(p)) - int(p) for p in recs["xa_off"][has_xa]])
    assert set(SAM_LONG_STRINGS) <= set(md_len.tolist()) and set(SAM_LONG_STRINGS) <= set(xa_len.tolist())
    for n in SAM_LONG_STRINGS:                      # every length at every residue of its first byte, on both strands (XA), with and without qualities
        assert set((md_at[md_len == n] % 4).tolist()) == {0, 1, 2, 3} and set((recs["xa_off"][has_xa][xa_len == n] % 4).tolist()) == {0, 1, 2, 3}, n
        for sel in (recs["is_rev"][has_xa][xa_len == n], np.array([quals[int(k)] is None for k in recs["read"][has_xa][xa_len == n]])):
            assert set(sel.astype(int).tolist()) == {0, 1}, n
    assert int(recs["xa_off"][-1]) + int(xa_len[-1]) + 1 == blob.shape[0] and xa_len[-1] >= 64
    assert set(SAM_LONG_NAMES) <= set(len(x) for x in names)
    clipped = (recs["which"] > 0) & (recs["is_alt"] == 0)
    for rev in (1, 0):
        assert set(SAM_LONG_READS) <= set(len(reads[int(k)]) for k in recs["read"][clipped & (recs["is_rev"] == rev)])
    wide = int(np.nonzero(recs["NM"] == 2 ** 31 - 1)[0][0])
    assert recs["pos"][wide] > 1 << 32 and recs["m_pos"][wide] > 1 << 32 and recs["score"][wide] == recs["sub"][wide] == 2 ** 31 - 1 and len(contigs[int(recs["rid"][wide])]) == 60
    g = synth.make_genome(120_000, seed=5)
    fa = str(tmp_path / "g.fa")
    synth.write_fasta(fa, g, contigs=2)
    prefix = build_index(fa, bits=12)
    cb, co = O.contig_table(contigs)
    own = [_own_blob(recs[k], blob) for k in range(recs.shape[0])]
    # k_sam_bounds' slot for a record: its parts + a fixed allowance of 192 bytes for the numeric fields and tags (csrc/meme_sam.hip)
    max_contig = max(len(c) for c in contigs)
    slot0 = np.array([len(names[int(R["read"])]) + 2 * len(reads[int(R["read"])]) + 12 * (int(R["n_cigar"]) + int(R["m_n_cigar"])) + 2 * max_contig + 192 for R in recs]) + md_len
    slot0[has_xa] += xa_len
    slack = []
    ctx = hipapi.Context(0)
    try:
        ctx.load_index_files(prefix)
        off = np.zeros(len(reads) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in reads])
        ctx.seed_batch_host(np.concatenate(reads), off)
        have = np.array([quals[int(k)] is not None for k in recs["read"]])
        for with_q in (True, False):
            sel = np.nonzero(have == with_q)[0]
            qbuf = b"".join(quals[k] if quals[k] is not None else b"!" * len(reads[k]) for k in range(len(reads))) if with_q else None
            ctx.sam_stage_text(names, qbuf)
            for softclip, rg in ((0, b""), (1, b"grp1"), (0, b"G" * 200)):
                text, toff, ms = ctx.sam_format_batch_host(recs[sel], blob, contigs, softclip, rg)
                assert toff.shape[0] == sel.shape[0] + 1 and toff[0] == 0 and toff[-1] == len(text)
                for i, k in enumerate(sel):
                    r, b = own[int(k)]
                    rd = int(r["read"])
                    want = O.aln2sam(r, b, names[rd], reads[rd], quals[rd] if with_q else None, cb, co, softclip, rg)
                    assert text[toff[i]:toff[i + 1]] == want, (int(k), softclip, len(rg), text[toff[i]:toff[i + 1]], want)
                    slack.append(int(slot0[k]) + len(rg) - len(want))
        # the widest text stays inside the allowance (the call succeeded: the kernel found the same); the record with every number at its widest leaves the least
        assert min(slack) >= 0 and min(slack) < 192, min(slack)
        print("least slack of k_sam_bounds' slots over these records: %d bytes" % min(slack))
    finally:
        ctx.close()


def test_sam_max_batch_refuses_more_slots_and_takes_that_many(staged):
    """Tuning "sam_max_batch": 11 record slots are refused with MEME_E_CAPACITY (the caller then formats in pieces), 10 give the text an unrestricted ctx gives."""
    free, recs, blob, names, reads, quals, contigs = staged
    free.sam_stage_text(names, None)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    ctx = hipapi.Context(0)
    try:
        ctx.replicate_index_from(free)
        ctx.seed_batch_host(np.concatenate(reads), off)
        ctx.sam_stage_text(names, None)
        ctx.set_tuning("sam_max_batch", 10)
        with pytest.raises(hipapi.MemeError, match="exceed the ctx's"):
            ctx.sam_format_batch_host(recs[:11], blob, contigs)
        a, b = ctx.sam_format_batch_host(recs[:10], blob, contigs), free.sam_format_batch_host(recs[:10], blob, contigs)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[1].shape[0] == 11 and len(a[0]) > 0
    finally:
        ctx.close()
