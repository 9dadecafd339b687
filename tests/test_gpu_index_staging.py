"""The index staging kernels and the shared prefix sum, each against a numpy restatement, bit for bit.

k_pack_text (the 2-bit text: its vector path, the scalar tail of a text that is no multiple of 32 bases, the 8 pad words), k_build_entries from the 5-byte image
and from the u64 array, k_pos5_from_sa (the on-disk encoding of the reference, src/Learnedindex.cpp:475-478: the upper 32 bits little-endian, then the low
byte) and k_rmi32 run for every index but were only checked through what is built on them.  meme_scan_exclusive sizes every stage's output; the second trip of
k_scan_tile_offsets' loop, with its carry, takes more than 256 x 2 048 counts, which no batch of the suite has."""
import ctypes as C

import numpy as np
import pytest
import torch

import index_cases as IC
from common import entry_keys, pos5_image
from pymeme import hipapi, hostapi

pytestmark = pytest.mark.gpu

GUARD = 0x5a5a5a5a5a5a5a5a
# n = 64 (the least), 66 and 74 (a scalar tail in the third word), 96 (whole words only), 4 000 (a multiple of 32: no tail) and 4 200 (more than one workgroup, a tail)
TEXTS = {"smallest": 64, "odd_33": 66, "odd_37": 74, "whole_words_96": 96, "no_ties_2000": 4000, "copies_3x700": 4200}


@pytest.fixture(scope="module")
def ctx():
    c = hipapi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _text_sa(name):
    fwd = IC.rand(48, 96) if name == "whole_words_96" else IC.FORWARD[name]
    text, sa = hostapi.build_sa(fwd)
    assert text.shape[0] == TEXTS[name]
    return text, sa


def _pack(text, words):
    """2 bits per base, the first base of a word in its top bits; T past the text, through the last pad word"""
    b = np.full(words * 32, 3, np.uint64)
    b[:text.shape[0]] = text
    w = np.zeros(words, np.uint64)
    for r in range(32):
        w = (w << np.uint64(2)) | b[r::32]
    return w


def _guarded(count, dtype, dev, guard=4):
    """`count` items and `guard` more behind them, all filled with a pattern no result has"""
    return torch.full((count + guard,), GUARD if dtype == torch.int64 else 0x5a, dtype=dtype, device=dev)


@pytest.mark.parametrize("name", list(TEXTS))
def test_text_words_and_entries(ctx, dev, name):
    text, sa = _text_sa(name)
    n = int(text.shape[0])
    L, h = hipapi.lib(), C.c_void_p(ctx.h)
    words = L.meme_index_pac64_words(n)
    assert words == (n + 31) // 32 + 8
    d_text = torch.from_numpy(text).to(dev)
    d_pac = _guarded(words, torch.int64, dev)
    d_sa = torch.from_numpy(sa.view(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    hipapi._check(L.meme_stage_pack_text(h, C.c_void_p(d_text.data_ptr()), C.c_int64(n), C.c_void_p(d_pac.data_ptr())))
    ctx.sync()
    pac = d_pac.cpu().numpy().view(np.uint64)
    want = _pack(text, words)
    assert np.array_equal(pac[:words], want), "first differing word %d of %d" % (np.nonzero(pac[:words] != want)[0][0], words)
    assert (pac[words:] == np.uint64(GUARD)).all() and torch.equal(d_text.cpu(), torch.from_numpy(text))
    # the 5-byte image of the array, then entries from the image and from the array itself
    d_pos5 = hipapi.pos5_from_sa_torch(ctx, d_sa, n)
    assert np.array_equal(d_pos5.cpu().numpy()[:5 * n], pos5_image(sa))
    d_e5, d_e8 = _guarded(2 * n, torch.int64, dev), _guarded(2 * n, torch.int64, dev)
    torch.cuda.synchronize(dev)
    hipapi._check(L.meme_stage_build_entries(h, C.c_void_p(d_pos5.data_ptr()), C.c_int64(n), C.c_void_p(d_pac.data_ptr()), C.c_void_p(d_e5.data_ptr())))
    hipapi._check(L.meme_stage_entries_from_sa(h, C.c_void_p(d_sa.data_ptr()), C.c_int64(n), C.c_void_p(d_pac.data_ptr()), C.c_void_p(d_e8.data_ptr())))
    ctx.sync()
    e5, e8 = d_e5.cpu().numpy().view(np.uint64), d_e8.cpu().numpy().view(np.uint64)
    assert np.array_equal(e5, e8) and (e5[2 * n:] == np.uint64(GUARD)).all()
    ent = e5[:2 * n].reshape(n, 2)
    keys = entry_keys(text, sa)
    assert np.array_equal(ent[:, 1], sa), "positions: first differing slot %d" % np.nonzero(ent[:, 1] != sa)[0][:1]
    assert np.array_equal(ent[:, 0], keys), "keys: first differing slot %d" % np.nonzero(ent[:, 0] != keys)[0][:1]


@pytest.mark.parametrize("name", list(TEXTS))
def test_rmi32_records(ctx, dev, name):
    """every field of every record, the pad word zero, nothing behind the last record"""
    text, sa = _text_sa(name)
    l1, l2 = hostapi.train_prmi(text, sa, bits=6, partial_threshold=20)
    rng = np.random.default_rng(TEXTS[name])
    any_bits = rng.integers(0, 1 << 63, size=(37, 3), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(37, 3), dtype=np.uint64)   # NaNs and all
    L, h = hipapi.lib(), C.c_void_p(ctx.h)
    for recs in (l2.view(np.uint64).reshape(-1, 3), l1.view(np.uint64).reshape(-1, 3), any_bits, any_bits[:1]):
        k = recs.shape[0]
        if k == 0:
            continue
        d_in = torch.from_numpy(np.ascontiguousarray(recs).view(np.int64).reshape(-1)).to(dev)
        d_out = _guarded(4 * k, torch.int64, dev)
        torch.cuda.synchronize(dev)
        hipapi._check(L.meme_stage_rmi32(h, C.c_void_p(d_in.data_ptr()), C.c_int64(k), C.c_void_p(d_out.data_ptr())))
        ctx.sync()
        out = d_out.cpu().numpy().view(np.uint64)
        got = out[:4 * k].reshape(k, 4)
        assert np.array_equal(got[:, :3], recs) and not got[:, 3].any() and (out[4 * k:] == np.uint64(GUARD)).all()
    d_out = _guarded(4, torch.int64, dev)
    torch.cuda.synchronize(dev)
    hipapi._check(L.meme_stage_rmi32(h, C.c_void_p(0), C.c_int64(0), C.c_void_p(d_out.data_ptr())))      # no record: nothing to do, nothing written
    ctx.sync()
    assert bool((d_out == GUARD).all())


def test_pos5_of_any_40_bit_value(ctx, dev):
    """the kernel only encodes: no index needed.  Byte for byte the reference's `.pos_packed` record: (value >> 8) as four little-endian bytes, then value & 0xff"""
    rng = np.random.default_rng(40)
    edge = [0, 1, 255, 256, 257, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) - 256, (1 << 40) - 1, 0x0102030405]
    v = np.concatenate([np.array(edge, np.uint64), rng.integers(0, 1 << 40, size=1000 - len(edge), dtype=np.uint64)])
    want = np.empty((v.shape[0], 5), np.uint8)
    for b in range(4):
        want[:, b] = ((v >> np.uint64(8 + 8 * b)) & np.uint64(0xff)).astype(np.uint8)
    want[:, 4] = (v & np.uint64(0xff)).astype(np.uint8)
    assert want[len(edge) - 1].tolist() == [4, 3, 2, 1, 5] and np.array_equal(want.reshape(-1), pos5_image(v))      # 0x0102030405
    n = int(v.shape[0])
    d_v = torch.from_numpy(v.view(np.int64)).to(dev)
    d_pos5 = _guarded(5 * n, torch.uint8, dev, guard=16)
    torch.cuda.synchronize(dev)
    hipapi._check(hipapi.lib().meme_stage_pos5_from_sa(C.c_void_p(ctx.h), C.c_void_p(d_v.data_ptr()), C.c_int64(n), C.c_void_p(d_pos5.data_ptr())))
    ctx.sync()
    got = d_pos5.cpu().numpy()
    assert np.array_equal(got[:5 * n].reshape(n, 5), want), "first differing value %d" % np.nonzero((got[:5 * n].reshape(n, 5) != want).any(axis=1))[0][:1]
    assert (got[5 * n:] == 0x5a).all()


# ---- the prefix sum ------------------------------------------------------------------------------------------------------------------------------------
# around a lane's 8 items, a tile of 2 048, the 256 tiles one trip of k_scan_tile_offsets' loop takes (524 288 counts), and three trips with a ragged end
SCAN_SIZES = (0, 1, 7, 8, 9, 2047, 2048, 2049, 524_287, 524_288, 524_289, 1_572_869)


def _scan(ctx, dev, counts, in_place=False):
    n = int(counts.shape[0])
    want = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=want[1:])
    d_in = _guarded(n + 1 if in_place else n, torch.int64, dev)
    d_in[:n] = torch.from_numpy(counts).to(dev)
    d_out = d_in if in_place else _guarded(n + 1, torch.int64, dev)
    torch.cuda.synchronize(dev)
    ctx.debug_scan_exclusive(d_in.data_ptr(), d_out.data_ptr(), n)
    out = d_out.cpu().numpy()
    if not np.array_equal(out[:n + 1], want):
        bad = np.nonzero(out[:n + 1] != want)[0]
        raise AssertionError("n = %d: %d sums differ, first at %d: %d vs %d" % (n, bad.size, bad[0], out[bad[0]], want[bad[0]]))
    assert out[n] == counts.sum() and (out[n + 1:] == GUARD).all()
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy()[:n], counts) and (d_in.cpu().numpy()[n:] == GUARD).all()


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_exclusive(ctx, dev, n):
    counts = np.random.default_rng(n).integers(0, 1001, size=n).astype(np.int64)
    _scan(ctx, dev, counts)
    _scan(ctx, dev, counts, in_place=True)                     # n + 1 values allocated: the total lands behind the counts


def test_scan_sums_beyond_32_bits(ctx, dev):
    _scan(ctx, dev, np.full(1_572_869, 1 << 33, np.int64))     # the total is 2^53.6
    _scan(ctx, dev, np.full(9, 1 << 33, np.int64))


def test_scan_refuses_bad_arguments(ctx, dev):
    d = torch.zeros(16, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    L, h = hipapi.lib(), C.c_void_p(ctx.h)
    assert L.meme_debug_scan_exclusive(h, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), C.c_int64(-1)) == -2
    assert L.meme_debug_scan_exclusive(h, C.c_void_p(0), C.c_void_p(d.data_ptr()), C.c_int64(4)) == -2
    assert L.meme_debug_scan_exclusive(h, C.c_void_p(d.data_ptr()), C.c_void_p(0), C.c_int64(4)) == -2
    _scan(ctx, dev, np.arange(15, dtype=np.int64))
