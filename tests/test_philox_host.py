"""CPU tests of the device-noise oracle (tests/helpers/philox_oracle.py) and of the counter layouts it restates from the kernels
("noise streams"): the cipher against the published Random123 known-answer vectors of Philox4x32-10, every
layout free of collisions, the streams / steps / per-rank seeds apart.  tests/test_gpu_philox.py holds the kernels to this oracle."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import philox_oracle as P      # noqa: E402

# counter ; key -> output (Random123's kat_vectors, philox4x32 with 10 rounds)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

# (D, K) of the latent tests of tests/test_gpu_kernels.py / test_gpu_philox.py (every D they use: 3, 10, 30, 64, 96, 256, 300, 512) ...
TEST_DK = [(3, 5), (10, 10), (30, 7), (30, 200), (64, 10), (64, 64), (96, 130), (256, 50), (300, 50), (512, 256), (200, 7), (256, 10), (100, 16)]
# ... and of the five configs of BASELINE.json
BASELINE_DK = [(10, 10), (64, 10), (128, 10), (256, 50), (512, 256)]
ALL_DK = sorted(set(TEST_DK + BASELINE_DK))
B_MAX = 4096


def test_known_answer_vectors():
    for ctr, key, out in KAT:
        got = P.philox4x32_10(np.array(ctr, dtype=np.uint64), key[0], key[1])
        assert [int(x) for x in got] == list(out)
    # vectorised: the three at once, keys per element
    got = P.philox4x32_10(np.array([k[0] for k in KAT], dtype=np.uint64), np.array([k[1][0] for k in KAT], dtype=np.uint64),
                          np.array([k[1][1] for k in KAT], dtype=np.uint64))
    np.testing.assert_array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint64))


def test_block_packs_the_counter_as_philox_block_does():
    """word 0 = low half of blk, word 1 = high half ^ (stream << 24), words 2, 3 = step, key = seed"""
    seed, step, sid, blk = 0xDEADBEEF12345678, (1 << 32) + 5, 3, (0x00ABCDEF << 32) | 0x89ABCDEF
    want = P.philox4x32_10(np.array([0x89ABCDEF, 0x00ABCDEF ^ (3 << 24), 5, 1], dtype=np.uint64), 0x12345678, 0xDEADBEEF)
    np.testing.assert_array_equal(P.block(seed, step, sid, blk), want)
    np.testing.assert_array_equal(P.block(seed, step, sid, np.array([blk, blk], dtype=np.uint64))[1], want)
    np.testing.assert_array_equal(P.words_flat(seed, step, sid, 7, first_block=blk)[:4], want)


def test_transforms_on_the_grid_and_at_its_ends():
    top, bot = np.uint64(0xFFFFFFFF), np.uint64(0)
    assert P.uniform(top) == 1.0 - 2.0 ** -24 and P.uniform(bot) == 0.0 and P.uniform(np.uint64(0x1FF)) == 2.0 ** -24
    assert P.u01(top) == 1.0 and P.u01(bot) == 2.0 ** -24 and P.u01(np.uint64(0xFFFFFF00)) == 1.0
    # Gumbel: the U = 1 atom is the float32 constant's logarithm, the other end -log(24 ln 2); in between -log(-log(U))
    assert float(P.gumbel(top)) == pytest.approx(-math.log(float(np.float32(1e-20))), rel=1e-15) == pytest.approx(46.0517, abs=1e-4)
    assert float(P.gumbel(bot)) == pytest.approx(-math.log(24 * math.log(2)), rel=1e-15) == pytest.approx(-2.8116, abs=1e-4)
    w = np.uint64(0x80000000)
    assert float(P.gumbel(w)) == pytest.approx(-math.log(-math.log((2 ** 23 + 1) * 2.0 ** -24)), rel=1e-15)
    # Box-Muller: words (0, 1) -> normals (0, 1), words (2, 3) -> normals (2, 3); radius 0 at u01 = 1, sqrt(48 ln 2) at 2^-24
    words = np.array([0xFFFFFF00, 0x40000000, 0, 0xBFFFFFFF], dtype=np.uint64)
    n = P.normal4(words)
    assert n[0] == 0.0 and n[1] == 0.0
    rad, ang = math.sqrt(48 * math.log(2)), 2 * math.pi * (0xBFFFFF + 1) * 2.0 ** -24
    assert n[2] == pytest.approx(rad * math.cos(ang), abs=1e-12) and n[3] == pytest.approx(rad * math.sin(ang), abs=1e-12)
    # the element forms: normal_at(idx) = normal (idx & 1) of block idx >> 1; gumbel_at / uniform_at(idx) = word (idx & 3) of block idx >> 2
    idx = np.arange(11, dtype=np.uint64) + np.uint64(6)
    blk = P.block(42, 3, 1, np.arange(0, 9, dtype=np.uint64))
    np.testing.assert_array_equal(P.normal_at(42, 3, 1, idx), P.normal4(blk)[:, :2].reshape(-1)[6:17])
    np.testing.assert_array_equal(P.gumbel_at(42, 3, 1, idx), P.gumbel(blk.reshape(-1)[6:17]))
    np.testing.assert_array_equal(P.uniform_at(42, 3, 1, idx), P.uniform(blk.reshape(-1)[6:17]))


def test_one_kernel_geometry_restates_the_launch():
    """latent.hip latent_geometry at the shapes whose chunking is spelled out in the kernels' tests and in DESIGN.md"""
    assert P.one_kernel_geometry(64, 3, 5) == (16, 16, 1, 1)
    assert P.one_kernel_geometry(128, 10, 10) == (16, 16, 1, 1)           # cfg1: DC = 16 (tests/test_gpu_heads_latent.py CASES)
    assert P.one_kernel_geometry(256, 20, 33) == (16, 32, 1, 2)           # DC = 32 (same place)
    assert P.one_kernel_geometry(4096, 64, 10) == (16, 64, 1, 4)          # cfg2
    assert P.one_kernel_geometry(1024, 128, 10) == (16, 128, 1, 8)        # cfg3's latent geometry at one round of the chip
    assert P.one_kernel_geometry(64, 256, 10) == (16, 256, 1, 16) and P.one_kernel_geometry(64, 200, 7) == (16, 256, 1, 16)
    assert P.one_kernel_geometry(128, 256, 50)[1:] == (64, 4, 4)          # cfg4: the prior tables in four D-chunks (tests/test_gpu_step.py WIDE)
    RB, DC, nchunks, DSL = P.one_kernel_geometry(192, 300, 50)
    assert (RB, DSL * 16, nchunks) == (16, DC, -(-300 // DC)) and nchunks > 1 and P.latent_lds_bytes(50, RB, DC) <= 60 * 1024
    assert P.one_kernel_geometry(16384, 128, 10)[0] == 32 and P.one_kernel_geometry(65536, 256, 50)[0] == 64


def _assert_injective(blk, slot, what):
    key = (blk.astype(np.uint64) * np.uint64(4) + slot.astype(np.uint64)).reshape(-1)
    assert int(blk.max()) < P.BLK_LIMIT, what
    assert np.unique(key).size == key.size, "%s: %d (block, slot) pairs drawn twice" % (what, key.size - np.unique(key).size)


@pytest.mark.parametrize("D,K", ALL_DK)
def test_layouts_are_injective(D, K):
    """(b, d) -> (block, slot) without collisions over B x D, B up to 4096, for every layout; over the PADDED width too where the lanes
    draw for padding columns (one-kernel: up to nchunks * DC; MFMA: up to D padded to 64): no padding column takes a slot of a real one"""
    for B in (1, 37, B_MAX):
        B_pad = (B + 63) // 64 * 64
        _assert_injective(*P.latent_one_kernel(B, D, K, B_pad), "one-kernel B=%d" % B)
        _assert_injective(*P.latent_one_kernel(B, D, K, B_pad, width=P.one_kernel_width(B_pad, D, K)), "one-kernel, padded, B=%d" % B)
        _assert_injective(*P.latent_mfma(B, D), "MFMA B=%d" % B)
        _assert_injective(*P.latent_mfma(B, D, width=(D + 63) // 64 * 64), "MFMA, padded, B=%d" % B)
        _assert_injective(*P.latent_vade(B, D), "VaDE B=%d" % B)
        _assert_injective(*P.gumbel_layout(B, K), "Gumbel B=%d" % B)
    # rows per block 32 and 64 (batches of 16 384 and 65 536 rows) change the LDS budget, hence possibly the chunk width
    for B_pad in (16384, 65536):
        _assert_injective(*P.latent_one_kernel(257, D, K, B_pad, width=P.one_kernel_width(B_pad, D, K)), "one-kernel B_pad=%d" % B_pad)
    # the real columns of the padded layout are the unpadded layout
    blk, slot = P.latent_one_kernel(37, D, K, 64, width=P.one_kernel_width(64, D, K))
    b0, s0 = P.latent_one_kernel(37, D, K, 64)
    assert np.array_equal(blk[:, :D], b0) and np.array_equal(slot[:, :D], s0)
    # normal slots 0..3; a layout on philox_normal_at uses 0 and 1 only
    assert set(np.unique(P.latent_vade(37, D)[1])) <= {0, 1} and set(np.unique(slot)) <= {0, 1, 2, 3}


@pytest.mark.parametrize("D", [3, 10, 64])
def test_eval_layout_is_injective(D):
    draws, n_rows = 10, 1100
    blk, slot = P.eval_draws(draws, n_rows, D)
    _assert_injective(blk, slot, "eval")
    # a batch's window is the whole set's layout at its rows (the draw of a row depends on its position, not on the batch)
    b2, s2 = P.eval_draws(draws, n_rows, D, first=9, n=83)
    assert np.array_equal(b2, blk[:, 9:92]) and np.array_equal(s2, slot[:, 9:92])


def test_one_kernel_and_mfma_forms_draw_different_eps():
    """documented in DESIGN.md: the two forms of the exact latent stage key the same (seed, step, b, d) differently.  (At D = 64 a row's
    sixteen blocks are the same in both and its columns a permutation of one another: d = 0, 21, 42, 63 are its fixed points.)"""
    a = P.eps_one_kernel(1234, 7, 8, 64, 10)
    b = P.eps_mfma(1234, 7, 8, 64)
    assert a.shape == b.shape == (8, 64) and (np.abs(a - b) > 1e-3).mean() > 0.9
    np.testing.assert_array_equal(np.sort(a, axis=1), np.sort(b, axis=1))
    a, b = P.eps_one_kernel(1234, 7, 8, 300, 50), P.eps_mfma(1234, 7, 8, 300)
    assert (np.abs(a - b) > 1e-3).mean() > 0.9


def _leading(seed, step, sid, n=4096):
    w = P.block(seed, step, sid, np.arange(n, dtype=np.uint64))
    return {tuple(int(x) for x in r) for r in w}


def test_streams_steps_and_rank_seeds_are_disjoint():
    seed, step = 1234, 7
    # streams 0..3 at the same (seed, step, blk): no block output shared, position by position and as sets
    sets = [_leading(seed, step, sid) for sid in range(4)]
    for i in range(4):
        assert len(sets[i]) == 4096
        for j in range(i + 1, 4):
            assert not (sets[i] & sets[j]), (i, j)
    # the stream id reaches the counter: dropping it would make every stream stream 0
    blk = np.arange(64, dtype=np.uint64)
    for sid in (1, 2, 3):
        assert (P.block(seed, step, sid, blk) != P.block(seed, step, 0, blk)).any(axis=1).all()
    # steps t and t + 1, also across the 32-bit boundary of the step (its high half is word 3)
    for t in (0, 7, (1 << 32) - 1, (1 << 40) + 3):
        assert not (_leading(seed, t, 0) & _leading(seed, t + 1, 0)), t
    assert not (_leading(seed, 5, 0) & _leading(seed, (1 << 32) + 5, 0))
    # base_models.py gives rank r the seed s + 7919 r
    for s in (0, 1234, (1 << 32) - 7919 * 3, 0xDEADBEEF12345678):
        ranks = [_leading((s + 7919 * r) & (2 ** 64 - 1), step, 0) for r in range(8)]
        for i in range(8):
            for j in range(i + 1, 8):
                assert not (ranks[i] & ranks[j]), (s, i, j)
    # both halves of the seed are key material
    assert not (_leading(0x12345678, step, 0) & _leading(0xDEADBEEF12345678, step, 0))


def test_block_index_stays_below_the_stream_bits():
    """stream_id << 24 is XORed into the HIGH counter word: bits 56..63 of the block index.  A block index of 2^56 or more would move a
    draw into another stream.  The largest index each consumer can form: its row count is a 32-bit int, and every element it keys is
    an element of an f32 array it writes, so B * D and B * K are below 2^38 / 4 (288 GB of HBM); the bound below takes the whole
    int range of B at the widest layout of the configs instead."""
    b_last = np.uint64((1 << 31) - 2)
    for D, K in ALL_DK:
        for B_pad in (64, 65536):
            blk, _ = P.latent_one_kernel(1, D, K, B_pad, width=P.one_kernel_width(B_pad, D, K))
            per_row = int(blk.max()) + 1                                   # row 0 holds blocks [0, per_row): the layout is row-major in b
            assert np.array_equal(P.latent_one_kernel(2, D, K, B_pad)[0][1], P.latent_one_kernel(1, D, K, B_pad)[0][0] + np.uint64(per_row))
            assert (int(b_last) + 1) * per_row < P.BLK_LIMIT
        assert (int(b_last) + 1) * ((D + 63) // 64 * 16) < P.BLK_LIMIT    # MFMA: Dp / 4 blocks per row
        assert ((int(b_last) + 1) * D) >> 1 < P.BLK_LIMIT                  # VaDE
        assert ((int(b_last) + 1) * K) >> 2 < P.BLK_LIMIT                  # Gumbel
    # eval: draws * n_rows * D elements, two per block: 1024 draws (EVAL_MAX_DRAWS) of 65 000 rows at the widest latent space of the configs
    assert (1024 * 65000 * 512) >> 1 < P.BLK_LIMIT
    blk, _ = P.eval_draws(1024, 65000, 512, first=64999, n=1)
    assert int(blk.max()) == (1024 * 65000 * 512 - 1) >> 1
    # k-means++ seeding: restarts * K * local trials uniform draws, four per block
    assert (1 << 31) >> 2 < P.BLK_LIMIT


def test_edge_words_of_the_gumbel_stream():
    """the first words of stream (42, 3, 1) at the two ends of the u01 grid, which tests/test_gpu_philox.py launches over"""
    assert P.find_edge_word(42, 3, 1, "bottom", max_blocks=1 << 22) == 5262247
    assert P.find_edge_word(42, 3, 1, "top", max_blocks=1 << 22) == 12300443
    w = P.words_flat(42, 3, 1, 4, first_block=12300443 >> 2)
    assert int(w[12300443 & 3]) >= 0xFFFFFF00
