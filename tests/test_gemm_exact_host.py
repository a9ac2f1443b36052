"""CPU checks of tests/helpers/gemm_exact.py: for every problem tests/test_gpu_gemm_forms.py generates, the conditions that make its
reference exact hold -- magnitudes, distinct rows / columns, an order-independent loss sum, float32 == float64 -- and the case table
is the one the GPU file parametrizes."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import gemm_exact as GX      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("key", GX.all_problem_keys(), ids=lambda k: "%s-%dx%dx%d" % k)
def test_reference_is_exact(key):
    p = GX.make(*key)
    bad = [what for what, ok in GX.exactness_report(p).items() if not ok]
    assert not bad, (key, bad)


def test_case_table_covers_the_matrix():
    dense = GX.dense_cases()
    ids = GX.all_case_ids()
    assert len(ids) == len(set(ids))
    by_form = {}
    for c in dense:
        by_form.setdefault(c.form.name, set()).add(c.pair.name)
        assert (c.M, c.N) == (5 * c.form.bm, GX.LATENT_D if c.pair.epi == GX.EPI_LATENT else 3 * c.form.bn)
        assert all(k % (64 * c.pair.split) == 0 and k // c.pair.split in GX.K_SET for k in c.Ks)
        assert max(c.Ks) // c.pair.split == (128 if c.form.short else 576) and min(c.Ks) // c.pair.split == 64
    every = set(GX.PAIRS)
    assert set(by_form) == set(GX.FORMS)
    for f in ("64x64", "128x64w4", "128x64w8"):
        assert by_form[f] == every                                               # all ten (layout, epilogue) pairs of gemm_bf16_dispatch, both recon kinds, both splits
    for f in ("64x128", "128x128w4", "128x128w8"):
        assert by_form[f] == every - {"dx_latent"}                               # LATENT: N = D = 64
    assert by_form["64x64s2"] == {n for n, p in GX.PAIRS.items() if p.layout != GX.DW and p.epi != GX.EPI_BIAS_RECON}
    assert {(p.layout, p.epi) for p in GX.PAIRS.values()} == {(0, 0), (0, 1), (0, 2), (0, 7), (0, 5), (1, 5), (1, 3), (1, 4), (2, 5), (2, 6)}
    assert {c.group_m for c in GX.supertile_cases()} == {2, 3, 4} and all(c.M // c.form.bm == 5 and c.N // c.form.bn == 3 for c in GX.supertile_cases())
    assert [c.pair.name for c in GX.f32_cases()] == list(GX.PAIRS)
    assert all(K > 256 or len(GX.GROUP_DX) > 2 for (_, _, K) in GX.GROUP_DX) and all(K == 128 and N % 128 == 0 for (_, N, K) in GX.GROUP_DX_STREAM)


def test_gpu_file_parametrizes_this_table():
    src = open(os.path.join(ROOT, "tests", "test_gpu_gemm_forms.py")).read()
    for table in ("GX.dense_cases()", "GX.supertile_cases()", "GX.THIN_CASES", "GX.grouped_cases()", "GX.f32_cases()", "GX.GROUP_DX_STREAM"):
        assert table in src, table
    assert not re.search(r"pytest\.mark\.(skip|xfail)|pytest\.(skip|xfail)\(", src)


def test_epilogue_ids_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "dmvae_hip.h")).read()
    for name in ("BIAS_RELU", "BIAS_F32", "BIAS_RECON", "RELU_MASK", "LATENT", "STORE_F32", "ATOMIC_F32", "BIAS_SIGMOID"):
        m = re.search(r"DMVAE_EPI_%s\s*=\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(GX, "EPI_" + name), name


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([256.0, 257.0, 258.0, 259.0, 261.0, 263.0, -257.0, -259.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 4352.0, 4353.0, 0.0, 2.0 ** -126])
    want = np.array([256.0, 256.0, 258.0, 260.0, 260.0, 264.0, -256.0, -260.0, 1.0, 1.0 + 2.0 ** -6, 4352.0, 4352.0, 0.0, 2.0 ** -126])
    np.testing.assert_array_equal(GX.bf16_round(x), want)
    rng = np.random.RandomState(0)
    y = np.concatenate([rng.randint(-5000, 5000, size=4096).astype(np.float64), rng.randint(-80, 80, size=4096) / 1024.0])
    np.testing.assert_array_equal(GX.bf16_round(y), GX.bf16_round_bits(y))


def test_tile_sums_and_binary_reference():
    t = np.arange(128 * 192, dtype=np.float64).reshape(128, 192)
    s = GX.tile_sums(t, 64, 64)
    assert s.shape == (2, 3) and s[1, 2] == t[64:, 128:].sum() and s.sum() == t.sum()
    p = GX.make("fwd_recon_binary", 320, 192, 64)
    per, d = GX.binary_reference(p, p.expected["out2"][0])
    assert not per[p.m_valid:].any() and not per[:, p.n_valid:].any() and not d[p.m_valid:].any() and (per[:p.m_valid, :p.n_valid] > 0).all()
