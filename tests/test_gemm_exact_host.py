"""CPU checks of tests/helpers/gemm_exact.py: for every problem tests/test_gpu_gemm_forms.py and tests/test_gpu_gemm256_forms.py generate,
the conditions that make its reference exact hold -- magnitudes, distinct rows / columns, an order-independent loss sum, float32 == float64 -- and the case table
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


# ------------------------------------------------------------------------------------------------ the 256 x 256 macro tile
def test_macro_table_covers_the_instantiations():
    cases = GX.macro_cases()
    big = [c for c in cases if (c.M, c.N) == GX.MACRO_SHAPE]
    one = [c for c in cases if (c.M, c.N, c.Ks) == (256, 256, (64,))]
    assert len(big) + len(one) == len(cases) and one
    assert GX.MACRO_SHAPE == (5 * 256, 3 * 256) and all(c.Ks == GX.K_SET for c in big) and max(GX.K_SET) == 576
    # the non-Adam pairs of gemm_bf16_256_launch (csrc/gemm_bf16_256.hip), both reconstruction kinds; DW + ADAM: tests/test_gpu_dw_adam_forms.py
    src = open(os.path.join(ROOT, "deep-mixture-vae_amd", "csrc", "gemm_bf16_256.hip")).read()
    lay = {"DMVAE_GEMM_FWD": GX.FWD, "DMVAE_GEMM_DX": GX.DX, "DMVAE_GEMM_DW": GX.DW}
    inst = {(lay[l], getattr(GX, e.replace("DMVAE_", ""))) for l, e in re.findall(r"CASE256\((DMVAE_GEMM_\w+), (DMVAE_EPI_\w+)\)", src) if e != "DMVAE_EPI_ADAM"}
    assert len(inst) == 6 and {(c.pair.layout, c.pair.epi) for c in big} == inst == {(c.pair.layout, c.pair.epi) for c in one}
    assert {c.pair.recon_kind for c in big if c.pair.epi == GX.EPI_BIAS_RECON} == {0, 1}
    rest = GX.macro_fallback_cases()
    assert all((c.pair.layout, c.pair.epi) not in inst or c.pair.split > 1 for c in rest) and all(c.M % 256 == 0 and c.N % 256 == 0 for c in rest)
    assert {c.pair.name for c in cases} | {c.pair.name for c in rest} == set(GX.PAIRS) - {"dw_atomic_s4"}
    assert max(M * N * K for (_, M, N, K) in GX.all_problem_keys() if M % 256 == 0 and N % 256 == 0) <= 1280 * 768 * 576


@pytest.mark.parametrize("K", GX.K_SET)
def test_macro_loss_partial_of_a_tile_is_exact_in_any_order(K):
    p = GX.make("fwd_recon_real", GX.MACRO_SHAPE[0], GX.MACRO_SHAPE[1], K)
    t = np.abs(p.expected["terms"][0])
    assert (t * 32 == np.rint(t * 32)).all() and GX.tile_sums(t, 256, 256).max() * 32 < 2 ** 24
    # rows m and m + 2 K of the one-hot A coincide: a 256-row tile holds repeats at K = 64 (the integer pairs cover swapped halves there)
    assert GX.tile_sums(t, 256, 256).min() > 0


@pytest.mark.parametrize("key", [k for k in GX.CSUM_OUT_CASES if k[0] not in GX.INEXACT] + [GX.CHAIN_DX], ids=lambda k: "%s-%dx%dx%d" % k)
def test_column_sums_are_exact_in_any_order(key):
    p = GX.make(*key)
    o = GX.bf16_round(p.expected["out"][0])
    if p.pair.epi == GX.EPI_BIAS_RECON:
        assert (o == p.expected["out"][0]).all() and not o[p.m_valid:].any() and not o[:, p.n_valid:].any()
    bad = [what for what, ok in GX.colsum_exact_report(o).items() if not ok]
    assert not bad, (key, bad)
    want = GX.csum_out_expected(p)
    assert want.shape == (p.M // 256, p.N) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert (np.abs(want).sum(1) > 0).all() and len(np.unique(want, axis=0)) == len(want)       # no two tile rows alike: a wrong tm shows
    # dropping a row class (a lane group g handles the rows r of each 64-row block with r % 4 == g) or a wave row changes some column of every tile row
    rows = np.arange(p.M)
    o2 = o.copy()
    if p.pair.epi == GX.EPI_BIAS_RECON:
        o2[p.m_valid:] = 0
        o2[:, p.n_valid:] = 0
    for drop in [(rows % 4) == g for g in range(4)] + [((rows // 64) % 2) == w for w in range(2)]:
        part = GX.tile_colsums(np.where(drop[:, None], 0.0, o2))
        assert (part != want).any(axis=1).all()


def test_column_sum_quantum_condition_rejects_what_it_should():
    assert all(GX.colsum_exact_report(np.full((256, 4), 3.0)).values())
    assert all(GX.colsum_exact_report(np.full((256, 4), 2.0 ** 17)).values())                    # 256 quanta of 2^17
    a = np.full((256, 4), 2.0 ** 17)
    a[0, 0] = 1.0
    assert not all(GX.colsum_exact_report(a).values())                                          # q = 1, the sum 2^25


def test_csum_in_partials_and_the_chain():
    for (M, N, K, rows) in GX.CSUM_IN_CASES:
        part = GX.csum_in_partials(M, N, K, rows)
        p = GX.make("dw_store_db", M, N, K)
        assert part.shape == (rows, N) and (part == np.rint(part)).all() and np.abs(part).sum(0).max() < 2 ** 24
        assert not np.array_equal(part.sum(0), p.expected["out2"][0].reshape(N))                 # not what a recomputation from dY gives
    assert sorted(r for (_, _, _, r) in GX.CSUM_IN_CASES) == [1, 2, 5]
    assert len(GX.CSUM_IN_MERGED) >= 2 and all(0 <= i < len(GX.CSUM_IN_CASES) for i in GX.CSUM_IN_MERGED)
    p, X, dY, dW, db = GX.chain_problem()
    assert (GX.bf16_round(X) == X).all() and (GX.bf16_round(dY) == dY).all() and (dY == np.rint(dY)).all()
    assert (np.abs(X).T @ np.abs(dY)).max() < 2 ** 24 and np.abs(dY).sum(0).max() < 2 ** 24
    assert np.array_equal(GX.tile_colsums(dY).sum(0), db) and np.array_equal(db, GX.csum_out_expected(p).sum(0)) and np.abs(db).max() > 0
    assert len(np.unique(X.T, axis=0)) == GX.CHAIN_X
    M, N, K = GX.CHAIN_DW                                                                          # (no make() problem: not in all_problem_keys())
    assert (M, N, K) == dW.shape + (p.M,) and M % 256 == 0 and N % 256 == 0 and K % 64 == 0 and M * N * K <= 1280 * 768 * 576


def test_k_slice_partial_products():
    assert {ks for (_, _, ks, n) in GX.SLICE_CASES if n > 1} == {64, 128, 192} and {n for (_, _, _, n) in GX.SLICE_CASES} == {1, 2, 3}
    merged = [GX.SLICE_CASES[i] for i in GX.SLICE_MERGED]
    assert sorted(n for (_, _, _, n) in merged) == [1, 2, 3]
    for (M, N, ks, nsl) in GX.SLICE_CASES:
        p = GX.make("dw_store_db", M, N, ks * nsl)
        parts = GX.slice_partials(p, ks, nsl)
        assert parts.shape == (nsl, M, N) and np.array_equal(parts.sum(0), p.expected["out"][0])
        assert (np.abs(p.A) @ np.abs(p.B)).max() < 2 ** 24                                       # bounds every slice's partial sums too
        for y in range(nsl):
            for z in range(y):
                assert not np.array_equal(parts[y], parts[z])                                    # a slice that ignores its K offset shows
            assert nsl == 1 or not np.array_equal(parts[y], p.expected["out"][0])


def test_macro_gpu_file_parametrizes_this_table():
    src = open(os.path.join(ROOT, "tests", "test_gpu_gemm256_forms.py")).read()
    for table in ("GX.macro_cases()", "GX.macro_fallback_cases()", "GX.CSUM_OUT_CASES", "GX.CSUM_IN_CASES", "GX.CSUM_IN_MERGED", "GX.CHAIN_DW", "GX.chain_problem()", "GX.SLICE_CASES", "GX.SLICE_MERGED"):
        assert table in src, table
    assert not re.search(r"pytest\.mark\.(skip|xfail)|pytest\.(skip|xfail)\(", src)
    assert "test_gpu_gemm256_forms.py" in open(os.path.join(ROOT, "include", "dmvae_hip_debug.h")).read()


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
