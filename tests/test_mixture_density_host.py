"""CPU tests (-m "not gpu") of the posterior diagnostics (dmvae_hip/density.py, csrc/mixture_density.hip): the float64 oracle of
tests/helpers/mixture_density_oracle.py against sklearn's GaussianMixture.score_samples and against closed forms, the sequential-float32
yardstick against the oracle's bar (and the expanded form refused by it on the floor kind), the new symbols in the header / the
library / the binding, and the --diagnostics flag."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import mixture_density_oracle as MO      # noqa: E402
import trained_latents as TL             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dmvae_mixture_logpdf_ws_bytes", "dmvae_mixture_logpdf_split", "dmvae_mixture_logpdf", "dmvae_posterior_sample",
               "dmvae_column_stats_ws_bytes", "dmvae_column_stats", "dmvae_sum_f64")
YARD_SHAPES = [(37, 300, 10), (20, 130, 64), (9, 70, 130)]


def sk_gmm(mu, lv, w):
    skm = pytest.importorskip("sklearn.mixture")
    g = skm.GaussianMixture(n_components=len(mu), covariance_type="diag")
    g.weights_, g.means_, g.covariances_ = w, mu, np.exp(lv)
    g.precisions_cholesky_ = np.exp(-lv / 2)
    return g


@pytest.mark.parametrize("J,D", [(1, 1), (5, 3), (12, 33), (300, 10)])
def test_oracle_equals_sklearn_score_samples(J, D):
    rng = np.random.RandomState(J + D)
    mu, lv = rng.randn(J, D), 0.7 * rng.randn(J, D)
    w = rng.gamma(1.0, size=J) + 1e-3
    w /= w.sum()
    Z = rng.randn(40, D)
    want = sk_gmm(mu, lv, w).score_samples(Z)
    got = MO.logpdf(Z, mu, lv, np.log(w))
    assert np.abs(got - want).max() <= 1e-10
    uni = sk_gmm(mu, lv, np.full(J, 1.0 / J)).score_samples(Z)
    assert np.abs(MO.logpdf(Z, mu, lv) - uni).max() <= 1e-10     # None = uniform weights


def test_closed_forms_of_the_log_density():
    rng = np.random.RandomState(0)
    D = 6
    mu, lv, Z = rng.randn(1, D), rng.randn(1, D), rng.randn(9, D)
    plain = -0.5 * np.sum((Z - mu) ** 2 * np.exp(-lv) + lv + MO.LOG_2PI, axis=1)
    assert np.abs(MO.logpdf(Z, mu, lv) - plain).max() <= 1e-12                       # J = 1: the plain Gaussian
    mu, lv = rng.randn(7, D), rng.randn(7, D)
    one = MO.logpdf(Z, mu, lv)
    assert np.abs(MO.logpdf(Z, np.tile(mu, (3, 1)), np.tile(lv, (3, 1))) - one).max() <= 1e-12       # duplicated components change nothing
    lw = np.log(np.full(7, 1.0 / 7))
    lw2 = lw.copy()
    lw2[2] = -np.inf                                                                 # a weight of 0 is a component that is not there
    keep = np.arange(7) != 2
    assert np.abs(MO.logpdf(Z, mu, lv, lw2) - MO.logpdf(Z, mu[keep], lv[keep], lw[keep])).max() <= 1e-12
    l, b = MO.logpdf_and_bar(Z, mu, lv, np.full(7, -np.inf))
    assert np.all(np.isneginf(l)) and not b.any()


def test_closed_forms_of_the_diagnostics():
    rng = np.random.RandomState(1)
    N, D, K = 60, 4, 5
    pm, plv = rng.randn(K, D), 0.3 * rng.randn(K, D)
    eps = rng.randn(N, D)
    # identical posteriors for every row: q(z) = q(z|x), mi = 0
    mean, lv = np.tile(TL.r32(rng.randn(1, D)), (N, 1)), np.tile(rng.randn(1, D), (N, 1))      # (float32 values: their float64 mean is exact)
    z, a = MO.sample(mean, lv, eps)
    d = MO.diagnostics(mean, lv, pm, plv, z, a)
    assert abs(d["mi"]) <= 1e-12 and d["active_units"] == 0 and not d["var_of_mean"].any()
    assert abs(d["mi"] + d["marginal_kl"] - d["rate"]) <= 1e-12
    # the posteriors ARE the prior rows (N = K): q(z) = p(z), marginal_kl = 0
    z, a = MO.sample(pm, plv, eps[:K])
    d = MO.diagnostics(pm, plv, pm, plv, z, a)
    assert abs(d["marginal_kl"]) <= 1e-12 and abs(d["mi"] - d["rate"]) <= 1e-12
    # anything: the split adds up, mi <= log N; far-apart posteriors saturate at the cap
    mean, lv = rng.randn(N, D), rng.randn(N, D) - 2.0
    z, a = MO.sample(mean, lv, eps)
    d = MO.diagnostics(mean, lv, pm, plv, z, a)
    assert abs(d["mi"] + d["marginal_kl"] - d["rate"]) <= 1e-10 and d["mi"] <= d["mi_cap"] == math.log(N)
    assert d["active_units"] == D and np.allclose(d["var_of_mean"] , mean.var(axis=0)) and np.allclose(d["mean_of_var"], np.exp(lv).mean(axis=0))
    far = 100.0 * np.arange(N)[:, None] * np.ones((1, D))
    z, a = MO.sample(far, np.zeros((N, D)), eps)
    d = MO.diagnostics(far, np.zeros((N, D)), pm, plv, z, a)
    assert abs(d["mi"] - math.log(N)) <= 1e-9
    assert np.array_equal(MO.subsample_rows(203, 50), np.floor(np.arange(50) * 203 / 50).astype(np.int64))


@pytest.mark.parametrize("kind", TL.KINDS)
@pytest.mark.parametrize("shape", YARD_SHAPES)
def test_sequential_float32_stays_well_inside_the_bar_and_the_bar_is_not_vacuous(shape, kind):
    M, J, D = shape
    c = TL.case(J, D, 10, kind, seed=M + J + D + TL.KINDS.index(kind))
    rows = MO.subsample_rows(J, M)
    Z = TL.r32(c["mean"][rows] + np.exp(c["lv"][rows] / 2) * c["eps"][rows])
    ref, bar = MO.logpdf_and_bar(Z, c["mean"], c["lv"])
    err = np.abs(MO.yardstick(Z, c["mean"], c["lv"]) - ref)
    print("%s %s: max yardstick error / bar = %.3f, bar %.2e .. %.2e" % (shape, kind, (err / bar).max(), bar.min(), bar.max()))
    assert (err / bar).max() <= 0.25                             # 0.13 was seen; the kernel's blocked order should do no worse than the sequential one
    assert 1e-6 <= bar.min() and bar.max() <= 1e-2


def test_the_floor_kind_refuses_the_expanded_form():
    """posterior variances of 1e-6: z^2 s - 2 z mu s + mu^2 s loses the digits the bar holds the kernel to; the difference form keeps them"""
    worst = 0.0
    for M, J, D in YARD_SHAPES:
        c = TL.case(J, D, 10, "floor", seed=M + J + D + TL.KINDS.index("floor"))
        rows = MO.subsample_rows(J, M)
        Z = TL.r32(c["mean"][rows] + np.exp(c["lv"][rows] / 2) * c["eps"][rows])
        ref, bar = MO.logpdf_and_bar(Z, c["mean"], c["lv"])
        worst = max(worst, float((np.abs(MO.expanded(Z, c["mean"], c["lv"]) - ref) / bar).max()))
    print("expanded form on the floor kind: max error / bar = %.3g" % worst)
    assert worst > 4.0


def test_case_list_is_the_shapes_of_the_issue():
    assert MO.SHAPES[:10] == [(1, 1, 1, 1), (17, 5, 3, 5), (16, 256, 4, 4), (33, 257, 4, 4), (37, 300, 10, 10), (20, 130, 64, 64), (9, 70, 130, 130),
                              (5, 1030, 2, 2), (3, 5000, 8, 8), (700, 12, 33, 33)]
    for s in MO.SHAPES:
        assert "mild" in MO.regimes_of(s) and ("separated" in MO.regimes_of(s)) == (s[0] <= 4096)
    assert [s for s in MO.SHAPES if "floor" in MO.regimes_of(s)] == [(37, 300, 10, 10), (20, 130, 64, 64), (9, 70, 130, 130), (700, 12, 33, 33)]
    c = MO.case((17, 5, 3, 5), "separated", "given")
    assert c["Z"].shape == (17, 3) and c["mu"].shape == (5, 3) and abs(np.exp(c["log_w"]).sum() - 1.0) <= 1e-6 and (c["bar"] > 0).all()


def test_the_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "dmvae_hip.h")).read()
    binding = open(os.path.join(ROOT, "deep-mixture-vae_amd", "dmvae_hip", "_lib.py")).read()
    api = open(os.path.join(ROOT, "deep-mixture-vae_amd", "csrc", "api.hip")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header), sym
        assert re.search(r'extern "C" \w+ %s\(' % sym, api), sym
        assert '"%s"' % sym in binding, sym
    assert re.search(r"#define\s+DMVAE_ABI_VERSION\s+5\b", header)
    build = open(os.path.join(ROOT, "deep-mixture-vae_amd", "build.py")).read()
    assert '"mixture_density.hip"' in build


def test_train_py_has_the_flag_and_it_is_off_by_default():
    src = open(os.path.join(ROOT, "deep-mixture-vae_amd", "train.py")).read()
    assert re.search(r'add_argument\("--diagnostics", action="store_true", default=False', src)
    for key in ("mi_test", "marginal_kl_test", "rate_test", "mi_cap_test", "active_units_test", "miTest", "auTest"):
        assert key in src, key
