"""GPU tests of the device GMM fit (csrc/gmm_fit.hip behind dmvae_hip.gmm) against the float64 restatement of sklearn in
tests/helpers/gmm_oracle.py (held against sklearn itself by tests/test_gmm_host.py) and, for Lloyd and the whole fit, sklearn.

Tolerances of the comparisons with the oracle are not constants: for each case, 4 x the deviation of the SAME oracle run in float32
NumPy from the float64 run (a CPU quantity that does not involve the device), with a floor of 1e-6 x max(1, largest magnitude of the
compared quantity).  Compared: weights (abs), means (abs, in units of the data's standard deviation), covariances (relative), lower
bound (abs)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import gmm_oracle as G      # noqa: E402

pytestmark = pytest.mark.gpu


def deviations(got, ref, scale):
    """(weights abs, means abs / scale, covariances rel, bound abs) of got = (w, mu, var, lb, ...) against ref"""
    return (np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max() / scale, np.abs(got[2] / ref[2] - 1).max(), abs(got[3] - ref[3]))


def tolerances(X, labels, K, T, tol, ref, scale, **kw):
    f32 = G.em(X, labels, K, T, tol, dtype=np.float32, **kw)
    dev32 = deviations([np.asarray(v, dtype=np.float64) for v in f32[:3]] + [f32[3]], ref, scale)
    mags = (np.abs(ref[0]).max(), np.abs(ref[1]).max() / scale, 1.0, abs(ref[3]))
    return tuple(max(4 * d, 1e-6 * max(1.0, m)) for d, m in zip(dev32, mags)), dev32


def device_fit(X, labels, K, T, tol, weights_init="uniform", **kw):
    from dmvae_hip.gmm import DiagGMM
    wi = np.ones(K) / K if isinstance(weights_init, str) else weights_init
    g = DiagGMM(K, max_iter=T, tol=tol, weights_init=wi, **kw).fit(X, labels=labels)
    return g, (g.weights_, g.means_, g.covariances_, g.lower_bound_, g.n_iter_, g.converged_)


def check_against_oracle(X, labels, K, T, tol, what, **kw):
    ref = G.em(X, labels, K, T, tol, **kw)
    scale = float(np.asarray(X, dtype=np.float64).std())
    tols, dev32 = tolerances(X, labels, K, T, tol, ref, scale, **kw)
    g, got = device_fit(X, labels, K, T, tol, **kw)
    dev = deviations(got, ref, scale)
    print("%s: device dw %.2e dmu %.2e dvar(rel) %.2e dlb %.2e | f32 NumPy %s | allowed %s | n_iter %d / %d" % (
        what, dev[0], dev[1], dev[2], dev[3], " ".join("%.2e" % v for v in dev32), " ".join("%.2e" % v for v in tols), got[4], ref[4]))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all() and np.isfinite(got[3])
    for name, d, t in zip(("weights", "means", "covariances", "lower bound"), dev, tols):
        assert d <= t, (what, name, d, t)
    assert got[4] == ref[4] and got[5] == ref[5], (what, got[4:], ref[4:])
    return g, ref


@pytest.mark.parametrize("T", [1, 10])
@pytest.mark.parametrize("shape", [(1000, 10, 10), (65000, 10, 10), (4099, 64, 10), (3001, 33, 3), (5000, 16, 50)])
def test_device_em_matches_oracle(shape, T):
    N, D, K = shape
    X, labels = G.overlapping(N, D, K, seed=N % 97)
    check_against_oracle(X, labels, K, T, 0.0, "N=%d D=%d K=%d T=%d" % (N, D, K, T))


def test_initial_weights_come_from_the_labels_without_weights_init():
    X, labels = G.overlapping(3000, 7, 4, seed=8)
    check_against_oracle(X, labels, 4, 3, 0.0, "weights_init=None", weights_init=None)


@pytest.mark.parametrize("case", [(8000, 8, 6, 3, 1.5), (6000, 6, 5, 5, 2.0)])
def test_stopping_rule_follows_the_oracle(case):
    N, D, K, seed, spread = case
    tol = 1e-3
    X, labels = G.overlapping(N, D, K, seed=seed, spread=spread)
    h = []
    ref = G.em(X, labels, K, 200, tol, history=h)
    d = np.abs(np.diff(h))
    # the data set must not be borderline: every step before the stop is >= 2 tol, the stopping one <= tol / 2
    assert ref[5] and 2 <= ref[4] < 200 and d[-1] <= tol / 2 and (d[:-1] >= 2 * tol).all(), (ref[4], d)
    g, got = device_fit(X, labels, K, 200, tol)
    assert (got[4], got[5]) == (ref[4], True), (got[4:], ref[4:])
    check_against_oracle(X, labels, K, 200, tol, "stop N=%d" % N)


def test_max_iter_reached_unconverged():
    tol = 1e-3
    X, labels = G.overlapping(8000, 8, 6, seed=3, spread=1.5)
    h = []
    ref = G.em(X, labels, 6, 2, tol, history=h)
    assert not ref[5] and ref[4] == 2 and abs(h[1] - h[0]) >= 2 * tol
    g, _ = check_against_oracle(X, labels, 6, 2, tol, "max_iter reached")
    assert (g.n_iter_, g.converged_) == (2, False)


def label_sets(X, K, R, seed):
    """R label sets of different quality: the nearest of K random rows"""
    rs = np.random.RandomState(seed)
    X64 = X.astype(np.float64)
    out = []
    for _ in range(R):
        c = X64[rs.choice(len(X), K, replace=False)]
        out.append(((X64[:, None, :] - c[None]) ** 2).sum(-1).argmin(1).astype(np.int32))
    return np.stack(out)


def test_restarts_side_by_side_equal_single_runs_and_the_best_is_selected():
    from dmvae_hip.gmm import DiagGMM
    N, D, K, R, T = 6000, 6, 5, 5, 4
    X, _ = G.overlapping(N, D, K, seed=5, spread=2.0)
    L = label_sets(X, K, R, seed=0)
    kw = dict(max_iter=T, tol=0.0, weights_init=np.ones(K) / K)
    Xd = torch.as_tensor(X).cuda()
    many = DiagGMM(K, **kw).fit(Xd, labels=L)
    assert many.restarts_["lower_bound"].shape == (R,)
    for r in range(R):
        one = DiagGMM(K, **kw).fit(Xd, labels=L[r])
        assert one.lower_bound_ == many.restarts_["lower_bound"][r]
        for name, single in (("weights", one.weights_), ("means", one.means_), ("covariances", one.covariances_)):
            assert np.array_equal(single.astype(np.float32), many.restarts_[name][r]), (r, name)
    refs = [G.em(X, L[r], K, T, 0.0) for r in range(R)]
    bounds = np.array([v[3] for v in refs])
    best = int(bounds.argmax())
    scale = float(X.astype(np.float64).std())
    tols, _ = tolerances(X, L[best], K, T, 0.0, refs[best], scale)
    order = np.sort(bounds)
    assert order[-1] - order[-2] > 2 * tols[3], bounds           # the label sets must separate the best from the rest
    print("restart bounds: oracle %s device %s" % (bounds, many.restarts_["lower_bound"]))
    assert many.best_restart_ == best
    assert many.lower_bound_ == many.restarts_["lower_bound"][best]
    assert np.array_equal(many.means_.astype(np.float32), many.restarts_["means"][best])
    dev = deviations((many.weights_, many.means_, many.covariances_, many.lower_bound_), refs[best], scale)
    assert all(d <= t for d, t in zip(dev, tols)), (dev, tols)
    # identical label sets tie: the first of them is kept
    worst = int(bounds.argmin())
    tie = DiagGMM(K, **kw).fit(Xd, labels=np.stack([L[worst], L[best], L[best]]))
    assert tie.restarts_["lower_bound"][1] == tie.restarts_["lower_bound"][2] and tie.best_restart_ == 1


def test_two_runs_are_bit_identical():
    from dmvae_hip.gmm import DiagGMM
    X, labels = G.overlapping(65000, 10, 10, seed=1)
    a = DiagGMM(10, max_iter=10, tol=0.0).fit(X, labels=labels)
    b = DiagGMM(10, max_iter=10, tol=0.0).fit(X, labels=labels)
    assert a.lower_bound_ == b.lower_bound_
    assert np.array_equal(a.weights_, b.weights_) and np.array_equal(a.means_, b.means_) and np.array_equal(a.covariances_, b.covariances_)
    c = DiagGMM(10, max_iter=5, n_init=3, kmeans_iter=20, seed=4).fit(X)
    d = DiagGMM(10, max_iter=5, n_init=3, kmeans_iter=20, seed=4).fit(X)
    assert c.lower_bound_ == d.lower_bound_ and np.array_equal(c.means_, d.means_) and np.array_equal(c.restarts_["kmeans_iter"], d.restarts_["kmeans_iter"])


def test_a_label_that_never_occurs():
    N, D, K = 3001, 5, 4
    X, labels = G.overlapping(N, D, K - 1, seed=6)           # labels 0..2 only: component 3 is empty
    X = X + 3.0                                              # no row near the origin, where the empty component's mean lands
    assert labels.max() == K - 2
    g, ref = check_against_oracle(X, labels, K, 1, 0.0, "empty component")
    assert np.array_equal(g.means_[K - 1], np.zeros(D)) and np.allclose(g.covariances_[K - 1], 1e-6, rtol=1e-6, atol=0)
    assert np.abs(ref[1][K - 1]).max() == 0.0 and np.allclose(ref[2][K - 1], 1e-6)
    assert 0 < g.weights_[K - 1] < 1e-15


def test_rows_with_a_leading_dimension_and_a_ragged_tail():
    N, D, K = 1000 + 13, 10, 6
    X, labels = G.overlapping(N, D, K, seed=9)
    wide = torch.full((N, D + 6), float("nan"), device="cuda")
    wide[:, :D] = torch.as_tensor(X).cuda()
    view = wide[:, :D]
    assert view.stride(0) == D + 6
    from dmvae_hip.gmm import DiagGMM
    a = DiagGMM(K, max_iter=5, tol=0.0).fit(view, labels=labels)
    b = DiagGMM(K, max_iter=5, tol=0.0).fit(X, labels=labels)
    assert a.lower_bound_ == b.lower_bound_ and np.array_equal(a.means_, b.means_) and np.array_equal(a.covariances_, b.covariances_)
    assert np.isfinite(a.lower_bound_)
    check_against_oracle(X, labels, K, 5, 0.0, "ragged N=%d" % N, weights_init=None)


def test_tables_that_do_not_fit_raise_with_the_limit():
    from dmvae_hip import DmvaeError
    from dmvae_hip.gmm import DiagGMM
    X = np.random.RandomState(0).randn(500, 512).astype(np.float32)
    with pytest.raises(DmvaeError, match=r"K \* D <= 3328"):
        DiagGMM(10, max_iter=2).fit(X, labels=np.zeros(500, dtype=np.int32))
    with pytest.raises(DmvaeError):
        DiagGMM(4, max_iter=0).fit(X[:, :8], labels=np.zeros(500, dtype=np.int32))


@pytest.mark.parametrize("shape", [(20000, 10, 10), (5003, 33, 7)])
def test_lloyd_matches_sklearn_on_separated_data(shape):
    from sklearn.cluster import KMeans
    from dmvae_hip.gmm import kmeans, kmeans_plusplus
    N, D, K = shape
    X, _ = G.separated(N, D, K, seed=N % 89)
    c0 = kmeans_plusplus(X, K, np.random.RandomState(1)).astype(np.float32)
    km = KMeans(K, init=c0.astype(np.float64), n_init=1, algorithm="lloyd", max_iter=300, tol=1e-4).fit(X.astype(np.float64))
    d = np.sqrt(((X.astype(np.float64)[:, None, :] - km.cluster_centers_[None]) ** 2).sum(-1))
    own = d[np.arange(N), km.labels_]
    d[np.arange(N), km.labels_] = np.inf
    assert (2 * own <= d.min(1)).all()                      # well separated in sklearn's own solution
    c, labels, it = kmeans(X, c0, max_iter=300)
    scale = float(X.astype(np.float64).std())
    c32, _, _ = G.lloyd(X, c0, dtype=np.float32)
    c64, l64, it64 = G.lloyd(X, c0)
    tol = max(4 * np.abs(c32.astype(np.float64) - c64).max() / scale, 1e-6 * max(1.0, np.abs(c64).max() / scale))
    dev = np.abs(c - km.cluster_centers_).max() / scale
    print("Lloyd N=%d D=%d K=%d: device dc %.2e allowed %.2e n_iter %d / sklearn %d / oracle %d" % (N, D, K, dev, tol, it, km.n_iter_, it64))
    assert np.array_equal(labels, km.labels_)
    assert dev <= tol, (dev, tol)


def test_whole_fit_reaches_sklearns_bound():
    """k-means++ seeding, Lloyd, EM, 20 restarts on the overlapping 65 000 x 10 set against the best of three sklearn fits; both are
    stochastic searches, so the allowed shortfall is the spread of sklearn's own bounds (floor: one tol)."""
    from sklearn.mixture import GaussianMixture
    from dmvae_hip.gmm import DiagGMM
    K = 10
    X, _ = G.overlapping(65000, 10, K, seed=1)
    g = DiagGMM(K, n_init=20, max_iter=200, weights_init=np.ones(K) / K, seed=0).fit(X)
    sk = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for s in range(3):
            sk.append(GaussianMixture(K, covariance_type="diag", n_init=20, max_iter=200, weights_init=np.ones(K) / K, random_state=s).fit(X).lower_bound_)
    allowed = max(max(sk) - min(sk), 1e-3)
    print("whole fit: device %.6f (restart %d, n_iter %d, seeding %.3f s, device %.3f s) sklearn %s allowed shortfall %.2e" % (
        g.lower_bound_, g.best_restart_, g.n_iter_, g.seed_seconds_, g.device_seconds_, ["%.6f" % v for v in sk], allowed))
    assert g.converged_
    assert g.lower_bound_ >= max(sk) - allowed, (g.lower_bound_, sk)
