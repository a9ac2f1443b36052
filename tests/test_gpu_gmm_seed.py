"""GPU tests of the device k-means++ seeding (csrc/gmm_seed.hip behind dmvae_hip.gmm.kmeans_plusplus_device / DiagGMM(seeding="device"))
against the float64 oracle of tests/helpers/kmeanspp_oracle.py (held against the host seeding and sklearn by tests/test_gmm_seed_host.py).

The device keeps d2 in f32 and the oracle in f64, so a draw u * tot that falls within rounding of a row's boundary may land on either
neighbour.  The comparison therefore replays the oracle round by round CONDITIONED on the rows the device chose so far and allows the margin
    m = 4 (D + 2) 2^-24 tot.
Derivation: a squared distance is a sum of D products of f32 differences.  Each difference x - c is rounded once (relative 2^-24), its square
once more and each of the D - 1 additions once: to first order the f32 value is off by at most (D + 2) 2^-24 relative, every term being
non-negative (no cancellation).  The running sums themselves are f64 on both sides (2^-53 per addition: nothing at this scale), so a prefix
sum_{n<=i} d2_n of the device differs from the oracle's by at most (D + 2) 2^-24 times that prefix <= (D + 2) 2^-24 tot; the device's target
u * tot' carries the same bound once more.  Two such errors meet in every comparison of a prefix with the target; the factor 4 doubles that.
The same m bounds the error of a candidate's potential sum_n min(d2_n, dist_n) <= tot."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import gmm_oracle as G           # noqa: E402
import kmeanspp_oracle as KPP    # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 10, 10), (65000, 10, 10), (4099, 64, 10), (3001, 33, 3), (5000, 16, 50)]


def uniforms(R, K, T, seed):
    """f32 in [0, 1)"""
    u = np.random.RandomState(seed).random_sample((R, K, T)).astype(np.float32)
    return np.minimum(u, np.float32(1.0 - 2.0 ** -24))


def seed_on_device(X, K, R, local_trials, u, seed=0):
    from dmvae_hip.gmm import kmeans_plusplus_device
    c, rows, cands = kmeans_plusplus_device(X, K, n_init=R, seed=seed, local_trials=local_trials, u=u, return_trials=True)
    torch.cuda.synchronize()
    return c.cpu().numpy(), rows.cpu().numpy(), cands.cpu().numpy()


def check_every_round(X, K, R, local_trials, u, rows, cands, what):
    """every round of every restart against the oracle replayed on the device's own earlier rows; returns the number of checked draws"""
    X64 = np.asarray(X, dtype=np.float64)
    N, D = X64.shape
    T = KPP.trials(K, local_trials)
    assert rows.shape == (R, K) and cands.shape == (R, K, T)
    checked = worst = 0
    for r in range(R):
        first = KPP.uniform_row(u[r, 0, 0], N)
        assert rows[r, 0] == first and cands[r, 0, 0] == first and (cands[r, 0, 1:] == -1).all(), (what, r, rows[r, 0], first)
        d2 = KPP.dist2(X64, rows[r, 0])
        for k in range(1, K):
            cum = np.cumsum(d2)
            tot = float(cum[-1])
            m = 4 * (D + 2) * 2.0 ** -24 * tot
            for t in range(T):
                i = int(cands[r, k, t])
                assert 0 <= i < N, (what, r, k, t, i)
                if tot > 0:
                    target = np.float64(u[r, k, t]) * tot
                    lo = cum[i - 1] if i > 0 else 0.0
                    worst = max(worst, (lo - target) / tot, (target - cum[i]) / tot)
                    assert lo - m <= target <= cum[i] + m, (what, r, k, t, i, lo, target, cum[i], m)
                    assert d2[i] > 0, (what, r, k, t, i)
                else:
                    assert i == KPP.uniform_row(u[r, k, t], N), (what, r, k, t, i)
                checked += 1
            if T > 1:
                pots = KPP.potentials(X64, d2, cands[r, k])
                order = np.argsort(pots, kind="stable")
                if pots[order[1]] - pots[order[0]] > m:
                    assert rows[r, k] == cands[r, k, order[0]], (what, r, k, rows[r, k], cands[r, k], pots)
                else:
                    assert rows[r, k] in (cands[r, k, order[0]], cands[r, k, order[1]]), (what, r, k, rows[r, k], cands[r, k], pots)
            else:
                assert rows[r, k] == cands[r, k, 0]
            d2 = np.minimum(d2, KPP.dist2(X64, rows[r, k]))
    print("%s: %d draws checked, worst excursion past a boundary %.2e of tot (allowed %.2e)" % (what, checked, max(worst, 0.0), 4 * (D + 2) * 2.0 ** -24))
    return checked


@pytest.mark.parametrize("local_trials", [1, 0])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_round_follows_the_oracle(shape, R, local_trials):
    N, D, K = shape
    X, _ = G.overlapping(N, D, K, seed=N % 97)
    T = KPP.trials(K, local_trials)
    u = uniforms(R, K, T, seed=N + R + T)
    c, rows, cands = seed_on_device(X, K, R, local_trials, u)
    n = check_every_round(X, K, R, local_trials, u, rows, cands, "N=%d D=%d K=%d R=%d T=%d" % (N, D, K, R, T))
    assert n == R * (K - 1) * T                      # no round and no trial is left out
    assert np.array_equal(c, X[rows])                # every centre is the row `rows` names, bit for bit


@pytest.mark.parametrize("local_trials", [1, 0])
@pytest.mark.parametrize("shape", [(1000 + 13, 10, 6), (4099, 64, 10)])
def test_rows_with_a_leading_dimension(shape, local_trials):
    N, D, K = shape
    X, _ = G.overlapping(N, D, K, seed=9)
    wide = torch.full((N, D + 6), float("nan"), device="cuda")
    wide[:, :D] = torch.as_tensor(X).cuda()
    view = wide[:, :D]
    assert view.stride(0) == D + 6
    T = KPP.trials(K, local_trials)
    u = uniforms(3, K, T, seed=21)
    c, rows, cands = seed_on_device(view, K, 3, local_trials, u)
    assert np.isfinite(c).all()
    check_every_round(X, K, 3, local_trials, u, rows, cands, "ldx=%d N=%d T=%d" % (D + 6, N, T))
    c2, rows2, cands2 = seed_on_device(X, K, 3, local_trials, u)
    assert np.array_equal(c, c2) and np.array_equal(rows, rows2) and np.array_equal(cands, cands2)


@pytest.mark.parametrize("local_trials", [1, 0])
def test_more_than_one_row_per_thread(local_trials):
    """N > 65536: a row workgroup's threads own two rows each, the select's threads two consecutive ones"""
    N, D, K = 70001, 3, 4
    X, _ = G.overlapping(N, D, K, seed=12)
    T = KPP.trials(K, local_trials)
    u = uniforms(2, K, T, seed=5)
    c, rows, cands = seed_on_device(X, K, 2, local_trials, u)
    check_every_round(X, K, 2, local_trials, u, rows, cands, "N=%d T=%d" % (N, T))
    assert np.array_equal(c, X[rows])


@pytest.mark.parametrize("local_trials", [1, 0])
def test_separated_clusters_are_all_found(local_trials):
    """uniforms from RandomState(3): chosen on the CPU so that the ORACLE finds all six clusters (seeds 0..14 all do, with either rule)"""
    X, gen = G.separated(2000, 4, 6, seed=5)
    T = KPP.trials(6, local_trials)
    u = uniforms(1, 6, T, seed=3)
    orows, _, _ = KPP.kmeanspp(X, 6, u[0], local_trials)

    def clusters(rows):
        return sorted(((X[rows].astype(np.float64)[:, None, :] - gen[None]) ** 2).sum(-1).argmin(1))
    assert clusters(orows) == list(range(6))
    c, rows, cands = seed_on_device(X, 6, 1, local_trials, u)
    assert clusters(rows[0]) == list(range(6)), (rows, orows)
    assert np.array_equal(c[0], X[rows[0]])


@pytest.mark.parametrize("local_trials", [1, 0])
def test_restarts_in_one_call_equal_single_calls(local_trials):
    N, D, K, R = 6000, 6, 5, 5
    X, _ = G.overlapping(N, D, K, seed=5, spread=2.0)
    Xd = torch.as_tensor(X).cuda()
    T = KPP.trials(K, local_trials)
    u = uniforms(R, K, T, seed=8)
    c, rows, cands = seed_on_device(Xd, K, R, local_trials, u)
    assert len({tuple(v) for v in rows}) > 1          # the restarts differ
    for r in range(R):
        c1, rows1, cands1 = seed_on_device(Xd, K, 1, local_trials, u[r:r + 1])
        assert np.array_equal(c1[0], c[r]) and np.array_equal(rows1[0], rows[r]) and np.array_equal(cands1[0], cands[r]), r


def test_two_runs_are_bit_identical():
    X, _ = G.overlapping(65000, 10, 10, seed=1)
    Xd = torch.as_tensor(X).cuda()
    for lt in (1, 0):
        a = seed_on_device(Xd, 10, 20, lt, None, seed=4)
        b = seed_on_device(Xd, 10, 20, lt, None, seed=4)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), lt
        d = seed_on_device(Xd, 10, 20, lt, None, seed=5)
        assert not np.array_equal(a[1], d[1])


@pytest.mark.parametrize("local_trials", [1, 0])
def test_without_uniforms_the_draws_are_the_philox_stream(local_trials):
    from dmvae_hip.gmm import philox_uniform
    N, D, K, R, seed = 4099, 8, 7, 3, 1234567
    X, _ = G.overlapping(N, D, K, seed=2)
    T = KPP.trials(K, local_trials)
    u = philox_uniform(R * K * T, seed, step=0, stream_id=3).cpu().numpy()
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))
    assert len(np.unique(u)) == len(u)
    assert not np.array_equal(u, philox_uniform(R * K * T, seed, step=0, stream_id=2).cpu().numpy())
    a = seed_on_device(X, K, R, local_trials, None, seed=seed)
    b = seed_on_device(X, K, R, local_trials, u.reshape(R, K, T), seed=0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    check_every_round(X, K, R, local_trials, u.reshape(R, K, T), a[1], a[2], "philox T=%d" % T)


@pytest.mark.parametrize("local_trials", [1, 0])
def test_edge_cases(local_trials):
    # all rows equal: tot = 0 from round 1 on, every draw is min(floor(u N), N - 1) (greedy: all potentials tie at 0, trial 0 is kept)
    N, D, K = 1000, 5, 4
    X = np.tile(np.float32([1.5, -2.0, 0.25, 3.0, 7.0]), (N, 1))
    T = KPP.trials(K, local_trials)
    u = uniforms(2, K, T, seed=1)
    c, rows, cands = seed_on_device(X, K, 2, local_trials, u)
    want = np.array([[KPP.uniform_row(u[r, k, 0], N) for k in range(K)] for r in range(2)])
    assert np.array_equal(rows, want) and np.array_equal(c, X[rows])
    check_every_round(X, K, 2, local_trials, u, rows, cands, "equal rows T=%d" % T)
    # K = 1: the uniform draw alone
    X, _ = G.overlapping(777, 3, 2, seed=4)
    T = KPP.trials(1, local_trials)
    u = uniforms(3, 1, T, seed=2)
    c, rows, cands = seed_on_device(X, 1, 3, local_trials, u)
    assert np.array_equal(rows[:, 0], [KPP.uniform_row(u[r, 0, 0], 777) for r in range(3)]) and np.array_equal(c, X[rows])
    # K = N: distinct rows are all chosen, each once (a chosen row has d2 = 0 and is never drawn again)
    X, _ = G.overlapping(9, 3, 2, seed=6)
    assert len(np.unique(X, axis=0)) == 9
    T = KPP.trials(9, local_trials)
    u = uniforms(2, 9, T, seed=3)
    c, rows, cands = seed_on_device(X, 9, 2, local_trials, u)
    assert all(sorted(v) == list(range(9)) for v in rows)
    check_every_round(X, 9, 2, local_trials, u, rows, cands, "K = N T=%d" % T)
    # ragged N: one row past a workgroup's 256, and one short of two
    for N in (257, 511):
        X, _ = G.overlapping(N, 4, 3, seed=N)
        T = KPP.trials(5, local_trials)
        u = uniforms(2, 5, T, seed=N)
        u[0, 1:, 0] = np.float32(1.0 - 2.0 ** -24)           # the top of the range: the last row with d2 > 0 at the latest
        c, rows, cands = seed_on_device(X, 5, 2, local_trials, u)
        check_every_round(X, 5, 2, local_trials, u, rows, cands, "ragged N=%d T=%d" % (N, T))
        assert np.array_equal(c, X[rows])


def test_bad_arguments_raise():
    from dmvae_hip import DmvaeError
    from dmvae_hip.gmm import kmeans_plusplus_device
    X = np.random.RandomState(0).randn(50, 4).astype(np.float32)
    with pytest.raises(DmvaeError):
        kmeans_plusplus_device(X, 51)                          # K > N
    with pytest.raises(DmvaeError):
        kmeans_plusplus_device(X, 5, local_trials=9)
    with pytest.raises(ValueError):
        kmeans_plusplus_device(X, 5, n_init=2, u=np.zeros((2, 5, 3), dtype=np.float32))


def test_whole_fit_with_device_seeding_reaches_sklearns_bound():
    """DiagGMM(seeding="device"), plain and greedy, on the overlapping 65 000 x 10 set against the best of three sklearn fits, with the shortfall
    tests/test_gpu_gmm.py::test_whole_fit_reaches_sklearns_bound allows (1e-3)."""
    from sklearn.mixture import GaussianMixture
    from dmvae_hip.gmm import DiagGMM
    K = 10
    X, _ = G.overlapping(65000, 10, K, seed=1)
    kw = dict(n_init=20, max_iter=200, weights_init=np.ones(K) / K, seed=0, seeding="device")
    plain = DiagGMM(K, **kw).fit(X)
    greedy = DiagGMM(K, local_trials=0, **kw).fit(X)
    sk = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for s in range(3):
            sk.append(GaussianMixture(K, covariance_type="diag", n_init=20, max_iter=200, weights_init=np.ones(K) / K, random_state=s).fit(X).lower_bound_)
    allowed = 1e-3
    print("whole fit, device seeding: plain %.6f (restart %d, n_iter %d, %.3f s) greedy %.6f (restart %d, n_iter %d, %.3f s) sklearn %s allowed shortfall %.2e" % (
        plain.lower_bound_, plain.best_restart_, plain.n_iter_, plain.device_seconds_, greedy.lower_bound_, greedy.best_restart_, greedy.n_iter_,
        greedy.device_seconds_, ["%.6f" % v for v in sk], allowed))
    assert plain.seed_seconds_ is None and greedy.seed_seconds_ is None        # no synchronise between the seeding and the fit unless asked for
    for g in (plain, greedy):
        assert g.converged_
        assert g.lower_bound_ >= max(sk) - allowed, (g.lower_bound_, sk)
    timed = DiagGMM(K, time_parts=True, **kw).fit(X)
    assert timed.seed_seconds_ > 0 and timed.device_seconds_ > 0 and timed.lower_bound_ == plain.lower_bound_


def test_model_fits_its_prior_with_the_device_seeding(tmp_path):
    """DeepMixtureVAE(gmm="device", gmm_seeding="device").pretrain_prior: finite tables, the ones DiagGMM(seeding="device") gives by hand on the
    encoder means, and identical for two identically seeded models"""
    import base_models
    from dmvae_hip.gmm import DiagGMM
    from includes.utils import Dataset
    rng = np.random.RandomState(4)
    N = 16 * 12 + 6
    X = (rng.rand(N, 40) * (rng.rand(N, 40) < 0.4)).astype(np.float32)
    labels = rng.randint(0, 5, N)
    tables = []
    for i in range(2):
        m = base_models.DeepMixtureVAE("m", "binary", 40, 6, 5, activation="relu", initializer="xavier", batch_size=16, dtype="fp32", noise="host",
                                       seed=3, gmm="device", gmm_seeding="device", enc_layers=(70, 50), head_dim=90,
                                       dec_layers=(90, 50, 30)).build_graph()
        m.define_train_step(0.002, 1000, 0.9)
        m.path = str(tmp_path / ("ckpt_%d" % i))
        m.define_pretrain_step(0.003, 0.004)
        data = Dataset((X, labels), batch_size=16, shuffle=False)
        m.pretrain_vae(None, data, 2)
        want = DiagGMM(5, max_iter=3, n_init=20, weights_init=np.ones(5) / 5, seed=3, seeding="device").fit(m.encode_means_device(X))
        m.pretrain_prior(None, data, 3)
        p = m.engine.get_parameters()
        assert np.isfinite(p["prior_means"]).all() and np.isfinite(p["prior_log_vars"]).all() and np.abs(p["prior_means"]).max() > 0
        assert np.array_equal(p["prior_means"], want.means_.astype(np.float32))
        assert np.array_equal(p["prior_log_vars"], np.log(want.covariances_ + 1e-20).astype(np.float32))
        tables.append((p["prior_means"].copy(), p["prior_log_vars"].copy()))
    assert np.array_equal(tables[0][0], tables[1][0]) and np.array_equal(tables[0][1], tables[1][1])
