"""GPU tests of dmvae_sinkhorn_softmin (csrc/sinkhorn.hip) and dmvae_hip.sinkhorn against the float64 oracle of
tests/helpers/sinkhorn_oracle.py.

The softmin pass is held, at EVERY row, to the oracle's own bar (sinkhorn_oracle.softmin_d2: formed from the oracle's weights, distances and
potentials; the oracle asserts that it stays below 1e-4 (|out| + eps) on every case it hands out).  The solver is held to the sum of the
pass bars of every pass it ran -- softmin is 1-Lipschitz in the sup norm with respect to its potential -- and the divergence to twice the
(a, b) problem's sum plus the two symmetric problems'.  Every test prints its measured error / bar before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import sinkhorn_oracle as SO      # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 2, 1), (17, 257, 5), (16, 256, 32), (33, 513, 64), (100, 300, 33), (300, 517, 70), (33, 700, 300)]
WIDE = [s for s in SHAPES if s[2] >= 5]
IDS = lambda s: "x".join(str(v) for v in s)


@functools.lru_cache(maxsize=None)
def case(shape):
    """(X, Y, d2 float64, scale, mean cost) of a shape: computed once, shared, left unchanged"""
    N, M, D = shape
    rng = np.random.RandomState(N + 7 * M + 13 * D)
    X, Y = rng.randn(N, D).astype(np.float32), (0.5 + 0.8 * rng.randn(M, D)).astype(np.float32)
    d2 = SO.pair_d2(X, Y)
    scale, mean_cost = SO.scale_and_mean_cost(X, Y)
    for a in (X, Y, d2):
        a.setflags(write=False)
    return X, Y, d2, scale, mean_cost


def padded(a, pad):
    """a [n][D] as a device VIEW at row stride D + pad, NaN between the rows: reading there would poison a distance"""
    a = np.array(a, dtype=np.float32)                            # (a copy: the shared cases are read-only)
    t = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device="cuda")
    t[:, :a.shape[1]] = torch.as_tensor(a).cuda()
    return t[:, :a.shape[1]]


def dev(v):
    return None if v is None else torch.as_tensor(np.array(v, dtype=np.float32)).cuda()


def device_pass(X, Y, eps, g=None, log_b=None, prev=None, pads=(3, 1)):
    """one launch on row-padded inputs into a guarded buffer, then once more into the same buffer: (out float64 [N]); the guard words
    behind out are untouched and the second call writes the same bits"""
    from dmvae_hip.sinkhorn import softmin_enqueue
    N = len(X)
    Xd, Yd, gd, ld, pd = padded(X, pads[0]), padded(Y, pads[1]), dev(g), dev(log_b), dev(prev)
    buf = torch.full((N + 2,), -3.0, dtype=torch.float32, device="cuda")
    softmin_enqueue(Xd, Yd, eps, gd, ld, pd, out=buf[:N])
    first = buf.clone()
    buf[:N] = 7.0
    softmin_enqueue(Xd, Yd, eps, gd, ld, pd, out=buf[:N])
    torch.cuda.synchronize()
    assert torch.equal(buf[N:], torch.full((2,), -3.0, device="cuda"))           # nothing behind out is written
    assert torch.equal(first.view(torch.int32), buf.view(torch.int32))           # the same buffers written twice hold the same bits
    return buf[:N].cpu().numpy().astype(np.float64)


def ratio(got, want, bar):
    assert not np.isnan(got).any()
    return float(np.max(np.abs(got - want) / bar))


@pytest.mark.parametrize("rel", [0.05, 0.005])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_softmin_pass_is_under_the_oracles_bar_at_every_row(shape, rel):
    X, Y, d2, _, mean_cost = case(shape)
    (N, M, D), rng = shape, np.random.RandomState(3)
    eps = float(np.float32(rel * mean_cost))
    g = (3.0 * eps * rng.randn(M)).astype(np.float32)
    log_b = np.log(rng.dirichlet(np.ones(M))).astype(np.float32)
    prev = (mean_cost * rng.rand(N)).astype(np.float32)
    worst = 0.0
    for gg in (None, g):
        for ll in (None, log_b):
            for pp in (None, prev):
                want, bar = SO.softmin_d2(d2, D, eps, gg, ll, pp)
                worst = max(worst, ratio(device_pass(X, Y, eps, gg, ll, pp), want, bar))
    print("softmin %s eps = %g x mean cost: max error / bar %.3f" % (shape, rel, worst))
    assert worst <= 1.0


def test_one_column_is_the_closed_form():
    X, Y, d2, _, mean_cost = case((100, 300, 33))
    eps, g, log_b = float(np.float32(0.05 * mean_cost)), np.float32([1.25]), np.float32([-0.5])
    want, bar = SO.softmin_d2(d2[:, :1], 33, eps, g, log_b)
    assert np.allclose(want, d2[:, 0] - eps * (float(log_b[0]) + float(g[0]) / eps), rtol=0, atol=1e-12 * mean_cost)
    r = ratio(device_pass(X, Y[:1], eps, g, log_b), want, bar)
    print("one column: max error / bar %.3f" % r)
    assert r <= 1.0


def test_identical_rows_with_uniform_weights_give_zero():
    row = case((17, 257, 5))[0][:1]
    X, Y, eps = np.tile(row, (37, 1)), np.tile(row, (300, 1)), 0.3
    want, bar = SO.softmin(X, Y, eps)
    got = device_pass(X, Y, eps)
    print("identical rows: max |out| / bar %.3f" % float(np.max(np.abs(got) / bar)))
    assert np.all(np.abs(want) <= 1e-15) and np.all(np.abs(got) <= bar)


def test_a_column_without_mass_changes_nothing_and_no_mass_at_all_gives_inf():
    X, Y, d2, _, mean_cost = case((33, 513, 64))
    rng = np.random.RandomState(4)
    eps = float(np.float32(0.05 * mean_cost))
    g, log_b = (3.0 * eps * rng.randn(513)).astype(np.float32), np.log(rng.dirichlet(np.ones(513))).astype(np.float32)
    drop = np.array([0, 100, 255, 256, 512])                     # in the first tile, on a tile's edges, the last column
    keep = np.setdiff1d(np.arange(513), drop)
    masked = log_b.copy()
    masked[drop] = -np.inf
    want, bar = SO.softmin_d2(d2[:, keep], 64, eps, g[keep], log_b[keep])
    with_col, without = device_pass(X, Y, eps, g, masked), device_pass(X, Y[keep], eps, g[keep], log_b[keep])
    print("-inf columns: error / bar %.3f and %.3f, between the two calls %.3f" % (ratio(with_col, want, bar), ratio(without, want, bar),
                                                                                  ratio(with_col, without, bar)))
    assert ratio(with_col, want, bar) <= 1.0 and ratio(without, want, bar) <= 1.0 and ratio(with_col, without, bar) <= 1.0      # (the tile order shifts)
    empty = device_pass(X, Y, eps, g, np.full(513, -np.inf, dtype=np.float32))
    assert np.all(np.isposinf(empty))                            # +inf, and no NaN
    assert np.all(np.isposinf(device_pass(X, Y, eps, g, np.full(513, -np.inf, dtype=np.float32), prev=np.ones(33, dtype=np.float32))))


def test_huge_potentials_stay_finite_and_under_the_bar():
    X, Y, d2, _, mean_cost = case((100, 300, 33))
    eps = float(np.float32(0.05 * mean_cost))
    g = (1e4 * eps * np.where(np.random.RandomState(5).rand(300) < 0.5, -1.0, 1.0)).astype(np.float32)      # g / eps = +-1e4 over the columns
    want, bar = SO.softmin_d2(d2, 33, eps, g)
    got = device_pass(X, Y, eps, g)
    print("g / eps = +-1e4: max error / bar %.3f" % ratio(got, want, bar))
    assert np.all(np.isfinite(got)) and ratio(got, want, bar) <= 1.0


def groups_of(shape):
    N, M, _ = shape
    return np.random.RandomState(6).randint(0, 4, N), np.arange(M) % 3


@pytest.mark.parametrize("max_iter", [1, 12])
@pytest.mark.parametrize("shape", [(17, 257, 5), (100, 300, 33), (33, 513, 64)], ids=IDS)
def test_fixed_iteration_counts_give_the_oracles_potentials(shape, max_iter):
    from dmvae_hip.sinkhorn import sinkhorn_divergence
    X, Y, _, scale, mean_cost = case(shape)
    res = sinkhorn_divergence(padded(X, 3), padded(Y, 1), eps_rel=0.05, tol=0.0, max_iter=max_iter)
    assert abs(res["scale"] - scale) <= 1e-9 * scale and abs(res["eps"] - 0.05 * mean_cost) <= 2.0 ** -23 * res["eps"]
    ref = SO.divergence(X, Y, res["eps"], res["scale"], iters=(max_iter,) * 3)
    assert res["n_iter"] == ref["n_iter"] == (len(SO.schedule(scale, res["eps"])) + max_iter,) * 3      # tol = 0: exactly max_iter at eps
    f_bar, a_bar, b_bar = ref["bars"]
    errs = [float(np.max(np.abs(d.cpu().numpy().astype(np.float64) - r))) / bar
            for d, r, bar in zip(res["potentials"], ref["potentials"], (f_bar, f_bar, a_bar, b_bar))]
    print("potentials %s after %d iterations at eps: max error / summed bars %s" % (shape, max_iter, ["%.4f" % e for e in errs]))
    assert max(errs) <= 1.0 and all(np.isfinite(e) and e >= 0 for e in res["err"])


@pytest.mark.parametrize("shape", WIDE, ids=IDS)
def test_divergence_end_to_end_is_under_the_oracles_bar(shape):
    from dmvae_hip.sinkhorn import sinkhorn_divergence
    X, Y, _, scale, mean_cost = case(shape)
    g_r, g_f = groups_of(shape)
    Xd, Yd = padded(X, 3), padded(Y, 1)
    res = sinkhorn_divergence(Xd, Yd, eps_rel=0.05, tol=0.0, max_iter=40, real_groups=g_r, fake_groups=torch.as_tensor(g_f.astype(np.int32)).cuda())
    ref = SO.divergence(X, Y, res["eps"], res["scale"], iters=(40, 40, 40), real_groups=g_r, fake_groups=g_f)
    share = res["divergence"] / res["ot"]
    print("S_eps %s: device %.9g oracle %.9g, |difference| / bar %.2e, bar / S %.2e, S / OT %.3f" % (
        shape, res["divergence"], ref["divergence"], abs(res["divergence"] - ref["divergence"]) / ref["bar"], ref["bar"] / ref["divergence"], share))
    assert abs(res["divergence"] - ref["divergence"]) <= ref["bar"]
    for name in ("ot", "ot_real", "ot_fake"):
        assert abs(res[name] - ref[name]) <= 2.0 * ref["bar"]
    assert 0.05 < share < 0.95                                   # a constant cannot pass
    # the group sums: float64 sums of the device's own per-row terms, and they add up to the divergence
    rt, ft = res["real_terms"].cpu().numpy().astype(np.float64), res["fake_terms"].cpu().numpy().astype(np.float64)
    assert res["real_terms"].dtype == res["fake_terms"].dtype == torch.float32 and res["real_terms"].is_cuda
    for got, terms, groups in ((res["per_real_group"], rt, g_r), (res["per_fake_group"], ft, g_f)):
        want = np.bincount(groups, weights=terms)
        assert np.all(np.abs(np.array(got) - want) <= 1e-12 * np.abs(want).max())
    total = sum(res["per_real_group"]) + sum(res["per_fake_group"])
    assert abs(total - res["divergence"]) <= 1e-12 * abs(res["divergence"]) and abs(rt.sum() + ft.sum() - res["divergence"]) <= 1e-12 * abs(res["divergence"])
    # a group's sum is off by at most its mass x the potentials' bars, so its sum and its mean are within the end-to-end bar as well
    for name in ("per_real_group", "per_fake_group", "mean_per_real_group", "mean_per_fake_group"):
        assert np.all(np.abs(np.array(res[name]) - ref[name]) <= ref["bar"]), name
    again = sinkhorn_divergence(Xd, Yd, eps_rel=0.05, tol=0.0, max_iter=40, real_groups=g_r, fake_groups=g_f)
    for name in ("divergence", "ot", "ot_real", "ot_fake", "eps", "scale", "n_iter", "err", "per_real_group", "per_fake_group"):
        assert res[name] == again[name], name                   # two calls: the same bits
    assert torch.equal(res["real_terms"], again["real_terms"]) and torch.equal(res["fake_terms"], again["fake_terms"])


@pytest.mark.parametrize("shape", [(257, 1003, 3), (100, 300, 33), (300, 517, 70), (33, 700, 300)], ids=IDS)
def test_the_tolerance_rule_stops_where_the_oracle_stops(shape):
    from dmvae_hip.sinkhorn import sinkhorn_divergence
    X, Y, _, scale, mean_cost = case(shape)
    res = sinkhorn_divergence(X, Y, eps_rel=0.05, tol=1e-4, check_every=5)
    ref = SO.divergence(X, Y, res["eps"], res["scale"], tol=1e-4)
    print("tol = 1e-4 %s: iterations device %s oracle %s, residuals %s" % (shape, res["n_iter"], ref["n_iter"], ["%.2e" % e for e in res["err"]]))
    assert max(res["err"]) <= 1e-4
    assert all(abs(a - b) <= 5 for a, b in zip(res["n_iter"], ref["n_iter"]))
    assert max(res["n_iter"]) <= 60 and max(ref["n_iter"]) <= 60


def test_a_set_against_itself_gives_zero_within_the_bar():
    from dmvae_hip.sinkhorn import sinkhorn_divergence
    X, _, _, _, _ = case((100, 300, 33))
    res = sinkhorn_divergence(X, X.copy(), eps_rel=0.05, tol=0.0, max_iter=40)
    ref = SO.divergence(X, X, res["eps"], res["scale"], iters=(40, 40, 40))
    print("F = R: S device %.3e oracle %.3e bar %.3e" % (res["divergence"], ref["divergence"], ref["bar"]))
    assert abs(res["divergence"]) <= ref["bar"] and abs(ref["divergence"]) <= ref["bar"]
    assert res["ot"] > 100 * ref["bar"]                          # OT_eps itself is far from 0: the debiasing is what is tested


def test_weights_and_rows_without_mass():
    from dmvae_hip.sinkhorn import sinkhorn_divergence
    X, Y, _, _, mean_cost = case((100, 300, 33))
    rng = np.random.RandomState(8)
    la, lb = np.log(rng.dirichlet(np.ones(100))).astype(np.float32), np.log(rng.dirichlet(np.ones(300))).astype(np.float32)
    eps = 0.05 * mean_cost
    res = sinkhorn_divergence(X, Y, eps=eps, tol=0.0, max_iter=20, log_a=la, log_b=lb)
    ref = SO.divergence(X, Y, res["eps"], res["scale"], iters=(20, 20, 20), log_a=la, log_b=lb)
    print("weighted: |difference| / bar %.2e" % (abs(res["divergence"] - ref["divergence"]) / ref["bar"]))
    assert res["eps"] == float(np.float32(eps)) and abs(res["divergence"] - ref["divergence"]) <= ref["bar"]
    # a row of weight -inf carries nothing: a zero term, no NaN anywhere, and the oracle's value for the same weights
    X2, la2 = np.concatenate([X, 1.0 + X[:1]]), np.concatenate([la, np.float32([-np.inf])])
    more = sinkhorn_divergence(X2, Y, eps=eps, tol=0.0, max_iter=20, log_a=la2, log_b=lb)
    ref2 = SO.divergence(X2, Y, more["eps"], more["scale"], iters=(20, 20, 20), log_a=la2, log_b=lb)
    assert abs(more["divergence"] - ref2["divergence"]) <= ref2["bar"] and float(more["real_terms"][-1]) == 0.0 and ref2["real_terms"][-1] == 0.0
    assert not any(np.isnan(v) for v in (more["divergence"], more["ot"], more["ot_real"], more["ot_fake"]))
    assert not any(bool(torch.isnan(t).any()) for t in more["potentials"])
