"""GPU tests of csrc/mixture_density.hip through dmvae_hip/density.py: dmvae_mixture_logpdf against the float64 oracle of
tests/helpers/mixture_density_oracle.py at every point under the oracle's own per-point bar

    bar_i = 2^-24 [ (D + 5 + max |lv|) sum_j w_ij (Q_ij / 2 + 1/2 sum_d |lv_jd|) + 8 (|l_i| + 1) ]

(no point excluded; a result that must be -inf is compared as -inf), dmvae_posterior_sample, dmvae_column_stats, dmvae_sum_f64 and
DiagGMM.score_samples.  Properties -- weights of 0, sentinels, a dirty workspace, reproducibility, strided views, refused arguments -- exact.
Measured max error / bar per case: DESIGN.md section 20."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import mixture_density_oracle as MO      # noqa: E402
import philox_oracle as PO               # noqa: E402
import trained_latents as TL             # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def strided(a, ld, fill=1e30):
    """the rows of a inside a wider device buffer (ld columns, `fill` between the rows): a row-strided view"""
    a = np.asarray(a, np.float32)
    buf = np.full((a.shape[0], ld), fill, dtype=np.float32)
    buf[:, :a.shape[1]] = a
    return dev(buf)[:, :a.shape[1]]


def run(Z, mu, lv, log_w=None, ld=None, **kw):
    from dmvae_hip import density
    D = np.shape(mu)[1]
    up = (lambda a: strided(a, ld)) if ld is not None and ld > D else dev
    return density.mixture_logpdf(up(Z), up(mu), up(lv), None if log_w is None else dev(log_w), **kw).cpu().numpy()


def assert_within(got, ref, bar, what):
    got = got.astype(np.float64)
    inf = np.isneginf(ref)
    assert not np.isnan(got).any(), what
    assert np.array_equal(np.isneginf(got), inf), what
    err = np.abs(got[~inf] - ref[~inf])
    ratio = float((err / bar[~inf]).max()) if err.size else 0.0
    print("%s: max |out - oracle| = %.3g, max error / bar = %.3f (bar %.2e .. %.2e)" % (what, err.max() if err.size else 0.0, ratio,
                                                                                       bar[~inf].min() if err.size else 0.0, bar[~inf].max() if err.size else 0.0))
    assert ratio <= 1.0, (what, ratio, int(np.argmax(err / bar[~inf])))


@pytest.mark.parametrize("shape,regime,weights", MO.CASES, ids=[MO.shape_id(*c) for c in MO.CASES])
def test_mixture_logpdf_against_the_oracle(shape, regime, weights):
    c = MO.case(shape, regime, weights)
    got = run(c["Z"], c["mu"], c["lv"], c["log_w"], ld=shape[3])
    assert_within(got, c["ref"], c["bar"], MO.shape_id(shape, regime, weights))


def test_the_split_is_what_the_case_list_says():
    from dmvae_hip import density
    want = {(1, 1, 1): 1, (17, 5, 3): 1, (16, 256, 4): 1, (33, 257, 4): 2, (37, 300, 10): 2, (20, 130, 64): 1, (9, 70, 130): 1, (5, 1030, 2): 5,
            (3, 5000, 8): 20, (700, 12, 33): 1, (16390, 300, 2): 1, (16368, 300, 2): 2, (5, 1 << 20, 10): 1024, (70000, 70000, 64): 1}
    for (M, J, D), n in want.items():
        assert density.mixture_split(M, J, D) == n, (M, J, D)


def test_a_far_point_at_small_variances_is_finite_and_within_the_bar():
    rng = np.random.RandomState(3)
    J, D = 300, 10
    mu = TL.r32(rng.randn(J, D))
    lv = np.full((J, D), -13.0)
    Z = TL.r32(1e4 / math.sqrt(D) * np.ones((2, D)) * np.array([[1.0], [-1.0]]))      # 1e4 away from every component
    ref, bar = MO.logpdf_and_bar(Z, mu, lv)
    got = run(Z, mu, lv)
    assert np.isfinite(got).all() and (ref < -1e13).all() and (ref > -1e14).all()
    assert_within(got, ref, bar, "far point")


def test_weights_of_zero_contribute_nothing():
    rng = np.random.RandomState(4)
    M, J, D = 21, 600, 5
    mu, lv = TL.r32(rng.randn(J, D)), TL.r32(0.5 * rng.randn(J, D))
    Z = TL.r32(mu[rng.randint(0, J, M)] + 0.05 * rng.randn(M, D))
    base = TL.r32(np.log(np.full(J, 1.0 / J)))
    nearest = np.unique(np.argmax(-((Z[:, None] - mu[None]) ** 2).sum(2), axis=1))
    for what, off in (("the nearest components", nearest), ("the whole first tile", np.arange(256)), ("every component of thread 44", np.arange(44, J, 256)),
                      ("all but one", np.arange(1, J))):
        lw = base.copy()
        lw[off] = -np.inf
        ref, bar = MO.logpdf_and_bar(Z, mu, lv, lw)
        assert np.isfinite(ref).all()
        assert_within(run(Z, mu, lv, lw), ref, bar, what)
    got = run(Z, mu, lv, np.full(J, -np.inf))
    assert np.isneginf(got).all()                                # no component left: -inf, not NaN
    lw = np.full(300, -np.inf)                                   # (21 points x 300 components: J split in two, the first part is all of weight 0)
    lw[299] = 0.0
    ref, bar = MO.logpdf_and_bar(Z, mu[:300], lv[:300], lw)
    assert_within(run(Z, mu[:300], lv[:300], lw), ref, bar, "one component in the second part")


@pytest.mark.parametrize("shape", [(37, 300, 10, 10), (700, 12, 33, 33), (3, 5000, 8, 8)])
def test_same_bits_sentinels_dirty_workspace_and_strided_views(shape):
    from dmvae_hip import density, _lib as L
    M, J, D, _ = shape
    c = MO.case(shape, "mild", "given")
    Z, mu, lv, lw = dev(c["Z"]), dev(c["mu"]), dev(c["lv"]), dev(c["log_w"])
    need = int(L.lib.dmvae_mixture_logpdf_ws_bytes(M, J, D))
    out = torch.full((M + 8,), -7.0, device="cuda")
    ws0 = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    density.mixture_logpdf(Z, mu, lv, lw, out=out[4:M + 4], ws=ws0[:need])
    first = out.cpu().numpy()
    assert (first[:4] == -7.0).all() and (first[M + 4:] == -7.0).all() and not ws0[need:].any()      # nothing behind out[M] or behind the workspace
    ws1 = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")                               # every float a NaN, every double a NaN
    again = density.mixture_logpdf(Z, mu, lv, lw, ws=ws1).cpu().numpy()
    assert again.tobytes() == first[4:M + 4].tobytes()
    assert density.mixture_logpdf(Z, mu, lv, lw).cpu().numpy().tobytes() == again.tobytes()
    views = density.mixture_logpdf(strided(c["Z"], D + 3), strided(c["mu"], D + 1), strided(c["lv"], D + 7), lw).cpu().numpy()
    assert views.tobytes() == again.tobytes()


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    from dmvae_hip import _lib as L
    M, J, D = 20, 300, 6
    rng = np.random.RandomState(0)
    Z, mu, lv = dev(rng.randn(M, D)), dev(rng.randn(J, D)), dev(rng.randn(J, D))
    need = int(L.lib.dmvae_mixture_logpdf_ws_bytes(M, J, D))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.full((M,), -5.0, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(M_=M, J_=J, D_=D, ldz=D, ldm=D, ldv=D, Zp=Z.data_ptr(), mp=mu.data_ptr(), vp=lv.data_ptr(), ws_ptr=ws.data_ptr(), nbytes=need, op=out.data_ptr()):
        return L.lib.dmvae_mixture_logpdf(stream, Zp, ldz, M_, D_, mp, ldm, vp, ldv, J_, None, ws_ptr, nbytes, op)

    for kw, text in ((dict(M_=0), "M=0"), (dict(J_=0), "J=0"), (dict(M_=(1 << 20) + 1), "M=1048577"), (dict(J_=(1 << 20) + 1), "J=1048577"),
                     (dict(D_=0, ldz=0, ldm=0, ldv=0), "D=0"), (dict(ldz=D - 1), "ldz=5"), (dict(ldm=D - 1), "ldm=5"), (dict(ldv=D - 1), "ldv=5"),
                     (dict(nbytes=need - 1), "%d bytes" % need), (dict(ws_ptr=None), "%d bytes" % need), (dict(ws_ptr=ws.data_ptr() + 4, nbytes=need + 4), "aligned"),
                     (dict(Zp=None), "must be given"), (dict(mp=None), "must be given"), (dict(vp=None), "must be given"), (dict(op=None), "must be given")):
        assert call(**kw) == -1, kw                              # DMVAE_EINVAL
        assert text.encode() in L.lib.dmvae_last_error(), (kw, L.lib.dmvae_last_error())
    assert L.lib.dmvae_mixture_logpdf_ws_bytes(0, J, D) == -1 and L.lib.dmvae_mixture_logpdf_ws_bytes(M, J, 0) == -1
    z2, a2 = torch.full((M, D), -5.0, device="cuda"), torch.full((M,), -5.0, device="cuda")
    samp = lambda n=M, D_=D, ld=D, mp=Z.data_ptr(), pos0=0: L.lib.dmvae_posterior_sample(stream, mp, ld, Z.data_ptr(), D, n, D_, None, 0, 1, 2, pos0, z2.data_ptr(), D,
                                                                                        a2.data_ptr())
    assert samp(n=0) == -1 and samp(D_=0) == -1 and samp(ld=D - 1) == -1 and samp(mp=None) == -1 and samp(pos0=-1) == -1
    st = torch.full((3, D), -5.0, dtype=torch.float64, device="cuda")
    sneed = int(L.lib.dmvae_column_stats_ws_bytes(M, D))
    sws = torch.zeros(sneed, dtype=torch.uint8, device="cuda")
    stat = lambda n=M, ld=D, nbytes=sneed, op=st.data_ptr(): L.lib.dmvae_column_stats(stream, Z.data_ptr(), ld, Z.data_ptr(), D, n, D, sws.data_ptr(), nbytes, op)
    assert stat(n=0) == -1 and stat(ld=D - 1) == -1 and stat(nbytes=sneed - 1) == -1 and stat(op=None) == -1
    assert L.lib.dmvae_sum_f64(stream, None, 4, st.data_ptr()) == -1 and L.lib.dmvae_sum_f64(stream, Z.data_ptr(), 0, st.data_ptr()) == -1
    torch.cuda.synchronize()
    assert not ws.any() and not sws.any() and (out == -5.0).all() and (z2 == -5.0).all() and (a2 == -5.0).all() and (st == -5.0).all()
    assert call() == 0                                           # and the same buffers still run
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------- posterior_sample
def sample_bars(mean, lv, eps):
    D = mean.shape[1]
    z, a = MO.sample(mean, lv, eps)
    return z, a, 2 * U * (np.abs(mean) + np.abs(np.exp(lv / 2) * eps)), (D + 4) * U * 0.5 * np.sum(eps * eps + np.abs(lv), axis=1)


@pytest.mark.parametrize("n,D", [(1, 1), (37, 10), (300, 64), (50, 130)])
def test_posterior_sample_with_the_callers_noise(n, D):
    from dmvae_hip import density
    c = TL.case(max(n, 8), max(D, 9), 4, "floor", seed=n + D)     # means at 0.5 with variances of 1e-6 among them
    mean, lv, eps = c["mean"][:n, :D], c["lv"][:n, :D], c["eps"][:n, :D]
    z, a, bz, ba = sample_bars(mean, lv, eps)
    gz, ga = density.posterior_sample(strided(mean, D + 2), strided(lv, D + 1), eps=strided(eps, D + 5))
    gz, ga = gz.cpu().numpy().astype(np.float64), ga.cpu().numpy().astype(np.float64)
    print("n %d D %d: max z error / bar %.3f, max a error / bar %.3f" % (n, D, (np.abs(gz - z) / bz).max(), (np.abs(ga - a) / ba).max()))
    assert (np.abs(gz - z) <= bz).all() and (np.abs(ga - a) <= ba).all()


def test_posterior_sample_draws_philox_stream_6():
    from dmvae_hip import density
    n, D, seed, counter, pos0 = 70, 10, 12345, 9, 1000
    rng = np.random.RandomState(5)
    mean, lv = TL.r32(rng.randn(n, D)), TL.r32(0.5 * rng.randn(n, D))
    idx = (pos0 + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(D) + np.arange(D, dtype=np.uint64)[None]
    eps = PO.normal_at(seed, counter, 6, idx)
    gz, ga = density.posterior_sample(dev(mean), dev(lv), seed=seed, counter=counter, pos0=pos0)
    got_eps = (gz.cpu().numpy().astype(np.float64) - mean) * np.exp(-lv / 2)
    assert np.abs(got_eps - eps).max() <= 1e-3                   # the bar of tests/test_gpu_philox.py: a wrong word is O(1) away
    other, _ = density.posterior_sample(dev(mean), dev(lv), seed=seed, counter=counter + 1, pos0=pos0)
    assert not torch.equal(other, gz)
    same, same_a = density.posterior_sample(dev(mean), dev(lv), seed=seed, counter=counter, pos0=pos0)
    assert torch.equal(same, gz) and torch.equal(same_a, ga)
    fed = TL.r32(eps)                                            # those normals fed back: the tight bars
    z, a, bz, ba = sample_bars(mean, lv, fed)
    fz, fa = density.posterior_sample(dev(mean), dev(lv), eps=dev(fed))
    assert (np.abs(fz.cpu().numpy() - z) <= bz).all() and (np.abs(fa.cpu().numpy() - a) <= ba).all()
    assert np.abs(fz.cpu().numpy() - gz.cpu().numpy()).max() <= 1e-3 * np.exp(lv / 2).max() + 1e-6


# ---------------------------------------------------------------------------------------------------------------- column_stats, sum
@pytest.mark.parametrize("n,D", [(1, 1), (203, 5), (5000, 33), (70001, 3)])
def test_column_stats_against_numpy_float64(n, D):
    from dmvae_hip import density
    rng = np.random.RandomState(n + D)
    mean, lv = TL.r32(rng.randn(n, D)), TL.r32(4.0 * rng.randn(n, D) - 6.0)
    mean[:, 0] = TL.r32(1000.0 + 1e-3 * rng.randn(n))            # a column at 1000 +- 1e-3 keeps its 1e-6 variance
    if D > 1:
        mean[:, 1] = np.float32(0.3)                             # an all-equal column: exactly 0
    got = density.column_stats(strided(mean, D + 3), strided(lv, D + 1)).cpu().numpy()
    cm, vm, mv = MO.column_stats(mean, lv)
    assert got.shape == (3, D) and got.dtype == np.float64
    np.testing.assert_allclose(got[0], cm, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[1], vm, rtol=1e-9, atol=0)
    if D > 1:
        assert got[1, 1] == 0.0 and got[0, 1] == np.float64(np.float32(0.3))
    if n > 1:
        assert got[1, 0] > 0
    rel = np.abs(got[2] - mv) / mv
    assert (rel <= (np.abs(lv).max() + 4) * U).all(), rel.max()
    again = density.column_stats(dev(mean), dev(lv)).cpu().numpy()
    assert again.tobytes() == got.tobytes()                      # strided views and contiguous copies, two calls: the same bits


@pytest.mark.parametrize("n", [1, 255, 257, 70000])
def test_sum_f64_is_the_float64_sum(n):
    from dmvae_hip import density
    x = (np.random.RandomState(n).randn(n) * 100).astype(np.float32)
    got = density.sum_f64(dev(x)).item()
    assert abs(got - math.fsum(x.astype(np.float64))) <= 1e-12 * np.abs(x).sum()
    assert density.sum_f64(dev(x)).item() == got


# ---------------------------------------------------------------------------------------------------------------- DiagGMM.score_samples
@pytest.mark.parametrize("N,K,D", [(500, 8, 5), (300, 70, 64)])
def test_diag_gmm_score_samples_equal_sklearn(N, K, D):
    skm = pytest.importorskip("sklearn.mixture")
    from dmvae_hip.gmm import DiagGMM
    assert (K * D > 3328) == (K == 70)                           # the second shape is past the E-step's K * D limit
    rng = np.random.RandomState(K)
    centres = 3.0 * rng.randn(K, D)
    Z = (centres[rng.randint(0, K, N)] + rng.randn(N, D)).astype(np.float32)
    g = DiagGMM(K, seed=1)
    if K * D <= 3328:
        g.fit(Z)
    else:                                                        # (the device fit stops at K * D = 3328: parameters by hand)
        g.weights_, g.means_ = rng.dirichlet(np.ones(K)), TL.r32(centres)
        g.covariances_ = TL.r32(np.exp(0.3 * rng.randn(K, D)))
    sk = skm.GaussianMixture(n_components=K, covariance_type="diag")
    sk.weights_, sk.means_, sk.covariances_ = g.weights_, g.means_, g.covariances_
    sk.precisions_cholesky_ = 1.0 / np.sqrt(g.covariances_)
    want = sk.score_samples(Z.astype(np.float64))
    lv = np.log(g.covariances_).astype(np.float32).astype(np.float64)
    lw = np.log(g.weights_).astype(np.float32).astype(np.float64)
    ref, bar = MO.logpdf_and_bar(Z.astype(np.float64), g.means_.astype(np.float32).astype(np.float64), lv, lw)
    got = g.score_samples(Z)
    assert got.dtype == np.float64 and got.shape == (N,)
    assert_within(got, ref, bar, "DiagGMM.score_samples %s" % ((N, K, D),))
    # against sklearn itself: the parameters pass through float32 on their way to the device -- |d log w| <= u |log w|, a log-variance rounded
    # by u |lv| moves a component's term by at most u |lv| (Q + 1) / 2 per dimension
    Q = np.max(-2.0 * (ref + 0.5 * D * MO.LOG_2PI))
    slack = U * (np.abs(lw).max() + np.abs(lv).max() * (max(Q, 0.0) + D) + 2 * (max(Q, 0.0) + D))
    assert np.abs(got - want).max() <= bar.max() + slack, (np.abs(got - want).max(), bar.max(), slack)
    assert abs(g.score(Z) - want.mean()) <= bar.max() + slack
