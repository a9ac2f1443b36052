"""GPU tests of the linear probe's kernels (csrc/probe.hip: dmvae_softmax_xent, dmvae_linear_scores) and of the solver on top of them
(dmvae_hip.probe.LogisticRegression) against the float64 oracles of tests/helpers/probe_oracle.py.

Bars: a gradient array within 1e-4 max|ref|, the loss within 1e-4 max(1, |ref|), the scores within
1e-5 |ref| + 1e-5 max(1, max|ref|); an absolute part is raised to twice the error of the oracle's own f32 algebra (xent_f32) where that
is larger.  Every case prints kernel error / yardstick error per output before it asserts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import probe_oracle as PO      # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 2), (257, 3, 2), (1000, 10, 10), (513, 64, 10), (300, 65, 17), (130, 512, 32), (200, 64, 256), (5000, 16, 4)]
REGIMES = ["mild", "saturated", "optimum"]
LAMBDA = 0.05                                                     # the penalised problem of the "optimum" regime: C_reg = 1 / (LAMBDA n)
_cache = {}


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def case(shape, regime, shifted):
    """(Z, y, W, b, shift, scale, ref, f32) of one case, NumPy, computed once"""
    key = (shape, regime, shifted)
    if key in _cache:
        return _cache[key]
    n, D, Cn = shape
    rng = np.random.RandomState(1000 * D + Cn + (7 if shifted else 0))
    Z = rng.randn(n, D).astype(np.float32)
    y = rng.randint(0, Cn, n)
    sh, sc = ((0.3 * rng.randn(D)).astype(np.float32), (0.5 + rng.rand(D)).astype(np.float32)) if shifted else (None, None)
    if regime == "mild":
        W, b = 0.1 * rng.randn(D, Cn), 0.1 * rng.randn(Cn)
    elif regime == "saturated":
        x_std = float(np.sqrt((PO.features(Z, sh, sc) ** 2).mean())) or 1.0
        W, b = 25.0 / (np.sqrt(D) * x_std) * rng.randn(D, Cn), rng.randn(Cn)
        l0 = PO.scores(Z[:1], W, np.zeros(Cn), sh, sc)[0]         # row 0: logits spread over +-200, its class the smallest of them
        k = 400.0 / max(np.ptp(l0), 1e-30)
        Z[0] = (Z[0] * k if sh is None else sh + k * (Z[0] - sh)).astype(np.float32)
        y[0] = int(np.argmin(PO.scores(Z[:1], W, b, sh, sc)[0]))
    else:
        W, b = PO.optimum(Z, y, Cn, 1.0 / (LAMBDA * n), sh, sc, gtol=1e-6, maxiter=60, maxcor=10)
    W, b = W.astype(np.float32), b.astype(np.float32)            # what the kernel is given
    ref = PO.xent(Z, y, W, b, sh, sc) + (PO.scores(Z, W, b, sh, sc),)
    f32 = PO.xent_f32(Z, y, W, b, sh, sc)
    _cache[key] = (Z, y, W, b, sh, sc, ref, f32)
    return _cache[key]


def strided(a, pad):
    """a [r][c] on the device as a view of a [r][c + pad] buffer (pad = 0: contiguous)"""
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev())
    if not pad:
        return t
    big = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=dev())
    big[:, :a.shape[1]] = t
    return big[:, :a.shape[1]]


def check_outputs(tag, got, ref, f32, n_scale=1.0):
    """the bars of the module docstring; got / ref / f32 = (loss, gW, gb[, scores]); prints error over yardstick error"""
    names = ("loss", "gW", "gb", "scores")
    worst = {}
    for name, g, r, y in zip(names, got, ref, f32):
        g, r, y = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64) * n_scale, np.asarray(y, dtype=np.float64) * n_scale
        err, yard = np.abs(g - r), float(np.abs(y - r).max())
        if name == "loss":
            bar = max(1e-4 * max(1.0, abs(float(r))), 2.0 * yard)
            raised = 2.0 * yard > 1e-4 * max(1.0, abs(float(r)))
            frac = float(err) / bar
        elif name == "scores":
            absb = max(1e-5 * max(1.0, float(np.abs(r).max())), 2.0 * yard)
            raised = 2.0 * yard > 1e-5 * max(1.0, float(np.abs(r).max()))
            frac = float((err / (1e-5 * np.abs(r) + absb)).max())
        else:
            bar = max(1e-4 * float(np.abs(r).max()), 2.0 * yard)
            raised = 2.0 * yard > 1e-4 * float(np.abs(r).max())
            frac = float(err.max()) / bar if bar > 0 else (0.0 if err.max() == 0 else np.inf)
        worst[name] = (float(err.max()), yard, frac, raised)
        print("probe %-44s %-6s err %.3e  yardstick %.3e  ratio %s  of bar %.3f%s" % (
            tag, name, float(err.max()), yard, "%.2f" % (float(err.max()) / yard) if yard > 0 else "-", frac, "  (raised bar)" if raised else ""))
        assert np.all(np.isfinite(g)), (tag, name)
    for name, (e, yard, frac, raised) in worst.items():
        assert frac <= 1.0, (tag, name, e, yard, frac, raised)
    return worst


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_D%d_C%d" % s)
def test_softmax_xent_and_scores_against_the_float64_oracle(shape, regime):
    from dmvae_hip import probe
    n, D, Cn = shape
    for shifted in (False, True):
        Z, y, W, b, sh, sc, ref, f32 = case(shape, regime, shifted)
        assert np.isfinite(ref[0]) and np.isfinite(f32[0])
        if regime == "saturated":
            assert np.exp(np.float32(ref[3][0, y[0]] - ref[3][0].max())) == 0.0          # the true class's probability underflows in f32
        for zpad in (0, 3):
            for wpad in (0, 1):
                Zd, Wd = strided(Z, zpad), strided(W, wpad)
                assert (Zd.stride(0) == D + zpad or n == 1) and Wd.stride(0) == Cn + wpad
                loss, gW, gb = probe.softmax_xent(Zd, y, Wd, b, sh, sc)
                bd = torch.as_tensor(b).to(dev())
                shd, scd = (None, None) if sh is None else (torch.as_tensor(sh).to(dev()), torch.as_tensor(sc).to(dev()))
                scores = probe.scores_enqueue(Zd, Wd, bd, shd, scd).cpu().numpy()
                check_outputs("%s %s shift=%d ldz+%d ldw+%d" % (shape, regime, shifted, zpad, wpad), (loss, gW, gb, scores), ref, f32)
                if regime == "optimum":                          # a small sum of large cancelling terms: the data gradient is -LAMBDA W
                    resid = np.abs(ref[1] + LAMBDA * W.astype(np.float64)).max()             # (where the test's own short optimisation stopped)
                    assert resid <= 0.02 * np.abs(ref[1]).max() + 1e-6
                    assert np.abs(gW + LAMBDA * W.astype(np.float64)).max() <= resid + max(1e-4 * np.abs(ref[1]).max(), 2 * np.abs(f32[1] - ref[1]).max())


def raw_call(Zd, cls, Wd, bd, sh=None, sc=None, n=None, D=None, Cn=None, ldz=None, ldw=None, ws=None, ws_bytes=None, out=None, flag=None, z_null=False):
    """dmvae_softmax_xent through ctypes with any argument overridden: (rc, out tensor, flag tensor, error text)"""
    from dmvae_hip import _lib, probe
    n0, D0 = Zd.shape
    C0 = Wd.shape[1]
    if ws is None:
        ws, out_, flag_ = probe.xent_workspace(n0, D0, C0, Zd.device)
        out = out_ if out is None else out
        flag = flag_ if flag is None else flag
    out.fill_(-7.0)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    rc = _lib.lib.dmvae_softmax_xent(C.c_void_p(torch.cuda.current_stream().cuda_stream), None if z_null else ptr(Zd), Zd.stride(0) if ldz is None else ldz,
                                     n0 if n is None else n, D0 if D is None else D, ptr(sh), ptr(sc), ptr(cls), C0 if Cn is None else Cn, ptr(Wd),
                                     Wd.stride(0) if ldw is None else ldw, ptr(bd), ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, ptr(out), ptr(flag))
    torch.cuda.synchronize()
    return rc, out, flag, _lib.lib.dmvae_last_error()


def test_two_calls_return_the_same_bits():
    from dmvae_hip import probe
    for shape in ((5000, 16, 4), (513, 64, 10), (200, 64, 256)):
        Z, y, W, b, sh, sc, _, _ = case(shape, "mild", True)
        a = probe.softmax_xent(Z, y, W, b, sh, sc)
        c = probe.softmax_xent(Z, y, W, b, sh, sc)
        assert a[0] == c[0] and np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])
        Zd, Wd, bd = strided(Z, 0), strided(W, 0), torch.as_tensor(b).to(dev())
        assert torch.equal(probe.scores_enqueue(Zd, Wd, bd), probe.scores_enqueue(Zd, Wd, bd))


def test_classes_out_of_range_set_the_flag_and_add_nothing():
    from dmvae_hip import probe
    shape = (1000, 10, 10)
    Z, y, W, b, sh, sc, _, _ = case(shape, "mild", True)
    yb = y.copy()
    bad = [0, 31, 32, 500, 999]
    yb[bad] = (-1, 10, -5, 1 << 30, 10)
    keep = np.ones(len(y), bool)
    keep[bad] = False
    ref, f32 = PO.xent(Z[keep], y[keep], W, b, sh, sc), PO.xent_f32(Z[keep], y[keep], W, b, sh, sc)
    Zd, Wd, bd = strided(Z, 0), strided(W, 0), torch.as_tensor(b).to(dev())
    cls = torch.as_tensor(yb.astype(np.int32)).to(dev())
    rc, out, flag, _ = raw_call(Zd, cls, Wd, bd, torch.as_tensor(sh).to(dev()), torch.as_tensor(sc).to(dev()))
    assert rc == 0 and int(flag.item()) == 1
    host = out.cpu().numpy()
    got = (host[0], host[1:1 + 100].reshape(10, 10), host[101:])
    check_outputs("flagged rows", got, ref[:3], f32[:3], n_scale=keep.sum() / len(y))
    with pytest.raises(IndexError):
        probe.softmax_xent(Z, yb, W, b, sh, sc)
    with pytest.raises(IndexError):
        probe.LogisticRegression(n_classes=10, max_iter=2).fit(Zd, cls)


def test_bad_arguments_are_refused_by_name_and_leave_out_untouched():
    from dmvae_hip import _lib
    Z, y, W, b, _, _, _, _ = case((257, 3, 2), "mild", False)
    Zd, Wd, bd = strided(Z, 0), strided(W, 0), torch.as_tensor(b).to(dev())
    cls = torch.as_tensor(y.astype(np.int32)).to(dev())
    one = torch.ones(3, dtype=torch.float32, device=dev())
    bads = [dict(z_null=True), dict(ldz=2), dict(ldw=1), dict(ws_bytes=8), dict(n=0), dict(n=(1 << 22) + 1), dict(D=0), dict(D=513), dict(Cn=1),
            dict(Cn=257), dict(D=65, Cn=253, ldz=65, ldw=253), dict(sh=one), dict(sc=one)]
    for kw in bads:
        rc, out, flag, err = raw_call(Zd, cls, Wd, bd, **kw)
        assert rc == -1 and b"dmvae_softmax_xent" in err and b"ws_bytes" not in err.split(b":")[0], (kw, err)
        assert bool((out == -7.0).all()) and int(flag.item()) == 0, kw
    rc, out, _, _ = raw_call(Zd, cls, Wd, bd)
    assert rc == 0 and bool((out != -7.0).all())
    sco = torch.full((257, 2), -7.0, dtype=torch.float32, device=dev())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    args = dict(Z=p(Zd), ldz=3, M=257, D=3, W=p(Wd), ldw=2, b=p(bd), Cn=2, scores=p(sco), lds=2)
    for kw in (dict(Z=None), dict(W=None), dict(b=None), dict(scores=None), dict(ldz=2), dict(ldw=1), dict(lds=1), dict(M=0), dict(M=(1 << 22) + 1), dict(D=0),
               dict(D=513), dict(Cn=1), dict(Cn=257), dict(D=65, Cn=253, ldz=65, ldw=253, lds=253)):
        a = dict(args, **kw)
        rc = _lib.lib.dmvae_linear_scores(stream, a["Z"], a["ldz"], a["M"], a["D"], None, None, a["W"], a["ldw"], a["b"], a["Cn"], a["scores"], a["lds"])
        torch.cuda.synchronize()
        assert rc == -1 and b"dmvae_linear_scores" in _lib.lib.dmvae_last_error(), kw
        assert bool((sco == -7.0).all()), kw


def test_scores_stay_inside_their_columns_and_a_tie_goes_to_the_smaller_class():
    from dmvae_hip import probe
    from dmvae_hip.metrics import argmax_labels
    for shape in ((300, 65, 17), (257, 3, 2), (200, 64, 256)):
        n, D, Cn = shape
        Z, y, W, b, sh, sc, ref, _ = case(shape, "mild", False)
        Zd, Wd, bd = strided(Z, 3), strided(W, 1), torch.as_tensor(b).to(dev())
        big = torch.full((n + 1, Cn + 5), -7.0, dtype=torch.float32, device=dev())
        probe.scores_enqueue(Zd, Wd, bd, out=big[:n, :Cn])
        host = big.cpu().numpy()
        assert np.all(host[:n, Cn:] == -7.0) and np.all(host[n] == -7.0) and np.all(host[:n, :Cn] != -7.0)
        assert np.abs(host[:n, :Cn] - ref[3]).max() <= 1e-5 * max(1.0, np.abs(ref[3]).max()) * 2
    Z, y, W, b, _, _, _, _ = case((1000, 10, 10), "mild", False)
    W, b = W.copy(), b.copy()
    W[:, 7] = W[:, 2]                                            # classes 2 and 7 score the same bits on every row, above all others
    b[2] = b[7] = 50.0
    scores = probe.scores_enqueue(strided(Z, 0), strided(W, 0), torch.as_tensor(b).to(dev()))
    assert torch.equal(scores[:, 2], scores[:, 7])
    assert bool((argmax_labels(scores) == 2).all())


# ---------------------------------------------------------------------------------------------------------------- the solver
SOLVER_CASES = [(600, 8, 3, 1.5, 0.05), (1000, 10, 10, 1.5, 0.01), (500, 64, 10, 0.5, 0.01), (400, 33, 17, 0.7, 0.02)]
TOL = 1e-4


@pytest.mark.parametrize("cfg", SOLVER_CASES, ids=lambda c: "n%d_D%d_C%d" % c[:3])
def test_fit_reaches_the_float64_optimum(cfg):
    from dmvae_hip import probe
    n, D, Cn, sep, lam = cfg
    Z, y, Zt, yt = PO.blobs(n, D, Cn, sep)
    C_reg = 1.0 / (lam * n)
    clf = probe.LogisticRegression(C=C_reg, tol=TOL, max_iter=100, standardize=True).fit(Z, y)
    assert np.array_equal(clf.classes_, np.arange(Cn)) and clf.coef_.shape == (Cn, D) and clf.intercept_.shape == (Cn,)
    # 1. the float64 gradient of the full objective where the fit stopped: gtol = tol on a gradient evaluated in f32 (error about 1e-6)
    _, gW, gb = PO.objective(Z, y, clf.coef_std_.T, clf.intercept_std_, C_reg, clf.shift_, clf.scale_)
    gmax = max(np.abs(gW).max(), np.abs(gb).max())
    print("probe fit %s: |g|max = %.3e = %.2f tol, n_iter %d, n_fev %d" % (cfg, gmax, gmax / TOL, clf.n_iter_, clf.n_fev_))
    assert gmax <= 2 * TOL
    # 2. the predictions against the float64 optimum's, wherever that one has a margin
    sh, sc = PO.standardization(Z)
    assert np.allclose(sh, clf.shift_, rtol=1e-6, atol=1e-7) and np.allclose(sc, clf.scale_, rtol=1e-6, atol=0)
    Wo, bo = PO.optimum(Z, y, Cn, C_reg, sh, sc)
    lo = PO.scores(Zt, Wo, bo, sh, sc)
    top = np.sort(lo, axis=1)
    clear = top[:, -1] - top[:, -2] >= 0.1
    got = clf.decision_function(Zt).cpu().numpy()
    pred = clf.predict(Zt)
    print("probe fit %s: %.1f%% of the rows below the margin, largest logit deviation %.4f, accuracy %.4f" % (
        cfg, 100.0 * (1 - clear.mean()), np.abs((got - got.mean(1, keepdims=True)) - (lo - lo.mean(1, keepdims=True))).max(), np.mean(pred == yt)))
    assert 1 - clear.mean() <= 0.05
    assert np.array_equal(pred[clear], np.argmax(lo, axis=1)[clear])
    assert clf.score(Zt, yt) == float(np.mean(pred == yt))
    # raw-space coefficients reproduce the scores; the probabilities are a softmax of them
    raw = Zt.astype(np.float64) @ clf.coef_.T + clf.intercept_[None, :]
    assert np.abs(raw - got).max() <= 1e-4 * max(1.0, np.abs(raw).max())
    pp = clf.predict_proba(Zt)
    assert pp.shape == (300, Cn) and np.allclose(pp.sum(axis=1), 1.0, rtol=0, atol=1e-12) and np.array_equal(np.argmax(pp, axis=1), np.argmax(got, axis=1))
    # 3. the fit is a function of its inputs
    again = probe.LogisticRegression(C=C_reg, tol=TOL, max_iter=100, standardize=True).fit(torch.as_tensor(Z).to(dev()), y)
    assert np.array_equal(again.coef_, clf.coef_) and np.array_equal(again.intercept_, clf.intercept_)
    assert clf.n_iter_ <= 100 and clf.converged_ and clf.n_fev_ >= clf.n_iter_


def test_fit_options():
    from dmvae_hip import probe
    Z, y, Zt, yt = PO.blobs(600, 8, 3, 1.5)
    C_reg = 1.0 / (0.05 * 600)
    plain = probe.LogisticRegression(C=C_reg, tol=TOL).fit(Z, y)                 # without standardisation: the raw space is the fitted one
    assert plain.shift_ is None and np.array_equal(plain.coef_, plain.coef_std_)
    _, gW, gb = PO.objective(Z, y, plain.coef_std_.T, plain.intercept_std_, C_reg)
    assert max(np.abs(gW).max(), np.abs(gb).max()) <= 2 * TOL and plain.converged_
    nob = probe.LogisticRegression(C=C_reg, tol=TOL, fit_intercept=False).fit(Z, y)
    assert not nob.intercept_.any() and np.abs(PO.objective(Z, y, nob.coef_std_.T, nob.intercept_std_, C_reg)[1]).max() <= 2 * TOL
    names = np.array(["b", "a", "c"])[y]                                         # labels of any kind: classes_ are their sorted values
    lab = probe.LogisticRegression(C=C_reg, tol=TOL, standardize=True).fit(Z, names)
    assert lab.classes_.tolist() == ["a", "b", "c"] and lab.score(Zt, np.array(["b", "a", "c"])[yt]) > 0.8
    short = probe.LogisticRegression(C=1e4, tol=1e-12, max_iter=3, standardize=True).fit(Z, y)
    assert short.n_iter_ <= 3 and not short.converged_
    const = Z.copy()
    const[:, 4] = 2.5                                                            # a zero variance gives scale 1
    cz = probe.LogisticRegression(C=C_reg, tol=TOL, standardize=True).fit(const, y)
    assert cz.scale_[4] == 1.0 and np.isfinite(cz.coef_).all() and cz.converged_
