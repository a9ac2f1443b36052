"""Oracles of the linear probe (csrc/probe.hip, dmvae_hip/probe.py) in NumPy: the softmax-regression evaluation in float64, the kernel's
own algebra in float32 (the yardstick of its error, as moe_oracle.head_f32 is for the MoE head), and the float64 optimum of the
penalised objective.  W is [D][C] as the kernels take it; classes outside [0, C) add nothing and the divisor stays n."""
import numpy as np
from scipy.optimize import minimize


def features(Z, shift=None, scale=None):
    """x = (Z - shift) * scale in float64 from the values as they are (f32 inputs are exact in float64)"""
    x = np.asarray(Z, dtype=np.float64)
    if shift is not None:
        x = (x - np.asarray(shift, dtype=np.float64)[None, :]) * np.asarray(scale, dtype=np.float64)[None, :]
    return x


def scores(Z, W, b, shift=None, scale=None):
    return features(Z, shift, scale) @ np.asarray(W, dtype=np.float64) + np.asarray(b, dtype=np.float64)[None, :]


def xent(Z, y, W, b, shift=None, scale=None):
    """(loss, gW [D][C], gb [C]) in float64: the mean cross-entropy of softmax(x W + b) against y and its gradient, no penalty"""
    x, y = features(Z, shift, scale), np.asarray(y).reshape(-1).astype(np.int64)
    n, C = x.shape[0], np.asarray(W).shape[1]
    ok = (y >= 0) & (y < C)
    x, yv = x[ok], y[ok]
    l = x @ np.asarray(W, dtype=np.float64) + np.asarray(b, dtype=np.float64)[None, :]
    m = l.max(axis=1)
    e = np.exp(l - m[:, None])
    s = e.sum(axis=1)
    rows = np.arange(len(yv))
    loss = np.log(s) + m - l[rows, yv]
    r = e / s[:, None]
    r[rows, yv] -= 1.0
    return loss.sum() / n, x.T @ r / n, r.sum(axis=0) / n


def xent_f32(Z, y, W, b, shift=None, scale=None):
    """the same by the kernel's algebra: x, the logits (b first, then one fused multiply-add per column d, ascending), the maximum, the
    exponentials, their sum (classes ascending), the quotient and the row's loss all in float32; the rows are then added in float64.
    The fused multiply-add is the float64 product (exact) added in float64 and rounded to float32.  Returns (loss, gW, gb, scores f32)."""
    f = np.float32
    x = np.asarray(Z, dtype=f)
    if shift is not None:
        x = (x - np.asarray(shift, dtype=f)[None, :]) * np.asarray(scale, dtype=f)[None, :]
    y = np.asarray(y).reshape(-1).astype(np.int64)
    W32, b32 = np.asarray(W, dtype=f), np.asarray(b, dtype=f)
    n, D = x.shape
    C = W32.shape[1]
    l = np.broadcast_to(b32[None, :], (n, C)).astype(f)
    for d in range(D):
        l = (x[:, d:d + 1].astype(np.float64) * W32[d][None, :].astype(np.float64) + l.astype(np.float64)).astype(f)
    sc = l.copy()
    ok = (y >= 0) & (y < C)
    x, l, yv = x[ok], l[ok], y[ok]
    m = l.max(axis=1)
    e = np.exp(l - m[:, None]).astype(f)
    s = np.zeros(len(yv), dtype=f)
    for c in range(C):
        s = s + e[:, c]
    rows = np.arange(len(yv))
    loss = (np.log(s).astype(f) + m) - l[rows, yv]
    r = (e / s[:, None]).astype(f)
    r[rows, yv] = r[rows, yv] - f(1)
    r64 = r.astype(np.float64)
    return loss.astype(np.float64).sum() / n, x.astype(np.float64).T @ r64 / n, r64.sum(axis=0) / n, sc


def objective(Z, y, W, b, C_reg, shift=None, scale=None):
    """(f, gW, gb) of  mean_i loss_i + ||W||_F^2 / (2 C_reg n)  in float64 (the bias unpenalised)"""
    loss, gW, gb = xent(Z, y, W, b, shift, scale)
    W = np.asarray(W, dtype=np.float64)
    pen = 1.0 / (C_reg * np.asarray(Z).shape[0])
    return loss + 0.5 * pen * float((W * W).sum()), gW + pen * W, gb


def optimum(Z, y, n_classes, C_reg, shift=None, scale=None, gtol=1e-12, maxiter=5000, maxcor=30):
    """(W [D][C], b [C]) minimising the objective: scipy's L-BFGS-B in float64 from zeros"""
    x = features(Z, shift, scale)
    D, C = x.shape[1], int(n_classes)

    def fun(theta):
        f, gW, gb = objective(x, y, theta[:D * C].reshape(D, C), theta[D * C:], C_reg)
        return f, np.concatenate([gW.reshape(-1), gb])

    res = minimize(fun, np.zeros((D + 1) * C), jac=True, method="L-BFGS-B",
                   options=dict(gtol=gtol, ftol=1e-30, maxiter=maxiter, maxfun=4 * maxiter, maxcor=maxcor))
    return res.x[:D * C].reshape(D, C).copy(), res.x[D * C:].copy()


def standardization(Z):
    """(shift, scale) as float32: the column mean and 1 / std (population) in float64; a zero variance gives scale 1"""
    x = np.asarray(Z, dtype=np.float64)
    mean, var = x.mean(axis=0), x.var(axis=0)
    return mean.astype(np.float32), np.where(var > 0, 1.0 / np.sqrt(np.where(var > 0, var, 1.0)), 1.0).astype(np.float32)


def blobs(n, D, C, sep, n_test=300):
    """the solver tests' data: (Z f32, y, Zt f32, yt)"""
    r = np.random.RandomState(1)
    cen = r.randn(C, D) * sep
    y = r.randint(0, C, n)
    Z = (cen[y] + r.randn(n, D)).astype(np.float32)
    r = np.random.RandomState(2)
    yt = r.randint(0, C, n_test)
    Zt = (cen[yt] + r.randn(n_test, D)).astype(np.float32)
    return Z, y, Zt, yt
