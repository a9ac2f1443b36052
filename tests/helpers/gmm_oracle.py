"""NumPy restatement of sklearn's diagonal-covariance GaussianMixture and of Lloyd's k-means (sklearn's documented algorithms),
the yardstick of the device fit (dmvae_hip.gmm).  tests/test_gmm_host.py holds it against sklearn itself; `dtype` runs the same
arithmetic in float32, whose deviation from the float64 run sets the tolerances of tests/test_gpu_gmm.py."""
import numpy as np


def logsumexp(a):
    m = a.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(axis=1, keepdims=True)))[:, 0]


def mstep(X, resp, reg=1e-6):
    nk = resp.sum(0) + 10 * np.finfo(resp.dtype).eps
    mu = resp.T @ X / nk[:, None]
    var = resp.T @ (X * X) / nk[:, None] - mu ** 2 + reg
    return nk / nk.sum(), mu, var


def estep(X, w, mu, var):
    D = X.shape[1]
    dt = X.dtype.type
    prec = dt(1) / var
    lp = (dt(-0.5) * (dt(D * np.log(2 * np.pi)) + (mu ** 2 * prec).sum(1) - dt(2) * X @ (mu * prec).T + (X ** 2) @ prec.T)
          + dt(0.5) * np.log(prec).sum(1) + np.log(w))
    n = logsumexp(lp)
    return n.mean(dtype=X.dtype), np.exp(lp - n[:, None])


def em(X, labels, K, T, tol, dtype=np.float64, reg=1e-6, weights_init="uniform", history=None):
    """fit from hard labels: (w, mu, var, lb, n_iter, converged).  weights_init: "uniform", None (the initial M-step's) or a vector.
    history: a list that receives every iteration's lower bound."""
    X = np.asarray(X).astype(dtype)
    resp = np.eye(K, dtype=dtype)[np.asarray(labels)]
    w0, mu, var = mstep(X, resp, dtype(reg))
    if weights_init is None:
        w = w0
    elif isinstance(weights_init, str):
        w = np.full(K, 1.0 / K, dtype=dtype)
    else:
        w = np.asarray(weights_init, dtype=dtype)
    lb, it, conv = -np.inf, 0, False
    for it in range(1, T + 1):
        prev = lb
        lb, resp = estep(X, w, mu, var)
        w, mu, var = mstep(X, resp.astype(dtype), dtype(reg))
        if history is not None:
            history.append(float(lb))
        if abs(lb - prev) < tol:
            conv = True
            break
    return w, mu, var, float(lb), it, conv


def init_tables(X, labels, K, reg=1e-6):
    """(mu0, var0): the M-step of the one-hot labels in float64 (what means_init / precisions_init = 1 / var0 hand to sklearn)"""
    X = np.asarray(X, dtype=np.float64)
    _, mu, var = mstep(X, np.eye(K)[np.asarray(labels)], reg)
    return mu, var


def lloyd(X, centers, max_iter=300, tol=1e-4, dtype=np.float64):
    """Lloyd's k-means as sklearn runs it (KMeans(init=centers, n_init=1, algorithm="lloyd")): (centers, labels, n_iter).
    Stops when no label changed or sum_k ||c'_k - c_k||^2 <= tol * mean_d Var(X_d); first index on distance ties."""
    X = np.asarray(X).astype(dtype)
    c = np.asarray(centers).astype(dtype)
    K = c.shape[0]
    thr = tol * X.astype(np.float64).var(axis=0).mean()
    labels = np.full(len(X), -1)
    it, strict = 0, False
    for it in range(1, max_iter + 1):
        new = ((X[:, None, :] - c[None]) ** 2).sum(-1).argmin(1)
        cn = c.copy()
        for k in range(K):
            if (new == k).any():
                cn[k] = X[new == k].mean(0)
        same = np.array_equal(new, labels)
        labels = new
        shift = ((cn - c) ** 2).sum()
        c = cn
        if same:
            strict = True
            break
        if shift <= thr:
            break
    if not strict:
        labels = ((X[:, None, :] - c[None]) ** 2).sum(-1).argmin(1)
    return c, labels, it


def overlapping(N, D, K, seed=1, spread=0.8):
    """(X f32, labels of the nearest generating centre): K overlapping diagonal Gaussians"""
    rs = np.random.RandomState(seed)
    c = rs.randn(K, D) * spread
    s = np.exp(rs.randn(K, D) * 0.4)
    k = rs.randint(0, K, N)
    X = (c[k] + s[k] * rs.randn(N, D)).astype(np.float32)
    d2 = np.stack([((X.astype(np.float64) - c[j]) ** 2).sum(1) for j in range(K)], axis=1)
    return X, d2.argmin(1).astype(np.int32)


def separated(N, D, K, seed=2):
    """(X f32, generating centres): tight clusters far apart"""
    rs = np.random.RandomState(seed)
    c = rs.randn(K, D) * 10.0
    k = rs.randint(0, K, N)
    X = (c[k] + 0.3 * rs.randn(N, D)).astype(np.float32)
    return X, c
