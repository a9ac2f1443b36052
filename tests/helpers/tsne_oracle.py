"""float64 NumPy restatement of the exact t-SNE of include/dmvae_hip.h (dmvae_tsne_*): sklearn's method="exact" with alpha = 1 and two
output dimensions, with a perplexity search of exactly 64 bisection steps and no early stopping.  It imports nothing of the package;
tests/test_tsne_host.py holds it against sklearn's own joint probabilities and its gradient against a finite difference of its KL."""
import numpy as np

SEARCH_STEPS = 64


def sq_distances(X):
    """d2_ij = sum_d (x_id - x_jd)^2 from the differences (no norm expansion)"""
    X = np.asarray(X, dtype=np.float64)
    return ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)


def _off_diagonal(N):
    return ~np.eye(N, dtype=bool)


def _shifted(d2):
    """d'_ij = d2_ij - min_{j != i} d2_ij, the diagonal set to +inf (its exp is 0 at every beta > 0)"""
    d = np.array(d2, dtype=np.float64)
    np.fill_diagonal(d, np.inf)
    return d - d.min(1, keepdims=True)


def _row_sums(dp, beta):
    """s_i and sum_j d'_j exp(-beta_i d'_j) over j != i"""
    e = np.exp(-beta[:, None] * dp)
    with np.errstate(invalid="ignore"):
        num = np.where(np.isfinite(dp), dp * e, 0.0).sum(1)
    return e, e.sum(1), num


def entropy(d2, beta):
    """H_i = log s_i + beta_i sum_j d'_j exp(-beta_i d'_j) / s_i (nats) of every row at the given beta"""
    dp = _shifted(d2)
    beta = np.asarray(beta, dtype=np.float64)
    _, s, num = _row_sums(dp, beta)
    return np.log(s) + beta * num / s


def conditional_p(d2, perplexity, steps=SEARCH_STEPS):
    """(p_{j|i} [N][N] with a zero diagonal, beta [N]): beta from 1, exactly `steps` bisection steps, all rows at once"""
    dp = _shifted(d2)
    N = dp.shape[0]
    target = np.log(float(perplexity))
    beta, lo, hi = np.ones(N), np.zeros(N), np.full(N, np.inf)
    for _ in range(steps):
        _, s, num = _row_sums(dp, beta)
        H = np.log(s) + beta * num / s
        up = H > target
        lo = np.where(up, beta, lo)
        hi = np.where(up, hi, beta)
        beta = np.where(up, np.where(np.isinf(hi), beta * 2.0, (beta + hi) / 2.0), (beta + lo) / 2.0)
    e, s, _ = _row_sums(dp, beta)
    return e / s[:, None], beta


def joint_p(d2, perplexity):
    """P_ij = (p_{j|i} + p_{i|j}) / 2N: symmetric, zero diagonal, no floors"""
    p, _ = conditional_p(d2, perplexity)
    return (p + p.T) / (2.0 * p.shape[0])


def _q(Y):
    Y = np.asarray(Y, dtype=np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    q = 1.0 / (1.0 + (diff ** 2).sum(-1))
    np.fill_diagonal(q, 0.0)
    return diff, q


def gradient(P, Y, exaggeration=1.0):
    """g_i = 4 [ e sum_j P_ij q_ij (y_i - y_j) - (1 / Z) sum_j q_ij^2 (y_i - y_j) ]"""
    diff, q = _q(Y)
    Z = q.sum()
    attr = ((np.asarray(P, dtype=np.float64) * q)[:, :, None] * diff).sum(1)
    rep = ((q * q)[:, :, None] * diff).sum(1)
    return 4.0 * (exaggeration * attr - rep / Z)


def kl(P, Y):
    """sum over P_ij > 0 of P_ij (log P_ij - log q_ij + log Z)"""
    _, q = _q(Y)
    P = np.asarray(P, dtype=np.float64)
    m = P > 0
    return float((P[m] * (np.log(P[m]) - np.log(q[m]) + np.log(q.sum()))).sum())


def step(P, Y, U, G, exaggeration, momentum, learning_rate):
    """sklearn's _gradient_descent, one iteration; returns (Y, U, G, g), the inputs untouched"""
    g = gradient(P, Y, exaggeration)
    inc = U * g < 0.0
    G = np.maximum(np.where(inc, G + 0.2, G * 0.8), 0.01)
    U = momentum * U - learning_rate * (G * g)
    return Y + U, U, G, g


def auto_learning_rate(N, early_exaggeration=12.0):
    return max(N / early_exaggeration / 4.0, 50.0)


def fit(P, Y0, n_iter=1000, exaggeration_iters=250, early_exaggeration=12.0, learning_rate=None, dtype=np.float64):
    """all n_iter iterations from Y0 (U = 0, G = 1); returns (Y, KL).  dtype=np.float32 rounds the state after every step."""
    N = P.shape[0]
    lr = auto_learning_rate(N, early_exaggeration) if learning_rate is None else learning_rate
    Y = np.asarray(Y0, dtype=dtype)
    U, G = np.zeros_like(Y), np.ones_like(Y)
    for it in range(n_iter):
        e, m = (early_exaggeration, 0.5) if it < exaggeration_iters else (1.0, 0.8)
        Y, U, G, _ = (a.astype(dtype) for a in step(P, Y.astype(np.float64), U.astype(np.float64), G.astype(np.float64), e, m, lr))
    return Y, kl(P, Y)


def blobs(N, D, seed=1):
    """three Gaussian blobs: centres 4 * randn(3, D) plus unit noise from RandomState(seed), rows dealt i % 3 -> (X f32, labels)"""
    rs = np.random.RandomState(seed)
    centres = 4.0 * rs.randn(3, D)
    lab = np.arange(N) % 3
    return (centres[lab] + rs.randn(N, D)).astype(np.float32), lab
