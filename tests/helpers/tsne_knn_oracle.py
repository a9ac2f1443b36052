"""float64 NumPy restatement of the kNN-sparse t-SNE of include/dmvae_hip.h (dmvae_tsne_knn_*): neighbour lists ordered by (d2, j), the
conditional p over each row's k entries by the 64-step search of tsne_oracle, the joint P over the union graph as CSR sorted by
(row, column), and -- through the densified P, the shapes here are small -- tsne_oracle's gradient, KL and fit, which are exact over all
pairs.  It imports nothing of the package; tests/test_tsne_knn_host.py holds it against sklearn's _joint_probabilities_nn, against
the dense oracle at k = N - 1 and its gradient against a finite difference of its KL."""
import numpy as np

import tsne_oracle as T

SEARCH_STEPS = T.SEARCH_STEPS


def n_neighbors(N, perplexity):
    """sklearn's n_neighbors of method="barnes_hut": min(N - 1, int(3 perplexity + 1))"""
    return min(int(N) - 1, int(3.0 * float(np.float32(perplexity)) + 1.0))


def knn_lists(X, k):
    """(idx int64 [N][k], d2 f64 [N][k]): every row's k nearest other rows by (d2, j) ascending"""
    d2 = T.sq_distances(X)
    N = d2.shape[0]
    np.fill_diagonal(d2, np.inf)
    idx = np.stack([np.lexsort((np.arange(N), d2[i]))[:k] for i in range(N)])
    return idx, np.take_along_axis(d2, idx, 1)


def conditional_p(d2k, perplexity, steps=SEARCH_STEPS):
    """(p [N][k], beta [N]) over the lists' squared distances d2k [N][k], nearest first: d' = d2 - d2[:, 0], beta from 1, `steps` bisections"""
    d2k = np.asarray(d2k, dtype=np.float64)
    dp = d2k - d2k[:, :1]
    N = dp.shape[0]
    target = np.log(float(perplexity))
    beta, lo, hi = np.ones(N), np.zeros(N), np.full(N, np.inf)

    def sums(beta):
        e = np.exp(-beta[:, None] * dp)
        return e, e.sum(1), (dp * e).sum(1)

    for _ in range(steps):
        _, s, num = sums(beta)
        H = np.log(s) + beta * num / s
        up = H > target
        lo = np.where(up, beta, lo)
        hi = np.where(up, hi, beta)
        beta = np.where(up, np.where(np.isinf(hi), beta * 2.0, (beta + hi) / 2.0), (beta + lo) / 2.0)
    e, s, _ = sums(beta)
    return e / s[:, None], beta


def entropy(d2k, beta):
    """H_i (nats) of every row's k entries at the given beta"""
    d2k = np.asarray(d2k, dtype=np.float64)
    dp = d2k - d2k[:, :1]
    beta = np.asarray(beta, dtype=np.float64)
    e = np.exp(-beta[:, None] * dp)
    s = e.sum(1)
    return np.log(s) + beta * (dp * e).sum(1) / s


def joint_csr(idx, p):
    """(indptr int64 [N + 1], indices int32 [nnz], values f64 [nnz]) of P_ij = (p_{j|i} + p_{i|j}) / 2N over the UNION of the lists, an
    absent direction counting 0, sorted by (row, column); an entry of the union stays even where its p underflowed to 0"""
    idx = np.asarray(idx)
    N, k = idx.shape
    A = np.zeros((N, N))
    S = np.zeros((N, N), dtype=bool)
    rows = np.repeat(np.arange(N), k)
    A[rows, idx.reshape(-1)] = np.asarray(p, dtype=np.float64).reshape(-1)
    S[rows, idx.reshape(-1)] = True
    S |= S.T
    P = (A + A.T) / (2.0 * N)
    r, c = np.nonzero(S)                      # row-major: sorted by (row, column)
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=N), out=indptr[1:])
    return indptr, c.astype(np.int32), P[r, c]


def dense(indptr, indices, values):
    """the [N][N] f64 matrix of a CSR"""
    N = len(indptr) - 1
    out = np.zeros((N, N))
    out[np.repeat(np.arange(N), np.diff(indptr)), np.asarray(indices, dtype=np.int64)] = np.asarray(values, dtype=np.float64)
    return out


def joint_p(X, perplexity):
    """the dense [N][N] joint P of the sparse form of X, and its CSR"""
    idx, d2k = knn_lists(X, n_neighbors(len(X), perplexity))
    p, _ = conditional_p(d2k, perplexity)
    csr = joint_csr(idx, p)
    return dense(*csr), csr


def gradient(csr, Y, exaggeration=1.0):
    """attraction over the CSR entries, repulsion and Z over all pairs"""
    return T.gradient(dense(*csr), Y, exaggeration)


def kl(csr, Y):
    """sum over the entries with P_ij > 0 of P_ij log(P_ij Z / q_ij), Z over all pairs"""
    return T.kl(dense(*csr), Y)


def fit(csr, Y0, **kw):
    """tsne_oracle.fit on the densified P: (Y, KL)"""
    return T.fit(dense(*csr), Y0, **kw)
