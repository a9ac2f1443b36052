"""float64 oracle of the k-nearest-neighbour entries (csrc/knn.hip), straight from the definition: all-pairs squared distances in
float64, the total order (d2, row) by np.lexsort, ranks by counting, trustworthiness from sklearn's formula.  No sklearn."""
import numpy as np


def pair_d2(Q, X):
    """d2[i][j] = sum_c (q_ic - x_jc)^2 in float64, from the differences (no norm expansion)"""
    Q, X = np.asarray(Q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    out = np.empty((len(Q), len(X)), dtype=np.float64)
    for i in range(len(Q)):
        d = X - Q[i]
        out[i] = np.einsum("jc,jc->j", d, d)
    return out


def order_rows(d2, self_first=-1):
    """per query: the database rows by (d2, row) ascending, the excluded row self_first + i left out"""
    out = []
    for i in range(len(d2)):
        o = np.lexsort((np.arange(d2.shape[1]), d2[i]))
        if self_first >= 0:
            o = o[o != self_first + i]
        out.append(o)
    return out


def knn(Q, X, k, self_first=-1):
    """(idx int64 [M][k], d2 float64 [M][k], the full d2 matrix)"""
    d2 = pair_d2(Q, X)
    idx = np.stack([o[:k] for o in order_rows(d2, self_first)])
    return idx, np.take_along_axis(d2, idx, axis=1), d2


def ranks(X, idx):
    """ranks[i][t] = #{l != i: (d2(i, l), l) < (d2(i, j), j)}, j = idx[i][t], by counting"""
    d2 = pair_d2(X, X)
    n = len(d2)
    rows = np.arange(n)
    out = np.empty(idx.shape, dtype=np.int64)
    for i in range(n):
        other = rows != i
        for t, j in enumerate(idx[i]):
            below = (d2[i] < d2[i, j]) | ((d2[i] == d2[i, j]) & (rows < j))
            out[i, t] = np.count_nonzero(below & other)
    return out


def trustworthiness_from_ranks(rk, n, k):
    """T = 1 - 2 / (n k (2n - 3k - 1)) * sum max(0, rank + 1 - k), the sum in integers"""
    penalty = int(np.maximum(np.asarray(rk, dtype=np.int64) + 1 - k, 0).sum())
    return 1.0 - penalty * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def trustworthiness(X, Y, k):
    n = len(X)
    if not 2 * k < n:
        raise ValueError("n_neighbors (%d) should be less than n_samples / 2 (%g)" % (k, n / 2))
    idx, _, _ = knn(Y, Y, k, self_first=0)
    return trustworthiness_from_ranks(ranks(X, idx), n, k)


def vote(idx, classes, C):
    """(counts int64 [M][C], the uniform-weight prediction: the smallest class among the most frequent)"""
    counts = np.stack([np.bincount(np.asarray(classes)[row], minlength=C) for row in idx])
    return counts, np.argmax(counts, axis=1)


def u_bar(D):
    """the relative bar of a returned d2: D f32 fused multiply-adds of squared f32 differences -- each difference carries 2^-24, its
    square 2 * 2^-24, the running sum at most D * 2^-24 more -- rounded up to (D + 3) 2^-24"""
    return (D + 3) * 2.0 ** -24
