"""float64 oracle of label spreading on a symmetric kNN graph (csrc/label_spread.hip, dmvae_hip/spread.py), straight from
the definition (Zhou et al. 2004): the dense graph builders with the (d2, row) total order of knn_oracle.py, the normalisation
S = D^-1/2 W D^-1/2, the T-step iteration F <- alpha S F + (1 - alpha) Y with its change_t = max |F^(t+1) - F^t|, the closed form
F* = (1 - alpha)(I - alpha S)^-1 Y, a float32 yardstick that runs the same iteration in np.float32, and the case makers.  NumPy only: no sklearn,
no scipy.  Graphs travel as CSR (indptr int64, indices int32 ascending within a row, values), the layout the kernels take."""
import functools

import numpy as np

f64 = np.float64


# ------------------------------------------------------------------------------------------------------------------ graphs
def knn_lists(X, k):
    """(idx int64 [N][k], d2 float64 [N][k]): the k nearest other rows of every row of X by (d2, row) ascending, d2 from float64 differences.
    An exact tie goes to the lower row, as in knn_oracle.knn(X, X, k, self_first=0); written over whole arrays so that thousands of rows take
    a second."""
    X = np.asarray(X, dtype=f64)
    N = len(X)
    assert 0 <= k <= N - 1 or N == 1
    if k == 0 or N == 1:
        return np.zeros((N, 0), dtype=np.int64), np.zeros((N, 0), dtype=f64)
    idx, dd = np.empty((N, k), dtype=np.int64), np.empty((N, k), dtype=f64)
    for i0 in range(0, N, 512):
        rows = np.arange(i0, min(N, i0 + 512))
        diff = X[rows][:, None, :] - X[None, :, :]
        d2 = np.einsum("ijc,ijc->ij", diff, diff)
        d2[np.arange(len(rows)), rows] = np.inf                      # the row itself is left out
        cand = np.argpartition(d2, k - 1, axis=1)[:, :k]              # the k smallest in any order; which of several equal k-th ones: below
        dc = np.take_along_axis(d2, cand, axis=1)
        o = np.lexsort((cand, dc), axis=1)
        cand, dc = np.take_along_axis(cand, o, axis=1), np.take_along_axis(dc, o, axis=1)
        tied = (d2 == dc[:, -1:]).sum(axis=1) != (dc == dc[:, -1:]).sum(axis=1)      # equal rows across the cut: the full stable sort decides
        for i in np.flatnonzero(tied):
            cand[i] = np.argsort(d2[i], kind="stable")[:k]            # stable: ties by ascending row
            dc[i] = d2[i][cand[i]]
        idx[rows], dd[rows] = cand, dc
    return idx, dd


def dense_graph(idx, d2, weights="connectivity"):
    """W = (A + A^T) / 2 as a dense float64 [N][N]: A_ij = 1 (connectivity) or exp(-d2_ij / (2 sigma2)) (heat), sigma2 the mean over rows of the
    squared distance to the k-th neighbour, for j in the list of i; 0 elsewhere"""
    N, k = idx.shape
    A = np.zeros((N, N), dtype=f64)
    if k:
        if weights == "connectivity":
            a = np.ones_like(d2)
        elif weights == "heat":
            a = np.exp(-d2 / (2.0 * np.mean(d2[:, k - 1])))
        else:
            raise ValueError(weights)
        A[np.repeat(np.arange(N), k), idx.reshape(-1)] = a.reshape(-1)
    return 0.5 * (A + A.T)


def csr_from_dense(W):
    """(indptr int64 [N + 1], indices int32 [nnz], values float32 [nnz]) of the non-zero entries, rows and columns ascending"""
    W = np.asarray(W)
    rows, cols = np.nonzero(W)
    indptr = np.zeros(len(W) + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=len(W)), out=indptr[1:])
    return indptr, cols.astype(np.int32), W[rows, cols].astype(np.float32)


def dense_from_csr(indptr, indices, values):
    N = len(indptr) - 1
    W = np.zeros((N, N), dtype=f64)
    W[np.repeat(np.arange(N), np.diff(indptr)), indices] = values
    return W


# ------------------------------------------------------------------------------------------------------------------ the algorithm
def normalize(indptr, indices, values):
    """(s float64 [nnz], r float64 [N]): d_i = sum_j W_ij, r_i = d_i^-1/2 (0 for a row without edges), s_ij = W_ij r_i r_j"""
    v = np.asarray(values, dtype=f64)
    N = len(indptr) - 1
    rows = np.repeat(np.arange(N), np.diff(indptr))
    d = np.bincount(rows, weights=v, minlength=N) if len(v) else np.zeros(N)
    r = np.zeros(N, dtype=f64)
    r[d > 0] = d[d > 0] ** -0.5
    return v * r[rows] * r[np.asarray(indices, dtype=np.int64)], r


def one_hot(y, C, dtype=f64):
    y = np.asarray(y)
    Y = np.zeros((len(y), C), dtype=dtype)
    lab = np.flatnonzero(y >= 0)
    Y[lab, y[lab]] = 1
    return Y


def spmm(indptr, indices, s, F):
    """S F by rows, in the dtype of s and F: the products of a row are added in CSR order (np.add.reduceat)"""
    N = len(indptr) - 1
    if len(s) == 0:
        return np.zeros((N, F.shape[1]), dtype=F.dtype)
    prod = np.zeros((F.shape[1], len(s) + 1), dtype=F.dtype)          # [C][nnz + 1]: the sums run over contiguous memory; one spare column, so
    prod[:, :-1] = np.take(np.ascontiguousarray(F.T), np.asarray(indices, dtype=np.int64), axis=1) * s[None, :]      # that indptr = nnz is a valid start
    out = np.add.reduceat(prod, indptr[:-1], axis=1).T
    out[np.diff(indptr) == 0] = 0                                     # (reduceat gives an empty range the element at its start)
    return np.ascontiguousarray(out)


def iterate(indptr, indices, s, y, C, alpha, T, F0=None, dtype=f64):
    """(F^T [N][C], change [T]) from F^0 = F0 or 0, everything in `dtype` (float64: the oracle; float32: the yardstick).  y [P][N] -- P label
    vectors at once, their columns side by side in one pass over the graph: the columns of F never meet -- gives (F [P][N][C], change [P][T])."""
    y = np.asarray(y)
    if y.ndim == 2:
        P, N = y.shape
        F0 = None if F0 is None else np.concatenate(list(np.asarray(F0)), axis=1)
        F, change = _iterate(indptr, indices, s, np.concatenate([one_hot(v, C, dtype) for v in y], axis=1), alpha, T, F0, dtype, P)
        return np.stack(np.split(F, P, axis=1)), change
    F, change = _iterate(indptr, indices, s, one_hot(y, C, dtype), alpha, T, F0, dtype, 1)
    return F, change[0]


def _iterate(indptr, indices, s, Y, alpha, T, F0, dtype, P):
    s = np.asarray(s, dtype=dtype)
    al = dtype(alpha)
    base = (dtype(1) - al if dtype is f64 else dtype(1.0 - float(alpha))) * Y
    F = np.zeros_like(base) if F0 is None else np.asarray(F0, dtype=dtype)
    change = np.zeros((P, T), dtype=dtype)
    for t in range(T):
        Fn = al * spmm(indptr, indices, s, F) + base
        change[:, t] = np.max(np.abs(Fn - F).reshape(len(F), P, -1), axis=(0, 2)) if Fn.size else 0
        F = Fn
    return F, change


def iterate_f32(indptr, indices, s, y, C, alpha, T, F0=None):
    return iterate(indptr, indices, s, y, C, alpha, T, F0, dtype=np.float32)


def closed_form(indptr, indices, s, y, C, alpha):
    """F* = (1 - alpha)(I - alpha S)^-1 Y by a dense float64 solve"""
    S = dense_from_csr(indptr, indices, np.asarray(s, dtype=f64))
    return (1.0 - alpha) * np.linalg.solve(np.eye(len(S)) - alpha * S, one_hot(y, C))


def row_normalize(F):
    """every row over its sum; a row without mass stays zero (sklearn divides by 1 there)"""
    t = F.sum(axis=1, keepdims=True)
    return F / np.where(t == 0, 1.0, t)


def predict(F):
    """np.argmax per row; -1 for a row that no label reached (all zero)"""
    F = np.asarray(F)
    return np.where(np.any(F != 0, axis=1), np.argmax(F, axis=1), -1)


# ------------------------------------------------------------------------------------------------------------------ cases
def blobs(N, C, D, seed):
    """(X float32 [N][D], classes int64 [N]): unit-variance Gaussian blobs, class c = row % C, centres 3 sigma apart: centre c sits at
    (3 / sqrt 2)(1 + c // D) on axis c % D"""
    rng = np.random.RandomState(seed)
    cls = np.arange(N) % C
    centres = np.zeros((C, D))
    centres[np.arange(C), np.arange(C) % D] = (3.0 / np.sqrt(2.0)) * (1 + np.arange(C) // D)
    return (centres[cls] + rng.randn(N, D)).astype(np.float32), cls.astype(np.int64)


@functools.lru_cache(maxsize=None)
def blobs_graph(N, C, D, seed, k, weights="connectivity"):
    """(X, classes, (indptr, indices, values f32)) of the blobs' kNN graph"""
    X, cls = blobs(N, C, D, seed)
    idx, d2 = knn_lists(X, k)
    if N <= 2048:
        return X, cls, csr_from_dense(dense_graph(idx, d2, weights))
    assert weights == "connectivity"                                  # thousands of rows: the union graph without the dense matrix
    rows = np.repeat(np.arange(N), k)
    keys = np.concatenate([rows * N + idx.reshape(-1), idx.reshape(-1) * N + rows])
    uniq, counts = np.unique(keys, return_counts=True)
    indptr = np.searchsorted(uniq, np.arange(N + 1) * N).astype(np.int64)
    return X, cls, (indptr, (uniq % N).astype(np.int32), (0.5 * counts).astype(np.float32))


def star_and_ring(n):
    """CSR of the graph on n nodes in which node 0 is joined to every node of the ring 1 .. n - 1 (hub degree n - 1, every other node 3);
    weights 1 on the spokes, 0.5 on the ring"""
    W = np.zeros((n, n))
    W[0, 1:] = W[1:, 0] = 1.0
    ring = np.arange(1, n)
    nxt = np.roll(ring, -1)
    W[ring, nxt] = W[nxt, ring] = 0.5
    return csr_from_dense(W)


def islands():
    """(csr, y, C): a ring of 6 nodes with two labels (node 0: class 0, node 3: class 2), a ring of 5 nodes (6 .. 10) without any label, and
    the rows 11 and 12 without edges, row 12 labelled (class 1): it keeps (1 - alpha) of its own label and gives nothing to anybody"""
    W = np.zeros((13, 13))
    for ring in (np.arange(0, 6), np.arange(6, 11)):
        nxt = np.roll(ring, -1)
        W[ring, nxt] = W[nxt, ring] = 1.0
    W[0, 2] = W[2, 0] = 0.25
    y = np.full(13, -1, dtype=np.int32)
    y[0], y[3], y[12] = 0, 2, 1
    return csr_from_dense(W), y, 3
