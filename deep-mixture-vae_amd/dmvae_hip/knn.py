"""Exact k-nearest neighbours on the device (dmvae_knn / dmvae_knn_vote / dmvae_knn_ranks of include/dmvae_hip.h, csrc/knn.hip): all
pairs, no N x M array stored, one distance -- d2 = sum_c (q_c - x_c)^2 in f32 differences, c ascending, fused multiply-adds -- and
one TOTAL order, (d2, row) ascending, so an exact tie goes to the lower row and two calls agree bit for bit.  On top of them
sklearn's uniform-weight brute-force KNeighborsClassifier (Euclidean) and sklearn.manifold.trustworthiness.  Nothing here imports
sklearn."""
import ctypes as C

import numpy as np
import torch

from ._lib import lib, check
from .gmm import _device_of, _rows_f32
from .metrics import argmax_labels

MAX_K = 256


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ld(t):
    """the row stride of a 2-D tensor with unit column stride, as the entries take it"""
    return max(t.stride(0), t.shape[1])


def _int32_vector(v, dev):
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(v).astype(np.int32)).reshape(-1))
    return t.to(device=dev, dtype=torch.int32).contiguous().reshape(-1)


def knn_enqueue(Q, X, k, self_first=-1):
    """dmvae_knn on the current stream for device tensors Q [M][D] and X [N][D] (f32, unit column stride): (idx int32 [M][k], d2 f32
    [M][k]) without a synchronisation.  The workspace is returned to torch's allocator, which keeps it for the stream's later work."""
    assert Q.is_cuda and X.is_cuda and Q.dtype == X.dtype == torch.float32 and Q.dim() == X.dim() == 2
    (M, D), (N, Dx), dev, k = Q.shape, X.shape, X.device, int(k)
    if D != Dx:
        raise ValueError("queries and database rows differ in width: %d != %d" % (D, Dx))
    nbytes = lib.dmvae_knn_ws_bytes(M, N, D, k)
    if nbytes < 0:
        check(int(nbytes), "dmvae_knn_ws_bytes")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev) if nbytes else None
    idx = torch.empty((M, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((M, k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dmvae_knn(_stream(dev), Q.data_ptr(), _ld(Q), M, X.data_ptr(), _ld(X), N, D, k, int(self_first), ws.data_ptr() if nbytes else None,
                            int(nbytes), idx.data_ptr(), d2.data_ptr(), k), "dmvae_knn")
    return idx, d2


def kneighbors(Q, X, k, self_first=-1):
    """(idx int32 [M][k], d2 f32 [M][k]) as device tensors: the k rows of X nearest every row of Q, nearest first, ties to the lower
    row, and their squared distances.  Device tensors (row-strided f32 views included) are used where they lie; arrays are uploaded.
    self_first >= 0 leaves row self_first + i of X out of query i's neighbours (self-kNN, also of a slice of the queries)."""
    dev = _device_of(X if isinstance(X, torch.Tensor) and X.is_cuda else Q)
    return knn_enqueue(_rows_f32(Q, dev), _rows_f32(X, dev), k, self_first)


def vote_enqueue(idx, classes, n_classes, flag=None):
    """dmvae_knn_vote: (counts f32 [M][C], flag int32 [1]) for the neighbours idx [M][k] (device int32) and the database rows' classes
    (device int32 [N]); only enqueues.  flag: a device int32 to OR the error bit into (default: a fresh zero)"""
    assert idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 2 and (idx.shape[1] == 1 or idx.stride(1) == 1)
    assert classes.is_cuda and classes.dtype == torch.int32 and classes.is_contiguous() and classes.dim() == 1
    (M, k), dev, Cn = idx.shape, idx.device, int(n_classes)
    counts = torch.empty((M, Cn), dtype=torch.float32, device=dev)
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
    assert flag.is_cuda and flag.dtype == torch.int32 and flag.numel() == 1
    with torch.cuda.device(dev):
        check(lib.dmvae_knn_vote(_stream(dev), idx.data_ptr(), _ld(idx), M, k, classes.data_ptr(), classes.numel(), Cn, counts.data_ptr(), Cn,
                                 flag.data_ptr()), "dmvae_knn_vote")
    return counts, flag


def ranks_enqueue(X, idx):
    """dmvae_knn_ranks: (ranks int32 [N][k], flag int32 [1]): the 0-based rank of row idx[i][t] among row i's neighbours in X; only enqueues"""
    assert X.is_cuda and X.dtype == torch.float32 and X.dim() == 2
    assert idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 2 and idx.shape[0] == X.shape[0] and (idx.shape[1] == 1 or idx.stride(1) == 1)
    (N, D), k, dev = X.shape, idx.shape[1], X.device
    ranks = torch.empty((N, k), dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dmvae_knn_ranks(_stream(dev), X.data_ptr(), _ld(X), N, D, idx.data_ptr(), _ld(idx), k, ranks.data_ptr(), k, flag.data_ptr()),
              "dmvae_knn_ranks")
    return ranks, flag


class KNeighborsClassifier:
    """sklearn.neighbors.KNeighborsClassifier(n_neighbors, weights="uniform", algorithm="brute", metric="euclidean") on the device:
    fit keeps the rows and their classes in HBM, predict votes among the n_neighbors nearest and takes the smallest class among the
    tied ones.  classes_ are the sorted distinct values of y; predictions are returned in y's values (NumPy)."""

    def __init__(self, n_neighbors=5):
        if not 1 <= int(n_neighbors) <= MAX_K:
            raise ValueError("n_neighbors must be in 1 .. %d" % MAX_K)
        self.n_neighbors = int(n_neighbors)

    def fit(self, X, y):
        dev = _device_of(X)
        self._X = _rows_f32(X, dev)
        y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
        if len(y) != self._X.shape[0]:
            raise ValueError("y must hold one entry per row of X: %d != %d" % (len(y), self._X.shape[0]))
        if self.n_neighbors > len(y):
            raise ValueError("n_neighbors = %d exceeds the %d fitted rows" % (self.n_neighbors, len(y)))
        self.classes_, inv = np.unique(y, return_inverse=True)
        self._y = _int32_vector(inv, dev)
        return self

    def kneighbors(self, Q, n_neighbors=None):
        """(idx int32 [M][k], d2 f32 [M][k]) device tensors: SQUARED distances, nearest first"""
        return kneighbors(Q, self._X, self.n_neighbors if n_neighbors is None else n_neighbors)

    def vote_counts(self, Q):
        """the f32 counts [M][len(classes_)] of the neighbours' classes on the device (exact small integers)"""
        idx, _ = self.kneighbors(Q)
        counts, flag = vote_enqueue(idx, self._y, len(self.classes_))
        return counts, flag

    def predict(self, Q):
        counts, flag = self.vote_counts(Q)
        labels = argmax_labels(counts).cpu().numpy()
        if int(flag.item()):
            raise IndexError("kNN vote: a neighbour or a class out of range")
        return self.classes_[labels]

    def score(self, Q, y):
        y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
        return float(np.mean(self.predict(Q) == y))


def trustworthiness_terms(X, Y, n_neighbors=5):
    """(idx, ranks, flag) on the device for sklearn.manifold.trustworthiness: the n_neighbors nearest rows of every row of the embedding
    Y (the row itself left out), and the ranks of those pairs among the rows of X"""
    dev = _device_of(X if isinstance(X, torch.Tensor) and X.is_cuda else Y)
    Xd, Yd = _rows_f32(X, dev), _rows_f32(Y, dev)
    n, k = Xd.shape[0], int(n_neighbors)
    if Yd.shape[0] != n:
        raise ValueError("X and Y must hold the same rows: %d != %d" % (n, Yd.shape[0]))
    if not (1 <= k and 2 * k < n):
        raise ValueError("n_neighbors (%d) should be less than n_samples / 2 (%g)" % (k, n / 2))
    idx, _ = knn_enqueue(Yd, Yd, k, self_first=0)
    ranks, flag = ranks_enqueue(Xd, idx)
    return idx, ranks, flag


def trustworthiness(X, Y, n_neighbors=5):
    """sklearn.manifold.trustworthiness(X, Y, n_neighbors=...) with the Euclidean metric: 1 - 2 / (n k (2n - 3k - 1)) * sum over rows i
    and their k nearest rows j in the embedding Y of max(0, rank_X(i, j) + 1 - k), rank_X the 0-based rank of j among i's neighbours
    in X.  Both all-pairs halves run on the device; the penalty is summed in integers.  ValueError unless n_neighbors < n / 2."""
    _, ranks, flag = trustworthiness_terms(X, Y, n_neighbors)
    n, k = ranks.shape
    penalty = int(torch.clamp(ranks.to(torch.int64) + (1 - k), min=0).sum().item())
    if int(flag.item()):
        raise IndexError("trustworthiness: a neighbour index out of range")
    return 1.0 - penalty * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))
