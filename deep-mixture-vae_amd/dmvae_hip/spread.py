"""Label spreading on the device (dmvae_graph_sym_normalize / dmvae_label_spread of include/dmvae_hip.h, csrc/label_spread.hip): Zhou et al.
2004, "Learning with local and global consistency" -- the few labels y (-1: none) flow along the symmetric nearest-neighbour graph that ALL
rows define,
  W = (A + A^T) / 2,  A_ij = 1 (or exp(-d2_ij / 2 sigma^2)) for j among the k nearest rows of i (dmvae_hip.knn, the row itself left out),
  S = D^-1/2 W D^-1/2,      F <- alpha S F + (1 - alpha) Y      until max |F' - F| < tol,
and a row takes the class of its largest F.  With sklearn.semi_supervised.LabelSpreading(kernel=<a callable returning W>, alpha=alpha) this is
sklearn's algorithm (its own kernel="knn" builds a different, asymmetric graph).  Every iteration is one launch; the host reads the changes of a
chunk of iterations in one copy, as dmvae_hip.sinkhorn reads its residual.  Nothing here imports sklearn."""
import ctypes as C

import numpy as np
import torch

from ._lib import lib, check
from .gmm import _device_of, _rows_f32
from .knn import MAX_K, _int32_vector, _stream, knn_enqueue
from .metrics import argmax_labels

ERR_INDEX, ERR_LABEL = 1, 2          # SPREAD_ERR_* of csrc/label_spread.h
MAX_C = 1024
WEIGHTS = ("connectivity", "heat")


def _csr(indptr, indices, values):
    assert indptr.is_cuda and indptr.dtype == torch.int64 and indptr.is_contiguous() and indptr.dim() == 1 and indptr.numel() >= 2
    assert indices.is_cuda and indices.dtype == torch.int32 and indices.is_contiguous() and indices.dim() == 1
    assert values.is_cuda and values.dtype == torch.float32 and values.is_contiguous() and values.numel() == indices.numel()
    return indptr.numel() - 1, indices.numel()


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def sym_normalize_enqueue(indptr, indices, values, flag=None):
    """dmvae_graph_sym_normalize on the current stream for the CSR (indptr int64 [N + 1], indices int32, values f32) of a symmetric matrix on the
    device: (s f32 [nnz], r f32 [N], flag int32 [1]) without a synchronisation.  flag: a device int32 to OR the error bits into"""
    N, nnz = _csr(indptr, indices, values)
    dev = indptr.device
    s, r = torch.empty(nnz, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev)
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dmvae_graph_sym_normalize(_stream(dev), indptr.data_ptr(), _ptr(indices), _ptr(values), N, nnz, _ptr(s), r.data_ptr(), flag.data_ptr()),
              "dmvae_graph_sym_normalize")
    return s, r, flag


def sym_normalize(indptr, indices, values):
    """(s, r): S_ij = W_ij r_i r_j in the layout of `values`, r_i = (sum_j W_ij)^-1/2 (0 for a row without edges).  IndexError on a column
    index outside [0, N) (one small read)."""
    s, r, flag = sym_normalize_enqueue(indptr, indices, values)
    if int(flag.item()) & ERR_INDEX:
        raise IndexError("sym_normalize: a column index outside [0, %d)" % (indptr.numel() - 1))
    return s, r


def workspace(N, n_classes, dev):
    nbytes = lib.dmvae_label_spread_ws_bytes(int(N), int(n_classes))
    if nbytes < 0:
        check(int(nbytes), "dmvae_label_spread_ws_bytes")
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


def spread_enqueue(indptr, indices, s, labels, n_classes, alpha, n_iter, F, change, ws, flag, F_in=None):
    """n_iter iterations of dmvae_label_spread on the current stream from F_in (None: zeros; F itself: continue in place) into F [N][>= C] f32,
    their changes into change [>= n_iter] f32; only enqueues"""
    N, nnz = _csr(indptr, indices, s)
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == N
    assert F.is_cuda and F.dtype == torch.float32 and F.dim() == 2 and F.shape[0] == N and F.shape[1] >= n_classes and F.stride(1) == 1
    assert change.is_cuda and change.dtype == torch.float32 and change.is_contiguous() and change.numel() >= n_iter
    assert F_in is None or (F_in.is_cuda and F_in.dtype == torch.float32 and F_in.shape == F.shape and F_in.stride(1) == 1)
    dev = indptr.device
    with torch.cuda.device(dev):
        check(lib.dmvae_label_spread(_stream(dev), indptr.data_ptr(), _ptr(indices), _ptr(s), N, nnz, labels.data_ptr(), int(n_classes), float(alpha),
                                     int(n_iter), None if F_in is None else F_in.data_ptr(), 0 if F_in is None else F_in.stride(0), F.data_ptr(),
                                     F.stride(0), change.data_ptr(), ws.data_ptr(), ws.numel(), flag.data_ptr()), "dmvae_label_spread")


def spread(indptr, indices, s, labels, n_classes, alpha=0.8, max_iter=1000, tol=1e-6, check_every=8):
    """(F [N][n_classes] f32 on the device, n_iter, change): F <- alpha S F + (1 - alpha) Y from F = 0 for the normalised CSR graph (indptr,
    indices, s) and the labels (int [N], -1: none).  The host enqueues check_every iterations, reads that chunk of changes in one copy and
    stops at the first chunk whose LAST change is < tol, or at max_iter: n_iter is the number of iterations run, change the last one's
    max |F' - F|.  ValueError on a label outside {-1} u [0, n_classes), IndexError on a column index outside [0, N)."""
    n_classes, max_iter, check_every = int(n_classes), int(max_iter), int(check_every)
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError("alpha = %r: 0 < alpha < 1" % (alpha,))
    if not 2 <= n_classes <= MAX_C:
        raise ValueError("n_classes = %d: 2 .. %d" % (n_classes, MAX_C))
    if max_iter < 1 or check_every < 1 or not tol >= 0:
        raise ValueError("max_iter = %r, check_every = %r, tol = %r: max_iter >= 1, check_every >= 1, tol >= 0" % (max_iter, check_every, tol))
    N, _ = _csr(indptr, indices, s)
    dev = indptr.device
    labels = _int32_vector(labels, dev)
    if labels.numel() != N:
        raise ValueError("labels must hold one entry per row: %d != %d" % (labels.numel(), N))
    F = torch.empty((N, n_classes), dtype=torch.float32, device=dev)
    change = torch.empty(check_every, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = workspace(N, n_classes, dev)
    done, last = 0, float("inf")
    while done < max_iter:
        n = min(check_every, max_iter - done)
        spread_enqueue(indptr, indices, s, labels, n_classes, alpha, n, F, change, ws, flag, F_in=F if done else None)
        done += n
        last = float(change[:n].cpu()[n - 1])                        # the chunk's one read
        if last < tol:
            break
    bits = int(flag.item())
    if bits & ERR_LABEL:
        raise ValueError("spread: a label outside {-1} u [0, %d)" % n_classes)
    if bits & ERR_INDEX:
        raise IndexError("spread: a column index outside [0, %d)" % N)
    return F, done, last


def knn_graph(X, n_neighbors, weights="connectivity"):
    """(indptr, indices, values) on the device: W = (A + A^T) / 2 over the union of the lists of the n_neighbors nearest other rows of every
    row of X (dmvae_knn; tsne.knn_symmetrize, whose constant factor 1 / 2N the normalisation removes).  A = 1 ("connectivity") or
    exp(-d2 / 2 sigma^2) ("heat"), sigma^2 the mean over rows of the squared distance to the n_neighbors-th neighbour (float64 on the
    device, rounded to f32 once).  Reads one integer (nnz) back."""
    from .tsne import knn_symmetrize
    if weights not in WEIGHTS:
        raise ValueError("weights = %r: one of %s" % (weights, ", ".join(WEIGHTS)))
    N, k = X.shape[0], int(n_neighbors)
    if not 1 <= k <= min(MAX_K, N - 1):
        raise ValueError("n_neighbors = %d: 1 .. min(%d, the %d rows - 1)" % (k, MAX_K, N))
    idx, d2 = knn_enqueue(X, X, k, self_first=0)
    if weights == "connectivity":
        A = torch.ones_like(d2)
    else:
        dd = d2.double()
        A = torch.exp(-dd / (2.0 * dd[:, k - 1].mean())).float()
    return knn_symmetrize(idx, A)


class LabelSpreading:
    """sklearn.semi_supervised.LabelSpreading's surface on the device, for the symmetric kNN graph above.  fit(X, y): X [N][D] NumPy or a torch
    tensor (a CUDA tensor is used where it is), y int [N] with -1 for the rows without a label.  Sets classes_ (the sorted distinct labels),
    label_distributions_ (device f32 [N][len(classes_)], every row over its sum; a row no label reaches stays zero), transduction_ (NumPy,
    in y's values: np.argmax's rule, -1 for an unreached row), n_iter_ (a multiple of the chunk of 8 unless max_iter cut it), change_ (the
    last max |F' - F|), n_unreached_ and graph_ = (indptr, indices, values)."""

    def __init__(self, n_neighbors=7, alpha=0.8, weights="connectivity", max_iter=1000, tol=1e-6):
        if weights not in WEIGHTS:
            raise ValueError("weights = %r: one of %s" % (weights, ", ".join(WEIGHTS)))
        if not 0.0 < float(alpha) < 1.0:
            raise ValueError("alpha = %r: 0 < alpha < 1" % (alpha,))
        if int(n_neighbors) < 1 or int(max_iter) < 1 or not tol >= 0:
            raise ValueError("n_neighbors = %r, max_iter = %r, tol = %r: n_neighbors >= 1, max_iter >= 1, tol >= 0" % (n_neighbors, max_iter, tol))
        self.n_neighbors, self.alpha, self.weights, self.max_iter, self.tol = int(n_neighbors), float(alpha), weights, int(max_iter), float(tol)

    def fit(self, X, y):
        dev = _device_of(X)
        Xd = _rows_f32(X, dev)
        N = Xd.shape[0]
        y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
        if len(y) != N:
            raise ValueError("y must hold one entry per row of X: %d != %d" % (len(y), N))
        lab = y != -1
        self.classes_, inv = np.unique(y[lab], return_inverse=True)
        if len(self.classes_) < 1:
            raise ValueError("no row carries a label")
        n_classes = max(2, len(self.classes_))
        codes = np.full(N, -1, dtype=np.int32)
        codes[lab] = inv
        self.graph_ = knn_graph(Xd, self.n_neighbors, self.weights)
        indptr, indices, values = self.graph_
        s, _, nflag = sym_normalize_enqueue(indptr, indices, values)
        F, self.n_iter_, self.change_ = spread(indptr, indices, s, codes, n_classes, self.alpha, self.max_iter, self.tol)
        assert int(nflag.item()) == 0
        F = F[:, :len(self.classes_)]
        total = F.sum(dim=1, keepdim=True)
        self.label_distributions_ = F / torch.where(total == 0, torch.ones_like(total), total)
        pred = torch.where((F != 0).any(dim=1), argmax_labels(F), torch.full((N,), -1, dtype=torch.int32, device=dev)).cpu().numpy()
        self.n_unreached_ = int((pred < 0).sum())
        out = np.full(N, -1, dtype=self.classes_.dtype if np.issubdtype(self.classes_.dtype, np.integer) else np.int64)
        out[pred >= 0] = self.classes_[pred[pred >= 0]]
        self.transduction_ = out
        return self

    def score(self, y_true, mask=None):
        """the share of the rows `mask` (a boolean or index array; None: all rows) whose transduction_ is y_true there; an unreached row is wrong"""
        y_true = np.asarray(y_true.cpu() if isinstance(y_true, torch.Tensor) else y_true).reshape(-1)
        ok = self.transduction_ == y_true
        return float(np.mean(ok if mask is None else ok[np.asarray(mask)]))
