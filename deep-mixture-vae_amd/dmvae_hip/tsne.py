"""Exact t-SNE on the device (dmvae_tsne_* of include/dmvae_hip.h, csrc/tsne.hip): what `sklearn.manifold.TSNE(n_components=2,
method="exact")` computes for the scatter of the prior samples (includes/visualization.py: cluster_scatter), dense O(N^2) per
iteration, no Barnes-Hut approximation, a function of (X, the initial Y) alone: two runs agree bit for bit.

Deviations from sklearn, both so that the result does not depend on a host read in the middle: the perplexity search runs exactly
64 bisection steps, and all n_iter iterations run (no n_iter_without_progress / min_grad_norm stop).  Nothing here imports sklearn.

method="knn" (dmvae_tsne_knn_*, csrc/tsne_knn.hip; knn_joint_p / knn_gradient / knn_step / knn_fit below) lifts the dense form's cap of
32768 rows: P is what sklearn's method="barnes_hut" builds -- conditional probabilities over the min(N - 1, int(3 perplexity + 1))
nearest rows (dmvae_hip.knn), symmetrised over the union graph into CSR -- and the repulsive term stays exact over all pairs."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .gmm import _device_of, _rows_f32

EXAGGERATION_ITERS = 250      # sklearn's _EXPLORATION_MAX_ITER


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def workspace(cfg, dev):
    """the caller's scratch of one (N, D) as a uint8 device tensor: the dense [N][N] f32 matrix first"""
    nbytes = lib.dmvae_tsne_ws_bytes(C.byref(cfg))
    if nbytes < 0:
        check(int(nbytes), "dmvae_tsne_ws_bytes")
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


def config(N, D, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", n_iter=1000, exaggeration_iters=EXAGGERATION_ITERS, seed=0):
    lr = max(N / float(early_exaggeration) / 4.0, 50.0) if isinstance(learning_rate, str) else float(learning_rate)
    return _lib.TsneConfig(N=int(N), D=int(D), perplexity=float(perplexity), early_exaggeration=float(early_exaggeration), learning_rate=lr,
                           n_iter=int(n_iter), exaggeration_iters=int(exaggeration_iters), seed=int(seed), flags=0)


def joint_p(X, cfg, ws):
    """steps 1-3 on the current stream; returns (P [N][N] f32: a view of the workspace, beta [N] f32) without a synchronisation"""
    beta = torch.empty(cfg.N, dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        check(lib.dmvae_tsne_joint_p(_stream(X.device), C.byref(cfg), X.data_ptr(), X.stride(0), ws.data_ptr(), ws.numel(), beta.data_ptr()),
              "dmvae_tsne_joint_p")
    assert lib.dmvae_tsne_p(ws.data_ptr()) == ws.data_ptr()
    return ws[:cfg.N * cfg.N * 4].view(torch.float32).reshape(cfg.N, cfg.N), beta


def gradient(cfg, ws, Y, exaggeration):
    """the gradient [N][2] at Y for the P that joint_p left in ws"""
    grad = torch.empty((cfg.N, 2), dtype=torch.float32, device=Y.device)
    with torch.cuda.device(Y.device):
        check(lib.dmvae_tsne_gradient(_stream(Y.device), C.byref(cfg), ws.data_ptr(), ws.numel(), Y.data_ptr(), float(exaggeration), grad.data_ptr()),
              "dmvae_tsne_gradient")
    return grad


def step(cfg, ws, Y, U, G, exaggeration, momentum):
    """one iteration in place on Y, U (velocity), G (gains), each [N][2] f32 and contiguous"""
    with torch.cuda.device(Y.device):
        check(lib.dmvae_tsne_step(_stream(Y.device), C.byref(cfg), ws.data_ptr(), ws.numel(), Y.data_ptr(), U.data_ptr(), G.data_ptr(),
                                  float(exaggeration), float(momentum)), "dmvae_tsne_step")


def fit(X, cfg, ws, Y0=None):
    """the whole run on the current stream; returns (Y [N][2] f32, kl [1] f64) device tensors without a synchronisation"""
    Y = torch.empty((cfg.N, 2), dtype=torch.float32, device=X.device)
    kl = torch.empty(1, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        check(lib.dmvae_tsne_fit(_stream(X.device), C.byref(cfg), X.data_ptr(), X.stride(0), None if Y0 is None else Y0.data_ptr(), ws.data_ptr(),
                                 ws.numel(), Y.data_ptr(), kl.data_ptr()), "dmvae_tsne_fit")
    return Y, kl


# ---- the kNN-sparse form (dmvae_tsne_knn_* of include/dmvae_hip.h, csrc/tsne_knn.hip): sklearn's method="barnes_hut" P -- conditional
# probabilities over the k nearest rows, symmetrised over the union graph -- with the repulsion kept exact over all pairs
EXACT_MAX_N = 32768           # TSNE_MAX_N of csrc/tsne.h: the dense form's cap


def n_neighbors(N, perplexity):
    """k = min(N - 1, int(3 perplexity + 1)), sklearn's n_neighbors of the Barnes-Hut form (perplexity as the f32 the config carries)"""
    return min(int(N) - 1, int(3.0 * float(np.float32(perplexity)) + 1.0))


def knn_config(N, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", n_iter=1000, exaggeration_iters=EXAGGERATION_ITERS, seed=0,
               col_splits=0, nnz=0):
    lr = max(N / float(early_exaggeration) / 4.0, 50.0) if isinstance(learning_rate, str) else float(learning_rate)
    return _lib.TsneKnnConfig(N=int(N), k=n_neighbors(N, perplexity), nnz=int(nnz), perplexity=float(perplexity),
                              early_exaggeration=float(early_exaggeration), learning_rate=lr, n_iter=int(n_iter),
                              exaggeration_iters=int(exaggeration_iters), col_splits=int(col_splits), seed=int(seed), flags=0)


def knn_workspace(cfg, dev):
    """the caller's scratch of one (N, col_splits) as a uint8 device tensor: O(S N), no N x N array"""
    nbytes = lib.dmvae_tsne_knn_ws_bytes(C.byref(cfg))
    if nbytes < 0:
        check(int(nbytes), "dmvae_tsne_knn_ws_bytes")
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


class KnnP:
    """the joint P of the kNN-sparse form as CSR on the device -- indptr int64 [N + 1], indices int32 [nnz], values f32 [nnz], sorted by
    (row, column) -- with the beta_i [N] and the neighbour lists idx / d2 [N][k] it was built from"""

    def __init__(self, indptr, indices, values, beta, idx, d2, cond):
        self.indptr, self.indices, self.values, self.beta, self.idx, self.d2, self.cond = indptr, indices, values, beta, idx, d2, cond
        self.nnz = int(indices.numel())

    def dense(self):
        """[N][N] f32 on the device (small N: tests and plots)"""
        N = self.indptr.numel() - 1
        rows = torch.repeat_interleave(torch.arange(N, device=self.indptr.device), self.indptr[1:] - self.indptr[:-1])
        out = torch.zeros((N, N), dtype=torch.float32, device=self.indptr.device)
        out[rows, self.indices.long()] = self.values
        return out


def knn_cond_p(d2, cfg):
    """p_{j|i} [N][k] f32 and beta [N] f32 from the squared distances d2 [N][k] of the lists, nearest first; only enqueues"""
    assert d2.is_cuda and d2.dtype == torch.float32 and d2.dim() == 2 and tuple(d2.shape) == (cfg.N, cfg.k) and d2.stride(1) == 1
    p = torch.empty((cfg.N, cfg.k), dtype=torch.float32, device=d2.device)
    beta = torch.empty(cfg.N, dtype=torch.float32, device=d2.device)
    with torch.cuda.device(d2.device):
        check(lib.dmvae_tsne_knn_cond_p(_stream(d2.device), C.byref(cfg), d2.data_ptr(), d2.stride(0), p.data_ptr(), cfg.k, beta.data_ptr()),
              "dmvae_tsne_knn_cond_p")
    return p, beta


def knn_symmetrize(idx, p):
    """(indptr, indices, values): P_ij = (p_{j|i} + p_{i|j}) / 2N over the union of the lists idx [N][k] with their p [N][k], an absent
    direction counting 0.  Every entry is keyed twice, as (i, j) and as (j, i); a stable sort brings the at most two copies of a key
    together, and the sum of two floats does not depend on their order: P_ij and P_ji are the same bits.  Reads one integer (nnz) back."""
    N, k = idx.shape
    dev = idx.device
    rows = torch.arange(N, dtype=torch.int64, device=dev).repeat_interleave(k)
    cols = idx.reshape(-1).to(torch.int64)
    keys, order = torch.sort(torch.cat([rows * N + cols, cols * N + rows]), stable=True)
    vals = torch.cat([p.reshape(-1), p.reshape(-1)])[order]
    first = torch.ones_like(keys, dtype=torch.bool)
    first[1:] = keys[1:] != keys[:-1]
    partner = torch.zeros_like(vals)
    partner[:-1] = torch.where(first[1:], torch.zeros_like(vals[1:]), vals[1:])
    keys = keys[first]
    values = (vals + partner)[first] / torch.tensor(2.0 * N, dtype=torch.float32, device=dev)
    indptr = torch.searchsorted(keys, torch.arange(N + 1, dtype=torch.int64, device=dev) * N)
    return indptr.contiguous(), (keys % N).to(torch.int32).contiguous(), values.contiguous()


def knn_joint_p(X, cfg):
    """the neighbour lists (dmvae_knn, the row itself left out), the conditional p and the CSR of the joint P of X [N][D] on the current
    stream; returns a KnnP and sets cfg.nnz"""
    from .knn import knn_enqueue
    if X.shape[0] != cfg.N:
        raise ValueError("X holds %d rows, the config %d" % (X.shape[0], cfg.N))
    nbytes = lib.dmvae_tsne_knn_ws_bytes(C.byref(cfg))         # the limits on (N, perplexity, k) answer before the neighbour search
    if nbytes < 0:
        check(int(nbytes), "dmvae_tsne_knn_ws_bytes")
    idx, d2 = knn_enqueue(X, X, cfg.k, self_first=0)
    cond, beta = knn_cond_p(d2, cfg)
    indptr, indices, values = knn_symmetrize(idx, cond)
    P = KnnP(indptr, indices, values, beta, idx, d2, cond)
    cfg.nnz = P.nnz
    return P


def knn_gradient(cfg, P, ws, Y, exaggeration):
    """the gradient [N][2] at Y for the CSR P"""
    grad = torch.empty((cfg.N, 2), dtype=torch.float32, device=Y.device)
    with torch.cuda.device(Y.device):
        check(lib.dmvae_tsne_knn_gradient(_stream(Y.device), C.byref(cfg), P.indptr.data_ptr(), P.indices.data_ptr(), P.values.data_ptr(), ws.data_ptr(),
                                          ws.numel(), Y.data_ptr(), float(exaggeration), grad.data_ptr()), "dmvae_tsne_knn_gradient")
    return grad


def knn_step(cfg, P, ws, Y, U, G, exaggeration, momentum):
    """one iteration in place on Y, U (velocity), G (gains), each [N][2] f32 and contiguous"""
    with torch.cuda.device(Y.device):
        check(lib.dmvae_tsne_knn_step(_stream(Y.device), C.byref(cfg), P.indptr.data_ptr(), P.indices.data_ptr(), P.values.data_ptr(), ws.data_ptr(),
                                      ws.numel(), Y.data_ptr(), U.data_ptr(), G.data_ptr(), float(exaggeration), float(momentum)),
              "dmvae_tsne_knn_step")


def knn_fit(X, cfg, ws, Y0=None, P=None):
    """the whole run on the current stream; returns (Y [N][2] f32, kl [1] f64) device tensors.  P: what knn_joint_p(X, cfg) returned, or
    None to build it here (the one host read of the run: nnz); the iterations read nothing back."""
    if P is None:
        P = knn_joint_p(X, cfg)
    dev = P.indptr.device
    Y = torch.empty((cfg.N, 2), dtype=torch.float32, device=dev)
    kl = torch.empty(1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.dmvae_tsne_knn_fit(_stream(dev), C.byref(cfg), P.indptr.data_ptr(), P.indices.data_ptr(), P.values.data_ptr(),
                                     None if Y0 is None else Y0.data_ptr(), ws.data_ptr(), ws.numel(), Y.data_ptr(), kl.data_ptr()),
              "dmvae_tsne_knn_fit")
    return Y, kl


class TSNE:
    """sklearn.manifold.TSNE's surface for the exact method on the device.  X: NumPy or a torch tensor [N][D]; a CUDA tensor is
    used where it is (a row-strided f32 view too), with no host copy.  init: "random" (1e-4 * the Philox normals of random_state,
    stream id 5) or an [N][2] array.  Sets embedding_ (NumPy f32 [N][2]), embedding_device_ (the same as a device tensor),
    kl_divergence_, n_iter_ and learning_rate_ (what "auto" resolved to: max(N / early_exaggeration / 4, 50)).
    method: "exact" (the dense P, up to 32768 rows) or "knn" (P over the int(3 perplexity + 1) nearest rows as sklearn's Barnes-Hut
    form takes it, the repulsion still exact over all pairs, up to 2^20 rows; sets n_neighbors_ and nnz_ too)."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", n_iter=1000, init="random",
                 random_state=0, session=None, method="exact", col_splits=0):
        if n_components != 2:
            raise ValueError("the device t-SNE embeds into two dimensions: n_components must be 2")
        if method not in ("exact", "knn"):
            raise ValueError("method must be 'exact' or 'knn'")
        self.method, self.col_splits = method, int(col_splits)
        if isinstance(learning_rate, str) and learning_rate != "auto":
            raise ValueError("learning_rate must be 'auto' or a number")
        if isinstance(init, str) and init != "random":
            raise ValueError("init must be 'random' or an [N][2] array")
        self.n_components, self.perplexity, self.early_exaggeration = 2, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.n_iter, self.init = learning_rate, int(n_iter), init
        self.random_state = 0 if random_state is None else int(random_state)
        self.session = session

    def fit(self, X):
        dev = _device_of(X)
        Xd = _rows_f32(X, dev)
        N, D = Xd.shape
        knn = self.method == "knn"
        if knn:
            cfg = knn_config(N, self.perplexity, self.early_exaggeration, self.learning_rate, self.n_iter, seed=self.random_state,
                             col_splits=self.col_splits)
        else:
            cfg = config(N, D, self.perplexity, self.early_exaggeration, self.learning_rate, self.n_iter, seed=self.random_state)
        Y0 = None
        if not isinstance(self.init, str):
            Y0 = self.init if isinstance(self.init, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(self.init, dtype=np.float32)))
            Y0 = Y0.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(Y0.shape) != (N, 2):
                raise ValueError("init must be [N][2] = %s, got %s" % ([N, 2], list(Y0.shape)))
        if knn:
            P = knn_joint_p(Xd, cfg)
            Y, kl = knn_fit(Xd, cfg, knn_workspace(cfg, dev), Y0, P)
            self.n_neighbors_, self.nnz_ = int(cfg.k), P.nnz
        else:
            try:
                ws = workspace(cfg, dev)
            except _lib.DmvaeError as err:
                if N > EXACT_MAX_N:
                    raise _lib.DmvaeError('%s; method="knn" embeds up to 2^20 rows' % err) from None
                raise
            Y, kl = fit(Xd, cfg, ws, Y0)
        torch.cuda.synchronize(dev)
        self.learning_rate_ = float(cfg.learning_rate)
        self.embedding_device_ = Y
        self.embedding_ = Y.cpu().numpy()
        self.kl_divergence_ = float(kl.item())
        self.n_iter_ = self.n_iter
        return self

    def fit_transform(self, X):
        return self.fit(X).embedding_

    def trustworthiness(self, X, n_neighbors=5):
        """sklearn.manifold.trustworthiness(X, embedding_, n_neighbors=...) of the fitted scatter, both all-pairs halves on the device
        (dmvae_hip.knn.trustworthiness on embedding_device_): how far the neighbourhoods it draws are neighbourhoods of X"""
        from .knn import trustworthiness
        return trustworthiness(X, self.embedding_device_, n_neighbors)
