"""Exact t-SNE on the device (dmvae_tsne_* of include/dmvae_hip.h, csrc/tsne.hip): what `sklearn.manifold.TSNE(n_components=2,
method="exact")` computes for the scatter of the prior samples (includes/visualization.py: cluster_scatter), dense O(N^2) per
iteration, no Barnes-Hut approximation, a function of (X, the initial Y) alone: two runs agree bit for bit.

Deviations from sklearn, both so that the result does not depend on a host read in the middle: the perplexity search runs exactly
64 bisection steps, and all n_iter iterations run (no n_iter_without_progress / min_grad_norm stop).  Nothing here imports sklearn."""
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


class TSNE:
    """sklearn.manifold.TSNE's surface for the exact method on the device.  X: NumPy or a torch tensor [N][D]; a CUDA tensor is
    used where it is (a row-strided f32 view too), with no host copy.  init: "random" (1e-4 * the Philox normals of random_state,
    stream id 5) or an [N][2] array.  Sets embedding_ (NumPy f32 [N][2]), embedding_device_ (the same as a device tensor),
    kl_divergence_, n_iter_ and learning_rate_ (what "auto" resolved to: max(N / early_exaggeration / 4, 50))."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", n_iter=1000, init="random",
                 random_state=0, session=None):
        if n_components != 2:
            raise ValueError("the device t-SNE embeds into two dimensions: n_components must be 2")
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
        cfg = config(N, D, self.perplexity, self.early_exaggeration, self.learning_rate, self.n_iter, seed=self.random_state)
        Y0 = None
        if not isinstance(self.init, str):
            Y0 = self.init if isinstance(self.init, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(self.init, dtype=np.float32)))
            Y0 = Y0.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(Y0.shape) != (N, 2):
                raise ValueError("init must be [N][2] = %s, got %s" % ([N, 2], list(Y0.shape)))
        ws = workspace(cfg, dev)
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
