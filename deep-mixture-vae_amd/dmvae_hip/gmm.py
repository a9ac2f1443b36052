"""Diagonal-covariance Gaussian mixture fitted on the device (dmvae_gmm_fit / dmvae_gmm_kmeans of include/dmvae_hip.h):
what `sklearn.mixture.GaussianMixture(covariance_type="diag")` computes for the prior tables' initialisation
(base_models.py: pretrain_prior), with the restarts side by side in one call and a fit that is a function of (Z, seed) alone.

By default only the seeding runs on the host: k-means++ (D^2 sampling) per restart in NumPy from `np.random.RandomState(seed)`.
Lloyd's k-means from those centres, the initial M-step of its labels and the EM iterations are HIP kernels (csrc/gmm_fit.hip).
`seeding="device"` draws the centres on the device as well (dmvae_gmm_seed, csrc/gmm_seed.hip: all restarts in one call, optional
greedy local trials as sklearn's own seeding, no host copy of Z).  Nothing here imports sklearn."""
import ctypes as C
import time

import numpy as np
import torch

from . import _lib
from ._lib import lib, check


def kmeans_plusplus(X, n_clusters, rs):
    """k-means++ seeding (Arthur & Vassilvitskii 2007): the first centre uniform, every further one with probability
    proportional to the squared distance to the nearest centre chosen so far.  X [N][D] NumPy; rs a RandomState."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    centers = np.empty((n_clusters, X.shape[1]), dtype=np.float64)
    centers[0] = X[rs.randint(n)]
    d2 = ((X - centers[0]) ** 2).sum(1)
    for k in range(1, n_clusters):
        tot = d2.sum()
        i = rs.randint(n) if not tot > 0 else min(int(np.searchsorted(np.cumsum(d2), rs.random_sample() * tot)), n - 1)
        centers[k] = X[i]
        d2 = np.minimum(d2, ((X - centers[k]) ** 2).sum(1))
    return centers


def _device_of(Z):
    return Z.device if isinstance(Z, torch.Tensor) and Z.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _rows_f32(Z, dev):
    """Z as a 2-D f32 device tensor with unit column stride (a row-strided view is taken as it is: ldx = its row stride)"""
    if not isinstance(Z, torch.Tensor):
        Z = torch.as_tensor(np.ascontiguousarray(np.asarray(Z, dtype=np.float32)))
    Z = Z.to(device=dev, dtype=torch.float32)
    if Z.dim() != 2:
        raise ValueError("Z must be [N][D]")
    if Z.stride(1) != 1 or Z.stride(0) < Z.shape[1]:
        Z = Z.contiguous()
    return Z


def _run(fn_name, Z, cfg, labels, centers, weights_init, want):
    """One dmvae_gmm_fit / dmvae_gmm_kmeans call on the current stream; returns {name: NumPy array} of `want`."""
    dev = Z.device
    R, N, K, D = cfg.n_init, cfg.N, cfg.K, cfg.D
    nbytes = lib.dmvae_gmm_ws_bytes(C.byref(cfg))
    if nbytes < 0:
        check(int(nbytes), "dmvae_gmm_ws_bytes")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    shapes = {"weights": ((K,), torch.float32), "means": ((K, D), torch.float32), "covariances": ((K, D), torch.float32),
              "lower_bound": ((1,), torch.float64), "n_iter": ((1,), torch.int32), "converged": ((1,), torch.int32),
              "best_restart": ((1,), torch.int32), "lower_bounds": ((R,), torch.float64), "n_iters": ((R,), torch.int32),
              "convergeds": ((R,), torch.int32), "all_weights": ((R, K), torch.float32), "all_means": ((R, K, D), torch.float32),
              "all_covariances": ((R, K, D), torch.float32), "centers": ((R, K, D), torch.float32), "labels": ((R, N), torch.int32),
              "kmeans_iters": ((R,), torch.int32)}
    out = {n: torch.zeros(shapes[n][0], dtype=shapes[n][1], device=dev) for n in want}
    res = _lib.GmmResult(**{n: t.data_ptr() for n, t in out.items()})
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if fn_name == "dmvae_gmm_kmeans":
            rc = lib.dmvae_gmm_kmeans(stream, C.byref(cfg), Z.data_ptr(), Z.stride(0), centers.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(res))
        else:
            rc = lib.dmvae_gmm_fit(stream, C.byref(cfg), Z.data_ptr(), Z.stride(0), None if labels is None else labels.data_ptr(),
                                   None if centers is None else centers.data_ptr(), None if weights_init is None else weights_init.data_ptr(),
                                   ws.data_ptr(), ws.numel(), C.byref(res))
        check(rc, fn_name)
        torch.cuda.synchronize(dev)
    return {n: t.cpu().numpy() for n, t in out.items()}


def _stack(a, R, shape, dtype, dev, what):
    """labels [N] or [R][N] / centers [K][D] or [R][K][D] -> a contiguous device tensor with the restart axis"""
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    t = t.to(device=dev, dtype=dtype)
    if t.dim() == len(shape):
        t = t.unsqueeze(0)
    if tuple(t.shape[1:]) != tuple(shape):
        raise ValueError("%s must be %s or [n_restarts]%s, got %s" % (what, list(shape), list(shape), list(t.shape)))
    return t.contiguous()


def sklearn_local_trials(n_clusters):
    """the number of candidates sklearn's greedy k-means++ draws per centre: 2 + int(ln K)"""
    return 2 + int(np.log(n_clusters))


def kmeans_plusplus_device(Z, n_clusters, n_init=1, seed=0, local_trials=1, u=None, return_trials=False):
    """k-means++ seeding on the device (dmvae_gmm_seed), n_init restarts side by side, enqueued on the current stream without a
    synchronisation.  local_trials: 1 plain D^2 sampling, 0 sklearn's 2 + int(ln K) greedy trials, 2..8 that many.  u: the uniforms
    [n_init][K][T] in [0, 1) (NumPy or tensor), or None: the Philox stream (seed, step 0, stream id 3) of dmvae_philox_uniform.
    Returns (centers [n_init][K][D] f32, rows [n_init][K] int32) as device tensors; with return_trials also every round's candidate
    rows [n_init][K][T] (round 0: trial 0, the others -1)."""
    dev = _device_of(Z)
    Z = _rows_f32(Z, dev)
    N, D = Z.shape
    R, K = int(n_init), int(n_clusters)
    cfg = _lib.GmmSeedConfig(N=N, D=D, K=K, n_init=R, local_trials=int(local_trials), seed=int(seed), flags=0)
    nbytes = lib.dmvae_gmm_seed_ws_bytes(C.byref(cfg))
    if nbytes < 0:
        check(int(nbytes), "dmvae_gmm_seed_ws_bytes")
    T = int(local_trials) if local_trials else sklearn_local_trials(K)
    ud = None
    if u is not None:
        ud = (u if isinstance(u, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(u, dtype=np.float32))))
        ud = ud.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(ud.shape) != (R, K, T):
            raise ValueError("u must be [n_init][K][trials] = %s, got %s" % ([R, K, T], list(ud.shape)))
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    centers = torch.empty((R, K, D), dtype=torch.float32, device=dev)
    rows = torch.empty((R, K), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        check(lib.dmvae_gmm_seed(stream, C.byref(cfg), Z.data_ptr(), Z.stride(0), None if ud is None else ud.data_ptr(), ws.data_ptr(),
                                 ws.numel(), centers.data_ptr(), rows.data_ptr()), "dmvae_gmm_seed")
    if return_trials:
        return centers, rows, ws[:R * K * T * 4].view(torch.int32).reshape(R, K, T).clone()
    return centers, rows


def philox_uniform(n, seed, step=0, stream_id=3, device=None):
    """n uniforms in [0, 1) of the Philox stream (seed, step, stream_id) as a device f32 tensor (dmvae_philox_uniform)"""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty(int(n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dmvae_philox_uniform(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), out.data_ptr(), out.numel(), int(seed), int(step),
                                       int(stream_id)), "dmvae_philox_uniform")
    return out


def kmeans(Z, centers, max_iter=300):
    """Lloyd's k-means on the device from centers [K][D] (or [R][K][D]: R runs side by side).  Returns (centers, labels, n_iter)
    with the restart axis kept only when it was given."""
    dev = _device_of(Z)
    Z = _rows_f32(Z, dev)
    squeeze = (centers.dim() if isinstance(centers, torch.Tensor) else np.asarray(centers).ndim) == 2
    K = int(centers.shape[-2])
    c = _stack(centers, None, (K, Z.shape[1]), torch.float32, dev, "centers")
    cfg = _lib.GmmConfig(N=Z.shape[0], D=Z.shape[1], K=K, n_init=c.shape[0], max_iter=1, kmeans_iter=int(max_iter), tol=0.0, reg_covar=0.0, flags=0)
    o = _run("dmvae_gmm_kmeans", Z, cfg, None, c, None, ("centers", "labels", "kmeans_iters"))
    if squeeze:
        return o["centers"][0].astype(np.float64), o["labels"][0], int(o["kmeans_iters"][0])
    return o["centers"].astype(np.float64), o["labels"], o["kmeans_iters"]


class DiagGMM:
    """GaussianMixture(covariance_type="diag") on the device.  fit(Z) seeds every restart with k-means++: seeding="host" (the
    default) on a host copy of Z in NumPy, seeding="device" with dmvae_gmm_seed on the resident rows (local_trials as in
    kmeans_plusplus_device; the seeding and the fit are enqueued back to back: no host copy of Z, no synchronisation in between).
    fit(Z, labels=...) / fit(Z, centers=...) start from the given hard labels ([N] or [R][N]) / centres ([K][D] or [R][K][D])
    instead (their leading axis then is the number of restarts).  Results under sklearn's names, NumPy float64.
    time_parts (device seeding only): synchronise after the seeding so that seed_seconds_ and device_seconds_ time the two parts
    apart; without it seed_seconds_ is None and device_seconds_ spans the seeding and the fit."""

    def __init__(self, n_components, max_iter=100, n_init=1, tol=1e-3, reg_covar=1e-6, weights_init=None, kmeans_iter=300, seed=0,
                 seeding="host", local_trials=1, time_parts=False):
        self.n_components, self.max_iter, self.n_init = int(n_components), int(max_iter), int(n_init)
        self.tol, self.reg_covar, self.kmeans_iter, self.seed = float(tol), float(reg_covar), int(kmeans_iter), int(seed)
        if seeding not in ("host", "device"):
            raise ValueError("seeding must be 'host' or 'device'")
        if int(local_trials) != local_trials or not 0 <= int(local_trials) <= 8:
            raise ValueError("local_trials must be 0 (sklearn's 2 + int(ln K)) or 1..8")
        if seeding == "host" and int(local_trials) != 1:
            raise ValueError("the host seeding is plain D^2 sampling: local_trials needs seeding='device'")
        self.seeding, self.local_trials, self.time_parts = seeding, int(local_trials), bool(time_parts)
        self.weights_init = None if weights_init is None else np.asarray(weights_init, dtype=np.float32)
        if self.weights_init is not None and self.weights_init.shape != (self.n_components,):
            raise ValueError("weights_init must have n_components entries")

    def seed_centers(self, Z):
        """[n_init][K][D] k-means++ centres, restart r from the r-th stretch of RandomState(seed)'s stream"""
        Zh = Z.detach().cpu().numpy() if isinstance(Z, torch.Tensor) else np.asarray(Z)
        rs = np.random.RandomState(self.seed)
        return np.stack([kmeans_plusplus(Zh, self.n_components, rs) for _ in range(self.n_init)]).astype(np.float32)

    def fit(self, Z, labels=None, centers=None):
        if labels is not None and centers is not None:
            raise ValueError("give labels or centers, not both")
        dev = _device_of(Z)
        K = self.n_components
        on_device = self.seeding == "device" and labels is None and centers is None
        wi = None if self.weights_init is None else torch.as_tensor(self.weights_init).to(dev)      # (before the seeding: nothing between it and the fit)
        if on_device:
            Zd = _rows_f32(Z, dev)
            if self.time_parts:
                torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            centers, _ = kmeans_plusplus_device(Zd, K, n_init=self.n_init, seed=self.seed, local_trials=self.local_trials)
            self.seed_seconds_ = None
            if self.time_parts:
                torch.cuda.synchronize(dev)
                self.seed_seconds_ = time.perf_counter() - t0
        else:
            t0 = time.perf_counter()
            if labels is None and centers is None:
                centers = self.seed_centers(Z)
            self.seed_seconds_ = time.perf_counter() - t0
            Zd = _rows_f32(Z, dev)
        N, D = Zd.shape
        lab = cen = None
        if labels is not None:
            lab = _stack(labels, None, (N,), torch.int32, dev, "labels")
        else:
            cen = _stack(centers, None, (K, D), torch.float32, dev, "centers")
        R = (lab if lab is not None else cen).shape[0]
        cfg = _lib.GmmConfig(N=N, D=D, K=K, n_init=R, max_iter=self.max_iter, kmeans_iter=self.kmeans_iter, tol=self.tol,
                             reg_covar=self.reg_covar, flags=0)
        want = ["weights", "means", "covariances", "lower_bound", "n_iter", "converged", "best_restart", "lower_bounds", "n_iters",
                "convergeds", "all_weights", "all_means", "all_covariances"]
        if cen is not None:
            want.append("kmeans_iters")
        if not on_device:
            torch.cuda.synchronize(dev)
        if not on_device or self.time_parts:
            t0 = time.perf_counter()
        o = _run("dmvae_gmm_fit", Zd, cfg, lab, cen, wi, want)
        self.device_seconds_ = time.perf_counter() - t0        # _run synchronises before it reads back
        self.weights_ = o["weights"].astype(np.float64)
        self.means_ = o["means"].astype(np.float64)
        self.covariances_ = o["covariances"].astype(np.float64)
        self.lower_bound_ = float(o["lower_bound"][0])
        self.n_iter_ = int(o["n_iter"][0])
        self.converged_ = bool(o["converged"][0])
        self.best_restart_ = int(o["best_restart"][0])
        self.restarts_ = {"lower_bound": o["lower_bounds"], "n_iter": o["n_iters"], "converged": o["convergeds"].astype(bool),
                          "weights": o["all_weights"], "means": o["all_means"], "covariances": o["all_covariances"]}
        if cen is not None:
            self.restarts_["kmeans_iter"] = o["kmeans_iters"]
        return self

    def score_samples_device(self, Z):
        """log sum_k w_k N(z; mean_k, diag cov_k) of every row of Z as a device f32 [N] (dmvae_mixture_logpdf: any K * D); only enqueues"""
        from .density import mixture_logpdf
        if not hasattr(self, "means_"):
            raise RuntimeError("DiagGMM.score_samples: fit first (or set weights_, means_, covariances_)")
        with np.errstate(divide="ignore"):
            lw = np.log(np.asarray(self.weights_, dtype=np.float64))
        return mixture_logpdf(Z, np.asarray(self.means_, dtype=np.float32), np.log(np.asarray(self.covariances_, dtype=np.float64)).astype(np.float32),
                              lw.astype(np.float32))

    def score_samples(self, Z):
        """sklearn's GaussianMixture.score_samples: the weighted log-likelihood of every row of Z, NumPy float64 [N]"""
        return self.score_samples_device(Z).cpu().numpy().astype(np.float64)

    def score(self, Z):
        """sklearn's GaussianMixture.score: the mean of score_samples(Z), summed in float64 on the device"""
        from .density import sum_f64
        s = self.score_samples_device(Z)
        return float(sum_f64(s).item()) / s.numel()
