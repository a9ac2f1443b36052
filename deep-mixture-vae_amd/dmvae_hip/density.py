"""Posterior diagnostics on the device (dmvae_mixture_logpdf / dmvae_posterior_sample / dmvae_column_stats / dmvae_sum_f64 of
include/dmvae_hip.h, csrc/mixture_density.hip): the log-density of points under a diagonal Gaussian mixture with
any number of components -- with the N encoder posteriors as components log q(z), the aggregate posterior; with the K prior rows
log p(z) -- and from them the split of the KL term of Hoffman & Johnson 2016,

    E_x KL(q(z|x) || p(z)) = I(x;z) + KL(q(z) || p(z)),

with I(x;z) estimated as in He et al. 2019, and the active units of Burda et al. 2016.  An all-pairs O(M J D) computation that stores no
M x J array and is a function of its inputs alone: two calls agree bit for bit.  Everything here only enqueues unless it says otherwise."""
import ctypes as C
import math

import numpy as np
import torch

from ._lib import lib, check
from .gmm import _device_of, _rows_f32

PHILOX_STREAM = 6       # posterior_sample's noise stream


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ld(t):
    return max(t.stride(0), t.shape[1])


def _is_rows(t):
    return t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1) and (t.shape[0] == 1 or t.stride(0) >= t.shape[1])


def _bytes(n, what):
    if n < 0:
        check(int(n), what)
    return int(n)


def mixture_split(M, J, D):
    """the number of parts dmvae_mixture_logpdf splits the J components into for M points (a function of (M, J, D) alone)"""
    return int(lib.dmvae_mixture_logpdf_split(int(M), int(J), int(D)))


def mixture_logpdf(Z, means, log_vars, log_weights=None, out=None, ws=None):
    """log sum_j w_j N(z_i; mu_j, diag exp(lv_j)) of every row of Z as a device f32 [M].  Z [M][D], means / log_vars [J][D]: device f32
    tensors with unit column stride (row-strided views are read where they are), or arrays that are uploaded; log_weights [J] (an
    entry of -inf: a component of weight 0) or None = uniform weights, -log J.  ws: a uint8 device tensor of at least
    dmvae_mixture_logpdf_ws_bytes(M, J, D) bytes, or None: allocated here."""
    dev = _device_of(Z if isinstance(Z, torch.Tensor) else means)
    Z, means, log_vars = (t if isinstance(t, torch.Tensor) and _is_rows(t) else _rows_f32(t, dev) for t in (Z, means, log_vars))
    (M, D), J = Z.shape, means.shape[0]
    if means.shape != (J, D) or log_vars.shape != (J, D):
        raise ValueError("means and log_vars must be [J][%d], got %s and %s" % (D, list(means.shape), list(log_vars.shape)))
    lw = None
    if log_weights is not None:
        lw = (log_weights if isinstance(log_weights, torch.Tensor) else torch.as_tensor(np.asarray(log_weights, dtype=np.float32)))
        lw = lw.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
        if lw.numel() != J:
            raise ValueError("log_weights must hold one entry per component: %d != %d" % (lw.numel(), J))
    if ws is None:
        ws = torch.empty(_bytes(lib.dmvae_mixture_logpdf_ws_bytes(M, J, D), "dmvae_mixture_logpdf_ws_bytes"), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(M, dtype=torch.float32, device=dev)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == M
    with torch.cuda.device(dev):
        check(lib.dmvae_mixture_logpdf(_stream(dev), Z.data_ptr(), _ld(Z), M, D, means.data_ptr(), _ld(means), log_vars.data_ptr(), _ld(log_vars), J,
                                       None if lw is None else lw.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr()), "dmvae_mixture_logpdf")
    return out


def posterior_sample(mean, log_var, eps=None, seed=0, counter=0, pos0=0):
    """(z [n][D], a [n]) as device f32 tensors: z = mean + exp(log_var / 2) eps and a = log q(z | x) of every row.  eps: device f32 [n][D], or
    None: Philox stream 6 keyed by (seed, counter), element (pos0 + i) D + d."""
    dev = _device_of(mean)
    mean, log_var = (t if isinstance(t, torch.Tensor) and _is_rows(t) else _rows_f32(t, dev) for t in (mean, log_var))
    n, D = mean.shape
    if log_var.shape != (n, D):
        raise ValueError("log_var must be [%d][%d]" % (n, D))
    if eps is not None:
        eps = eps if isinstance(eps, torch.Tensor) and _is_rows(eps) else _rows_f32(eps, dev)
        if eps.shape != (n, D):
            raise ValueError("eps must be [%d][%d]" % (n, D))
    Z = torch.empty((n, D), dtype=torch.float32, device=dev)
    a = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dmvae_posterior_sample(_stream(dev), mean.data_ptr(), _ld(mean), log_var.data_ptr(), _ld(log_var), n, D,
                                         None if eps is None else eps.data_ptr(), 0 if eps is None else _ld(eps), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                         int(counter) & 0xFFFFFFFFFFFFFFFF, int(pos0), Z.data_ptr(), D, a.data_ptr()), "dmvae_posterior_sample")
    return Z, a


def column_stats(mean, log_var):
    """device f64 [3][D]: the column means of `mean`, their population variance (two-pass) and the column means of exp(log_var)"""
    dev = _device_of(mean)
    mean, log_var = (t if isinstance(t, torch.Tensor) and _is_rows(t) else _rows_f32(t, dev) for t in (mean, log_var))
    n, D = mean.shape
    if log_var.shape != (n, D):
        raise ValueError("log_var must be [%d][%d]" % (n, D))
    ws = torch.empty(_bytes(lib.dmvae_column_stats_ws_bytes(n, D), "dmvae_column_stats_ws_bytes"), dtype=torch.uint8, device=dev)
    out = torch.empty((3, D), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.dmvae_column_stats(_stream(dev), mean.data_ptr(), _ld(mean), log_var.data_ptr(), _ld(log_var), n, D, ws.data_ptr(), ws.numel(),
                                     out.data_ptr()), "dmvae_column_stats")
    return out


def sum_f64(x, out=None):
    """the sum of a contiguous device f32 vector in float64, added in a fixed order, as a device f64 [1] (or into out, a 1-element view)"""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() >= 1
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=x.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.numel() == 1
    with torch.cuda.device(x.device):
        check(lib.dmvae_sum_f64(_stream(x.device), x.data_ptr(), x.numel(), out.data_ptr()), "dmvae_sum_f64")
    return out


def subsample_rows(N, M):
    """the rows floor(i N / M), i < M, of N evaluated rows"""
    return (np.arange(M, dtype=np.int64) * N) // M


def posterior_diagnostics_enqueue(mean, log_var, prior_means, prior_log_vars, seed=0, counter=0, max_points=None, eps=None):
    """Everything behind the encoder passes, on the current stream, without a synchronisation.  mean / log_var [N][D]: the encoder
    outputs of the evaluated rows; prior_means / prior_log_vars [K][D].  The points are all N rows, or with max_points = M < N the rows
    floor(i N / M); their noise is eps ([M][D], one row per point) or Philox stream 6 keyed by (seed, counter), element i D + d of point i.
    log q(z) runs over all N rows.  Returns dict(z [M][D], a [M], m [M], p [M] device f32; sums device f64 [3] = (sum a, sum m,
    sum p), each added in a fixed order; stats device f64 [3][D]; n_points, n_rows)."""
    dev = mean.device
    N, D = mean.shape
    M = N if max_points is None else max(1, min(int(max_points), N))
    if M < N:
        idx = torch.as_tensor(subsample_rows(N, M)).to(dev)
        pm, plv = mean.index_select(0, idx), log_var.index_select(0, idx)
    else:
        pm, plv = mean, log_var
    z, a = posterior_sample(pm, plv, eps=eps, seed=seed, counter=counter)
    m = mixture_logpdf(z, mean, log_var)
    p = mixture_logpdf(z, prior_means, prior_log_vars)
    sums = torch.empty(3, dtype=torch.float64, device=dev)
    for k, v in enumerate((a, m, p)):
        sum_f64(v, out=sums[k:k + 1])
    return dict(z=z, a=a, m=m, p=p, sums=sums, stats=column_stats(mean, log_var), n_points=M, n_rows=N)


def diagnostics_from(enq, au_threshold=0.01):
    """the one read-back: dict(mi, marginal_kl, rate, mi_cap, active_units, var_of_mean, mean_of_var, n_points, n_rows) of what
    posterior_diagnostics_enqueue left on the device"""
    M, N = enq["n_points"], enq["n_rows"]
    host = torch.cat([enq["sums"], enq["stats"].reshape(-1)]).cpu().numpy()
    sa, sm, sp = (float(v) for v in host[:3])
    stats = host[3:].reshape(3, -1)
    return dict(mi=(sa - sm) / M, marginal_kl=(sm - sp) / M, rate=(sa - sp) / M, mi_cap=math.log(N),
                active_units=int(np.count_nonzero(stats[1] > au_threshold)), var_of_mean=stats[1].copy(), mean_of_var=stats[2].copy(),
                n_points=M, n_rows=N)
