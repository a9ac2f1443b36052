"""Cluster quality beside the Hungarian-matched accuracy: NMI, ARI and purity from the integer confusion matrix [cluster][class]
(host arithmetic in float64 / Python ints), and the label-free silhouette coefficient of rows under labels on the device
(dmvae_argmax_labels / dmvae_silhouette of include/dmvae_hip.h, csrc/cluster_metrics.hip): an all-pairs O(N^2 D) computation that
stores no N x N array and is a function of (Z, labels) alone -- two calls agree bit for bit.  The definitions are those of
sklearn.metrics (normalized_mutual_info_score with the arithmetic mean, adjusted_rand_score, silhouette_samples with the Euclidean
metric).  Nothing here imports sklearn."""
import ctypes as C
import math

import numpy as np
import torch

from ._lib import lib, check
from .gmm import _device_of, _rows_f32


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def argmax_labels(scores, out=None):
    """labels [n] int32 on the device: the first index of the largest score of every row of the device f32 matrix `scores` [n][K]
    (a row-strided view is read where it is) -- np.argmax's rule, exact ties included.  Only enqueues."""
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and (scores.shape[1] == 1 or scores.stride(1) == 1)
    n, K = scores.shape
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=scores.device)
    assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == n
    with torch.cuda.device(scores.device):
        check(lib.dmvae_argmax_labels(_stream(scores.device), scores.data_ptr(), max(scores.stride(0), K), n, K, out.data_ptr()), "dmvae_argmax_labels")
    return out


def silhouette_enqueue(Z, labels, n_clusters):
    """dmvae_silhouette on the current stream for device tensors Z [n][D] f32 (unit column stride) and labels [n] int32; returns the
    device tensors (samples [n] f32, out [2] f64 = (sum of the samples, non-empty clusters), flag [1] int32) without a synchronisation"""
    assert Z.is_cuda and Z.dtype == torch.float32 and Z.dim() == 2 and (Z.shape[1] == 1 or Z.stride(1) == 1)
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == Z.shape[0]
    dev, (n, D) = Z.device, Z.shape
    nbytes = lib.dmvae_silhouette_ws_bytes(n, int(n_clusters))
    if nbytes < 0:
        check(int(nbytes), "dmvae_silhouette_ws_bytes")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    samples = torch.empty(n, dtype=torch.float32, device=dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dmvae_silhouette(_stream(dev), Z.data_ptr(), max(Z.stride(0), D), n, D, labels.data_ptr(), int(n_clusters), ws.data_ptr(), ws.numel(),
                                   samples.data_ptr(), out.data_ptr(), flag.data_ptr()), "dmvae_silhouette")
    return samples, out, flag


def _host_labels(labels):
    """labels given as an array (not a device tensor): int64 on the host, or None"""
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        return None
    return np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int64).reshape(-1)


def _check_range(host, K):
    if host is not None and len(host) and (host.min() < 0 or host.max() >= K):
        raise IndexError("silhouette: a label outside [0, %d)" % K)


def _prepare(Z, labels, n_clusters):
    dev = _device_of(Z if isinstance(Z, torch.Tensor) else labels)
    host = _host_labels(labels)
    if n_clusters is None:
        n_clusters = int(host.max() if host is not None else labels.max().item()) + 1
    _check_range(host, n_clusters)
    Zd = _rows_f32(Z, dev)
    ld = (torch.as_tensor(host.astype(np.int32)) if host is not None else labels).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
    if ld.numel() != Zd.shape[0]:
        raise ValueError("labels must hold one entry per row of Z: %d != %d" % (ld.numel(), Zd.shape[0]))
    return Zd, ld, int(n_clusters)


def _raise_flag(flag, K):
    if int(flag.item()):
        raise IndexError("silhouette: a label outside [0, %d)" % K)


def silhouette_samples(Z, labels, n_clusters=None):
    """s_i of every row as a device f32 [n] (sklearn.metrics.silhouette_samples, Euclidean).  Z [n][D] and labels [n] are device
    tensors, or arrays that are uploaded; n_clusters: an upper bound K on the labels (default: their maximum + 1).  A label outside
    [0, K) raises IndexError."""
    Zd, ld, K = _prepare(Z, labels, n_clusters)
    samples, _, flag = silhouette_enqueue(Zd, ld, K)
    _raise_flag(flag, K)
    return samples


def _check_number_of_clusters(used, n):
    if not 2 <= used <= n - 1:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % used)


def silhouette_score(Z, labels, n_clusters=None):
    """the mean of the samples as a float (sklearn.metrics.silhouette_score): ValueError unless 2 <= non-empty clusters <= n - 1,
    IndexError for a label outside [0, n_clusters).  Labels given as an array are checked on the host before anything is uploaded."""
    host = _host_labels(labels)
    if host is not None:
        if n_clusters is not None:
            _check_range(host, int(n_clusters))
        _check_number_of_clusters(len(np.unique(host)), len(host))
    Zd, ld, K = _prepare(Z, labels, n_clusters)
    _, out, flag = silhouette_enqueue(Zd, ld, K)
    total, used = out.cpu().tolist()
    _raise_flag(flag, K)
    _check_number_of_clusters(int(used), Zd.shape[0])
    return total / Zd.shape[0]


def _entropy(counts, n):
    c = counts[counts > 0].astype(np.float64)
    return float(-np.sum((c / n) * (np.log(c) - math.log(n))))


def scores_from_confusion(conf):
    """dict(acc, nmi, ari, purity) of an integer confusion matrix conf[cluster][class] (square or not; empty rows and columns are
    clusters / classes nobody is in).  acc: the Hungarian-matched accuracy (includes.utils.accuracy_from_confusion); nmi: mutual
    information over the arithmetic mean of the two entropies, natural log, 1.0 when both partitions are one group, 0.0 when the
    information is 0; ari: the adjusted Rand index from the pair counts in Python ints, 1.0 when no pair is split by either side
    alone; purity: sum over clusters of the largest class count / N."""
    from includes.utils import accuracy_from_confusion
    d = np.asarray(conf)
    if d.ndim != 2 or not np.issubdtype(d.dtype, np.integer) or (d < 0).any():
        raise ValueError("conf must be a 2-D matrix of non-negative integer counts")
    d = d.astype(np.int64)
    n = int(d.sum())
    if n == 0:
        raise ValueError("conf counts no row")
    R = max(d.shape)
    sq = np.zeros((R, R), dtype=np.int64)
    sq[:d.shape[0], :d.shape[1]] = d
    acc = float(accuracy_from_confusion(sq, n))
    rows, cols = d.sum(axis=1), d.sum(axis=0)            # cluster sizes, class sizes
    purity = float(d.max(axis=1).sum()) / n
    used_rows, used_cols = int((rows > 0).sum()), int((cols > 0).sum())

    if used_rows == 1 and used_cols == 1:
        nmi = 1.0
    elif used_rows == 1 or used_cols == 1:
        nmi = 0.0
    else:
        i, j = np.nonzero(d)
        v = d[i, j].astype(np.float64)
        outer = (rows[i] * cols[j]).astype(np.float64)
        mi = float(np.sum((v / n) * (np.log(v) - math.log(n)) + (v / n) * (2.0 * math.log(n) - np.log(outer))))
        mi = max(mi, 0.0)
        nmi = 0.0 if mi == 0.0 else mi / (0.5 * (_entropy(rows, n) + _entropy(cols, n)))

    sum_sq = sum(int(x) * int(x) for x in d[d > 0].ravel())
    rr, cc = sum(int(x) * int(x) for x in rows), sum(int(x) * int(x) for x in cols)
    tp = sum_sq - n                                      # ordered pairs: together in both
    fp = rr - sum_sq                                     # together in the cluster, apart in the class
    fn = cc - sum_sq                                     # together in the class, apart in the cluster
    tn = n * n - fp - fn - sum_sq
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    return dict(acc=acc, nmi=float(nmi), ari=float(ari), purity=purity)
