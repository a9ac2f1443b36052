"""Sample quality on the device (dmvae_prdc_counts of include/dmvae_hip.h, csrc/prdc.hip): improved precision and recall (Kynkaanniemi
et al. 2019) and density and coverage (Naeem et al. 2020) of generated rows against real rows.  All pairs, no N x M array stored, the
distance of dmvae_hip.knn -- d2 = sum_c (r_c - f_c)^2 in f32 differences, c ascending, fused multiply-adds -- and the k-th-neighbour radii
from dmvae_knn itself, SQUARED, balls CLOSED (d2 <= r2: the papers' definition; the `prdc` package's < differs at exact ties only).
Every count is an integer, so two calls agree bit for bit.  Nothing here imports sklearn or the prdc package."""
import numpy as np
import torch

from ._lib import lib, check
from .gmm import _device_of, _rows_f32
from .knn import MAX_K, _int32_vector, _ld, _stream, knn_enqueue

NOISE_STREAM = 7         # the Philox stream id of get_sample_quality's draws (ids 0 .. 6 are taken)


def philox_normal(n, seed, step=0, stream_id=NOISE_STREAM, device=None):
    """n standard normals of the Philox stream (seed, step, stream_id) as a device f32 tensor (dmvae_philox_normal)"""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty(int(n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dmvae_philox_normal(_stream(dev), out.data_ptr(), out.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF,
                                      int(stream_id)), "dmvae_philox_normal")
    return out


def radii_enqueue(X, k):
    """the squared distance of every row of X (device f32 [n][D]) to its k-th nearest OTHER row, f32 [n] on the device: column k - 1 of
    dmvae_knn(X, X, k, self_first=0).  Only enqueues.  ValueError unless 1 <= k <= min(256, n - 1)."""
    n, k = X.shape[0], int(k)
    if not 1 <= k <= min(MAX_K, n - 1):
        raise ValueError("k = %d: 1 <= k <= min(%d, the %d rows - 1)" % (k, MAX_K, n))
    return knn_enqueue(X, X, k, self_first=0)[1][:, k - 1].contiguous()


def counts_enqueue(R, F, rR2, rF2):
    """dmvae_prdc_counts on the current stream for device tensors R [N][D], F [M][D] (f32, unit column stride) and their squared radii rR2
    [N], rF2 [M] (f32, contiguous): (fake_in_real int32 [M], real_in_fake int32 [N], real_min_d2 f32 [N], real_min_j int32 [N]) without a
    synchronisation."""
    assert R.is_cuda and F.is_cuda and R.dtype == F.dtype == torch.float32 and R.dim() == F.dim() == 2
    (N, D), (M, Df), dev = R.shape, F.shape, R.device
    if D != Df:
        raise ValueError("real and generated rows differ in width: %d != %d" % (D, Df))
    for r, n in ((rR2, N), (rF2, M)):
        assert r.is_cuda and r.dtype == torch.float32 and r.is_contiguous() and r.dim() == 1 and r.numel() == n
    fake_in_real = torch.empty(M, dtype=torch.int32, device=dev)
    real_in_fake = torch.empty(N, dtype=torch.int32, device=dev)
    real_min_d2 = torch.empty(N, dtype=torch.float32, device=dev)
    real_min_j = torch.empty(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dmvae_prdc_counts(_stream(dev), R.data_ptr(), _ld(R), N, F.data_ptr(), _ld(F), M, D, rR2.data_ptr(), rF2.data_ptr(),
                                    fake_in_real.data_ptr(), real_in_fake.data_ptr(), real_min_d2.data_ptr(), real_min_j.data_ptr()), "dmvae_prdc_counts")
    return fake_in_real, real_in_fake, real_min_d2, real_min_j


def _groups(v, n, dev, what, G=None):
    """(the groups as an int64 device vector, their number): the number is taken on the host where the groups come from there; a device
    vector without a given number costs one small read"""
    if G is None and not isinstance(v, torch.Tensor):
        G = int(np.max(np.asarray(v))) + 1
    g = _int32_vector(v, dev)
    if g.numel() != n:
        raise ValueError("%s must hold one entry per row: %d != %d" % (what, g.numel(), n))
    return g.long(), (int(g.max().item()) + 1 if G is None else int(G))


def prdc_enqueue(R, F, k, real_groups=None, fake_groups=None, n_real_groups=None, n_fake_groups=None):
    """everything prdc() reads back, as ONE int64 device vector, and how to cut it: (flat, layout).  Only enqueues (_groups: unless a device vector of
    groups comes without their number)."""
    rR2, rF2 = radii_enqueue(R, k), radii_enqueue(F, k)
    fake_in_real, real_in_fake, real_min_d2, _ = counts_enqueue(R, F, rR2, rF2)
    precise, recalled, covered = fake_in_real > 0, real_in_fake > 0, real_min_d2 <= rR2
    parts = [("precision", precise.sum().reshape(1)), ("recall", recalled.sum().reshape(1)),
             ("density", fake_in_real.sum(dtype=torch.int64).reshape(1)), ("coverage", covered.sum().reshape(1))]
    dev = R.device
    # per group: integer index_add_ (order-free; a masked index or torch.bincount would synchronise for its output's size)
    gsum = lambda g, G, v: torch.zeros(G, dtype=torch.int64, device=dev).index_add_(0, g, v.to(torch.int64))
    if real_groups is not None:
        g, G = _groups(real_groups, R.shape[0], dev, "real_groups", n_real_groups)
        parts += [("real_group_rows", gsum(g, G, torch.ones_like(g))), ("coverage_per_group", gsum(g, G, covered)), ("recall_per_group", gsum(g, G, recalled))]
    if fake_groups is not None:
        g, G = _groups(fake_groups, F.shape[0], dev, "fake_groups", n_fake_groups)
        parts += [("fake_group_rows", gsum(g, G, torch.ones_like(g))), ("precision_per_group", gsum(g, G, precise)), ("density_per_group", gsum(g, G, fake_in_real))]
    return torch.cat([p.to(torch.int64) for _, p in parts]), [(name, p.numel()) for name, p in parts]


def prdc_from(flat, layout, N, M, k):
    """the dict of prdc() from prdc_enqueue's vector: one synchronising copy, the divisions in Python floats (a group without rows: nan)"""
    host, cut, o = flat.cpu().tolist(), {}, 0
    for name, n in layout:
        cut[name] = host[o:o + n]
        o += n
    res = dict(precision=cut["precision"][0] / M, recall=cut["recall"][0] / N, density=cut["density"][0] / (k * M), coverage=cut["coverage"][0] / N, k=k)
    ratio = lambda num, den, scale=1: [a / (scale * b) if b else float("nan") for a, b in zip(num, den)]
    if "real_group_rows" in cut:
        res["coverage_per_group"] = ratio(cut["coverage_per_group"], cut["real_group_rows"])
        res["recall_per_group"] = ratio(cut["recall_per_group"], cut["real_group_rows"])
    if "fake_group_rows" in cut:
        res["precision_per_group"] = ratio(cut["precision_per_group"], cut["fake_group_rows"])
        res["density_per_group"] = ratio(cut["density_per_group"], cut["fake_group_rows"], k)
    return res


def prdc(real, fake, k=5, real_groups=None, fake_groups=None):
    """dict(precision, recall, density, coverage, k) of the generated rows `fake` [M][D] against the real rows `real` [N][D], with rX2 the
    squared distance of a row to its k-th nearest other row of its own set and closed balls:
      precision = #{j : some i has d2(i, j) <= rR2[i]} / M        recall   = #{i : some j has d2(i, j) <= rF2[j]} / N
      density   = sum_j #{i : d2(i, j) <= rR2[i]} / (k M)         coverage = #{i : min_j d2(i, j) <= rR2[i]} / N
    real_groups (int [N], e.g. the classes) adds coverage_per_group and recall_per_group, fake_groups (int [M], e.g. the mixture component a
    row was drawn from) precision_per_group and density_per_group: lists over the groups 0 .. max, each the same ratio within the group (nan
    for a group without rows).  Device tensors (row-strided f32 views included) are used where they lie; arrays are uploaded.  Two self-kNNs
    and one pairs kernel; every sum is an integer sum on the device, one copy comes back, the divisions are Python floats.  ValueError
    unless 1 <= k <= min(256, N - 1, M - 1)."""
    dev = _device_of(real if isinstance(real, torch.Tensor) and real.is_cuda else fake)
    R, F = _rows_f32(real, dev), _rows_f32(fake, dev)
    flat, layout = prdc_enqueue(R, F, k, real_groups, fake_groups)
    return prdc_from(flat, layout, R.shape[0], F.shape[0], int(k))
