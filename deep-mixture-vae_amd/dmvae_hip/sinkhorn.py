"""Sinkhorn divergence on the device (dmvae_sinkhorn_softmin of include/dmvae_hip.h, csrc/sinkhorn.hip): the debiased entropic
optimal-transport cost S_eps (Feydy et al. 2019; Genevay et al. 2018) between two weighted row sets, cost C_ij = d2(x_i, y_j) -- the distance of
dmvae_hip.knn, no 1/2 factor, so S_eps -> W_2^2 as eps -> 0.  The solver works in the log domain on potentials; every pass over the pairs is
one launch of the softmin kernel and no N x M array is stored.  Nothing here imports geomloss, ot or sklearn."""
import numpy as np
import torch

from ._lib import lib, check
from .gmm import _device_of, _rows_f32
from .knn import _ld, _stream
from .prdc import _groups

ANNEAL = 0.7             # eps-scaling: eps_{t+1} = ANNEAL eps_t
GROUP_CHUNK = 64         # groups summed per masked reduction


def _vec(v, n, dev, what):
    """an optional f32 device vector of n entries, contiguous"""
    if v is None:
        return None
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(v, dtype=np.float32)).reshape(-1))
    t = t.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    if t.numel() != n:
        raise ValueError("%s must hold one entry per row: %d != %d" % (what, t.numel(), n))
    return t


def softmin_enqueue(X, Y, eps, g=None, log_b=None, prev=None, out=None):
    """dmvae_sinkhorn_softmin on the current stream for device tensors X [N][D], Y [M][D] (f32, unit column stride):
      out_i = -eps logsumexp_j (log_b_j + g_j / eps - d2(x_i, y_j) / eps)      f32 [N] on the device,
    or (prev_i + that) / 2 with prev given.  g, log_b (f32 [M]) and prev (f32 [N]) are contiguous device vectors or None (zeros, the uniform
    -log M, no averaging); out is written where given (it must not be g or prev: other workgroups still read them).  eps is rounded to f32.
    One launch, no synchronisation."""
    assert X.is_cuda and Y.is_cuda and X.dtype == Y.dtype == torch.float32 and X.dim() == Y.dim() == 2
    (N, D), (M, Dy), dev = X.shape, Y.shape, X.device
    if D != Dy:
        raise ValueError("the two row sets differ in width: %d != %d" % (D, Dy))
    for v, n in ((g, M), (log_b, M), (prev, N), (out, N)):
        assert v is None or (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.dim() == 1 and v.numel() == n)
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=dev)
    p = lambda v: None if v is None else v.data_ptr()
    with torch.cuda.device(dev):
        check(lib.dmvae_sinkhorn_softmin(_stream(dev), X.data_ptr(), _ld(X), N, Y.data_ptr(), _ld(Y), M, D, p(g), p(log_b), float(eps), p(prev),
                                         out.data_ptr()), "dmvae_sinkhorn_softmin")
    return out


def schedule(scale, eps):
    """the annealing values above eps, each rounded to f32: eps_0 = max(scale, eps), eps_{t+1} = 0.7 eps_t (in float64) while above eps"""
    out, e = [], max(float(scale), float(eps))
    while e > eps:
        out.append(float(np.float32(e)))
        e *= ANNEAL
    return out


def _mass(log_w, n, dev):
    """the weights in float64: exp(log_w), or 1 / n"""
    return torch.full((n,), 1.0 / n, dtype=torch.float64, device=dev) if log_w is None else torch.exp(log_w.double())


def _residual(w, old, new, eps):
    """sum_j w_j |1 - exp((old_j - new_j) / eps)| in float64, a device scalar; a row without mass adds nothing"""
    r = torch.abs(1.0 - torch.exp((old.double() - new.double()) / eps))
    return torch.where(w > 0, w * r, torch.zeros_like(r)).sum()


def _iterate(step, w, anneal, eps, tol, max_iter, check_every):
    """runs step(eps_t) -> (old, new) once per annealing value, then at eps until the residual of its pair is <= tol or max_iter iterations
    at eps are done; the residual is read every check_every iterations (never with tol = 0) and taken, unread, at the last.
    Returns (iterations run, annealing included; the last residual as a device scalar)."""
    for e in anneal:
        step(e)
    err = None
    for k in range(1, max_iter + 1):
        old, new = step(eps)
        look = tol > 0 and k % check_every == 0
        if look or k == max_iter:
            err = _residual(w, old, new, eps)
            if look and float(err.item()) <= tol:
                break
    return len(anneal) + k, err


def solve_pair(X, Y, log_a, log_b, anneal, eps, tol=0.0, max_iter=100, check_every=5):
    """OT_eps between the rows X (log-weights log_a or None) and Y (log_b or None): alternating f <- softmin_Y(g), g <- softmin_X(f) from g = 0.
    (f [N], g [M], iterations, residual as a device scalar); the residual is sum_j b_j |1 - exp((g_j - g_j^new) / eps)|."""
    dev, N, M = X.device, X.shape[0], Y.shape[0]
    f = torch.empty(N, dtype=torch.float32, device=dev)
    gs = [None, torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev)]      # (null: zeros)

    def step(e):
        softmin_enqueue(X, Y, e, g=gs[0], log_b=log_b, out=f)
        new = gs[2] if gs[0] is gs[1] else gs[1]
        softmin_enqueue(Y, X, e, g=f, log_b=log_a, out=new)
        old, gs[0] = gs[0], new
        return (torch.zeros_like(new) if old is None else old), new

    n, err = _iterate(step, _mass(log_b, M, dev), anneal, eps, tol, max_iter, check_every)
    return f, gs[0], n, err


def solve_self(X, log_a, anneal, eps, tol=0.0, max_iter=100, check_every=5):
    """OT_eps of the rows X with themselves, one potential: p <- (p + softmin_X(p)) / 2 from p = 0, then ONE plain pass p <- softmin_X(p)
    (not counted).  (p [N], iterations, residual as a device scalar: sum_i a_i |1 - exp((p_i - p_i^new) / eps)| of the last averaged update)."""
    dev, N = X.device, X.shape[0]
    ps = [torch.zeros(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev)]

    def step(e):
        softmin_enqueue(X, X, e, g=ps[0], log_b=log_a, prev=ps[0], out=ps[1])
        ps.reverse()
        return ps[1], ps[0]

    n, err = _iterate(step, _mass(log_a, N, dev), anneal, eps, tol, max_iter, check_every)
    return softmin_enqueue(X, X, eps, g=ps[0], log_b=log_a, out=ps[1]), n, err


def scale_and_mean_cost(X, Y):
    """device float64 [2]: (4 x the sum of the column variances of the pooled rows -- the population variance over the N + M rows; the mean
    squared distance over all pairs, mean |x|^2 + mean |y|^2 - 2 <mean x, mean y>), from float64 torch ops; rows are not weighted"""
    N, M = X.shape[0], Y.shape[0]
    xd, yd = X.double(), Y.double()
    mx, my, ex2, ey2 = xd.mean(dim=0), yd.mean(dim=0), (xd * xd).sum() / N, (yd * yd).sum() / M
    pooled = (N * mx + M * my) / (N + M)
    var = (N * ex2 + M * ey2) / (N + M) - (pooled * pooled).sum()
    return torch.stack([4.0 * var, ex2 + ey2 - 2.0 * (mx * my).sum()])


def _group_sums(g, G, v):
    """float64 [G]: the sum of v (float64 [n]) over the rows of each group.  A masked reduction, a fixed order: two calls give the same bits
    (index_add_ on the device is a float atomic, whose order changes from call to call)"""
    out = []
    for g0 in range(0, G, GROUP_CHUNK):
        ids = torch.arange(g0, min(G, g0 + GROUP_CHUNK), device=g.device)
        out.append(torch.where(g[:, None] == ids[None, :], v[:, None], torch.zeros((), dtype=v.dtype, device=v.device)).sum(dim=0))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.float64, device=g.device)


def _rows_of(x):
    return tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)


def sinkhorn_divergence(real, fake, eps=None, eps_rel=0.05, tol=1e-4, max_iter=500, check_every=5, real_groups=None, fake_groups=None, log_a=None,
                        log_b=None, n_real_groups=None, n_fake_groups=None):
    """The Sinkhorn divergence between the rows `real` [N][D] (weights a) and `fake` [M][D] (weights b), cost d2 (squared Euclidean, no 1/2):
      S_eps = OT_eps(a, b) - OT_eps(a, a) / 2 - OT_eps(b, b) / 2 = sum_i a_i (f_i - p_i) + sum_j b_j (g_j - q_j)
    with (f, g) the potentials of OT_eps(a, b) and p, q those of the two symmetric problems.  It is 0 when the two measures coincide, positive
    otherwise, and tends to the squared 2-Wasserstein distance as eps -> 0.  Weights are uniform unless log_a / log_b (f32 [N] / [M], the LOG
    of a probability vector, -inf for a row without mass; their normalisation is not checked) are given.
    eps: the entropic regularisation in squared-distance units; None: eps_rel x the mean squared distance over all pairs, mean |x|^2 + mean |y|^2
    - 2 <mean x, mean y>.  eps is rounded to f32, and so is every value handed to the kernel.  eps-scaling: one iteration at each of eps_0 =
    max(scale, eps), 0.7 eps_0, ... above eps, scale = 4 x the sum of the column variances of the pooled rows (float64 on the device; it and the
    default eps come back in one small read).  Then at eps until the marginal residual is <= tol or max_iter iterations at eps are done:
    err = sum_j b_j |1 - exp((g_j - g_j^new) / eps)| for (a, b), the same over p for a symmetric problem (update p <- (p + softmin(p)) / 2, ended
    by one plain pass).  The residual is read every check_every iterations -- the loops' only synchronisation; tol = 0 runs exactly max_iter
    iterations at eps and reads nothing inside the loop.
    Returns dict(divergence, ot, ot_real, ot_fake -- the three OT_eps values <a, f> + <b, g>, 2 <a, p>, 2 <b, q> --, eps, scale, n_iter and err
    -- 3-tuples over the problems (a, b), (a, a), (b, b), iterations with the annealing ones included --, real_terms = a_i (f_i - p_i) and
    fake_terms = b_j (g_j - q_j) as device f32 tensors, potentials = (f, g, p, q)).  The terms add up to the divergence (summed in float64 on
    the device); SINGLE TERMS MAY BE NEGATIVE -- only their sum is a divergence.  real_groups (int [N], e.g. the classes) adds per_real_group --
    the sums of real_terms over the groups 0 .. max (0.0 for a group without rows) -- and mean_per_real_group, each sum divided by the group's
    mass (nan for a group without mass); fake_groups (int [M], e.g. the mixture component a row was drawn from) per_fake_group and
    mean_per_fake_group.  The per-group sums of both sides add up to the divergence.  n_real_groups / n_fake_groups: the number of groups where
    the caller knows it (a device vector of groups without it costs one small read).
    Device tensors (row-strided f32 views included) are used where they lie; arrays are uploaded.  ValueError on rows of different width,
    eps <= 0 (or eps_rel <= 0 with eps None), tol < 0, max_iter < 1, check_every < 1, weights or groups of the wrong length."""
    (N, D), (M, Df) = _rows_of(real), _rows_of(fake)
    if D != Df:
        raise ValueError("real and generated rows differ in width: %d != %d" % (D, Df))
    if N < 1 or M < 1:
        raise ValueError("both sets need a row: %d, %d" % (N, M))
    if eps is not None and not (float(eps) > 0 and np.isfinite(eps)):
        raise ValueError("eps = %r: finite and > 0" % (eps,))
    if eps is None and not (float(eps_rel) > 0 and np.isfinite(eps_rel)):
        raise ValueError("eps_rel = %r: finite and > 0" % (eps_rel,))
    if not tol >= 0:
        raise ValueError("tol = %r: tol >= 0" % (tol,))
    if int(max_iter) < 1 or int(check_every) < 1:
        raise ValueError("max_iter = %r, check_every = %r: both >= 1" % (max_iter, check_every))
    for v, n, what in ((real_groups, N, "real_groups"), (fake_groups, M, "fake_groups"), (log_a, N, "log_a"), (log_b, M, "log_b")):
        if v is not None and int(np.prod(_rows_of(v))) != n:
            raise ValueError("%s must hold one entry per row: %d != %d" % (what, int(np.prod(_rows_of(v))), n))
    tol, max_iter, check_every = float(tol), int(max_iter), int(check_every)

    dev = _device_of(real if isinstance(real, torch.Tensor) and real.is_cuda else fake)
    X, Y = _rows_f32(real, dev), _rows_f32(fake, dev)
    la, lb = _vec(log_a, N, dev, "log_a"), _vec(log_b, M, dev, "log_b")
    scale, mean_cost = scale_and_mean_cost(X, Y).cpu().tolist()                                  # the one read before the loops
    eps = float(np.float32(eps_rel * mean_cost if eps is None else eps))
    if not eps > 0:
        raise ValueError("eps = %r: all rows coincide; give eps" % (eps,))
    anneal = schedule(scale, eps)
    f, g, n0, e0 = solve_pair(X, Y, la, lb, anneal, eps, tol, max_iter, check_every)
    p, n1, e1 = solve_self(X, la, anneal, eps, tol, max_iter, check_every)
    q, n2, e2 = solve_self(Y, lb, anneal, eps, tol, max_iter, check_every)

    a, b = _mass(la, N, dev), _mass(lb, M, dev)
    dot = lambda w, v: torch.where(w > 0, w * v.double(), torch.zeros_like(w))                   # (a row without mass adds nothing)
    term = lambda w, u, v: torch.where(w > 0, w * (u.double() - v.double()), torch.zeros_like(w))
    real_terms, fake_terms = term(a, f, p).float(), term(b, g, q).float()
    rt, ft = real_terms.double(), fake_terms.double()
    parts = [("head", torch.stack([rt.sum() + ft.sum(), dot(a, f).sum() + dot(b, g).sum(), 2.0 * dot(a, p).sum(), 2.0 * dot(b, q).sum(), e0, e1, e2]))]
    for groups, n, G, terms, w, name in ((real_groups, N, n_real_groups, rt, a, "real"), (fake_groups, M, n_fake_groups, ft, b, "fake")):
        if groups is not None:
            gi, G = _groups(groups, n, dev, name + "_groups", G)
            parts += [(name + "_sum", _group_sums(gi, G, terms)), (name + "_mass", _group_sums(gi, G, w))]
    host, cut, o = torch.cat([v for _, v in parts]).cpu().tolist(), {}, 0                        # the one read after them
    for name, v in parts:
        cut[name] = host[o:o + v.numel()]
        o += v.numel()
    h = cut["head"]
    res = dict(divergence=h[0], ot=h[1], ot_real=h[2], ot_fake=h[3], eps=eps, scale=scale, n_iter=(n0, n1, n2), err=(h[4], h[5], h[6]),
               real_terms=real_terms, fake_terms=fake_terms, potentials=(f, g, p, q))
    for name in ("real", "fake"):
        if name + "_sum" in cut:
            res["per_%s_group" % name] = cut[name + "_sum"]
            res["mean_per_%s_group" % name] = [s / m if m > 0 else float("nan") for s, m in zip(cut[name + "_sum"], cut[name + "_mass"])]
    return res
