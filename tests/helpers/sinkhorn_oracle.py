"""float64 oracle of the Sinkhorn divergence (csrc/sinkhorn.hip, dmvae_hip/sinkhorn.py), straight from the definitions: the softmin pass
  out_i = -eps logsumexp_j (log_b_j + g_j / eps - d2_ij / eps),     d2 the squared Euclidean distance,
the log-domain solver on the eps-scaling schedule and S_eps = OT(a, b) - OT(a, a) / 2 - OT(b, b) / 2.  Every result comes with an error bar
for an f32 device computation, formed from the oracle's own quantities (never from what a device returned).  No geomloss, no ot, no sklearn,
nothing of the package."""
import numpy as np

U = 2.0 ** -24           # the unit roundoff of f32
ANNEAL = 0.7
BAR_CAP = 1e-4           # a pass bar above BAR_CAP (|out| + eps) would be too slack to catch a wrong kernel: asserted on every case handed out
END_CAP = 2e-2           # the same for the end-to-end bar of a divergence, against (|S| + eps): it sums some 200 pass bars of potentials that may cancel
LSE_CONST = 8.0          # the constant of the running-logsumexp bar (the posterior diagnostics' mixture density): exp, f64 sum, log, final rounding


def pair_d2(X, Y):
    """d2 [N][M] in float64 from the differences (no norm expansion), in row chunks"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    out = np.empty((len(X), len(Y)))
    step = max(1, (1 << 22) // max(1, len(Y) * X.shape[1]))
    for s in range(0, len(X), step):
        e = X[s:s + step, None, :] - Y[None, :, :]
        out[s:s + step] = np.einsum("ijc,ijc->ij", e, e)
    return out


def softmin_d2(d2, D, eps, g=None, log_b=None, prev=None, cap=BAR_CAP):
    """(out [N], bar [N]) of one softmin pass over the cost matrix d2 [N][M] of rows of width D.  With w_ij the softmax weights of t_i.,
    L_i = logsumexp_j t_ij and u = 2^-24:
      bar_i = eps u [ sum_j w_ij ((D + 6) d2_ij / eps + 2 |h_j| + |t_ij|) + 8 (|L_i| + 1) ] + u |out_i|
    -- the distance contract's (D + 3) u with the rounding of 1 / eps and the fma; forming h_j; the rounding of t; the running logsumexp
    (f32 exponential, f64 sum, log, final rounding).  cap: the bar is asserted to stay below cap (|out_i| + eps) (the solver's own passes
    switch this off -- a potential may cancel to nothing against its cost -- and the divergence asserts END_CAP on their sum).  With prev the device writes (prev + raw) / 2 rounded once: half the bracket, and
    u |out_i| of what it writes.  A column with h_j = -inf has no weight; a row whose columns are all empty: (+inf, 0)."""
    eps = float(eps)
    N, M = d2.shape
    h = (np.full(M, -np.log(M)) if log_b is None else np.asarray(log_b, dtype=np.float64)) + (0.0 if g is None else np.asarray(g, dtype=np.float64) / eps)
    live = h > -np.inf
    if not live.any():
        return np.full(N, np.inf), np.zeros(N)
    hl, dl = h[live], d2[:, live]
    t = hl[None, :] - dl / eps
    mx = t.max(axis=1)
    ex = np.exp(t - mx[:, None])
    se = ex.sum(axis=1)
    L, w = mx + np.log(se), ex / se[:, None]
    raw = -eps * L
    bracket = (w * ((D + 6.0) * dl / eps + 2.0 * np.abs(hl)[None, :] + np.abs(t))).sum(axis=1) + LSE_CONST * (np.abs(L) + 1.0)
    out = raw if prev is None else 0.5 * (np.asarray(prev, dtype=np.float64) + raw)
    bar = (1.0 if prev is None else 0.5) * eps * U * bracket + U * np.abs(out)
    assert cap is None or np.all(bar <= cap * (np.abs(out) + eps)), "the bar of this case is too slack: %g" % float(np.max(bar / (np.abs(out) + eps)))
    return out, bar


def softmin(X, Y, eps, g=None, log_b=None, prev=None):
    """(out, bar) of the pass for rows X [N][D] against Y [M][D]"""
    return softmin_d2(pair_d2(X, Y), np.shape(X)[1], eps, g, log_b, prev)


def scale_and_mean_cost(X, Y):
    """(4 x the sum of the column variances of the pooled rows, the mean squared distance over all pairs)"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    return 4.0 * float(np.concatenate([X, Y]).var(axis=0).sum()), float(pair_d2(X, Y).mean())


def schedule(scale, eps):
    """the annealing values above eps, rounded to f32"""
    out, e = [], max(float(scale), float(eps))
    while e > eps:
        out.append(float(np.float32(e)))
        e *= ANNEAL
    return out


def _weights(log_w, n):
    return np.full(n, 1.0 / n) if log_w is None else np.exp(np.asarray(log_w, dtype=np.float64))


def _run(step, w, anneal, eps, iters, tol, max_iter):
    """step(eps_t) -> (old, new); exactly `iters` iterations at eps, or (iters None) until the residual, looked at after EVERY iteration, is
    <= tol or max_iter are done.  (iterations with the annealing ones, the last residual)"""
    for e in anneal:
        step(e)
    k, err = 0, np.inf
    while k < (max_iter if iters is None else iters):
        old, new = step(eps)
        k += 1
        err = float(np.sum(np.where(w > 0, w * np.abs(1.0 - np.exp((old - new) / eps)), 0.0)))
        if iters is None and err <= tol:
            break
    return len(anneal) + k, err


def solve_pair(X, Y, log_a, log_b, anneal, eps, iters=None, tol=1e-4, max_iter=500):
    """dict(f, g, n_iter, err, bar) of OT_eps(a, b) by alternating updates from g = 0; bar: the sum over every pass run of its largest row
    bar -- softmin is 1-Lipschitz in the sup norm with respect to its potential, so no potential is further from the device's than that"""
    C, D = pair_d2(X, Y), np.shape(X)[1]
    CT = np.ascontiguousarray(C.T)
    st = dict(f=None, g=None, bar=0.0)

    def step(e):
        f, bf = softmin_d2(C, D, e, st["g"], log_b, cap=None)
        g, bg = softmin_d2(CT, D, e, f, log_a, cap=None)
        old = np.zeros(len(g)) if st["g"] is None else st["g"]
        st.update(f=f, g=g, bar=st["bar"] + float(bf.max()) + float(bg.max()))
        return old, g

    n, err = _run(step, _weights(log_b, len(CT)), anneal, eps, iters, tol, max_iter)
    return dict(f=st["f"], g=st["g"], n_iter=n, err=err, bar=st["bar"])


def solve_self(X, log_a, anneal, eps, iters=None, tol=1e-4, max_iter=500):
    """dict(p, n_iter, err, bar) of OT_eps(a, a): p <- (p + softmin(p)) / 2 from p = 0, then one plain pass (not counted)"""
    C, D = pair_d2(X, X), np.shape(X)[1]
    st = dict(p=np.zeros(len(C)), bar=0.0)

    def step(e):
        p, b = softmin_d2(C, D, e, st["p"], log_a, prev=st["p"], cap=None)
        old = st["p"]
        st.update(p=p, bar=st["bar"] + float(b.max()))
        return old, p

    n, err = _run(step, _weights(log_a, len(C)), anneal, eps, iters, tol, max_iter)
    p, b = softmin_d2(C, D, eps, st["p"], log_a, cap=None)
    return dict(p=p, n_iter=n, err=err, bar=st["bar"] + float(b.max()))


def divergence(X, Y, eps, scale, iters=None, tol=1e-4, max_iter=500, log_a=None, log_b=None, real_groups=None, fake_groups=None):
    """The Sinkhorn divergence and its parts on the schedule of (scale, eps); eps is taken as it comes (callers pass the f32 value).
    iters: the three iteration counts at eps (a, b), (a, a), (b, b), or None for the tol rule.  bar: the end-to-end bar on the divergence,
    twice the (a, b) problem's sum of pass bars plus the two symmetric problems' (the weights sum to 1)."""
    eps = float(eps)
    anneal = schedule(scale, eps)
    it = (None, None, None) if iters is None else iters
    ab = solve_pair(X, Y, log_a, log_b, anneal, eps, it[0], tol, max_iter)
    aa = solve_self(X, log_a, anneal, eps, it[1], tol, max_iter)
    bb = solve_self(Y, log_b, anneal, eps, it[2], tol, max_iter)
    a, b = _weights(log_a, len(aa["p"])), _weights(log_b, len(bb["p"]))
    dot = lambda w, v: np.where(w > 0, w * v, 0.0)
    rt, ft = dot(a, ab["f"] - aa["p"]), dot(b, ab["g"] - bb["p"])
    res = dict(divergence=float(rt.sum() + ft.sum()), ot=float(dot(a, ab["f"]).sum() + dot(b, ab["g"]).sum()), ot_real=float(2 * dot(a, aa["p"]).sum()),
               ot_fake=float(2 * dot(b, bb["p"]).sum()), eps=eps, n_iter=(ab["n_iter"], aa["n_iter"], bb["n_iter"]), err=(ab["err"], aa["err"], bb["err"]),
               real_terms=rt, fake_terms=ft, potentials=(ab["f"], ab["g"], aa["p"], bb["p"]), bars=(ab["bar"], aa["bar"], bb["bar"]),
               bar=2.0 * ab["bar"] + aa["bar"] + bb["bar"])
    assert res["bar"] <= END_CAP * (abs(res["divergence"]) + eps), "the end-to-end bar of this case is too slack: %g" % res["bar"]
    for name, groups, terms, w in (("real", real_groups, rt, a), ("fake", fake_groups, ft, b)):
        if groups is not None:
            gi = np.asarray(groups).astype(np.int64)
            s, m = np.bincount(gi, weights=terms), np.bincount(gi, weights=w)
            res["per_%s_group" % name] = s
            with np.errstate(invalid="ignore", divide="ignore"):
                res["mean_per_%s_group" % name] = np.where(m > 0, s / m, np.nan)
    return res


def plan(X, Y, f, g, eps, log_a=None, log_b=None):
    """the dense transport plan P_ij = a_i b_j exp((f_i + g_j - d2_ij) / eps) of a pair of potentials"""
    a, b = _weights(log_a, len(f)), _weights(log_b, len(g))
    return a[:, None] * b[None, :] * np.exp((np.asarray(f)[:, None] + np.asarray(g)[None, :] - pair_d2(X, Y)) / float(eps))
