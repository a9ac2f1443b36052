"""Shared by tests/test_trained_latents_host.py and tests/test_gpu_trained_latents.py: inputs of the latent stage in the regime a
trained model lives in (prior tables from a Gaussian-mixture fit with small variances, posterior means on top of one cluster mean,
one-hot q(c|x) and gamma), the float64 oracle on them, and two float32 restatements of the stage on the CPU -- the yardsticks every
tolerance of those tests is defined against:

  direct(c, mode, ft=f32)      the algebra of csrc/latent_body.h (modes "exact", "relaxed") and csrc/latent_vade.hip ("vade"):
                               differences, then squares
  expanded(c, mode, ft=f32)    the algebra of csrc/latent_mfma.hip ("exact") and csrc/latent_vade_mfma.hip ("vade"): the squares expanded
                               into [x^2 | x] . [ip | -2 pm ip]^T + c2

With ft = float32 every sum over d, over k and over the batch is a SEQUENTIAL float32 accumulation (a Python loop over the contracted
index, vectorised over the rest): the worst typical order; the kernels' blocked and sliced orders should do no worse.  exp and log are
taken as the kernels take them (__expf(x) = exp2(fl(x log2 e)), __logf(x) = fl(log2 x) ln 2): the rounding of the argument is part of
the float32 algebra.  With ft = float64 the same code is the algebra in float64 (direct_f64 / expanded_f64 of the host test).

tolerance(name, oracle, yard): atol = max(t_abs, 2 max |yard - oracle|), rtol = t_rel, with (t_rel, t_abs) of
tests/test_gpu_kernels.py::test_latent_fwd_matches_oracle.  The factor 2 is the only margin: the kernel's order of additions is not the
yardstick's, and two runs of one float32 algebra in different orders differ by about the error of either."""
import functools
import math

import numpy as np

import dmvae_oracle as O

f32, f64 = np.float32, np.float64
r32 = lambda a: np.asarray(a).astype(f32).astype(f64)
E0 = 1e-20
KL_RATIO = 0.6
KINDS = ("separated", "competing", "floor", "vanishing")
SIG = dict(separated=0.3, competing=0.3, floor=0.15, vanishing=0.3)     # cluster sigma per kind.  floor: found on the CPU (0.1, 0.15, 0.2, 0.3 tried): at 0.2 the median top responsibility
                                                                            # at (100, 10, 10) falls to 0.976, at 0.1 five outputs of the (64, 512, 256) VaDE case miss the non-vacuity bound, at 0.15 one does
SPREAD = 1.0
FLOOR_VAR = 1e-6            # sklearn's reg_covar: what a dead dimension and a collapsed cluster are left with
N_DEAD, N_COLLAPSED_ROWS, N_VANISHING_ROWS = 8, 4, 4
GUMBEL_ATOM = -math.log(float(f32(1e-20)))          # the largest value oracle.sample_gumbel can return: U = 0


# ------------------------------------------------------------------------------------------------------------------ inputs
def _u(z, pm, plv):
    """VaDE's scores u_bk = -1/2 (sum_d (z - pm)^2 ip + sum_d plv), float64"""
    return -0.5 * (np.sum(np.square(z[:, None, :] - pm[None]) * np.exp(-plv)[None], axis=2) + np.sum(plv, axis=1)[None])


def top_two_gap(u):
    s = np.sort(u, axis=1)
    return s[:, -1] - s[:, -2]


def case(B, D, K, kind, seed):
    """float32-representable float64 arrays mean, lv, eps, logits, gumbel, pm, plv (and c: each row's cluster; comp: the rows moved between
    two clusters; vrows: the rows with vanishing probabilities)"""
    assert kind in KINDS
    rng = np.random.RandomState(seed)
    sig = SIG[kind]
    pm = rng.randn(K, D) * SPREAD
    plv = 2 * math.log(sig) + 0.3 * rng.randn(K, D)
    c = rng.randint(0, K, B)
    dead = np.zeros(D, bool)
    collapsed = -1
    if kind == "floor":
        dead[rng.choice(D, N_DEAD, replace=False)] = True
        collapsed = int(rng.randint(0, K))
        plv[collapsed] = math.log(FLOOR_VAR) + 0.3 * rng.randn(D)
        pm[:, dead], plv[:, dead] = 0.5, math.log(FLOOR_VAR)
        c[c == collapsed] = (collapsed + 1) % K
        c[rng.choice(B, N_COLLAPSED_ROWS, replace=False)] = collapsed
    noise = rng.randn(B, D) * np.exp(plv[c] / 2)
    mean = pm[c] + noise
    lv = plv[c] + 2 * math.log(0.5) + 0.3 * rng.randn(B, D)
    eps = rng.randn(B, D)
    logits = 12.0 * (np.arange(K)[None, :] == c[:, None]) + rng.randn(B, K)
    gumbel = O.sample_gumbel((B, K), rng)
    if kind == "floor":
        lv[:, dead] = math.log(FLOOR_VAR)         # (mean there is already 0.5 + 1e-3 randn: pm = 0.5, plv = log 1e-6)
    pm, plv, lv, eps = r32(pm), r32(plv), r32(lv), r32(eps)
    comp = np.zeros(B, bool)
    if kind in ("competing", "floor") and K > 1:
        # a quarter of the rows onto the segment between their cluster's mean and a second cluster's: position t by bisection on the float64
        # scores of the SAMPLE z = mean + exp(lv / 2) eps, so that u_c - u_c2 lands evenly in [0.5, 8] nats; the logits get the same gap
        rows = rng.permutation(np.flatnonzero(c != collapsed))[:max(B // 4, 1)]
        c2 = rng.randint(0, K, len(rows))
        while True:
            bad = (c2 == c[rows]) | (c2 == collapsed)
            if not bad.any():
                break
            c2[bad] = rng.randint(0, K, int(bad.sum()))
        want = 0.5 + 7.5 * (rng.permutation(len(rows)) + 0.5) / len(rows)
        step = pm[c2] - pm[c[rows]]
        two = np.arange(len(rows))

        def gap(t):
            m = r32(pm[c[rows]] + t[:, None] * step + noise[rows])
            u = _u(m + np.exp(lv[rows] / 2) * eps[rows], pm, plv)
            return u[two, c[rows]] - u[two, c2]
        lo, hi = np.zeros(len(rows)), np.ones(len(rows))
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            above = gap(mid) > want
            lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
        t = 0.5 * (lo + hi)
        mean[rows] = pm[c[rows]] + t[:, None] * step + noise[rows]
        got = gap(t)
        logits[rows, c2] = logits[rows, c[rows]] - got
        comp[rows] = True
    vrows = np.zeros(B, bool)
    if kind == "vanishing":
        rows = rng.choice(B, N_VANISHING_ROWS, replace=False)
        for b in rows:
            logits[b] = rng.permutation(np.linspace(-60.0, 60.0, K))
            gumbel[b, int(np.argmin(logits[b]))] = GUMBEL_ATOM
        vrows[rows] = True
    return dict(B=B, D=D, K=K, kind=kind, mean=r32(mean), lv=lv, eps=eps, logits=r32(logits), gumbel=r32(gumbel), pm=pm, plv=plv,
                c=c, comp=comp, vrows=vrows)


# ------------------------------------------------------------------------------------------------------------------ the float64 oracle
def oracle(c, mode, tau=1.0, r=KL_RATIO, q=None):
    """oracle/dmvae_oracle.py on the case: dict(Z, clv, w, klz, klc, gmu, glv, dlogits (DMVAE only), dpm, dplv; VaDE: u).  q: another softmax(logits)
    to carry through the gradient (the vanishing rows: q = 0 where float32 has it 0)"""
    mean, lv, eps, pm, plv = c["mean"], c["lv"], c["eps"], c["pm"], c["plv"]
    K = c["K"]
    Z = O.gaussian_reparam(mean, lv, eps)
    out = dict(Z=Z, clv=eps * 0.5 * np.exp(lv / 2))
    p = dict(prior_means=pm, prior_log_vars=plv)
    if mode == "vade":
        cfg = O.VadeConfig(4, c["D"], K, (4,), (4,))
        w = O.cluster_probs(Z, pm, plv)
        a = dict(mean=mean, logvar=lv, eps=eps, Z=Z, kl_ratio=r, w=w)
        _, _, dpm, dplv, gmu, glv = O.vade_latent_backward(cfg, a, p, np.zeros_like(mean))
        out.update(w=w, gmu=gmu, glv=glv, dpm=dpm, dplv=dplv, klz=O.kl_mixture_exact(mean, lv, w, pm, plv),
                   klc=float(np.mean(np.sum(w * (np.log(w + E0) + np.log(K)), axis=1))), u=_u(Z, pm, plv))
        return out
    cfg = O.Config(4, c["D"], K)
    qq = O.softmax(c["logits"]) if q is None else q
    a = dict(mean=mean, logvar=lv, eps=eps, q=qq, kl_ratio=r, temperature=tau, mode=mode)
    a["w"] = qq if mode == "exact" else O.gumbel_softmax(c["logits"], c["gumbel"], tau)
    gmu, glv, dlogits, dpm, dplv = O.latent_backward(cfg, a, p, np.zeros_like(mean))
    klz = (O.kl_mixture_exact if mode == "exact" else O.kl_mixture_relaxed)(mean, lv, a["w"], pm, plv)
    out.update(w=a["w"], gmu=gmu, glv=glv, dlogits=dlogits, dpm=dpm, dplv=dplv, klz=klz, klc=O.kl_categorical(c["logits"], K), q=qq)
    return out


# ------------------------------------------------------------------------------------------------------------------ the restatements
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


class _Arith:
    """one float type: exp / log as the kernels take them, sums in sequence"""

    def __init__(self, ft):
        self.ft = ft
        self.fast = ft is f32

    def exp(self, x):
        if self.fast:
            return np.exp2((x * f32(LOG2E)).astype(f64)).astype(f32)
        return np.exp(x)

    def log(self, x):
        with np.errstate(divide="ignore"):
            if self.fast:
                return np.log2(x.astype(f64)).astype(f32) * f32(LN2)
            return np.log(x)

    def seq(self, n, term):
        """sum_i term(i), one addition after another"""
        acc = term(0).astype(self.ft)
        for i in range(1, n):
            acc = acc + term(i)
        assert acc.dtype == self.ft
        return acc

    def seq_rows(self, row):
        """sum over the batch of one value per row"""
        return self.seq(len(row), lambda b: row[b])

    def softmax(self, x):
        ex = self.exp(x - x.max(1, keepdims=True))
        se = self.seq(x.shape[1], lambda k: ex[:, k])
        return ex / se[:, None]


def _setup(c, ft, r):
    A = _Arith(ft)
    mean, lv, eps, pm, plv = (c[k].astype(ft) for k in ("mean", "lv", "eps", "pm", "plv"))
    B, D, K = c["B"], c["D"], c["K"]
    rB = ft(r) * ft(f32(1.0 / B) if ft is f32 else 1.0 / B)
    e, sd = A.exp(lv), A.exp(ft(0.5) * lv)
    z, cl = mean + sd * eps, eps * ft(0.5) * sd
    ck = A.seq(D, lambda d: plv[:, d])
    rl = A.seq(D, lambda d: lv[:, d])
    return A, mean, lv, eps, pm, plv, B, D, K, rB, ft(0.5) * rB, A.log(np.asarray(K, ft)), e, z, cl, A.exp(-plv), ck, rl


def _finish(ft, **out):
    for k, v in out.items():
        assert np.asarray(v).dtype == ft or k == "u", (k, np.asarray(v).dtype)          # (u of the large-table form: double, as in the kernel)
    return {k: (float(v) if np.ndim(v) == 0 else np.asarray(v, f64)) for k, v in out.items()}


def _dq(A, q, rB, logK, floorless=False):
    ft = A.ft
    with np.errstate(invalid="ignore", divide="ignore"):
        lg = A.log(q) if floorless else A.log(q + ft(E0))
        return lg, rB * (lg + q / (q + ft(E0)) + logK)


def direct(c, mode, tau=1.0, r=KL_RATIO, ft=f32):
    A, mean, lv, eps, pm, plv, B, D, K, rB, rB2, logK, e, z, cl, ip, ck, rl = _setup(c, ft, r)
    h, one = ft(0.5), ft(1.0)
    if mode == "vade":
        su = A.seq(D, lambda d: np.square(z[:, d, None] - pm[None, :, d]) * ip[None, :, d])
        stt = A.seq(D, lambda d: (e[:, d, None] + np.square(mean[:, d, None] - pm[None, :, d])) * ip[None, :, d])
        u = -h * (su + ck[None])
        T = ck[None] - rl[:, None] - ft(D) + stt
        g = A.softmax(u)
        lg = A.log(g + ft(E0))
        G = rB * (h * T + lg + g / (g + ft(E0)) + logK)
        sgG = A.seq(K, lambda k: g[:, k] * G[:, k])
        du = g * (G - sgG[:, None])
        klz = A.seq_rows(A.seq(K, lambda k: h * g[:, k] * T[:, k]))
        klc = A.seq_rows(A.seq(K, lambda k: g[:, k] * (lg[:, k] + logK)))
        gm = A.seq(K, lambda k: g[:, k, None] * (mean - pm[k]) * ip[k])
        Ak = A.seq(K, lambda k: g[:, k, None] * ip[k])
        dzl = A.seq(K, lambda k: -(du[:, k, None] * (z - pm[k]) * ip[k]))
        dpm = A.seq(B, lambda b: -rB * g[b, :, None] * (mean[b] - pm) * ip + du[b, :, None] * (z[b] - pm) * ip)
        dplv = A.seq(B, lambda b: rB2 * g[b, :, None] * (one - (e[b] + np.square(mean[b] - pm)) * ip) + du[b, :, None] * h * (np.square(z[b] - pm) * ip - one))
        return _finish(ft, Z=z, clv=cl, w=g, klz=klz / ft(B), klc=klc / ft(B), gmu=rB * gm + dzl, glv=rB2 * (e * Ak - one) + dzl * cl, dpm=dpm, dplv=dplv, u=u)
    logits = c["logits"].astype(ft)
    q = A.softmax(logits)
    lg, dq = _dq(A, q, rB, logK)
    klc = A.seq_rows(A.seq(K, lambda k: q[:, k] * (lg[:, k] + logK)))
    s_qdq = A.seq(K, lambda k: q[:, k] * dq[:, k])
    if mode == "exact":
        w = q
        S = A.seq(D, lambda d: (e[:, d, None] + np.square(mean[:, d, None] - pm[None, :, d])) * ip[None, :, d])
        t = S + ck[None] - rl[:, None] - ft(D)
        klz = A.seq_rows(A.seq(K, lambda k: h * w[:, k] * t[:, k]))
        gm = A.seq(K, lambda k: w[:, k, None] * (mean - pm[k]) * ip[k])
        Ak = A.seq(K, lambda k: w[:, k, None] * ip[k])
        gmu, glv = rB * gm, rB2 * (e * Ak - one)
        dw, wscale = rB2 * t, one
        dpm = -rB * ip * A.seq(B, lambda b: w[b, :, None] * (mean[b] - pm))
        dplv = rB2 * A.seq(B, lambda b: w[b, :, None] * (one - (e[b] + np.square(mean[b] - pm)) * ip))
    else:
        w = A.softmax((logits + c["gumbel"].astype(ft)) / ft(tau))
        bm = A.seq(K, lambda k: w[:, k, None] * pm[k])
        bl = A.seq(K, lambda k: w[:, k, None] * plv[k])
        ib, diff = A.exp(-bl), mean - bm
        gmu, glv = rB * diff * ib, rB2 * (e * ib - one)
        integ = A.seq(D, lambda d: bl[:, d] - lv[:, d] - one + (e[:, d] + diff[:, d] * diff[:, d]) * ib[:, d])
        klz = A.seq(B, lambda b: h * integ[b])
        dbm, dbl = -gmu, rB2 * (one - (e + diff * diff) * ib)
        dw = A.seq(D, lambda d: dbm[:, d, None] * pm[None, :, d] + dbl[:, d, None] * plv[None, :, d])
        wscale = one / ft(tau)
        dpm = A.seq(B, lambda b: w[b, :, None] * dbm[b])
        dplv = A.seq(B, lambda b: w[b, :, None] * dbl[b])
    s_wdw = A.seq(K, lambda k: w[:, k] * dw[:, k])
    dl = q * (dq - s_qdq[:, None]) + wscale * w * (dw - s_wdw[:, None])
    return _finish(ft, Z=z, clv=cl, w=w, klz=klz / ft(B), klc=klc / ft(B), gmu=gmu, glv=glv, dlogits=dl, dpm=dpm, dplv=dplv, q=q)


CORRUPTIONS = ("no_c2", "pm_next", "drop64", "log_no_floor")


def expanded(c, mode, r=KL_RATIO, ft=f32, corrupt=None):
    """corrupt: one of CORRUPTIONS -- the kernel's algebra with one mistake in it (the host test: the tolerance sees each)"""
    assert mode in ("exact", "vade") and corrupt in (None,) + CORRUPTIONS
    A, mean, lv, eps, pm, plv, B, D, K, rB, rB2, logK, e, z, cl, ip, ck, rl = _setup(c, ft, r)
    h, one, two = ft(0.5), ft(1.0), ft(2.0)
    if mode == "vade":
        # the origin of every expanded product (csrc/latent_vade_mfma.hip: vade_origin_kernel): m0_d = sum_k w pm / sum_k w, w = ip^2 relative to
        # the dimension's largest -- the point that makes the GEMM operand column (pm - m0) ip smallest in the least-squares sense
        wk = A.exp(two * (plv.min(0, keepdims=True) - plv))
        m0 = A.seq(K, lambda k: wk[k] * pm[k]) / A.seq(K, lambda k: wk[k])
        mean, z0, pm = mean - m0[None], z, pm - m0[None]
        z = z - m0[None]
    c2 = A.seq(D, lambda d: pm[:, d] * pm[:, d] * ip[:, d])
    if corrupt == "no_c2":
        c2 = np.zeros_like(c2)
    pm2 = np.roll(pm, -1, axis=0) if corrupt == "pm_next" else pm
    T1 = np.concatenate([ip, pm * ip], axis=1)                      # [K][2D]
    T2 = np.concatenate([ip, -two * pm2 * ip], axis=1)
    n2 = 2 * D - (64 if corrupt == "drop64" else 0)
    floorless = corrupt == "log_no_floor"
    ones = np.ones((B, 1), ft)
    Xm = np.concatenate([e + mean * mean, mean, ones], axis=1)      # [B][2D + 1]
    S_mu = A.seq(n2, lambda j: Xm[:, j, None] * T2[None, :, j])
    if mode == "exact":
        q = A.softmax(c["logits"].astype(ft))
        lg, dq = _dq(A, q, rB, logK, floorless)
        klc = A.seq_rows(A.seq(K, lambda k: q[:, k] * (lg[:, k] + logK)))
        t = S_mu + c2[None] + ck[None] - rl[:, None] - ft(D)
        klz = A.seq_rows(A.seq(K, lambda k: h * q[:, k] * t[:, k]))
        AC = A.seq(K, lambda k: q[:, k, None] * T1[k])
        Ak, Ck = AC[:, :D], AC[:, D:]
        s_qdq = A.seq(K, lambda k: q[:, k] * dq[:, k])
        s_wdw = A.seq(K, lambda k: q[:, k] * (rB2 * t[:, k]))
        dl = q * (dq - s_qdq[:, None]) + q * (rB2 * t - s_wdw[:, None])
        Gm = A.seq(B, lambda b: q[b, :, None] * Xm[b])
        ge, gmm, wsum = Gm[:, :D], Gm[:, D:2 * D], Gm[:, 2 * D:]
        dpm = -rB * ip * (gmm - pm * wsum)
        dplv = rB2 * (wsum - ip * (ge - two * pm * gmm + pm * pm * wsum))
        return _finish(ft, Z=z, clv=cl, w=q, klz=klz / ft(B), klc=klc / ft(B), gmu=rB * (mean * Ak - Ck), glv=rB2 * (e * Ak - one), dlogits=dl, dpm=dpm, dplv=dplv, q=q)
    Xz = np.concatenate([z * z, z, ones], axis=1)
    S_z = A.seq(n2, lambda j: Xz[:, j, None] * T2[None, :, j])
    # the slabs of the scores, c2 and ck are added in double (csrc/latent_vade_mfma.hip: vade_score4)
    sm = S_mu.astype(f64) + c2.astype(f64)[None] + ck.astype(f64)[None]
    uz = S_z.astype(f64) + c2.astype(f64)[None] + ck.astype(f64)[None]
    T = sm.astype(ft) - (rl + ft(D))[:, None]
    u = -0.5 * uz
    ex = A.exp((u - u.max(1, keepdims=True)).astype(ft))
    g = ex / A.seq(K, lambda k: ex[:, k])[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        lg = A.log(g) if floorless else A.log(g + ft(E0))
        G = rB * (h * (T - T.min(1, keepdims=True)) + lg + g / (g + ft(E0)))
        sgG = A.seq(K, lambda k: g[:, k] * G[:, k])
        du = g * (G - sgG[:, None])
        klc = A.seq_rows(A.seq(K, lambda k: g[:, k] * (lg[:, k] + logK)))
    klz = A.seq_rows(A.seq(K, lambda k: h * g[:, k] * T[:, k]))
    AC = A.seq(K, lambda k: g[:, k, None] * T1[k])
    ACu = A.seq(K, lambda k: du[:, k, None] * T1[k])
    Ak, Ck, Au, Cu = AC[:, :D], AC[:, D:], ACu[:, :D], ACu[:, D:]
    dzl = -(z * Au - Cu)
    Gg = A.seq(B, lambda b: g[b, :, None] * Xm[b])
    Gu = A.seq(B, lambda b: du[b, :, None] * Xz[b])
    ge, gmm, wsum = Gg[:, :D], Gg[:, D:2 * D], Gg[:, 2 * D:]
    gzz, gz, usum = Gu[:, :D], Gu[:, D:2 * D], Gu[:, 2 * D:]
    dpm = -rB * ip * (gmm - pm * wsum) + ip * (gz - pm * usum)
    dplv = rB2 * (wsum - ip * (ge - two * pm * gmm + pm * pm * wsum)) + h * (ip * (gzz - two * pm * gz + pm * pm * usum) - usum)
    return _finish(ft, Z=z0, clv=cl, w=g, klz=klz / ft(B), klc=klc / ft(B), gmu=rB * (mean * Ak - Ck) + dzl, glv=rB2 * (e * Ak - one) + dzl * cl,
                   dpm=dpm, dplv=dplv, u=u)


direct_f32, direct_f64 = functools.partial(direct, ft=f32), functools.partial(direct, ft=f64)
expanded_f32, expanded_f64 = functools.partial(expanded, ft=f32), functools.partial(expanded, ft=f64)


# ------------------------------------------------------------------------------------------------------------------ the tolerance rule
# (t_rel, t_abs) per output: what tests/test_gpu_kernels.py::test_latent_fwd_matches_oracle applies to it; "/B": its atol is t_abs / B
T_REL_ABS = dict(Z=(2e-6, 2e-6, False), w=(1e-5, 1e-7, False), clv=(1e-5, 1e-6, False), gmu=(2e-4, 2e-5, True), glv=(2e-4, 2e-5, True),
                 dlogits=(5e-4, 5e-5, True), dpm=(2e-4, 1e-5, False), dplv=(2e-4, 1e-5, False), klz=(2e-5, 1e-5, False), klc=(2e-5, 1e-6, False))
MARGIN = 2.0
OUTPUTS = ("Z", "clv", "w", "klz", "klc", "gmu", "glv", "dlogits", "dpm", "dplv")


def yard_error(oracle_v, yard_v):
    return float(np.max(np.abs(np.asarray(yard_v, f64) - np.asarray(oracle_v, f64))))


def tolerance(name, oracle_v, yard_v):
    """(rtol, atol) of output `name`, given its float64 value and its yardstick value"""
    t_rel, t_abs, per_row = T_REL_ABS[name]
    if per_row:
        t_abs = t_abs / np.shape(oracle_v)[0]
    return t_rel, max(t_abs, MARGIN * yard_error(oracle_v, yard_v))


def within(name, got, oracle_v, yard_v):
    """does `got` meet tolerance(name, ...)?  -> (ok, max |got - oracle|, max |yard - oracle|)"""
    rtol, atol = tolerance(name, oracle_v, yard_v)
    got, ref = np.asarray(got, f64), np.asarray(oracle_v, f64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
        ok = bool(np.all(np.isfinite(got)) and np.all(err <= atol + rtol * np.abs(ref)))
    return ok, float(np.max(err)) if np.all(np.isfinite(got)) else float("inf"), yard_error(oracle_v, yard_v)


def u_error(u_oracle, u_yard):
    """max |u_yard - u_oracle| over the entries that decide the arg-max: each row's two best clusters in the oracle.  Over ALL entries the
    scores against a collapsed cluster would set it (kind floor: |u| ~ 1e7 there, one float32 ulp is a nat, and gamma is exactly 0); the
    restricted maximum is never the larger one, so never fewer rows are held to the oracle's arg-max."""
    top = np.argsort(u_oracle, axis=1)[:, -2:]
    return float(np.max(np.abs(np.take_along_axis(u_yard - u_oracle, top, axis=1))))


def clear_rows(u_oracle, u_yard):
    """rows whose oracle top-two gap is at least 4 max |u_yard - u_oracle|: the arg-max of gamma is the oracle's there"""
    return top_two_gap(u_oracle) >= 4.0 * u_error(u_oracle, u_yard)


# ------------------------------------------------------------------------------------------------------------------ the cases of the tests
# form -> (mode, yardstick, shapes, kinds, temperatures)
FORMS = dict(
    dmvae_exact=("exact", "direct", [(100, 10, 10), (130, 300, 50)], KINDS, (1.0,)),
    dmvae_relaxed=("relaxed", "direct", [(100, 10, 10), (130, 300, 50)], KINDS, (0.5, 0.1)),
    dmvae_mfma=("exact", "expanded", [(70, 96, 130), (128, 256, 50), (64, 512, 256)], KINDS, (1.0,)),
    vade=("vade", "direct", [(100, 10, 10), (70, 33, 3)], KINDS[:3], (1.0,)),
    vade_mfma_forced=("vade", "expanded", [(70, 96, 130)], KINDS[:3], (1.0,)),
    vade_mfma=("vade", "expanded", [(64, 256, 12), (64, 512, 256)], KINDS[:3], (1.0,)),
)
CASES = [(form, shape, kind, tau) for form, (_, _, shapes, kinds, taus) in FORMS.items() for shape in shapes for kind in kinds for tau in taus]
# the shapes at which both forms of a mode run: the cost of the expansion is printed there (never asserted)
BOTH_FORMS = [("exact", (130, 300, 50)), ("vade", (70, 33, 3))]
# (form, shape, kind, output) that the inputs are too harsh to test: 2 max |yard - oracle| is not below 1 % of max |oracle| there.  At most three.
# glv of VaDE's large-table form at (64, 512, 256), floor: 2 * 1.5e-2 against 1 % of 2.7 -- the yardstick's dZ_lat * clv term is sums of 256 products
# du (pm - m0) ip with ip ~ 44 added in sequence, on a glv whose largest entry is small
EXCLUDED = (("vade_mfma", (64, 512, 256), "floor", "glv"),)


# found on the CPU (shifts 0 .. 7 tried): with two live dimensions left of ten, the unshifted draw has max |du| = 1.3e-3 max |G| and a median
# top responsibility of 0.994, both next to their bounds; this one has 2.5e-3 and 0.9975
SEED_SHIFT = {((100, 10, 10), "floor"): 4}


def case_id(form, shape, kind, tau):
    return "%s-%dx%dx%d-%s%s" % (form, shape[0], shape[1], shape[2], kind, "" if tau == 1.0 else "-t%g" % tau)


def outputs_of(form, shape, kind):
    mode = FORMS[form][0]
    return [n for n in OUTPUTS if not (n == "dlogits" and mode == "vade") and (form, shape, kind, n) not in EXCLUDED]


@functools.lru_cache(maxsize=None)
def get_case(shape, kind):
    B, D, K = shape
    return case(B, D, K, kind, seed=1000 * KINDS.index(kind) + B + D + K + SEED_SHIFT.get((shape, kind), 0))


@functools.lru_cache(maxsize=None)
def get_oracle(shape, kind, mode, tau):
    return oracle(get_case(shape, kind), mode, tau)


@functools.lru_cache(maxsize=None)
def get_yard(shape, kind, mode, which, tau):
    c = get_case(shape, kind)
    return direct(c, mode, tau) if which == "direct" else expanded(c, mode)
