"""Shared by tests/test_mixture_density_host.py, tests/test_gpu_mixture_density.py and tests/test_gpu_posterior_diagnostics_model.py: the
definitions of the posterior diagnostics (include/dmvae_hip.h) in float64, a sequential-float32 yardstick of the
mixture log-density in the style of trained_latents.direct, the per-point error bar, and the cases of the GPU tests.

  logpdf(Z, mu, lv, log_w)        l_i = logsumexp_j (log_w_j - 1/2 sum_d ((z_id - mu_jd)^2 exp(-lv_jd) + lv_jd)) - (D/2) log 2 pi; log_w None = -log J
  bar(Z, mu, lv, log_w)           2^-24 [ (D + 5 + max |lv|) sum_j w_ij (Q_ij / 2 + 1/2 sum_d |lv_jd|) + 8 (|l_i| + 1) ], from the oracle's own
                                  responsibilities w_ij and quadratic forms Q_ij:  a sum of D non-negative rounded terms has relative error
                                  <= (D + 3) u, u = 2^-24; exp(-lv) carries (|lv| + 2) u; the error of a logsumexp is the responsibility-weighted
                                  mean of its terms' errors; a few u for exp, log and the final add.  No point is excluded.
  yardstick(Z, mu, lv, log_w)     the difference form in float32, every sum over d and over j SEQUENTIAL, exp / log as the kernels take them
  expanded(Z, mu, lv, log_w)      the same with the square expanded (z^2 s - 2 z mu s + mu^2 s): what the bar refuses on the floor kind
  sample(mean, lv, eps)           z = mean + exp(lv / 2) eps,  a = -1/2 sum_d (eps^2 + lv) - (D/2) log 2 pi
  diagnostics(...)                mi, marginal_kl, rate, mi_cap, the per-dimension vectors and the active units"""
import functools
import math

import numpy as np

import trained_latents as TL

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
LOG_2PI = math.log(2.0 * math.pi)
r32 = TL.r32


# ------------------------------------------------------------------------------------------------------------------ float64 definitions
def _terms(Z, mu, lv, log_w):
    Z, mu, lv = (np.asarray(a, f64) for a in (Z, mu, lv))
    J = mu.shape[0]
    Q = np.empty((Z.shape[0], J))
    for lo in range(0, J, 4096):                                  # [M][chunk][D] at a time
        e = Z[:, None, :] - mu[None, lo:lo + 4096]
        Q[:, lo:lo + 4096] = np.sum(e * e * np.exp(-lv[lo:lo + 4096])[None], axis=2)
    lw = np.full(J, -math.log(J)) if log_w is None else np.asarray(log_w, f64)
    t = lw[None] - 0.5 * Q - 0.5 * lv.sum(axis=1)[None]
    return Q, t


def _lse(t):
    m = t.max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(np.isfinite(m), np.log(np.sum(np.exp(t - np.where(np.isfinite(m), m, 0.0)[:, None]), axis=1)) + m, -np.inf)
    return s


def logpdf(Z, mu, lv, log_w=None):
    _, t = _terms(Z, mu, lv, log_w)
    return _lse(t) - 0.5 * np.shape(mu)[1] * LOG_2PI


def logpdf_and_bar(Z, mu, lv, log_w=None):
    """(l [M], bar [M]); a point whose components all have weight 0 has l = -inf and bar = 0: it is compared exactly"""
    Q, t = _terms(Z, mu, lv, log_w)
    D = np.shape(mu)[1]
    l = _lse(t)
    fin = np.isfinite(l)
    with np.errstate(invalid="ignore"):
        w = np.where(fin[:, None], np.exp(t - np.where(fin, l, 0.0)[:, None]), 0.0)
    l = l - 0.5 * D * LOG_2PI
    lv = np.asarray(lv, f64)
    cost = 0.5 * Q + 0.5 * np.abs(lv).sum(axis=1)[None]
    b = U * ((D + 5 + np.abs(lv).max()) * np.sum(w * cost, axis=1) + 8.0 * (np.abs(np.where(fin, l, 0.0)) + 1.0))
    return l, np.where(fin, b, 0.0)


def bar(Z, mu, lv, log_w=None):
    return logpdf_and_bar(Z, mu, lv, log_w)[1]


def sample(mean, lv, eps):
    mean, lv, eps = (np.asarray(a, f64) for a in (mean, lv, eps))
    return mean + np.exp(lv / 2) * eps, -0.5 * np.sum(eps * eps + lv, axis=1) - 0.5 * mean.shape[1] * LOG_2PI


def column_stats(mean, lv):
    mean, lv = np.asarray(mean, f64), np.asarray(lv, f64)
    return mean.mean(axis=0), mean.var(axis=0), np.exp(lv).mean(axis=0)


def subsample_rows(N, M):
    return (np.arange(M, dtype=np.int64) * N) // M


def diagnostics(mean, lv, pm, plv, z, a, au_threshold=0.01):
    """the reported quantities for the points z [M][D] with a_i = log q(z_i | x_i) given, against ALL rows of (mean, lv) and the K prior rows;
    also m, p and the per-point bars of both log-densities"""
    m, bm = logpdf_and_bar(z, mean, lv)
    p, bp = logpdf_and_bar(z, pm, plv)
    a = np.asarray(a, f64)
    _, vm, mv = column_stats(mean, lv)
    return dict(mi=float(np.mean(a - m)), marginal_kl=float(np.mean(m - p)), rate=float(np.mean(a - p)), mi_cap=math.log(len(mean)),
                active_units=int(np.count_nonzero(vm > au_threshold)), var_of_mean=vm, mean_of_var=mv, m=m, p=p, bar_m=bm, bar_p=bp)


# ------------------------------------------------------------------------------------------------------------------ float32 restatements
def yardstick(Z, mu, lv, log_w=None, form="difference"):
    A = TL._Arith(f32)
    Z, mu, lv = (np.asarray(a).astype(f32) for a in (Z, mu, lv))
    (M, D), J = Z.shape, mu.shape[0]
    iv = A.exp(-lv)
    h = f32(0.5)
    if form == "difference":
        def term(d):
            e = Z[:, d, None] - mu[None, :, d]
            return (e * e) * iv[None, :, d]
    else:
        def term(d):
            return (Z[:, d, None] * Z[:, d, None]) * iv[None, :, d] - (f32(2.0) * Z[:, d, None]) * (mu[None, :, d] * iv[None, :, d]) + ((mu[:, d] * mu[:, d]) * iv[:, d])[None]
    Q = A.seq(D, term)
    sl = A.seq(D, lambda d: lv[:, d])
    lw = np.full(J, f32(-math.log(J)), f32) if log_w is None else np.asarray(log_w).astype(f32)
    t = (lw - h * sl)[None] - h * Q
    m = t.max(axis=1)
    with np.errstate(invalid="ignore"):
        ex = np.where(np.isfinite(m)[:, None], A.exp(t - m[:, None]), f32(0.0)).astype(f32)
    s = A.seq(J, lambda j: ex[:, j])
    out = A.log(s) + m - f32(0.5 * D * LOG_2PI)
    return np.where(np.isfinite(m), out, -np.inf).astype(f64)


expanded = functools.partial(yardstick, form="expanded")


# ------------------------------------------------------------------------------------------------------------------ the cases of the GPU tests
# (M, J, D, ld): the smallest shapes that reach every path of csrc/mixture_density.hip -- one point and one component; a ragged point group, ld > D;
# exactly one full tile of 16 points x 256 components; one past it on both sides (two point groups, a second tile of ONE component, J split in 2);
# D = 10 (one ragged chunk), 64 (four full chunks), 130 (nine chunks, the last of 2 columns); five tiles for one point group (split in 5); twenty
# tiles (split in 20: the J split happens whenever ceil(M / 16) < 1024 and J > 256); many point groups against few components; and 1025 point
# groups against two tiles: NO split (ceil(M / 16) >= 1024), a thread walks both tiles itself
SHAPES = [(1, 1, 1, 1), (17, 5, 3, 5), (16, 256, 4, 4), (33, 257, 4, 4), (37, 300, 10, 10), (20, 130, 64, 64), (9, 70, 130, 130), (5, 1030, 2, 2),
          (3, 5000, 8, 8), (700, 12, 33, 33), (16390, 300, 2, 2)]
REGIMES = ("mild", "separated", "floor")


def regimes_of(shape):
    """the trained_latents kinds need what they plant: floor has 8 dead dimensions and 4 rows on a collapsed cluster (D > 8, J >= 8); the
    largest shape runs in the mild regime only (its oracle is 10^7 pair-dimensions per regime)"""
    M, J, D, _ = shape
    if M > 4096:
        return ("mild",)
    return tuple(r for r in REGIMES if r != "floor" or (D > TL.N_DEAD and J >= 8))


def shape_id(shape, regime, weights):
    return "%dx%dx%d-ld%d-%s-%s" % (shape + (regime, weights))


@functools.lru_cache(maxsize=None)
def case(shape, regime, weights):
    """dict(Z [M][D], mu, lv [J][D], log_w [J] or None, ref [M], bar [M]); every input float32-representable float64"""
    M, J, D, _ = shape
    rng = np.random.RandomState(7 * M + 3 * J + D + 1000 * REGIMES.index(regime))
    if regime == "mild":
        mu, lv = rng.randn(J, D), math.sqrt(0.5) * rng.randn(J, D)
    else:
        K = max(1, min(10, J // 3))
        c = TL.case(J, D, K, regime, seed=int(rng.randint(1 << 30)))
        mu, lv = c["mean"], c["lv"]
    mu, lv = r32(mu), r32(lv)
    rows = rng.permutation(J)[np.arange(M) % J]                   # every point is a sample of one component's Gaussian
    Z = r32(mu[rows] + np.exp(lv[rows] / 2) * rng.randn(M, D))
    log_w = None
    if weights == "given":
        w = rng.gamma(1.0, size=J) + 1e-3
        log_w = r32(np.log(w / w.sum()))
    ref, b = logpdf_and_bar(Z, mu, lv, log_w)
    return dict(Z=Z, mu=mu, lv=lv, log_w=log_w, ref=ref, bar=b)


CASES = [(s, r, w) for s in SHAPES for r in regimes_of(s) for w in ("uniform", "given")]
