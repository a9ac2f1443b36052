"""float64 NumPy restatement of the held-out log-likelihood estimate of csrc/eval_loglik.hip: the importance-weighted bound of
Burda et al. (2016) with S draws on the marginal mixture prior (uniform over the K clusters),

    z_s = mean + exp(log_var / 2) eps_s
    w_s = log p(x | z_s) + log p(z_s) - log q(z_s | x)
    L   = logsumexp_s w_s - log S

Encoder and decoder are those of oracle/dmvae_oracle.py; the device noise is stream 4 of tests/helpers/philox_oracle.py.  Every
term keeps its D log 2 pi (the device drops the pair that cancels)."""
import numpy as np

import dmvae_oracle as O
import philox_oracle as PH

STREAM_LOGLIK = 4
LOG_2PI = np.log(2.0 * np.pi)


def logsumexp(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def log_q(eps, log_var):
    """log N(z; mean, exp(log_var)) at z = mean + exp(log_var / 2) eps -> [...]"""
    return -0.5 * np.sum(np.square(eps) + log_var + LOG_2PI, axis=-1)


def log_prior(Z, prior_means, prior_log_vars):
    """log 1/K sum_k N(z; mu_k, exp(lambda_k)),  Z [n, D] -> [n]"""
    dz = Z[:, None, :] - prior_means[None]
    u = -0.5 * np.sum(np.square(dz) * np.exp(-prior_log_vars)[None] + prior_log_vars[None] + LOG_2PI, axis=-1)
    return logsumexp(u, 1) - np.log(prior_means.shape[0])


def log_px(X, xlogits, input_type):
    """binary: minus the step's sigmoid cross-entropy; real: a unit-variance Gaussian.  Sums over the input_dim real columns."""
    l = xlogits
    if input_type == "binary":
        return np.sum(X * l - np.maximum(l, 0) - np.log1p(np.exp(-np.abs(l))), axis=1)
    if input_type == "real":
        return -0.5 * np.sum(np.square(X - l), axis=1) - 0.5 * X.shape[1] * LOG_2PI
    raise NotImplementedError(input_type)


def posterior(p, cfg, X):
    """(mean, log_var) of q(z | x): the DMVAE encoder's z head, or VaDE's two dense layers off the trunk (by the config's class)"""
    if isinstance(cfg, O.VadeConfig):
        a = O.vade_forward(p, cfg, X, np.zeros((X.shape[0], cfg.latent_dim)))
    else:
        a = O.encode(p, cfg, X)
    return a["mean"], a["logvar"]


def draw_terms(p, cfg, X, mean, log_var, eps_s):
    """(log p(x | z), log p(z), log q) of ONE draw, each [n]"""
    Z = O.gaussian_reparam(mean, log_var, eps_s)
    xl = O.decode(p, cfg, Z)["xlogits"]
    return log_px(X, xl, cfg.input_type), log_prior(Z, p["prior_means"], p["prior_log_vars"]), log_q(eps_s, log_var)


def weights(p, cfg, X, eps):
    """w [S, n] for eps [S, n, D]"""
    mean, log_var = posterior(p, cfg, X)
    out = []
    for e in np.asarray(eps, dtype=np.float64):
        lpx, lpz, lq = draw_terms(p, cfg, X, mean, log_var, e)
        out.append(lpx + lpz - lq)
    return np.stack(out)


def bound(w):
    """L [n] of w [S, n]: the direct form"""
    return logsumexp(w, 0) - np.log(w.shape[0])


def bound_running(w):
    """the same as the device keeps it: draw 0 initialises (max, scaled sum), every later draw updates them"""
    m, s = w[0].copy(), np.ones_like(w[0])
    for ws in w[1:]:
        up = ws > m
        s = np.where(up, s * np.exp(m - ws) + 1.0, s + np.exp(ws - m))
        m = np.where(up, ws, m)
    return m + np.log(s) - np.log(w.shape[0])


def row_ll(p, cfg, X, eps):
    return bound(weights(p, cfg, X, eps))


def device_eps(seed, counter, draws, n_rows, D, first=0, n=None):
    """eps [draws, n, D] the kernel draws without a host buffer: philox_normal_at((s * n_rows + first + r) * D + d) of stream
    (seed, step = counter, id 4) -- the row's position in the evaluated order, not the batch size"""
    n = n_rows - first if n is None else n
    s = np.arange(draws, dtype=np.uint64)[:, None, None]
    pos = np.arange(first, first + n, dtype=np.uint64)[None, :, None]
    d = np.arange(D, dtype=np.uint64)[None, None, :]
    return PH.normal_at(seed, counter, STREAM_LOGLIK, (s * np.uint64(n_rows) + pos) * np.uint64(D) + d)


def closed_form_parameters(p, mu0, lam0):
    """Parameters under which every importance weight equals log p(x) of the bias-only decoder: K identical prior rows (mu0, lam0),
    a posterior that IS that prior (W_mean = W_logvar = 0, b_mean = mu0, b_logvar = lam0) and a decoder that ignores z (first
    matrix zero).  Returns a modified copy."""
    q = {k: np.array(v, dtype=np.float64) for k, v in p.items()}
    K = q["prior_means"].shape[0]
    q["prior_means"] = np.tile(mu0, (K, 1))
    q["prior_log_vars"] = np.tile(lam0, (K, 1))
    q["W_mean"][:] = 0.0
    q["W_logvar"][:] = 0.0
    q["b_mean"] = np.array(mu0, dtype=np.float64)
    q["b_logvar"] = np.array(lam0, dtype=np.float64)
    q["W_dec0"][:] = 0.0
    return q


def bias_only_log_px(p, cfg, X):
    """log p(x) when the decoder's first matrix is zero: its logits do not depend on z"""
    xl = O.decode(p, cfg, np.zeros((X.shape[0], cfg.latent_dim)))["xlogits"]
    return log_px(X, xl, cfg.input_type)
