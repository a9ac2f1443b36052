"""Shared by tests/test_vade_large_host.py and tests/test_gpu_vade_large.py: the contractions of the large-table form of VaDE's
latent stage (csrc/latent_vade_mfma.hip) restated in NumPy float64 -- every (row, cluster, dimension) sum as a matrix product with
the squares expanded -- and the inputs the GPU tests run it on."""
import math

import numpy as np

import dmvae_oracle as O

f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)


def expanded(mean, lv, eps, pm, plv, r):
    """the stage as csrc/latent_vade_mfma.hip computes it: dict(Z, clv, w, kl_z, kl_c, G, du, gmu, glv, dpm, dplv)"""
    B, D = mean.shape
    K = pm.shape[0]
    ip, e = np.exp(-plv), np.exp(lv)
    z = mean + np.exp(lv / 2) * eps
    cl = eps / 2 * np.exp(lv / 2)
    c2, ck = np.sum(pm * pm * ip, axis=1), np.sum(plv, axis=1)
    T2 = np.concatenate([ip, -2 * pm * ip], axis=1)                    # [K][2D]
    T1 = np.concatenate([ip, pm * ip], axis=1)
    one = np.ones((B, 1))
    Xm = np.concatenate([e + mean ** 2, mean, one], axis=1)            # [B][2D + 1]
    Xz = np.concatenate([z ** 2, z, one], axis=1)
    S_mu = Xm[:, :2 * D] @ T2.T + c2
    S_z = Xz[:, :2 * D] @ T2.T + c2
    T = S_mu + ck - np.sum(lv, axis=1, keepdims=True) - D
    u = -0.5 * (S_z + ck)
    g = np.exp(u - u.max(1, keepdims=True))
    g /= g.sum(1, keepdims=True)
    G = r / B * (T / 2 + np.log(g + 1e-20) + g / (g + 1e-20) + math.log(K))
    du = g * (G - np.sum(g * G, axis=1, keepdims=True))
    AC, ACu = g @ T1, du @ T1
    A, C, Au, Cu = AC[:, :D], AC[:, D:], ACu[:, :D], ACu[:, D:]
    dzl = -(z * Au - Cu)
    gmu = r / B * (mean * A - C) + dzl
    glv = r / (2 * B) * (e * A - 1) + dzl * cl
    Gg, Gu = g.T @ Xm, du.T @ Xz
    Gg_e, Gg_mu, Wsum = Gg[:, :D], Gg[:, D:2 * D], Gg[:, 2 * D:]
    Gu_zz, Gu_z, Usum = Gu[:, :D], Gu[:, D:2 * D], Gu[:, 2 * D:]
    dpm = -r / B * ip * (Gg_mu - pm * Wsum) + ip * (Gu_z - pm * Usum)
    dplv = r / (2 * B) * (Wsum - ip * (Gg_e - 2 * pm * Gg_mu + pm ** 2 * Wsum)) + 0.5 * (ip * (Gu_zz - 2 * pm * Gu_z + pm ** 2 * Usum) - Usum)
    return dict(Z=z, clv=cl, w=g, kl_z=np.mean(np.sum(0.5 * g * T, axis=1)), kl_c=np.mean(np.sum(g * (np.log(g + 1e-20) + math.log(K)), axis=1)),
                G=G, du=du, gmu=gmu, glv=glv, dpm=dpm, dplv=dplv)


TABLE_SCALE = 2.0           # c of pm = randn c / sqrt(D): found on the CPU (0.5 .. 3 tried) so that at every shape of the GPU tests the median top responsibility stays <= 0.9 and max |du| >= 1e-3 max |G|


def scaled_tables(rng, D, K, c=TABLE_SCALE):
    """prior tables under which gamma is not one-hot at large D: pm = randn c / sqrt(D), plv = randn 0.4 / sqrt(D)"""
    return f32(rng.randn(K, D) * c / math.sqrt(D)), f32(rng.randn(K, D) * 0.4 / math.sqrt(D))


def latent_case(B, D, K, scaled=True, kl_ratio=0.6):
    """inputs (float32-representable, as float64) of one run of the stage and its float64 oracle results"""
    rng = np.random.RandomState(B + D + K)
    mean, lv, eps = f32(rng.randn(B, D) * 1.2), f32(rng.randn(B, D) * 0.5 - 0.2), f32(rng.randn(B, D))
    pm, plv = scaled_tables(rng, D, K) if scaled else (f32(rng.randn(K, D)), f32(rng.randn(K, D) * 0.4))
    cfg = O.VadeConfig(4, D, K, (4,), (4,))
    a = dict(mean=mean, logvar=lv, eps=eps, Z=O.gaussian_reparam(mean, lv, eps), kl_ratio=kl_ratio)
    a["w"] = O.cluster_probs(a["Z"], pm, plv)
    _, _, dpm, dplv, gmu2, glv2 = O.vade_latent_backward(cfg, a, dict(prior_means=pm, prior_log_vars=plv), np.zeros_like(mean))
    klz = O.kl_mixture_exact(mean, lv, a["w"], pm, plv)
    klc = np.mean(np.sum(a["w"] * (np.log(a["w"] + 1e-20) + np.log(K)), axis=1))
    return dict(B=B, D=D, K=K, kl_ratio=kl_ratio, mean=mean, lv=lv, eps=eps, pm=pm, plv=plv, Z=a["Z"], w=a["w"], kl_z=klz, kl_c=klc,
                gmu=gmu2, glv=glv2, dpm=dpm, dplv=dplv)


def gamma_is_soft(mean, lv, eps, pm, plv, r):
    """the condition on the inputs, on the oracle's side: (median over rows of max_k gamma, max |du|, max |G|)"""
    x = expanded(mean, lv, eps, pm, plv, r)
    w = O.cluster_probs(O.gaussian_reparam(mean, lv, eps), pm, plv)
    return float(np.median(w.max(1))), float(np.abs(x["du"]).max()), float(np.abs(x["G"]).max())


def assert_gamma_is_soft(mean, lv, eps, pm, plv, r):
    med, du, G = gamma_is_soft(mean, lv, eps, pm, plv, r)
    assert med <= 0.9, med                       # the responsibilities are not one-hot ...
    assert du >= 1e-3 * G, (du, G)               # ... so the path through gamma carries gradient


STEP_KW = dict(input_dim=40, latent_dim=256, n_classes=12, enc_layers=(70, 50), dec_layers=(50, 30, 60))


def step_inputs(B, kw=STEP_KW, seed=1):
    """a batch, its noise and scaled prior tables for a whole VaDE step at a large latent width"""
    rng = np.random.RandomState(seed)
    X = (rng.rand(B, kw["input_dim"]) * (rng.rand(B, kw["input_dim"]) < 0.3)).astype(np.float32)
    eps = rng.randn(B, kw["latent_dim"]).astype(np.float32)
    pm, plv = scaled_tables(rng, kw["latent_dim"], kw["n_classes"])
    return X, eps, pm, plv


EVAL_KW = dict(input_dim=40, latent_dim=256, n_classes=10, enc_layers=(70, 50), dec_layers=(50, 30, 60))
EVAL_SEED = 5               # chosen on the CPU: the oracle's near-tie rows stay within the 2 % the test allows
EVAL_GAP = 1e-4


def eval_inputs(N, n, draws, kw=EVAL_KW, seed=EVAL_SEED):
    rng = np.random.RandomState(seed)
    X = (rng.rand(N, kw["input_dim"]) * (rng.rand(N, kw["input_dim"]) < 0.4)).astype(np.float32)
    cls = rng.randint(0, kw["n_classes"] + 2, N)
    order = rng.permutation(N)
    eps = rng.randn(draws, n, kw["latent_dim"]).astype(np.float32)
    pm, plv = scaled_tables(rng, kw["latent_dim"], kw["n_classes"])
    return X, cls, order, eps, pm, plv


def eval_oracle(p, kw, Xrows, eps):
    """averaged responsibilities of the draws eps [k][n][D] (float64) and which rows have a clear arg-max"""
    cfg = O.VadeConfig(kw["input_dim"], kw["latent_dim"], kw["n_classes"], kw["enc_layers"], kw["dec_layers"])
    a = O.vade_forward(p, cfg, Xrows.astype(np.float64), np.zeros((len(Xrows), kw["latent_dim"])))
    gam = np.stack([O.cluster_probs(O.gaussian_reparam(a["mean"], a["logvar"], e.astype(np.float64)), p["prior_means"], p["prior_log_vars"]) for e in eps])
    want = gam.mean(0)
    top = np.sort(want, axis=1)
    return want, (top[:, -1] - top[:, -2]) >= EVAL_GAP
