"""CPU tests of the held-out log-likelihood estimate (csrc/eval_loglik.hip; `train.py --loglik S`): the float64 oracle's own
identities, the new C entries and the host arithmetic of the scratch size."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import dmvae_oracle as O        # noqa: E402
import loglik_oracle as LO      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_case(model, input_type, seed=0, n=9, I=12, D=5, K=3):
    rng = np.random.RandomState(seed)
    if model == "vade":
        cfg = O.VadeConfig(I, D, K, (8, 7), (6, 9), input_type)
    else:
        cfg = O.Config(I, D, K, (8,), 7, (6, 9), input_type)
    p = O.init_params(cfg, seed + 1)
    p["prior_means"] = 0.5 * rng.randn(K, D)
    p["prior_log_vars"] = 0.3 * rng.randn(K, D)
    p["b_logvar"] = 0.2 * rng.randn(D)
    X = (rng.rand(n, I) < 0.4).astype(np.float64) if input_type == "binary" else rng.randn(n, I)
    return cfg, p, X, rng


def test_running_logsumexp_equals_the_direct_one():
    rng = np.random.RandomState(1)
    for S in (1, 2, 7, 50):
        w = 30.0 * rng.randn(S, 40) - 500.0                      # spread of tens of nats between draws, as real weights have
        w[:, 3] = w[0, 3]                                        # all draws equal: L = w
        np.testing.assert_allclose(LO.bound_running(w), LO.bound(w), rtol=1e-13, atol=0)
        assert np.all(LO.bound(w) <= w.max(0) + 1e-12) and np.all(LO.bound(w) >= w.max(0) - np.log(S) - 1e-12)
    np.testing.assert_allclose(LO.bound(w)[3], w[0, 3], rtol=1e-13)


@pytest.mark.parametrize("model", ["dmvae", "vade"])
@pytest.mark.parametrize("input_type", ["binary", "real"])
def test_one_draw_is_the_elbo_on_the_marginal_prior(model, input_type):
    cfg, p, X, rng = small_case(model, input_type)
    eps = rng.randn(1, len(X), cfg.latent_dim)
    mean, lv = LO.posterior(p, cfg, X)
    lpx, lpz, lq = LO.draw_terms(p, cfg, X, mean, lv, eps[0])
    np.testing.assert_allclose(LO.row_ll(p, cfg, X, eps), lpx + lpz - lq, rtol=1e-13)
    # the three terms against independent restatements: scipy-free Gaussian densities written out per element
    Z = mean + np.exp(lv / 2) * eps[0]
    q = -0.5 * (((Z - mean) ** 2) / np.exp(lv) + lv + np.log(2 * np.pi)).sum(1)
    np.testing.assert_allclose(lq, q, rtol=1e-12)
    comp = np.stack([-0.5 * (((Z - p["prior_means"][k]) ** 2) / np.exp(p["prior_log_vars"][k]) + p["prior_log_vars"][k] + np.log(2 * np.pi)).sum(1)
                     for k in range(cfg.n_classes)])
    np.testing.assert_allclose(lpz, np.log(np.exp(comp).mean(0)), rtol=1e-12)
    if input_type == "binary":                                   # minus the step's reconstruction loss, row by row
        xl = O.decode(p, cfg, Z)["xlogits"]
        assert abs(-lpx.mean() - O.recon_loss(cfg, X, xl)) <= 1e-12 * abs(lpx.mean())


def test_more_draws_tighten_the_bound_on_average():
    cfg, p, X, rng = small_case("dmvae", "binary", seed=3, n=200)
    eps = rng.randn(16, len(X), cfg.latent_dim)
    w = LO.weights(p, cfg, X, eps)
    l1, l4, l16 = w.mean(0).mean(), np.mean([LO.bound(w[i:i + 4]) for i in range(0, 16, 4)]), LO.bound(w).mean()
    assert l1 < l4 < l16


@pytest.mark.parametrize("model", ["dmvae", "vade"])
@pytest.mark.parametrize("input_type", ["binary", "real"])
def test_closed_form_holds_in_the_oracle(model, input_type):
    cfg, p, X, rng = small_case(model, input_type, seed=5)
    q = LO.closed_form_parameters(p, rng.randn(cfg.latent_dim), 0.4 * rng.randn(cfg.latent_dim))
    want = LO.bias_only_log_px(q, cfg, X)
    for S in (1, 9):
        np.testing.assert_allclose(LO.row_ll(q, cfg, X, rng.randn(S, len(X), cfg.latent_dim)), want, rtol=1e-12)


def test_device_noise_layout_follows_the_position_not_the_batch():
    whole = LO.device_eps(11, 7, 3, 63, 5)
    part = LO.device_eps(11, 7, 3, 63, 5, first=40, n=23)
    assert whole.shape == (3, 63, 5) and np.array_equal(whole[:, 40:], part)
    assert not np.array_equal(whole, LO.device_eps(11, 8, 3, 63, 5))
    import philox_oracle as PH
    assert not np.array_equal(whole, PH.eps_eval(11, 7, 3, 63, 5))          # stream 4 is not stream 2


def test_new_entries_are_declared_exported_and_bound():
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    for name, ret, nargs in (("dmvae_plan_eval_loglik_ws_bytes", "int64_t", 1), ("dmvae_plan_eval_loglik", "int", 13)):
        m = re.search(r"\b%s %s\s*\((.*?)\);" % (ret, name), hdr, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
        assert len(getattr(_lib.lib, name).argtypes) == nargs
    assert _lib.lib.dmvae_plan_eval_loglik_ws_bytes.restype is C.c_int64
    assert _lib.ABI_VERSION == 5 and _lib.lib.dmvae_abi_version() == 5


def make_plan(_lib, max_batch, dtype=0, model=0, D=10, K=10):
    cfg = _lib.Config()
    cfg.input_dim, cfg.latent_dim, cfg.n_classes = 70, D, K
    cfg.n_enc, cfg.n_dec, cfg.head_dim = 1, 1, 64
    cfg.enc[0], cfg.dec[0] = 64, 64
    cfg.dtype, cfg.max_batch, cfg.model = dtype, max_batch, model
    cfg.beta1, cfg.beta2, cfg.adam_eps, cfg.temperature = 0.9, 0.999, 1e-8, 1.0
    h = C.c_void_p()
    _lib.check(_lib.lib.dmvae_plan_create(C.byref(cfg), C.byref(h)), "dmvae_plan_create")
    sz = _lib.Sizes()
    _lib.check(_lib.lib.dmvae_plan_sizes(h, C.byref(sz)), "dmvae_plan_sizes")
    return h, sz


def test_scratch_size_grows_with_batch_pad_and_is_host_arithmetic():
    from dmvae_hip import _lib
    seen = {}
    for mb in (1, 100, 128, 129, 1000, 4096):
        for dtype in (0, 1):
            h, sz = make_plan(_lib, mb, dtype)
            n = int(_lib.lib.dmvae_plan_eval_loglik_ws_bytes(h))
            # three floats per padded row (a_s, running max, running scaled sum), rounded up to 256 bytes: no term in K, D or the dtype
            assert n == (3 * 4 * sz.batch_pad + 255) // 256 * 256
            seen.setdefault(sz.batch_pad, set()).add(n)
            h2, _ = make_plan(_lib, mb, dtype, model=1, D=300, K=40)
            assert int(_lib.lib.dmvae_plan_eval_loglik_ws_bytes(h2)) == n
            _lib.lib.dmvae_plan_destroy(h)
            _lib.lib.dmvae_plan_destroy(h2)
    pads = sorted(seen)
    assert all(len(v) == 1 for v in seen.values()) and len(pads) >= 4
    sizes = [next(iter(seen[b])) for b in pads]
    assert all(a < b for a, b in zip(sizes[:-1], sizes[1:]))
    assert int(_lib.lib.dmvae_plan_eval_loglik_ws_bytes(None)) < 0


def test_unbound_plan_is_refused_before_anything_else():
    from dmvae_hip import _lib
    h, _ = make_plan(_lib, 16)
    rc = _lib.lib.dmvae_plan_eval_loglik(h, None, 16, 16, 0, 1, None, 10, 0, None, 0, None, None)
    assert rc == -1 and b"not bound" in _lib.lib.dmvae_last_error()
    _lib.lib.dmvae_plan_destroy(h)


def test_cli_loglik_flag_defaults_to_off():
    sys.argv = ["train.py"]
    train = importlib.import_module("train")
    assert train.parser.parse_args([]).loglik == 0
    assert train.parser.parse_args(["--loglik", "50"]).loglik == 50
    with pytest.raises(SystemExit):
        train.parser.parse_args(["--loglik", "many"])


def test_model_classes_carry_the_method_and_the_moe_classes_do_not():
    import base_models
    import models
    assert callable(base_models.DeepMixtureVAE.get_log_likelihood)
    assert base_models.VaDE.get_log_likelihood is base_models.DeepMixtureVAE.get_log_likelihood
    assert not hasattr(models.DeepMoE, "get_log_likelihood") and not hasattr(models.DeepVariationalMoE, "get_log_likelihood")
    from dmvae_hip import StepEngine
    for name in ("eval_loglik", "loglik_buffer", "read_loglik"):
        assert callable(getattr(StepEngine, name))
