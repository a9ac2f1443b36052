"""GPU tests of get_posterior_diagnostics (base_models.py): small engines in the style of tests/test_gpu_cluster_metrics_model.py -- I = 70,
D = 5, K = 4, batch 40 over 203 rows, so the last batch is ragged -- against the float64 oracle of tests/helpers/mixture_density_oracle.py
on model.encode's means / log-variances and the returned sample.  Bars: mi / marginal_kl / rate within the mean of the per-point bars
of the log-densities they are differences of; the per-dimension vectors as tests/test_gpu_mixture_density.py holds column_stats."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import mixture_density_oracle as MO      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, D, K, B, N = 70, 5, 4, 40, 203
LAYERS = dict(enc_layers=(72,), head_dim=40, dec_layers=(48, 36))
KEYS = {"mi", "marginal_kl", "rate", "mi_cap", "active_units", "var_of_mean", "mean_of_var", "n_points", "n_rows"}
U = 2.0 ** -24


def dataset(seed=5):
    from includes.utils import Dataset
    rng = np.random.RandomState(3)
    protos = rng.rand(12, I) < 0.4
    which = rng.randint(0, 12, N)
    X = np.logical_xor(protos[which], rng.rand(N, I) < 0.03).astype(np.float32)
    np.random.seed(seed)
    return Dataset((X, (which % K).astype(np.int64)), batch_size=B)


def dmvae(dtype="fp32"):
    import base_models
    m = base_models.DeepMixtureVAE("dmvae", "binary", I, D, K, activation="relu", initializer="xavier", batch_size=B, dtype=dtype, seed=3,
                                   eval="device", **LAYERS).build_graph()
    p = m.engine.get_parameters()
    rng = np.random.RandomState(1)
    m.engine.set_parameters({"W_mean": 1.5 * rng.randn(*p["W_mean"].shape), "b_logvar": np.full(D, -3.0), "prior_means": 0.7 * rng.randn(K, D),
                             "prior_log_vars": 0.2 * rng.randn(K, D)})
    return m


def vade():
    import base_models
    m = base_models.VaDE("vade", "binary", I, D, K, activation="relu", initializer="xavier", batch_size=B, dtype="fp32", seed=3, eval="device",
                         enc_layers=(72,), dec_layers=(48, 36)).build_graph()
    p = m.engine.get_parameters()
    rng = np.random.RandomState(2)
    m.engine.set_parameters({"W_mean": 3.0 * rng.randn(*p["W_mean"].shape), "prior_means": 0.7 * rng.randn(K, D),
                             "prior_log_vars": np.zeros((K, D)), "b_logvar": np.full(D, -4.0)})
    return m


MODELS = {"fp32": lambda: dmvae("fp32"), "bf16": lambda: dmvae("bf16"), "vade": vade}


def encoded(m, data):
    out = m.encode(data._rows[data.order])
    return out[0].astype(np.float64), out[1].astype(np.float64)


def priors(m):
    p = m.engine.get_parameters()
    return p["prior_means"].astype(np.float64), p["prior_log_vars"].astype(np.float64)


def assert_against_the_oracle(res, z, a, mean, lv, pm, plv, rows, what):
    z, a = z.cpu().numpy().astype(np.float64), a.cpu().numpy().astype(np.float64)
    assert z.shape == (len(rows), D) and a.shape == (len(rows),)
    o = MO.diagnostics(mean, lv, pm, plv, z, a)
    # a is the device's own (held to its formula below); m and p carry the primitive's per-point bars
    bars = dict(mi=o["bar_m"].mean(), marginal_kl=(o["bar_m"] + o["bar_p"]).mean(), rate=o["bar_p"].mean())
    for k, b in bars.items():
        print("%s: %s = %.6f, |%s - oracle| = %.3g (bar %.3g)" % (what, k, res[k], k, abs(res[k] - o[k]), b))
        assert abs(res[k] - o[k]) <= b, (what, k, res[k], o[k], b)
    assert abs(res["mi"] + res["marginal_kl"] - res["rate"]) <= 1e-12 * max(1.0, abs(res["rate"]))
    assert res["mi_cap"] == math.log(len(mean)) and res["mi"] <= res["mi_cap"] + bars["mi"]
    assert res["n_points"] == len(rows) and res["n_rows"] == len(mean)
    # the sample is a sample of the rows `rows`: eps recovered from z reproduces a
    eps = (z - mean[rows]) * np.exp(-lv[rows] / 2)
    a_ref = -0.5 * np.sum(eps * eps + lv[rows], axis=1) - 0.5 * D * MO.LOG_2PI
    slack = np.sum(np.abs(eps) * 2 * U * (np.abs(mean[rows]) + np.abs(z)) * np.exp(-lv[rows] / 2), axis=1)      # z is rounded to float32 before eps is recovered
    assert (np.abs(a - a_ref) <= (D + 4) * U * 0.5 * np.sum(eps * eps + np.abs(lv[rows]), axis=1) + slack).all()
    assert np.abs(eps).max() < 6.0 and 0.5 < eps.std() < 1.5
    assert res["active_units"] == int(np.count_nonzero(mean.var(axis=0) > 0.01)) == o["active_units"]
    np.testing.assert_allclose(res["var_of_mean"], o["var_of_mean"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(res["mean_of_var"], o["mean_of_var"], rtol=(np.abs(lv).max() + 4) * U, atol=0)


@pytest.mark.parametrize("kind", ["fp32", "bf16", "vade"])
def test_against_the_oracle_on_encodes_outputs(kind):
    m, data = MODELS[kind](), dataset()
    res, z, a = m.get_posterior_diagnostics(None, data, counter=2, return_points=True)
    assert set(res) == KEYS and res["var_of_mean"].shape == (D,) and res["mean_of_var"].shape == (D,)
    mean, lv = encoded(m, data)
    pm, plv = priors(m)
    assert res["active_units"] >= 2                              # what this test needs of its parameters
    assert_against_the_oracle(res, z, a, mean, lv, pm, plv, np.arange(N), kind)
    # max_points: the rows floor(i N / M), scored against all N rows
    sub, zs, as_ = m.get_posterior_diagnostics(None, data, counter=2, max_points=50, return_points=True)
    rows = np.floor(np.arange(50) * N / 50).astype(np.int64)
    assert_against_the_oracle(sub, zs, as_, mean, lv, pm, plv, rows, kind + " max_points=50")
    assert np.array_equal(sub["var_of_mean"], res["var_of_mean"]) and sub["active_units"] == res["active_units"]
    # the caller's noise
    eps = np.random.RandomState(8).randn(N, D).astype(np.float32)
    fed, zf, _ = m.get_posterior_diagnostics(None, data, eps=eps, return_points=True)
    zr, _ = MO.sample(mean, lv, eps.astype(np.float64))
    assert (np.abs(zf.cpu().numpy() - zr) <= 2 * U * (np.abs(mean) + np.abs(zr - mean))).all()
    assert res["active_units"] == fed["active_units"] and fed["mi"] != res["mi"]
    assert m.get_posterior_diagnostics(None, data, au_threshold=1e9)["active_units"] == 0


@pytest.mark.parametrize("kind", ["fp32", "vade"])
def test_an_encoder_that_ignores_x_has_no_information_and_no_active_unit(kind):
    m, data = MODELS[kind](), dataset()
    sd = m.state_dict()
    sd["W_mean"], sd["W_logvar"] = np.zeros_like(sd["W_mean"]), np.zeros_like(sd["W_logvar"])
    m.load_state_dict(sd)
    res, z, a = m.get_posterior_diagnostics(None, data, return_points=True)
    mean, lv = encoded(m, data)
    assert not mean.var(axis=0).any() and not lv.var(axis=0).any()                       # every row has one posterior: q(z) = q(z|x)
    bar = MO.bar(z.cpu().numpy().astype(np.float64), mean, lv).mean() + (D + 4) * U * 0.5 * float(np.mean(np.sum(6.0 ** 2 + np.abs(lv), axis=1)))
    print("%s: mi = %.3g (bar %.3g), marginal_kl = %.4f" % (kind, res["mi"], bar, res["marginal_kl"]))
    assert abs(res["mi"]) <= bar and res["active_units"] == 0 and not res["var_of_mean"].any()
    assert abs(res["marginal_kl"] - res["rate"]) <= bar


def test_a_function_of_the_counter_that_leaves_the_training_state_alone():
    m, data = dmvae("bf16"), dataset()
    m.define_train_step(0.002, 100)
    m.train_op(None, data, 1.0)                                                  # non-zero moments to keep
    eng = m.engine
    torch.cuda.synchronize()
    arenas = [t.clone() for t in (eng.param, eng.m, eng.v)] + ([eng.param_bf16.clone()] if eng.param_bf16 is not None else [])
    state, order, rng_state = bytes(eng.read_state()), data.order.copy(), np.random.get_state()
    r1, z1, a1 = m.get_posterior_diagnostics(None, data, counter=3, return_points=True)
    r2, z2, a2 = m.get_posterior_diagnostics(None, data, counter=3, return_points=True)
    r3, z3, _ = m.get_posterior_diagnostics(None, data, counter=4, return_points=True)
    assert torch.equal(z1, z2) and torch.equal(a1, a2) and all(np.array_equal(r1[k], r2[k]) for k in KEYS)      # one counter: the same bits
    assert not torch.equal(z1, z3) and r1["mi"] != r3["mi"] and np.array_equal(r1["var_of_mean"], r3["var_of_mean"])      # another: other noise
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state())) and np.array_equal(order, data.order)
    now = [eng.param, eng.m, eng.v] + ([eng.param_bf16] if eng.param_bf16 is not None else [])
    assert all(torch.equal(a, b) for a, b in zip(arenas, now)) and bytes(eng.read_state()) == state


def test_a_train_op_behind_the_call_gives_the_bits_it_gives_without_one():
    outs = []
    for with_call in (True, False):
        m, data = dmvae("bf16"), dataset()
        m.define_train_step(0.002, 100)
        m.train_op(None, data, 1.0)
        if with_call:
            m.get_posterior_diagnostics(None, data, counter=1)
        loss = m.train_op(None, data, 1.0)
        torch.cuda.synchronize()
        outs.append((loss, m.engine.param.clone(), m.engine.m.clone(), m.engine.v.clone(), bytes(m.engine.read_state())))
    (la, pa, ma, va, sa), (lb, pb, mb, vb, sb) = outs
    assert la == lb and torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and sa == sb


def test_it_is_not_offered_on_the_moe_classes():
    import models
    assert not hasattr(models.MoE, "get_posterior_diagnostics") and not hasattr(models.DeepVariationalMoE, "get_posterior_diagnostics")


def test_train_py_diagnostics_adds_the_five_keys_and_nothing_without_the_flag(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    base = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--dataset", "synthetic", "--n_epochs", "1", "--eval", "device",
            "--batch_size", "1000", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    procs = []
    for name, extra in (("with", ["--diagnostics"]), ("without", [])):
        d = tmp_path / name
        d.mkdir()
        procs.append((d, subprocess.Popen(base + extra, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    outs = []
    for d, pr in procs:
        so, se = pr.communicate(timeout=900)
        assert pr.returncode == 0, (so[-2000:], se[-3000:])
        outs.append((so + se, [json.loads(l) for l in open(d / "dmvae_metrics.jsonl")]))
    (on, rec_on), (off, rec_off) = outs
    assert "miTest=" in on and "auTest=" in on and "miTest" not in off and "auTest" not in off
    assert len(rec_on) == 1 and len(rec_off) == 1
    assert set(rec_on[0]) - set(rec_off[0]) == {"mi_test", "marginal_kl_test", "rate_test", "mi_cap_test", "active_units_test"}
    assert set(rec_off[0]) <= set(rec_on[0])
    for k in ("loss", "acc_train", "acc_test"):                                  # the NumPy stream and the parameters are untouched
        assert rec_on[0][k] == rec_off[0][k], k
    r = rec_on[0]
    assert r["mi_test"] <= r["mi_cap_test"] + 1e-3 and abs(r["mi_test"] + r["marginal_kl_test"] - r["rate_test"]) <= 1e-9 * max(1.0, abs(r["rate_test"]))
    assert 0 <= r["active_units_test"] <= 10
