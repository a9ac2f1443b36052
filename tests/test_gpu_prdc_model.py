"""GPU tests of get_sample_quality (base_models.py, models.py) and of train.py --sample_quality: the tiny fp32 plan of
test_gpu_knn_model.py -- input 32, latent 4, K = 3, batch 8 -- on 50 rows (a ragged last batch) against M = 48 generated rows.  The method
must equal dmvae_hip.prdc on features rebuilt from the public pieces -- dmvae_philox_normal at the documented (seed, counter, stream id 7),
the prior views, decode and encode_means_device -- exactly, and the float64 oracle of tests/helpers/prdc_oracle.py on those features
wherever the oracle has nothing undecided."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import prdc_oracle as PO      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, D, K, B, N_ROWS, M, CLASSES = 32, 4, 3, 8, 50, 48, 4
LAYERS = dict(enc_layers=(24,), head_dim=16, dec_layers=(16, 24))
METRICS = ("precision", "recall", "density", "coverage")
VECTORS = ("precision_per_cluster", "density_per_cluster", "coverage_per_class", "recall_per_class")


def rows_and_classes(n, seed):
    """binary rows around 8 prototypes, 4 classes: rows of one prototype encode alike"""
    protos = np.random.RandomState(11).rand(8, I) < 0.4
    rng = np.random.RandomState(seed)
    which = rng.randint(0, 8, n)
    X = np.logical_xor(protos[which], rng.rand(n, I) < 0.15).astype(np.float32)
    return X, (which % CLASSES).astype(np.int64)


def dataset(make=None):
    from includes.utils import Dataset
    np.random.seed(5)                                            # shuffled at construction: the evaluated order is no identity
    make = make or (lambda X, cls: Dataset((X, cls), batch_size=B))
    return make(*rows_and_classes(N_ROWS, 1))


def spread(m):
    """prior components that overlap the encoder means in part: the metrics are neither all 0 nor all 1"""
    p = m.engine.get_parameters()
    rng = np.random.RandomState(1)
    m.engine.set_parameters({"W_mean": 3.0 * rng.randn(*p["W_mean"].shape), "prior_means": 2.0 * rng.randn(*p["prior_means"].shape),
                             "prior_log_vars": 1.0 + 0.5 * rng.randn(*p["prior_log_vars"].shape)})
    return m


def dmvae():
    import base_models
    return spread(base_models.DeepMixtureVAE("dmvae", "binary", I, D, K, activation="relu", initializer="xavier", batch_size=B, dtype="fp32", seed=3,
                                             eval="device", **LAYERS).build_graph())


def vade():
    import base_models
    return spread(base_models.VaDE("vade", "binary", I, D, K, activation="relu", initializer="xavier", batch_size=B, dtype="fp32", seed=3, eval="device",
                                   enc_layers=(24,), dec_layers=(16, 24)).build_graph())


def dvmoe():
    import models
    m = models.DeepVariationalMoE("dvmoe", "binary", I, D, CLASSES, K, True, featLearn=0, batch_size=B, dtype="fp32", seed=4, eval="device",
                                  **LAYERS).build_graph()
    spread(m.vae)
    return m


def rebuilt_features(vae, data, space, counter, n):
    """(real features, generated features, components, generated rows) from the public pieces, as the docstring documents them"""
    import torch
    from dmvae_hip import prdc
    comp = torch.arange(n, device="cuda") % K
    eps = prdc.philox_normal(n * D, vae.seed, step=counter, stream_id=7).view(n, D)
    mu, lv = vae.engine.param_view("prior_means"), vae.engine.param_view("prior_log_vars")
    Z = mu[comp] + torch.exp(lv[comp] / 2) * eps
    X = vae.decode(Z.cpu().numpy())                              # the decoder's mean image
    xs = data._rows[data.order]                                  # the evaluated order
    if space == "input":
        return xs, X, comp.cpu().numpy(), X
    return vae.encode_means_device(xs).cpu().numpy(), vae.encode_means_device(X).cpu().numpy(), comp.cpu().numpy(), X


def check_model(m, vae, data, k=3, space="latent", counter=0, n_samples=None):
    from dmvae_hip import prdc
    n = (N_ROWS // K) * K if n_samples is None else n_samples
    rng_state, order = np.random.get_state(), data.order.copy()
    res = m.get_sample_quality(None, data, k=k, space=space, counter=counter, n_samples=n_samples)
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state()))           # nothing drawn from the NumPy stream
    assert np.array_equal(order, data.order)                                                     # and no reshuffle
    assert (res["k"], res["n_real"], res["n_samples"], res["space"]) == (k, N_ROWS, n, space) and n == M
    again = m.get_sample_quality(None, data, k=k, space=space, counter=counter, n_samples=n_samples)
    for name in METRICS:
        assert res[name] == again[name] and 0.0 <= res[name] and (name == "density" or res[name] <= 1.0)      # a second call: the same bits
    for name in VECTORS:
        assert np.array_equal(res[name], again[name], equal_nan=True) and res[name].shape == ((K,) if "cluster" in name else (CLASSES,))

    R, F, comp, X = rebuilt_features(vae, data, space, counter, n)
    assert R.shape == (N_ROWS, D if space == "latent" else I) and F.shape == (n, R.shape[1])
    cls = data._cls[data.order]
    want = prdc.prdc(R, F, k, real_groups=cls, fake_groups=comp)
    for name in METRICS:
        assert res[name] == want[name], name
    for name, group in zip(VECTORS, ("precision_per_group", "density_per_group", "coverage_per_group", "recall_per_group")):
        assert np.array_equal(res[name], np.array(want[group]), equal_nan=True), name

    width = R.shape[1]
    u = PO.u_bar(width)
    rR2, rF2 = PO.radii(R, k), PO.radii(F, k)
    ref = PO.counts(R, F, rR2, rF2)
    slack = int(PO.undecided(ref["d2"], rR2[:, None], u).sum() + PO.undecided(ref["d2"], rF2[None, :], u).sum())
    for Xs in (R, F):
        srt = np.sort(PO.pair_d2(Xs, Xs), axis=1)[:, 1:]
        slack += int(np.count_nonzero(srt[:, k] - srt[:, k - 1] <= 2.0 * u * srt[:, k]))
    oracle = PO.prdc(R, F, k, real_groups=cls, fake_groups=comp)
    print("%s k=%d %s: %s; oracle slack %d" % (type(m).__name__, k, space, {n_: round(res[n_], 4) for n_ in METRICS}, slack))
    if space == "latent":
        assert slack == 0                                        # what this test needs of its rows: nothing for the f32 distance to decide
    if slack == 0:
        for name in METRICS:
            assert res[name] == oracle[name], name
        for name, group in zip(VECTORS, ("precision_per_group", "density_per_group", "coverage_per_group", "recall_per_group")):
            assert np.array_equal(res[name], oracle[group], equal_nan=True), name
    return res, X


def test_dmvae_equals_prdc_on_the_rebuilt_features_and_the_oracle():
    m = dmvae()
    data = dataset()
    res, X0 = check_model(m, m, data, k=3)
    assert any(0.0 < res[name] < 1.0 for name in ("precision", "recall", "coverage"))            # the model's prior neither covers all nor nothing
    check_model(m, m, data, k=5, n_samples=M)
    _, X1 = check_model(m, m, data, k=3, counter=1)
    assert not np.array_equal(X0, X1)                            # another counter: other samples
    assert X0.min() >= 0.0 and X0.max() <= 1.0 and len(np.unique(X0)) > 2      # the decoder's mean image, not a Bernoulli draw


def test_input_space_has_the_rows_width():
    m = dmvae()
    check_model(m, m, dataset(), k=3, space="input")


def test_vade_inherits_it():
    m = vade()
    check_model(m, m, dataset(), k=4)


def test_dvmoe_forwards_to_its_gate():
    from includes.utils import MEDataset
    m = dvmoe()
    data = dataset(lambda X, cls: MEDataset((X, cls, np.eye(CLASSES)[cls].astype(np.float32)), batch_size=B))
    check_model(m, m.vae, data, k=3)


def test_arguments_outside_their_range_are_refused():
    m = dmvae()
    data = dataset()
    for k in (0, M, 257):
        with pytest.raises(ValueError):
            m.get_sample_quality(None, data, k=k)
    with pytest.raises(ValueError):
        m.get_sample_quality(None, data, space="pixels")


def test_train_py_sample_quality_writes_its_keys_and_trains_as_without_the_flag(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    base = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--dataset", "synthetic", "--n_epochs", "2", "--eval", "device",
            "--batch_size", "1000", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    procs = []
    for name, extra in (("with", ["--sample_quality", "3"]), ("without", [])):
        d = tmp_path / name
        d.mkdir()
        procs.append((d, subprocess.Popen(base + extra, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    outs = []
    for d, pr in procs:
        so, se = pr.communicate(timeout=900)
        assert pr.returncode == 0, (so[-2000:], se[-3000:])
        outs.append((so + se, [json.loads(l) for l in open(d / "dmvae_metrics.jsonl")]))
    (on, rec_on), (off, rec_off) = outs
    assert "precTest=" in on and "covTest=" in on and "precTest" not in off
    assert len(rec_on) == 2 and len(rec_off) == 2
    gained = {"precTest", "recTest", "denTest", "covTest", "sq_k", "sq_samples", "precision_per_cluster", "density_per_cluster", "coverage_per_class",
              "recall_per_class"}
    for a, b in zip(rec_on, rec_off):
        assert set(a) - set(b) == gained and set(b) <= set(a)
        assert a["sq_k"] == 3 and len(a["precision_per_cluster"]) == len(a["density_per_cluster"]) and len(a["coverage_per_class"]) == len(a["recall_per_class"])
        assert all(0.0 <= a[n] <= 1.0 for n in ("precTest", "recTest", "covTest")) and a["denTest"] >= 0.0
        assert a["loss"] == b["loss"] and a["acc_test"] == b["acc_test"] and a["acc_train"] == b["acc_train"]      # the NumPy stream is untouched
