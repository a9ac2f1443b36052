"""GPU tests of get_cluster_metrics (base_models.py, models.py): small engines in the style of tests/test_gpu_loglik.py -- I = 70,
D = 5, K = 4, batch 40 over 203 rows, so the last batch is ragged -- against the host path (model.encode -> np.argmax), the device
confusion matrix of get_accuracy, sklearn's NMI / ARI on (labels, classes) and the float64 silhouette oracle on encode's means.
Bars: labels, matrix and accuracy exactly; nmi / ari / purity 1e-12; silhouette cluster_metrics_oracle.bar(D)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import cluster_metrics_oracle as CO      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, D, K, B, N = 70, 5, 4, 40, 203
LAYERS = dict(enc_layers=(72,), head_dim=40, dec_layers=(48, 36))
KEYS = {"acc", "nmi", "ari", "purity", "silhouette", "n_clusters_used"}


def rows_and_classes(n_classes=K, seed=3):
    """203 binary rows around 12 prototypes: rows of one prototype encode alike, so a random head spreads them over the clusters"""
    rng = np.random.RandomState(seed)
    protos = rng.rand(12, I) < 0.4
    which = rng.randint(0, 12, N)
    X = np.logical_xor(protos[which], rng.rand(N, I) < 0.03).astype(np.float32)
    return X, (which % n_classes).astype(np.int64)


def dataset(seed=5):
    from includes.utils import Dataset
    X, cls = rows_and_classes()
    np.random.seed(seed)
    return Dataset((X, cls), batch_size=B)


def dmvae(dtype="fp32"):
    import base_models
    m = base_models.DeepMixtureVAE("dmvae", "binary", I, D, K, activation="relu", initializer="xavier", batch_size=B, dtype=dtype, seed=3,
                                   eval="device", **LAYERS).build_graph()
    p = m.engine.get_parameters()
    rng = np.random.RandomState(1)
    m.engine.set_parameters({"W_logits": 4.0 * rng.randn(*p["W_logits"].shape), "W_mean": 3.0 * rng.randn(*p["W_mean"].shape)})
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


def confusion_of(labels, classes, R):
    d = np.zeros((R, R), dtype=np.int64)
    np.add.at(d, (labels.astype(np.int64), np.asarray(classes, dtype=np.int64)), 1)
    return d


def assert_silhouette(got, means, labels, what):
    ref = CO.silhouette_samples(means.astype(np.float32), labels, K).mean()
    print("%s: silhouette %.6f, |silhouette - oracle| = %.3g (bar %.3g), clusters %s" % (what, got, abs(got - ref), CO.bar(D),
                                                                                         np.bincount(labels, minlength=K).tolist()))
    assert abs(got - ref) <= CO.bar(D), (what, got, ref)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dmvae_against_the_host_path_sklearn_and_the_oracle(dtype):
    skm = pytest.importorskip("sklearn.metrics")
    from includes.utils import accuracy_from_confusion
    m, data = dmvae(dtype), dataset()
    res, labels = m.get_cluster_metrics(None, data, return_labels=True)
    assert set(res) == KEYS and labels.dtype == np.int32 and labels.shape == (N,)
    mean, _, logits = m.encode(data.data)
    host = np.argmax(logits, axis=1)
    assert np.count_nonzero(np.bincount(host, minlength=K)) >= 3                 # what this test needs of its parameters
    assert np.array_equal(labels, host)
    conf = m._device_confusion(data, data.order, K)                              # get_accuracy(eval="device")'s matrix on the same order
    assert np.array_equal(conf, confusion_of(labels, data.classes, K))
    assert res["acc"] == accuracy_from_confusion(conf, N) and res["n_clusters_used"] == np.count_nonzero(conf.sum(axis=1))
    assert abs(res["nmi"] - skm.normalized_mutual_info_score(data.classes, labels)) <= 1e-12
    assert abs(res["ari"] - skm.adjusted_rand_score(data.classes, labels)) <= 1e-12
    assert abs(res["purity"] - conf.max(axis=1).sum() / N) <= 1e-12
    assert_silhouette(res["silhouette"], mean, labels, "dmvae %s" % dtype)
    off = m.get_cluster_metrics(None, data, silhouette=False)
    assert np.isnan(off["silhouette"]) and {k: v for k, v in off.items() if k != "silhouette"} == {k: v for k, v in res.items() if k != "silhouette"}


def test_vade_against_its_device_confusion_and_the_oracle():
    from includes.utils import accuracy_from_confusion
    m, data = vade(), dataset()
    res, labels = m.get_cluster_metrics(None, data, counter=7, return_labels=True)
    conf = m._device_confusion(data, data.order, K, draws=10, eps=None, counter=7)
    assert np.array_equal(conf, confusion_of(labels, data.classes, K))            # the same Philox draws: stream 2, counter 7, 10 draws
    assert np.array_equal(np.bincount(labels, minlength=K), conf.sum(axis=1))
    assert res["acc"] == accuracy_from_confusion(conf, N) and res["n_clusters_used"] == np.count_nonzero(conf.sum(axis=1)) >= 2
    res_b, labels_b = m.get_cluster_metrics(None, data, counter=7, return_labels=True)
    assert np.array_equal(labels, labels_b) and res == res_b                     # a function of (parameters, data, counter)
    m.noise = "host"                                                             # whatever noise= says: the device noise
    assert m.get_cluster_metrics(None, data, counter=7) == res
    mean, _ = m.encode(data.data)
    assert_silhouette(res["silhouette"], mean, labels, "vade")


def test_dvmoe_delegates_to_its_gate_with_the_larger_matrix(monkeypatch):
    import models
    from dmvae_hip import StepEngine
    from includes.utils import MEDataset
    X, cls = rows_and_classes(n_classes=6)
    E = 4
    m = models.DeepVariationalMoE("dvmoe", "binary", I, D, 6, E, True, featLearn=0, batch_size=B, dtype="fp32", seed=4, eval="device",
                                  **LAYERS).build_graph()
    data = MEDataset((X, cls, np.eye(6)[cls].astype(np.float32)), batch_size=B)
    sizes, make = [], StepEngine.confusion_buffer
    monkeypatch.setattr(StepEngine, "confusion_buffer", staticmethod(lambda R, device: (sizes.append(R), make(R, device))[1]))
    res, labels = m.get_cluster_metrics(None, data, return_labels=True)
    assert sizes == [6] and set(res) == KEYS                                     # R = max(E, n_classes)
    assert all(np.isfinite(res[k]) for k in ("acc", "nmi", "ari", "purity")) and 1 <= res["n_clusters_used"] <= E
    assert labels.min() >= 0 and labels.max() < E
    assert np.isfinite(res["silhouette"]) == (2 <= res["n_clusters_used"])


@pytest.mark.parametrize("kind", ["dmvae", "vade"])
def test_the_call_draws_nothing_and_leaves_the_training_state_alone(kind):
    m, data = (dmvae("bf16") if kind == "dmvae" else vade()), dataset()
    m.define_train_step(0.002, 100)
    m.train_op(None, data, 1.0)                                                  # non-zero moments to keep
    eng = m.engine
    torch.cuda.synchronize()
    arenas = [t.clone() for t in (eng.param, eng.m, eng.v)] + ([eng.param_bf16.clone()] if eng.param_bf16 is not None else [])
    state, order, rng_state = bytes(eng.read_state()), data.order.copy(), np.random.get_state()
    res = m.get_cluster_metrics(None, data, counter=3)
    assert set(res) == KEYS
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state())) and np.array_equal(order, data.order)
    now = [eng.param, eng.m, eng.v] + ([eng.param_bf16] if eng.param_bf16 is not None else [])
    assert all(torch.equal(a, b) for a, b in zip(arenas, now)) and bytes(eng.read_state()) == state


def test_a_collapsed_model_reports_nan_and_does_not_raise():
    m, data = dmvae(), dataset()
    p = m.engine.get_parameters()
    m.engine.set_parameters({"W_logits": np.zeros_like(p["W_logits"]), "b_logits": np.zeros_like(p["b_logits"])})
    res, labels = m.get_cluster_metrics(None, data, return_labels=True)
    assert not labels.any() and res["n_clusters_used"] == 1 and np.isnan(res["silhouette"])      # every row in cluster 0
    assert res["nmi"] == 0.0 and res["ari"] == 0.0 and 0.0 < res["purity"] < 1.0


def test_train_py_metrics_adds_the_five_keys_and_nothing_without_the_flag(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    base = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--dataset", "synthetic", "--n_epochs", "1", "--eval", "device",
            "--batch_size", "1000", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    procs = []
    for name, extra in (("with", ["--metrics"]), ("without", [])):
        d = tmp_path / name
        d.mkdir()
        procs.append((d, subprocess.Popen(base + extra, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    outs = []
    for d, pr in procs:
        so, se = pr.communicate(timeout=900)
        assert pr.returncode == 0, (so[-2000:], se[-3000:])
        outs.append((so + se, [json.loads(l) for l in open(d / "dmvae_metrics.jsonl")]))
    (on, rec_on), (off, rec_off) = outs
    assert "nmiTest=" in on and "silTest=" in on and "nmiTest" not in off and "silTest" not in off
    assert len(rec_on) == 1 and len(rec_off) == 1
    assert set(rec_on[0]) - set(rec_off[0]) == {"nmi_test", "ari_test", "purity_test", "silhouette_test", "clusters_used_test"}
    assert set(rec_off[0]) <= set(rec_on[0])
    assert rec_on[0]["loss"] == rec_off[0]["loss"] and rec_on[0]["acc_test"] == rec_off[0]["acc_test"]      # the NumPy stream is untouched
    assert 0.0 <= rec_on[0]["nmi_test"] <= 1.0 and 1 <= rec_on[0]["clusters_used_test"] <= 10
