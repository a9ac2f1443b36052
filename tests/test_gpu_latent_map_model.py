"""GPU tests of get_latent_map (base_models.py, models.py) and includes.visualization.latent_map_plot: a small fp32 plan -- input 64, one
layer of 32, latent 8, K = 3, batch 100 -- trained for one epoch on 600 rows, mapped with the dense and with the kNN-sparse form.  The
trustworthiness is dmvae_hip.knn's on the same tensors (exact); the order, the determinism and the untouched NumPy stream are exact too."""
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I, D, K, B, N, CLASSES = 64, 8, 3, 100, 600, 4
LAYERS = dict(enc_layers=(32,), head_dim=32, dec_layers=(32,))


def dataset(make=None):
    """binary rows around 8 prototypes, 4 classes; shuffled at construction: the evaluated order is no identity"""
    from includes.utils import Dataset
    protos = np.random.RandomState(11).rand(8, I) < 0.4
    rng = np.random.RandomState(1)
    which = rng.randint(0, 8, N)
    X = np.logical_xor(protos[which], rng.rand(N, I) < 0.1).astype(np.float32)
    cls = (which % CLASSES).astype(np.int64)
    np.random.seed(5)
    return (make or (lambda X, cls: Dataset((X, cls), batch_size=B)))(X, cls)


def dmvae():
    import base_models
    return base_models.DeepMixtureVAE("dmvae_map", "binary", I, D, K, activation="relu", initializer="xavier", batch_size=B, dtype="fp32", seed=3,
                                      eval="device", **LAYERS).build_graph()


def vade():
    import base_models
    return base_models.VaDE("vade_map", "binary", I, D, K, activation="relu", initializer="xavier", batch_size=B, dtype="fp32", seed=3, eval="device",
                            enc_layers=(32,), dec_layers=(32,)).build_graph()


def png_pixels(path):
    blob = open(path, "rb").read()
    w, h, depth, ctype = struct.unpack(">IIBB", blob[16:26])
    assert (depth, ctype) == (8, 2)
    pos, idat = 8, b""
    while pos < len(blob):
        n, tag = struct.unpack(">I", blob[pos:pos + 4])[0], blob[pos + 4:pos + 8]
        if tag == b"IDAT":
            idat += blob[pos + 8:pos + 8 + n]
        pos += 12 + n
    return np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3)


def check_model(m, vae, data, tmp_path):
    import torch
    from dmvae_hip import knn
    from includes import visualization as V
    m.define_train_step(0.002, 1000, 0.9)
    m.train_op(None, data, 1.0)
    rng_state, order = np.random.get_state(), data.order.copy()
    res = {how: m.get_latent_map(None, data, n_iter=300, method=how, trust_neighbors=5, counter=2) for how in ("knn", "exact")}
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state()))           # nothing drawn from the NumPy stream
    assert np.array_equal(order, data.order)                                                     # and no reshuffle
    Z = vae._eval_means_device(data)
    _, labels = vae._cluster_metrics(data, max(K, CLASSES), False, 2, True)
    for how, r in res.items():
        assert set(r) == {"embedding", "classes", "clusters", "kl", "trustworthiness", "method", "n_neighbors", "seconds"}
        assert r["embedding"].shape == (N, 2) and r["embedding"].dtype == np.float32 and np.isfinite(r["embedding"]).all()
        assert np.array_equal(r["classes"], data._cls[data.order]) and r["classes"].shape == (N,)
        assert r["clusters"].shape == (N,) and np.array_equal(r["clusters"], labels) and 0 <= r["clusters"].min() and r["clusters"].max() < K
        assert r["method"] == how and r["n_neighbors"] == (91 if how == "knn" else None) and r["seconds"] > 0 and np.isfinite(r["kl"]) and r["kl"] > 0
        assert r["trustworthiness"] == knn.trustworthiness(Z, torch.as_tensor(r["embedding"]).cuda(), 5) and 0.5 < r["trustworthiness"] <= 1.0      # (0.5: what a random scatter scores)
        again = m.get_latent_map(None, data, n_iter=300, method=how, trust_neighbors=5, counter=2)
        assert np.array_equal(again["embedding"].view(np.uint32), r["embedding"].view(np.uint32)) and again["kl"] == r["kl"]
        assert again["trustworthiness"] == r["trustworthiness"] and np.array_equal(again["clusters"], r["clusters"])
    assert not np.array_equal(res["knn"]["embedding"], res["exact"]["embedding"])              # two forms of P
    assert m.get_latent_map(None, data, n_iter=2)["method"] == "exact"                           # auto: 600 rows lie under the dense cap
    with pytest.raises(ValueError):
        m.get_latent_map(None, data, method="barnes_hut")

    path = str(tmp_path / "latent.png")
    out = V.latent_map_plot(m, data, None, path, side=200, n_iter=300, method="knn", counter=2)
    assert np.array_equal(out["embedding"], res["knn"]["embedding"])
    px = png_pixels(path)
    assert px.shape == (200, 200 + 14 + 200, 3)
    white = {(255, 255, 255)}
    left = {tuple(c) for c in px[:, :200].reshape(-1, 3).tolist()}
    right = {tuple(c) for c in px[:, 214:].reshape(-1, 3).tolist()}
    assert left - white and left - white <= {tuple(c) for c in V._COLORS[np.unique(out["classes"])].astype(int).tolist()}       # dots, in the classes' colours alone
    assert right - white and right - white <= {tuple(c) for c in V._COLORS[np.unique(out["clusters"]) % 10].astype(int).tolist()}
    assert {tuple(c) for c in px[:, 200:214].reshape(-1, 3).tolist()} == white
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state())) and np.array_equal(order, data.order)


def test_dmvae_latent_map(tmp_path):
    m = dmvae()
    check_model(m, m, dataset(), tmp_path)


def test_vade_latent_map(tmp_path):
    m = vade()
    check_model(m, m, dataset(), tmp_path)


def test_dvmoe_forwards_to_its_gate(tmp_path):
    import models
    from includes.utils import MEDataset
    m = models.DeepVariationalMoE("dvmoe_map", "binary", I, D, CLASSES, K, True, featLearn=0, batch_size=B, dtype="fp32", seed=4, eval="device",
                                  **LAYERS).build_graph()
    data = dataset(lambda X, cls: MEDataset((X, cls, np.eye(CLASSES)[cls].astype(np.float32)), batch_size=B))
    r = m.get_latent_map(None, data, n_iter=20, method="knn")
    assert r["embedding"].shape == (N, 2) and np.array_equal(r["classes"], data._cls[data.order]) and r["clusters"].max() < max(K, CLASSES)
    assert np.array_equal(r["clusters"], m.get_cluster_metrics(None, data, silhouette=False, return_labels=True)[1])
