"""GPU tests of get_knn_accuracy / get_cluster_exemplars (base_models.py, models.py) and of train.py --knn: a tiny fp32 plan -- input
32, latent 4, K = 3, batch 8 -- on two data sets of 50 and 23 rows (ragged last batches), against dmvae_hip.knn's classifier on
encode_means_device of the same rows and against the float64 oracle of tests/helpers/knn_oracle.py on those means.  All exact: the
means are the same kernels' output on the same rows, and the oracle is asked only where it has no near tie to decide."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import knn_oracle as KO      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, D, K, B, N_TRAIN, N_TEST, CLASSES = 32, 4, 3, 8, 50, 23, 4
LAYERS = dict(enc_layers=(24,), head_dim=16, dec_layers=(16, 24))


def rows_and_classes(n, seed):
    """binary rows around 8 prototypes, 4 classes: rows of one prototype encode alike"""
    protos = np.random.RandomState(11).rand(8, I) < 0.4
    rng = np.random.RandomState(seed)
    which = rng.randint(0, 8, n)
    X = np.logical_xor(protos[which], rng.rand(n, I) < 0.15).astype(np.float32)
    return X, (which % CLASSES).astype(np.int64)


def datasets(make=None):
    from includes.utils import Dataset
    np.random.seed(5)                                            # both are shuffled at construction: the evaluated order is no identity
    make = make or (lambda X, cls: Dataset((X, cls), batch_size=B))
    return make(*rows_and_classes(N_TRAIN, 1)), make(*rows_and_classes(N_TEST, 2))


def spread(m):
    p = m.engine.get_parameters()
    rng = np.random.RandomState(1)
    m.engine.set_parameters({"W_mean": 3.0 * rng.randn(*p["W_mean"].shape), "prior_means": 2.0 * rng.randn(*p["prior_means"].shape)})
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


def check_model(m, vae, train, test, k=3):
    from dmvae_hip import knn
    rng_state, orders = np.random.get_state(), (train.order.copy(), test.order.copy())
    acc, conf = m.get_knn_accuracy(None, train, test, k=k, return_confusion=True)
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state()))           # nothing drawn from the NumPy stream
    assert np.array_equal(orders[0], train.order) and np.array_equal(orders[1], test.order)      # and no reshuffle
    assert m.get_knn_accuracy(None, train, test, k=k) == acc

    xs, ys = train._rows[train.order], train._cls[train.order]                                  # the evaluated order
    xq, yq = test._rows[test.order], test._cls[test.order]
    Zx, Zq = vae.encode_means_device(xs), vae.encode_means_device(xq)
    clf = knn.KNeighborsClassifier(n_neighbors=k).fit(Zx, ys)
    pred = clf.predict(Zq)
    assert acc == float(np.mean(pred == yq)) == clf.score(Zq, yq) and 0.0 <= acc <= 1.0
    want = np.zeros((CLASSES, CLASSES), dtype=np.int64)
    np.add.at(want, (pred, yq), 1)
    assert conf.shape == (CLASSES, CLASSES) and np.array_equal(conf, want) and conf.sum() == N_TEST

    zx, zq = Zx.cpu().numpy(), Zq.cpu().numpy()
    ref_idx, _, d2 = KO.knn(zq, zx, k)
    srt = np.sort(d2, axis=1)
    gap = np.diff(srt[:, :k + 1], axis=1)                        # between the t-th and the (t + 1)-th smallest, t < k
    clear = np.all((gap == 0.0) | (gap > 4.0 * KO.u_bar(D) * srt[:, 1:k + 1]), axis=1)       # an exact tie (equal rows) or none the f32 sum could make
    assert clear.sum() >= N_TEST // 2                            # what this test needs of its rows
    idx = clf.kneighbors(Zq)[0].cpu().numpy()
    assert np.array_equal(idx[clear], ref_idx[clear])
    assert np.array_equal(pred[clear], KO.vote(ref_idx, ys, CLASSES)[1][clear])

    ex = m.get_cluster_exemplars(None, train, n=5)
    assert np.array_equal(orders[0], train.order) and all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state()))
    prior = vae.engine.get_parameters()["prior_means"].astype(np.float32)                        # the prior means read from the engine
    eidx, _, ed2 = KO.knn(prior, zx, 5)
    esrt = np.sort(ed2, axis=1)
    assert ex.shape == (K, 5) and np.issubdtype(ex.dtype, np.integer)
    for c in range(K):
        egap = np.diff(esrt[c, :6])
        if np.all((egap == 0.0) | (egap > 4.0 * KO.u_bar(D) * esrt[c, 1:6])):
            assert np.array_equal(ex[c], train.order[eidx[c]]), c                                # the data set's own unpermuted numbering
        d_of = ed2[c][np.argsort(train.order)][ex[c]]                                            # in any case: nearest first, and the 5 nearest
        assert np.all(np.diff(d_of) >= -4.0 * KO.u_bar(D) * d_of[1:]) and d_of[-1] <= esrt[c, 4] * (1.0 + 4.0 * KO.u_bar(D))
    return acc


def test_dmvae_equals_the_classifier_on_its_means_and_the_oracle():
    m = dmvae()
    train, test = datasets()
    check_model(m, m, train, test, k=3)
    check_model(m, m, train, test, k=10)


def test_vade_inherits_it():
    m = vade()
    train, test = datasets()
    check_model(m, m, train, test, k=5)


def test_dvmoe_forwards_to_its_gate():
    from includes.utils import MEDataset
    m = dvmoe()
    train, test = datasets(lambda X, cls: MEDataset((X, cls, np.eye(CLASSES)[cls].astype(np.float32)), batch_size=B))
    check_model(m, m.vae, train, test, k=4)


def test_k_outside_its_range_is_refused():
    m = dmvae()
    train, test = datasets()
    for k in (0, N_TRAIN + 1, 257):
        with pytest.raises(ValueError):
            m.get_knn_accuracy(None, train, test, k=k)


def test_train_py_knn_writes_knn_test_and_trains_as_without_the_flag(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    base = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--dataset", "synthetic", "--n_epochs", "1", "--eval", "device",
            "--batch_size", "1000", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    procs = []
    for name, extra in (("with", ["--knn", "3"]), ("without", [])):
        d = tmp_path / name
        d.mkdir()
        procs.append((d, subprocess.Popen(base + extra, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    outs = []
    for d, pr in procs:
        so, se = pr.communicate(timeout=900)
        assert pr.returncode == 0, (so[-2000:], se[-3000:])
        outs.append((so + se, [json.loads(l) for l in open(d / "dmvae_metrics.jsonl")]))
    (on, rec_on), (off, rec_off) = outs
    assert "knnTest=" in on and "knnTest" not in off
    assert len(rec_on) == 1 and len(rec_off) == 1
    assert set(rec_on[0]) - set(rec_off[0]) == {"knnTest", "knn_k"} and set(rec_off[0]) <= set(rec_on[0])
    assert 0.0 <= rec_on[0]["knnTest"] <= 1.0 and rec_on[0]["knn_k"] == 3
    assert rec_on[0]["loss"] == rec_off[0]["loss"] and rec_on[0]["acc_test"] == rec_off[0]["acc_test"]      # the NumPy stream is untouched
