"""GPU tests of get_linear_probe_accuracy (base_models.py, models.py) and of train.py --probe: the tiny fp32 plan of the kNN model tests
-- input 32, latent 4, K = 3, batch 8 -- on two data sets of 50 and 23 rows (ragged last batches), against dmvae_hip.probe's
LogisticRegression on encode_means_device of the same rows (exactly: the same kernels on the same rows) and against the float64 optimum
of tests/helpers/probe_oracle.py wherever that one has a margin.  A large penalty (C = 0.02) keeps the optimum well conditioned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import probe_oracle as PO      # noqa: E402
from test_gpu_knn_model import B, CLASSES, N_TEST, N_TRAIN, ROOT, datasets, dmvae, dvmoe, vade      # noqa: E402

pytestmark = pytest.mark.gpu

C_REG = 0.02


def check_model(m, vae, train, test):
    from dmvae_hip import probe
    rng_state, orders = np.random.get_state(), (train.order.copy(), test.order.copy())
    acc, conf = m.get_linear_probe_accuracy(None, train, test, C=C_REG, return_confusion=True)
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state()))           # nothing drawn from the NumPy stream
    assert np.array_equal(orders[0], train.order) and np.array_equal(orders[1], test.order)      # and no reshuffle
    assert m.get_linear_probe_accuracy(None, train, test, C=C_REG) == acc
    fitted = m.last_linear_probe_
    assert fitted.converged_ and 1 <= fitted.n_iter_ <= 200

    xs, ys = train._rows[train.order], train._cls[train.order]                                  # the evaluated order
    xq, yq = test._rows[test.order], test._cls[test.order]
    Zx, Zq = vae.encode_means_device(xs), vae.encode_means_device(xq)
    clf = probe.LogisticRegression(C=C_REG, tol=1e-4, max_iter=200, standardize=True).fit(Zx, ys)
    assert np.array_equal(clf.classes_, np.arange(CLASSES))
    assert np.array_equal(clf.coef_, fitted.coef_) and np.array_equal(clf.intercept_, fitted.intercept_)
    pred = clf.predict(Zq)
    assert acc == float(np.mean(pred == yq)) == clf.score(Zq, yq) and 0.0 <= acc <= 1.0
    want = np.zeros((CLASSES, CLASSES), dtype=np.int64)
    np.add.at(want, (pred, yq), 1)
    assert conf.shape == (CLASSES, CLASSES) and np.array_equal(conf, want) and conf.sum() == N_TEST

    zx, zq = Zx.cpu().numpy(), Zq.cpu().numpy()
    sh, sc = PO.standardization(zx)
    Wo, bo = PO.optimum(zx, ys, CLASSES, C_REG, sh, sc)
    lo = PO.scores(zq, Wo, bo, sh, sc)
    top = np.sort(lo, axis=1)
    clear = top[:, -1] - top[:, -2] >= 0.1
    assert clear.sum() >= N_TEST // 2                            # what this test needs of its rows
    assert np.array_equal(pred[clear], np.argmax(lo, axis=1)[clear])
    return acc


def test_dmvae_equals_the_probe_on_its_means_and_the_oracle():
    m = dmvae()
    train, test = datasets()
    check_model(m, m, train, test)


def test_vade_inherits_it():
    m = vade()
    train, test = datasets()
    check_model(m, m, train, test)


def test_dvmoe_forwards_to_its_gate():
    from includes.utils import MEDataset
    m = dvmoe()
    train, test = datasets(lambda X, cls: MEDataset((X, cls, np.eye(CLASSES)[cls].astype(np.float32)), batch_size=B))
    check_model(m, m.vae, train, test)


def test_training_is_what_it_is_without_the_probe():
    def run(with_probe):
        m = dmvae()
        m.define_train_step(0.002, 1000, 0.9)
        train, test = datasets()
        out = [m.train_op(None, train, 1.0)]
        if with_probe:
            m.get_linear_probe_accuracy(None, train, test, C=C_REG)
        out.append(m.train_op(None, train, 1.0))
        # (K = 3 clusters on 4 classes: the clustering accuracy is not defined here; the kNN accuracy reads the same encoder)
        params = m.engine.get_parameters()
        return out + [m.get_knn_accuracy(None, train, test, k=3)], {k: np.array(v) for k, v in params.items()}
    (a, pa), (b, pb) = run(True), run(False)
    assert a == b and all(np.isfinite(v) for v in a)
    assert set(pa) == set(pb) and all(np.array_equal(pa[k], pb[k]) for k in pa)


def test_train_py_probe_writes_probe_test_and_trains_as_without_the_flag(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    base = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--dataset", "synthetic", "--n_epochs", "1", "--eval", "device",
            "--batch_size", "1000", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    procs = []
    for name, extra in (("with", ["--probe", "--probe_C", "0.5"]), ("without", [])):
        d = tmp_path / name
        d.mkdir()
        procs.append((d, subprocess.Popen(base + extra, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    outs = []
    for d, pr in procs:
        so, se = pr.communicate(timeout=900)
        assert pr.returncode == 0, (so[-2000:], se[-3000:])
        outs.append((so + se, [json.loads(l) for l in open(d / "dmvae_metrics.jsonl")]))
    (on, rec_on), (off, rec_off) = outs
    assert "probeTest=" in on and "probeTest" not in off
    assert len(rec_on) == 1 and len(rec_off) == 1
    assert set(rec_on[0]) - set(rec_off[0]) == {"probeTest", "probe_C", "probe_iters"} and set(rec_off[0]) <= set(rec_on[0])
    assert 0.0 <= rec_on[0]["probeTest"] <= 1.0 and rec_on[0]["probe_C"] == 0.5 and 1 <= rec_on[0]["probe_iters"] <= 200
    assert rec_on[0]["loss"] == rec_off[0]["loss"] and rec_on[0]["acc_test"] == rec_off[0]["acc_test"]      # the NumPy stream is untouched
