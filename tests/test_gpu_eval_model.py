"""GPU tests of eval="device" on the model classes and of `train.py --eval device`: the device confusion matrix equals the one
built on the host from the logits `encode` returns (the same encoder kernels on the same rows: exactly), get_accuracy agrees
between the two modes, the NumPy stream and the training result do not depend on the mode."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(enc_layers=(70, 50), head_dim=90, dec_layers=(90, 50, 30))       # the small model of tests/test_gpu_model.py
GAP = 2e-4                # 10 x the bar of the responsibilities (tests/test_gpu_eval.py)


def rows_and_classes(N, dim, K, seed):
    rng = np.random.RandomState(seed)
    return (rng.rand(N, dim) * (rng.rand(N, dim) < 0.4)).astype(np.float32), rng.randint(0, K, N)


def confusion(weights, classes, R):
    d = np.zeros((R, R), dtype=np.int64)
    np.add.at(d, (np.argmax(weights, axis=-1), np.asarray(classes, dtype=np.int64)), 1)
    return d


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def dmvae(dtype, eval, **kw):
    import base_models
    args = dict(SMALL, batch_size=16, dtype=dtype, noise="host", seed=3, eval=eval)
    args.update(kw)
    m = base_models.DeepMixtureVAE("dmvae", "binary", 40, 6, 5, activation="relu", initializer="xavier", **args).build_graph()
    m.define_train_step(0.002, 1000, 0.9)
    return m


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dmvae_device_confusion_and_accuracy_equal_the_host_path(dtype):
    from includes.utils import Dataset
    X, cls = rows_and_classes(16 * 7 + 5, 40, 5, 1)                # a short last batch
    m = dmvae(dtype, "device")
    np.random.seed(2)
    data = Dataset((X, cls), batch_size=16)
    m.train_op(None, data, 1.0)                                    # off the initial parameters
    order = data.order
    got = m._device_confusion(data, order, 5)
    want = confusion(m.encode(X[order])[2], cls[order], 5)
    assert np.array_equal(got, want) and got.sum() == len(X)
    state = np.random.get_state()
    acc_d = m.get_accuracy(None, data)
    after_d = np.random.get_state()
    np.random.set_state(state)
    m.eval = "host"
    acc_h = m.get_accuracy(None, data)
    assert acc_d == acc_h and 0.0 < acc_d <= 1.0
    assert same_state(after_d, np.random.get_state())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dvmoe_device_accuracy_equals_the_host_path(dtype):
    import models
    from includes.utils import MEDataset
    X, cls = rows_and_classes(16 * 5 + 9, 32, 10, 2)               # E = 5 experts on 10 classes: R = 10 > K
    Y = np.eye(10)[cls].astype(np.float32)
    layers = dict(enc_layers=(64,), head_dim=64, dec_layers=(64,))
    m = models.DeepVariationalMoE("dvmoe", "binary", 32, 4, 10, 5, True, featLearn=0, batch_size=16, dtype=dtype, seed=4,
                                  eval="device", **layers).build_graph()
    m.define_train_step(0.002, 100)
    np.random.seed(3)
    data = MEDataset((X, cls, Y), batch_size=16)
    m.train_op(None, data, 1.0)
    state = np.random.get_state()
    got_d = m.get_accuracy(None, data)
    after_d = np.random.get_state()
    np.random.set_state(state)
    m.eval = "host"
    got_h = m.get_accuracy(None, data)
    assert got_d == got_h and same_state(after_d, np.random.get_state())
    # and the matrix itself, through the plan entry, against the logits the gate's encoder returns for those rows
    eng, order = m.engine, data.order
    conf = eng.confusion_buffer(10, eng.device)
    cd, pd = data.device_classes(eng.device), torch.as_tensor(order.astype(np.int32)).to(eng.device)
    rows = data.device_rows(eng.device)
    for s in range(0, len(X), 16):
        n = min(16, len(X) - s)
        eng.load_batch(rows, pd, s, n)
        eng.eval_clusters(conf, cd, pd, s, n)
    assert np.array_equal(eng.read_confusion(conf), confusion(m.vae.encode(X[order])[2], cls[order], 10))


def vade(eval, noise, dtype="fp32"):
    import base_models
    m = base_models.VaDE("vade", "binary", 40, 6, 5, activation="relu", initializer="xavier", batch_size=16, dtype=dtype, noise=noise,
                         seed=3, enc_layers=(70, 50, 30), dec_layers=(30, 50, 70), eval=eval).build_graph()
    m.define_train_step(0.002, 1000, 0.9)
    rng = np.random.RandomState(9)
    m.engine.set_parameters({"prior_means": (0.3 * rng.randn(5, 6)).astype(np.float32)})
    return m


def test_vade_host_noise_consumes_the_same_stream_and_agrees_up_to_near_ties():
    from includes.utils import Dataset
    X, cls = rows_and_classes(16 * 6 + 3, 40, 5, 5)
    m = vade("device", "host")
    np.random.seed(4)
    data = Dataset((X, cls), batch_size=16)
    state = np.random.get_state()
    acc_d = m.get_accuracy(None, data, k=4)
    after_d = np.random.get_state()
    np.random.set_state(state)
    m.eval = "host"
    acc_h = m.get_accuracy(None, data, k=4)
    assert same_state(after_d, np.random.get_state()) and not same_state(state, after_d)
    # the share of rows whose two largest averaged responsibilities are within the gap: the two arg-maxes may differ there only
    np.random.set_state(state)
    w = np.mean(np.array([m.cluster_probabilities(data.data, m.sample_reparametrization_variables(len(X), variables=["Z"])[m.epsilon])
                          for _ in range(4)]), axis=0)
    top = np.sort(w, axis=1)
    near = float(((top[:, -1] - top[:, -2]) <= GAP).mean())
    print("acc device %.6f host %.6f, near-tie share %.4f" % (acc_d, acc_h, near))
    assert abs(acc_d - acc_h) <= near + 1e-12


def test_vade_device_noise_draws_nothing_from_numpy_and_is_reproducible():
    from includes.utils import Dataset
    X, cls = rows_and_classes(16 * 6 + 3, 40, 5, 6)
    np.random.seed(4)
    data = Dataset((X, cls), batch_size=16)
    accs = []
    for _ in range(2):
        m = vade("device", "device")
        state = np.random.get_state()
        accs.append([m.get_accuracy(None, data, k=3) for _ in range(2)])
        assert same_state(state, np.random.get_state())
    assert accs[0] == accs[1] and all(0.0 < a <= 1.0 for a in accs[0])


@pytest.mark.parametrize("dtype,noise", [("fp32", "host"), ("bf16", "device")])
def test_training_does_not_depend_on_the_evaluation_mode(dtype, noise):
    from includes.utils import Dataset
    X, cls = rows_and_classes(16 * 4 + 7, 40, 5, 7)
    out = []
    for mode in ("host", "device"):
        m = dmvae(dtype, mode, noise=noise)
        np.random.seed(11)
        data = Dataset((X, cls), batch_size=16)
        accs = []
        for _ in range(3):
            m.train_op(None, data, 1.0)
            accs.append(m.get_accuracy(None, data))
        torch.cuda.synchronize()
        out.append((accs, m.engine.param.clone(), m.engine.m.clone(), m.engine.v.clone(), np.random.get_state()))
    assert out[0][0] == out[1][0] and same_state(out[0][4], out[1][4])
    assert all(torch.equal(out[0][i], out[1][i]) for i in (1, 2, 3))


def test_train_py_eval_device_writes_eval_seconds(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    cmd = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--eval", "device", "--dataset", "synthetic", "--n_epochs", "1",
           "--batch_size", "1000", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    rec = [json.loads(l) for l in open(tmp_path / "dmvae_metrics.jsonl")]
    assert len(rec) == 1 and rec[0]["eval"] == "device" and rec[0]["eval_seconds"] > 0 and 0.0 < rec[0]["acc_test"] <= 1.0
