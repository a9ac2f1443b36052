"""GPU tests of the MoE model classes (models.py) and of `train.py --model dvmoe`: train_op on the reference's NumPy stream
(MEDataset order, C drawn before Z) against the float64 oracle, get_accuracy / predict against the oracle, the CLI end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import dmvae_oracle as O      # noqa: E402
import moe_oracle as MO       # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = dict(enc_layers=(64,), head_dim=64, dec_layers=(64,))


def _data(n, I, E, Od, classification, seed):
    r = np.random.RandomState(seed)
    X = (r.rand(n, I) * (r.rand(n, I) < 0.4)).astype(np.float32)
    cls = r.randint(0, 10, n)
    Y = np.eye(Od)[cls % Od] if classification else r.randn(n, Od)
    return X, cls, Y.astype(np.float32)


@pytest.mark.parametrize("gumbel", [False, True])
def test_train_op_host_noise_against_the_oracle(gumbel):
    import models
    from includes.utils import MEDataset
    I, E, Od, D, B = 32, 5, 6, 4, 16
    X, cls, Y = _data(40, I, E, Od, 1, 1)                 # 2 full batches + a short one of 8
    m = models.DeepVariationalMoE("dvmoe", "binary", I, D, Od, E, True, featLearn=0, batch_size=B, dtype="fp32", noise="host",
                                  gumbel=gumbel, seed=3, **LAYERS).build_graph()
    m.define_train_step(0.002, 100)
    p = {k: v.astype(np.float64) for k, v in m.engine.get_parameters().items()}
    cfg = O.Config(I, D, E, LAYERS["enc_layers"], LAYERS["head_dim"], LAYERS["dec_layers"], "binary")
    np.random.seed(5)
    data = MEDataset((X, cls, Y), batch_size=B)
    out = [m.train_op(None, data, 1.0) for _ in range(2)]
    # the oracle on the same stream: one permutation per epoch, then per batch C (gumbel) before Z
    np.random.seed(5)
    mm, vv = O.adam_tf_init(p)
    order = np.arange(40)
    t = 0
    for ep in range(2):
        order = order[np.random.permutation(40)]
        loss = loss_cls = 0.0
        for s in range(0, 40, B):
            o = order[s:s + B]
            n = len(o)
            g_ = O.sample_gumbel((n, 1, E)).reshape(n, E)          # C is drawn first in both modes (base_models.py:122-124)
            g_ = g_ if gumbel else None
            eps = np.random.randn(n, D)
            eps = eps.astype(np.float32).astype(np.float64)
            if g_ is not None:
                g_ = g_.astype(np.float32).astype(np.float64)
            a = MO.forward(p, cfg, X[o].astype(np.float64), eps, Y[o].astype(np.float64), E, Od, 0, 1, 1,
                           mode="relaxed" if gumbel else "exact", gumbel=g_)
            g = MO.backward(p, cfg, a, E, Od, 0, 1, 1)
            t += 1
            O.adam_tf(p, g, mm, vv, t, 0.002)
            loss += a["loss_total"] / data.epoch_len
            loss_cls += a["loss_moe"] / data.epoch_len
            batch_acc = 1 - a["error"] / n
        got = out[ep]
        assert abs(got[0] - loss) <= 1e-3 * max(1.0, abs(loss)), (ep, got[0], loss)
        assert abs(got[2] - loss_cls) <= 1e-3 * max(1.0, abs(loss_cls)), (ep, got[2], loss_cls)
        assert abs(got[1] - batch_acc) <= 1e-9, (ep, got[1], batch_acc)
    assert m.engine.read_state().adam_t == 6


@pytest.mark.parametrize("classification", [1, 0])
def test_get_accuracy_and_predict_against_the_oracle(classification):
    import models
    from includes.utils import MEDataset, get_moe_clustering_accuracy
    I, E, Od, B = 32, 5, 10 if classification else 3, 16
    X, cls, Y = _data(45, I, E, Od, classification, 2)
    m = models.DeepMoE("dmoe", "binary", I, Od, E, classification, featLearn=0, batch_size=B, dtype="fp32", seed=4, **LAYERS).build_graph()
    m.define_train_step(0.002, 100)
    p = {k: v.astype(np.float64) for k, v in m.engine.get_parameters().items()}
    data = MEDataset((X, cls, Y), batch_size=B, shuffle=False)
    acc, acc_cl = m.get_accuracy(None, data)                  # E = 5 experts on 10 classes: the reference would raise here
    cfg = O.Config(I, 1, E, LAYERS["enc_layers"], LAYERS["head_dim"], LAYERS["dec_layers"], "binary")
    a = O.encode(p, cfg, X.astype(np.float64))
    q = O.softmax(a["logits"])
    r = MO.head_forward(MO.expert_outputs(p, X.astype(np.float64), E, Od), q, Y.astype(np.float64), classification)
    if classification:
        assert abs(acc - (1 - r["err_rows"].sum() / 45)) <= 1.5 / 45
    else:
        ref = -sum(r["err_rows"][s:s + B].sum() / len(r["err_rows"][s:s + B]) for s in range(0, 45, B)) / data.epoch_len
        assert abs(acc - ref) <= 1e-4 * max(1.0, abs(ref))
    assert abs(acc_cl - get_moe_clustering_accuracy(a["logits"], cls, 10)) <= 1.5 / 45
    hard, soft = m.predict(X)
    np.testing.assert_allclose(soft, r["pred"], rtol=1e-4, atol=1e-5 * max(1.0, np.abs(r["pred"]).max()))
    if classification:
        assert np.array_equal(hard.sum(1), np.ones(45))


def test_train_py_dvmoe_classification_two_epochs(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    cmd = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--model", "dvmoe", "--classification", "--dataset",
           "synthetic", "--n_epochs", "2", "--batch_size", "500", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in open(tmp_path / "dvmoe_metrics.jsonl")]
    assert [l["epoch"] for l in lines] == [0, 1] and all(np.isfinite(l["loss"]) for l in lines)
    ck = tmp_path / "saved-models" / "synthetic" / "dvmoe" / "model" / "parameters.ckpt"
    with np.load(ck, allow_pickle=False) as f:
        assert f["regression_weights"].shape == (5, 10, 784) and f["regression_biases"].shape == (10, 5)
    r2 = subprocess.run(cmd[:-10] + ["--n_epochs", "1", "--batch_size", "500", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"],
                        cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0 and "Restored" in r2.stdout, (r2.stdout[-2000:], r2.stderr[-2000:])
