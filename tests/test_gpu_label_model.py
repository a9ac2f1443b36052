"""GPU test of semi-supervised training through the model class (base_models.DeepMixtureVAE(label_weight=...)): a toy of K = 4 separable
blobs in 32 dimensions squashed into [0, 1], 400 rows, 8 labelled per class, batches of 64 (six full ones and a tail of 16 per epoch), 40
epochs = 280 steps.  One model trains at label_weight = 1, one with the attachment at label_weight = 0, from the same seed and the same
NumPy stream.  The supervised run's cross-entropy on the labelled rows -- computed by the float64 oracle from encode()'s logits -- must lie
below its own value before training AND below the unweighted run's value after training: a comparison against the behaviour without the
feature; no accuracy threshold is set, nobody has measured one.  Then `train.py --n_labeled` end to end on the synthetic stand-in (two
epochs, bf16, the pipelined captured steps): the JSONL carries the new fields, every label is seen once per epoch, `--model vade` refuses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import label_xent_oracle as LO      # noqa: E402

pytestmark = pytest.mark.gpu

I, D, K, N, B, EPOCHS = 32, 4, 4, 400, 64, 40
LAYERS = dict(enc_layers=(64,), head_dim=64, dec_layers=(64,))


def blobs():
    rng = np.random.RandomState(12)
    centres = rng.randn(K, I) * 2.0
    cls = np.arange(N) % K
    X = centres[cls] + 0.5 * rng.randn(N, I)
    return (1.0 / (1.0 + np.exp(-X))).astype(np.float32), cls.astype(np.int64)


def train(X, cls, labeled, alpha):
    import base_models
    from includes.utils import Dataset
    m = base_models.DeepMixtureVAE("toy", "binary", I, D, K, batch_size=B, dtype="fp32", seed=3, label_weight=alpha, **LAYERS).build_graph()
    m.define_train_step(0.002, 10 ** 6)
    np.random.seed(21)
    data = Dataset((X, cls), batch_size=B, labeled=labeled)
    before = LO.mean_xent(m.encode(X[labeled])[2], cls[labeled])
    for _ in range(EPOCHS):
        loss = m.train_op(None, data, 1.0)
    after = LO.mean_xent(m.encode(X[labeled])[2], cls[labeled])
    return m, data, before, after, loss


def test_labels_pull_the_clusters_onto_their_classes():
    from includes.utils import choose_labeled
    X, cls = blobs()
    labeled = choose_labeled(cls, 8 * K, K, seed=0)
    sup, data, before, after, loss = train(X, cls, labeled, 1.0)
    ep = dict(sup.last_epoch)
    # the labelled rows of the epoch's batches, counted on the host from the order the epoch was trained in (one rank: every row is trained)
    order = data.order
    assert ep["rows"] == N and ep["label_rows"] == int((data.host_labels()[order[:ep["rows"]]] >= 0).sum()) == 8 * K
    assert np.isfinite(loss) and np.isfinite(ep["label_xent"]) and 0.0 <= ep["label_acc"] <= 1.0
    assert sup.engine.label_acc()[1] == 8 * K          # the accumulators hold ONE epoch: the capture's warm-up steps are not in them
    # get_direct_accuracy: the trace of the host confusion matrix over N
    logits = sup.encode(X)[2]
    conf = np.zeros((K, K), dtype=np.int64)
    np.add.at(conf, (np.argmax(logits, axis=1), cls), 1)
    state = np.random.get_state()
    direct = sup.get_direct_accuracy(None, data)
    assert direct == np.trace(conf) / N
    assert np.array_equal(state[1], np.random.get_state()[1])      # no reshuffle
    plain, _, before0, after0, _ = train(X, cls, labeled, 0.0)
    print("label model: xent on the labelled rows %.4f -> %.4f with labels, %.4f -> %.4f at weight 0; direct accuracy %.3f vs %.3f" % (
        before, after, before0, after0, direct, plain.get_direct_accuracy(None, data)))
    assert before == before0                           # the same start
    assert after < before and after < after0
    # the epoch's running mean of l_r (over the steps, while the weights move) and the final value agree in kind
    assert ep["label_xent"] < before
    assert plain.last_epoch["label_rows"] == 8 * K and plain.engine.label_err() == 0


def test_train_op_needs_labeled_rows_and_in_range_classes():
    import base_models
    from includes.utils import Dataset
    X, cls = blobs()
    m = base_models.DeepMixtureVAE("toy", "binary", I, D, K, batch_size=B, dtype="fp32", seed=3, label_weight=1.0, **LAYERS).build_graph()
    m.define_train_step(0.002, 10 ** 6)
    with pytest.raises(ValueError, match="labeled"):
        m.train_op(None, Dataset((X, cls), batch_size=B), 1.0)
    with pytest.raises(ValueError, match="n_classes"):
        m.train_op(None, Dataset((X, cls + 1), batch_size=B, labeled=np.arange(N)), 1.0)


def test_train_py_n_labeled_two_epochs(tmp_path):
    """the CLI end to end on the synthetic stand-in: the flags reach the model, the JSONL carries the new fields, and VaDE refuses"""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    cmd = [sys.executable, os.path.join(root, "deep-mixture-vae_amd", "train.py"), "--model", "dmvae", "--dataset", "synthetic", "--n_epochs", "2",
           "--batch_size", "500", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128", "--eval", "device",
           "--n_labeled", "100", "--label_weight", "0.5", "--label_seed", "3"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in open(tmp_path / "dmvae_metrics.jsonl")]
    assert [l["epoch"] for l in lines] == [0, 1]
    for l in lines:
        assert l["n_labeled"] == 100 and l["label_weight"] == 0.5 and l["label_rows"] == 100      # one rank trains every row: every label is seen once
        assert np.isfinite(l["label_xent"]) and 0.0 <= l["acc_direct_test"] <= 1.0 and 0.0 <= l["label_acc"] <= 1.0 and np.isfinite(l["loss"])
    r2 = subprocess.run(cmd[:3] + ["vade"] + cmd[4:], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode != 0 and "--n_labeled" in r2.stderr
