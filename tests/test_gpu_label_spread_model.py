"""GPU tests of dmvae_hip.spread.LabelSpreading, of get_few_label_accuracy (base_models.py, models.py) and of train.py --few_label: the
classifier against the float64 oracle of tests/helpers/label_spread_oracle.py built from the SAME dmvae_knn lists, the evaluator against the
classifier applied by hand to encode_means_device of the same rows with the same choose_labeled rows (exactly: the same kernels on the same
rows), and the CLI end to end on the synthetic stand-in."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import label_spread_oracle as LO      # noqa: E402
import moe_cases as MC                # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, D, K, B, N_TRAIN, N_TEST, CLASSES = MC.SMALL["input_dim"], 4, 4, 20, 120, 40, 4
KEYS = ("accuracy", "accuracy_unlabeled_train", "n_unreached", "n_iter", "change", "per_class", "knn1", "probe")


def test_label_spreading_fit_is_the_oracle_on_the_same_lists():
    import torch
    from dmvae_hip import knn, spread
    N, Cn, k = 1000, 10, 10
    X, cls = LO.blobs(N, Cn, 10, 7)
    y = np.where((np.arange(N) // Cn) % 10 == 0, cls, -1)              # 100 labels, ten of every class
    assert (y >= 0).sum() == 100
    Xd = torch.as_tensor(X).cuda()
    ls = spread.LabelSpreading(n_neighbors=k, alpha=0.8).fit(Xd, y)
    assert ls.n_unreached_ == 0 and ls.n_iter_ % 8 == 0 and 8 <= ls.n_iter_ < 1000 and ls.change_ < 1e-6
    assert np.array_equal(ls.classes_, np.arange(Cn))
    dist = ls.label_distributions_.cpu().numpy()
    assert dist.shape == (N, Cn) and np.allclose(dist.sum(axis=1), 1.0, atol=1e-5)

    idx, d2 = knn.knn_enqueue(Xd, Xd, k, self_first=0)
    indptr, indices, values = LO.csr_from_dense(LO.dense_graph(idx.cpu().numpy().astype(np.int64), d2.cpu().numpy().astype(np.float64)))
    gp, gi, gv = (t.cpu().numpy() for t in ls.graph_)
    assert np.array_equal(gp, indptr) and np.array_equal(gi, indices) and np.allclose(gv * float(N), values, rtol=1e-6)
    s, _ = LO.normalize(indptr, indices, values)
    Fo, _ = LO.iterate(indptr, indices, s, y, Cn, float(np.float32(0.8)), ls.n_iter_)
    Fy, _ = LO.iterate_f32(indptr, indices, s, y, Cn, 0.8, ls.n_iter_)
    assert np.all(MC.clear_rows(Fo, Fy))                               # what this comparison needs of its rows
    want = LO.predict(Fo)
    assert np.array_equal(ls.transduction_, want)
    free = y < 0
    assert ls.score(cls, free) >= float(np.mean(want[free] == cls[free])) >= 0.5
    assert ls.score(cls) == float(np.mean(ls.transduction_ == cls))
    heat = spread.LabelSpreading(n_neighbors=k, alpha=0.8, weights="heat").fit(Xd, y)
    assert heat.n_unreached_ == 0 and heat.score(cls, free) > 0.2      # (twice chance: the weighting is exercised end to end, not ranked)


def rows_and_classes(n, seed):
    """binary rows around 8 prototypes, 4 classes: rows of one prototype encode alike"""
    protos = np.random.RandomState(11).rand(8, I) < 0.4
    rng = np.random.RandomState(seed)
    which = np.arange(n) % 8
    X = np.logical_xor(protos[which], rng.rand(n, I) < 0.1).astype(np.float32)
    return X, (which % CLASSES).astype(np.int64)


def datasets():
    from includes.utils import Dataset
    np.random.seed(5)
    return Dataset(rows_and_classes(N_TRAIN, 1), batch_size=B), Dataset(rows_and_classes(N_TEST, 2), batch_size=B)


def small(kind):
    import base_models
    kw = dict(activation="relu", initializer="xavier", batch_size=B, dtype="fp32", seed=3, eval="device")
    if kind == "dmvae":
        return base_models.DeepMixtureVAE("dmvae", "binary", I, D, K, enc_layers=MC.SMALL["enc_layers"], head_dim=MC.SMALL["head_dim"],
                                          dec_layers=MC.SMALL["dec_layers"], **kw).build_graph()
    return base_models.VaDE("vade", "binary", I, D, K, enc_layers=MC.SMALL["enc_layers"], dec_layers=MC.SMALL["dec_layers"], **kw).build_graph()


@pytest.mark.parametrize("kind", ["dmvae", "vade"])
def test_few_label_accuracy_is_label_spreading_on_the_means(kind):
    import torch
    from dmvae_hip import spread
    from includes.utils import choose_labeled
    m = small(kind)
    m.define_train_step(0.002, 1000, 0.9)
    train, test = datasets()
    for _ in range(3):
        m.train_op(None, train, 1.0)
    rng_state, orders = np.random.get_state(), (train.order.copy(), test.order.copy())
    params = {k: np.array(v) for k, v in m.engine.get_parameters().items()}
    res = m.get_few_label_accuracy(None, train, test, n_labeled=20, seed=0, k=7, alpha=0.8)
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state()))           # nothing drawn from the NumPy stream
    assert np.array_equal(orders[0], train.order) and np.array_equal(orders[1], test.order)      # no reshuffle
    after = m.engine.get_parameters()
    assert all(np.array_equal(params[k], after[k]) for k in params)                              # and no parameter written
    for key in KEYS:
        assert key in res and np.all(np.isfinite(np.asarray(res[key], dtype=np.float64))), key
    assert res["n_labeled"] == 20 and len(res["per_class"]) == CLASSES and res["n_iter"] >= 8
    assert all(0.0 <= res[key] <= 1.0 for key in ("accuracy", "accuracy_unlabeled_train", "knn1", "probe"))

    def by_hand(rows):
        Z = torch.cat([m.encode_means_device(train._rows), m.encode_means_device(test._rows)])
        y = np.full(N_TRAIN + N_TEST, -1, dtype=np.int64)
        y[rows] = train._cls[rows]
        ls = spread.LabelSpreading(n_neighbors=7, alpha=0.8).fit(Z, y)
        return ls, float(np.mean(ls.transduction_[N_TRAIN:] == test._cls))

    rows = choose_labeled(train._cls, 20, CLASSES, 0)
    ls, acc = by_hand(rows)
    assert res["accuracy"] == acc and res["n_iter"] == ls.n_iter_ and res["n_unreached"] == ls.n_unreached_ and res["change"] == ls.change_
    assert np.array_equal(m.last_label_spreading_.transduction_, ls.transduction_)
    assert m.get_few_label_accuracy(None, train, test, n_labeled=20, seed=0) == res              # two calls, the same figures
    other = np.arange(0, N_TRAIN, 5)
    res2 = m.get_few_label_accuracy(None, train, test, n_labeled=20, seed=0, labeled=other)      # labeled= overrides the draw
    assert res2["n_labeled"] == len(other) and res2["accuracy"] == by_hand(other)[1]
    with pytest.raises(ValueError):
        m.get_few_label_accuracy(None, train, test, labeled=[N_TRAIN])                           # a test row may not carry a label


def test_train_py_few_label_writes_its_keys_and_nothing_without_the_flag(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    base = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--dataset", "synthetic", "--n_epochs", "2", "--eval", "device",
            "--batch_size", "1000", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    procs = []
    for name, extra in (("with", ["--few_label", "20"]), ("without", [])):
        d = tmp_path / name
        d.mkdir()
        procs.append((d, subprocess.Popen(base + extra, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    outs = []
    for d, pr in procs:
        so, se = pr.communicate(timeout=900)
        assert pr.returncode == 0, (so[-2000:], se[-3000:])
        outs.append((so + se, [json.loads(l) for l in open(d / "dmvae_metrics.jsonl")]))
    (on, rec_on), (off, rec_off) = outs
    keys = {"few_label_test", "few_label_unlabeled_train", "few_label_knn1", "few_label_probe", "few_label_unreached", "few_label_iters", "few_label_n"}
    assert "flTest=" in on and "flTest" not in off
    assert len(rec_on) == 2 and len(rec_off) == 2
    for a, b in zip(rec_on, rec_off):
        assert set(a) - set(b) == keys and set(b) <= set(a)
        assert a["few_label_n"] == 20 and a["few_label_iters"] >= 8 and a["few_label_unreached"] >= 0
        assert all(0.0 <= a[k] <= 1.0 for k in ("few_label_test", "few_label_unlabeled_train", "few_label_knn1", "few_label_probe"))
        assert a["loss"] == b["loss"] and a["acc_test"] == b["acc_test"]                         # the run trains as it does without the flag
