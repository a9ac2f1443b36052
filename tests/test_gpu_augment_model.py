"""Dataset(augment=...) / train_rows through the training loops, and get_augmentation_consistency, on the GPU.  The warp
itself is held to the float64 oracle in tests/test_gpu_augment.py; here the plumbing is held in bits to epochs on the kernel's own draws."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import binarize_oracle as BO                 # noqa: E402

pytestmark = pytest.mark.gpu

SIDE, I, D, K, B, N = 8, 64, 5, 3, 32, 96
SPEC = "rotate=25,translate=1.5,scale=0.8:1.2,shear=10"
IDENTITY = "rotate=0,translate=0,scale=1:1,shear=0"
FAR = "translate=1e6"                        # every row is pushed out of view (the tests read the draws back and assert it)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=torch.float32)


def small_model(seed=3, cls=None, **kw):
    import base_models
    cls = cls or base_models.DeepMixtureVAE
    layers = dict(enc_layers=(64, 48), dec_layers=(80, 48, 64))
    if cls is base_models.DeepMixtureVAE:
        layers["head_dim"] = 80
    m = cls("m", "binary", I, D, K, activation="relu", initializer="xavier", batch_size=B, dtype="bf16", seed=seed, **layers, **kw).build_graph()
    m.define_train_step(0.002, 1000, 0.9)
    return m


@pytest.fixture(scope="module")
def rows():
    rng = np.random.RandomState(17)
    X = (rng.rand(N, I) * (rng.rand(N, I) < 0.6)).astype(np.float32)
    return X, rng.randint(0, K, N)


def draw(X, spec, seed, counter):
    """the kernel's own draw of the rows, read back"""
    from dmvae_hip.augment import augment
    return augment(dev(X), spec, seed=seed, counter=counter).cpu().numpy()


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in a)


def epoch_on(data_of, n_epochs=1):
    m = small_model()
    np.random.seed(5)
    data = data_of()
    losses = [m.train_op(None, data, 1.0) for _ in range(n_epochs)]
    return m, data, np.float64(losses).view(np.uint64), m.state_dict(), np.random.get_state()


def test_without_augment_train_rows_is_device_rows_and_the_epoch_is_the_plain_one(rows):
    from includes.utils import Dataset
    X, cls = rows
    m, data, la, pa, sa = epoch_on(lambda: Dataset((X, cls), batch_size=B, augment=None, augment_seed=4))
    dv = m.engine.device
    assert data.train_rows(dv) is data.device_rows(dv) and data.train_rows(dv).data_ptr() == data.device_rows(dv).data_ptr()
    assert data.train_rows(dv) is data._device[str(dv)]
    assert not any(k.startswith(("augmented:", "train:")) for k in data._device)
    _, _, lb, pb, sb = epoch_on(lambda: Dataset((X, cls), batch_size=B))
    assert np.isfinite(la.view(np.float64)).all() and np.array_equal(la, lb) and same_bits(pa, pb)
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb))


def test_an_augmented_epoch_equals_an_epoch_on_its_draw(rows):
    from includes.utils import Dataset
    X, cls = rows
    want = draw(X, SPEC, 7, 0)
    assert not np.array_equal(want, X) and want.any()
    m, data, la, pa, sa = epoch_on(lambda: Dataset((X, cls), batch_size=B, augment=SPEC, augment_seed=7))
    _, plain, lb, pb, sb = epoch_on(lambda: Dataset((want, cls), batch_size=B))
    assert np.isfinite(la.view(np.float64)).all() and np.array_equal(la, lb) and same_bits(pa, pb)
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb)) and np.array_equal(data.order, plain.order)      # the same NumPy draws were consumed
    _, _, lc, pc, _ = epoch_on(lambda: Dataset((X, cls), batch_size=B))
    assert not np.array_equal(la, lc)                            # and it is no epoch on the clean rows


def test_two_epochs_redraw_in_place_and_keep_the_captured_step(rows):
    from includes.utils import Dataset
    X, cls = rows
    m = small_model()
    dv = m.engine.device
    np.random.seed(5)
    data = Dataset((X, cls), batch_size=B, augment=SPEC, augment_seed=9)
    assert data.draw_counter_augment() == 0
    l1 = m.train_op(None, data, 1.0)                             # draw 0, then the epoch's reshuffle: counter 1
    buf, replay = data._device["augmented:" + str(dv)], m._replay
    ptr = buf.data_ptr()
    assert replay is not None and data.draw_counter_augment() == 1
    assert np.array_equal(buf.cpu().numpy(), draw(X, SPEC, 9, 0))                # nobody has asked for the rows since
    # the evaluation sees the clean rows: the same accuracy as on a plain data set in the same order, which reshuffles as this one does
    plain = Dataset((X, cls), batch_size=B, shuffle=False)
    plain.order, plain.shuffle = data.order.copy(), True
    np.random.seed(8)
    acc = m.get_accuracy(None, data)                             # reshuffles: counter 2
    np.random.seed(8)
    assert acc == m.get_accuracy(None, plain) and np.array_equal(data.order, plain.order)
    assert data.draw_counter_augment() == 2
    assert data.device_rows(dv) is data._device[str(dv)] and np.array_equal(data.device_rows(dv).cpu().numpy(), X)
    assert np.array_equal(data.data, X[data.order])
    l2 = m.train_op(None, data, 1.0)                             # trains on draw 2, reshuffles: counter 3
    assert data.draw_counter_augment() == 3
    trained_on = buf.cpu().numpy().copy()
    assert np.array_equal(trained_on, draw(X, SPEC, 9, 2)) and not np.array_equal(trained_on, draw(X, SPEC, 9, 0))
    assert m._replay is replay                                   # no recapture: the graph holds the training buffer's address
    again = data.train_rows(dv)
    assert again is buf and again.data_ptr() == ptr and np.array_equal(again.cpu().numpy(), draw(X, SPEC, 9, 3))
    assert np.array_equal(data._device[str(dv)].cpu().numpy(), X) and np.isfinite([l1, l2]).all()
    # the second epoch is an epoch on draw 2: against a plain data set of those rows that continues the first one's order
    m2 = small_model()
    np.random.seed(5)
    d0 = Dataset((draw(X, SPEC, 9, 0), cls), batch_size=B)
    l1b = m2.train_op(None, d0, 1.0)
    np.random.seed(8)
    d0.reshuffle()                                               # (get_accuracy's reshuffle; the evaluation itself changes no parameter)
    d2 = Dataset((draw(X, SPEC, 9, 2), cls), batch_size=B, shuffle=False)
    d2.order, d2.shuffle = d0.order.copy(), True
    l2b = m2.train_op(None, d2, 1.0)
    assert np.array_equal(np.float64([l1, l2]).view(np.uint64), np.float64([l1b, l2b]).view(np.uint64)) and same_bits(m.state_dict(), m2.state_dict())


def test_with_dynamic_binarisation_the_warp_is_binarised(rows):
    from includes.utils import Dataset
    X, cls = rows
    m = small_model()
    dv = m.engine.device
    data = Dataset((X, cls), batch_size=B, shuffle=False, binarize="dynamic", binarize_seed=4, augment=SPEC, augment_seed=9)
    t0 = data.train_rows(dv)
    assert np.array_equal(t0.cpu().numpy(), BO.binarize(draw(X, SPEC, 9, 0), seed=4, counter=0))
    assert np.array_equal(data.device_rows(dv).cpu().numpy(), BO.binarize(X, seed=4, counter=0))      # the clean draw, as ever
    data.reshuffle()
    t1 = data.train_rows(dv)
    assert t1 is t0 and np.array_equal(t1.cpu().numpy(), BO.binarize(draw(X, SPEC, 9, 1), seed=4, counter=1))
    assert np.array_equal(data._device["augmented:" + str(dv)].cpu().numpy(), draw(X, SPEC, 9, 1))
    loss = m.train_op(None, data, 1.0)                           # trains on it
    assert np.isfinite(loss) and set(np.unique(t1.cpu().numpy())) <= {0.0, 1.0}
    held = Dataset((X, cls), batch_size=B, shuffle=False, binarize="static", binarize_seed=4, augment=SPEC, augment_seed=9)
    held.reshuffle()                                             # a static set keeps its binarisation counter, the warp moves on
    assert np.array_equal(held.train_rows(dv).cpu().numpy(), BO.binarize(draw(X, SPEC, 9, 1), seed=4, counter=0))


def test_consistency_under_the_identity_and_under_maps_that_clear_the_image(rows):
    from includes.utils import Dataset
    X, cls = rows
    m = small_model(eval="device")
    np.random.seed(5)
    data = Dataset((X, cls), batch_size=B)
    m.train_op(None, data, 1.0)                                  # (any parameters will do; an epoch moves them off the initial ones)
    order, state = data.order.copy(), np.random.get_state()
    res = m.get_augmentation_consistency(None, data, IDENTITY, n_draws=3, seed=1, counter=2)
    assert res["agree"] == 1.0 and res["acc_aug"] == res["acc_clean"] and res["n"] == N and res["n_draws"] == 3
    assert all(a == 1.0 for a in res["agree_per_class"]) and len(res["agree_per_class"]) == K
    metrics, labels = m.get_cluster_metrics(None, data, silhouette=False, return_labels=True)
    assert res["acc_clean"] == metrics["acc"]
    # every warped row is zeros: all of them fall into the cluster of the zero row
    for j in range(4):
        assert not draw(X, FAR, 6, 4 * 3 + j).any()
    zero_labels = m.get_cluster_metrics(None, Dataset((np.zeros((B, I), np.float32), np.zeros(B, int)), batch_size=B, shuffle=False), silhouette=False,
                                        return_labels=True)[1]
    assert len(set(zero_labels.tolist())) == 1
    share = float((labels == zero_labels[0]).sum()) / N
    far = m.get_augmentation_consistency(None, data, FAR, n_draws=4, seed=6, counter=3)
    print("agree under FAR = %.6f, the share of clean rows in cluster %d = %.6f" % (far["agree"], zero_labels[0], share))
    assert far["agree"] == share and far["acc_clean"] == res["acc_clean"] and 0.0 <= far["acc_aug"] <= 1.0
    per = [float(((labels == zero_labels[0]) & (cls[order] == c)).sum()) / max(1, (cls[order] == c).sum()) for c in range(K)]
    assert far["agree_per_class"] == per
    # a real spec: between the two, and the same bits when asked again; nothing was reshuffled or drawn from NumPy
    a = m.get_augmentation_consistency(None, data, SPEC, n_draws=4, seed=6, counter=3)
    b = m.get_augmentation_consistency(None, data, SPEC, n_draws=4, seed=6, counter=3)
    assert a == b and 0.0 <= a["agree"] <= 1.0 and a["acc_clean"] == res["acc_clean"]
    assert np.array_equal(data.order, order) and all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))
    with pytest.raises(ValueError, match="n_draws"):
        m.get_augmentation_consistency(None, data, SPEC, n_draws=0)
    with pytest.raises(ValueError, match="flip"):
        m.get_augmentation_consistency(None, data, "flip=1")


def test_consistency_runs_for_vade_and_is_refused_for_the_moe_models(rows):
    import base_models
    import models
    from includes.utils import Dataset
    X, cls = rows
    v = small_model(cls=base_models.VaDE, eval="device")
    np.random.seed(5)
    data = Dataset((X, cls), batch_size=B)
    state = np.random.get_state()
    res = v.get_augmentation_consistency(None, data, IDENTITY, n_draws=2, counter=1)
    assert res["agree"] == 1.0 and res["acc_aug"] == res["acc_clean"]          # the same device noise for the clean and the warped rows
    a = v.get_augmentation_consistency(None, data, SPEC, n_draws=2, counter=1)
    assert a == v.get_augmentation_consistency(None, data, SPEC, n_draws=2, counter=1) and 0.0 <= a["agree"] <= 1.0
    assert a["acc_clean"] == v.get_cluster_metrics(None, data, silhouette=False, counter=1)["acc"]
    assert all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))
    moe = models.DeepVariationalMoE("dvmoe", "binary", I, D, 4, K, True, featLearn=0, batch_size=B, dtype="fp32", seed=4, eval="device",
                                    enc_layers=(24,), head_dim=16, dec_layers=(16, 24)).build_graph()
    with pytest.raises(NotImplementedError, match="DeepVariationalMoE: the MoE data set carries regression labels that are functions of the grey rows"):
        moe.get_augmentation_consistency(None, data, SPEC)
