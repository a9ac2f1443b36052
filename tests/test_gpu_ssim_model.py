"""GPU tests of get_reconstruction_quality and get_sample_diversity (base_models.py, models.py) and of train.py --recon_quality
--sample_diversity: a tiny fp32 plan -- input 144 = 12 x 12, latent 4, K = 3, batch 8 -- on 50 rows with classes (a ragged last batch, one
class without rows, a few repeated rows so that SSIM values tie), the default 11-tap window (4 windows per image).  The methods must
equal dmvae_hip.ssim on images rebuilt from the public pieces -- reconstruct(X), sample_prior_device -- exactly, and the float64 oracle of
tests/helpers/ssim_oracle.py on those images within the kernel's bound 8 (11^2 + 3) 2^-24."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import ssim_oracle as SO      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, I, D, K, B, N_ROWS, CLASSES = 12, 144, 4, 3, 8, 50, 5
LAYERS = dict(enc_layers=(24,), head_dim=16, dec_layers=(16, 24))
C1, C2 = SO.constants()
W11 = SO.gaussian_window()
BOUND = SO.u_bound(11)


def rows_and_classes():
    """MNIST-like 12 x 12 rows; classes 0, 1, 2, 4 (class 3 has no row); rows 20, 21, 33 repeat rows 3, 3, 7: their SSIM values tie"""
    X = SO.mnist_like(N_ROWS, 1, SIDE, SIDE, seed=2)
    X[20], X[21], X[33] = X[3], X[3], X[7]
    cls = np.array([0, 1, 2, 4])[np.random.RandomState(3).randint(0, 4, N_ROWS)].astype(np.int64)
    return X, cls


def dataset(make=None):
    from includes.utils import Dataset
    np.random.seed(5)                                            # shuffled at construction: the evaluated order is no identity
    make = make or (lambda X, cls: Dataset((X, cls), batch_size=B))
    return make(*rows_and_classes())


def spread(m):
    """prior components apart and wide: the draws of a component differ, and so do the components"""
    p = m.engine.get_parameters()
    rng = np.random.RandomState(1)
    m.engine.set_parameters({"prior_means": 2.0 * rng.randn(*p["prior_means"].shape), "prior_log_vars": 1.0 + 0.5 * rng.randn(*p["prior_log_vars"].shape)})
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


def check_reconstruction(m, vae, data):
    from dmvae_hip import ssim as S
    rng_state, order = np.random.get_state(), data.order.copy()
    res, images = m.get_reconstruction_quality(None, data, return_images=True)
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state()))           # nothing drawn from the NumPy stream
    assert np.array_equal(order, data.order)                                                     # and no reshuffle
    again = m.get_reconstruction_quality(None, data)
    assert set(again) == set(res) == {"ssim", "mse", "psnr", "n", "image_shape", "worst", "worst_ssim", "ssim_per_class", "mse_per_class"}
    for name in res:                                             # a second call: the same bits
        assert np.array_equal(res[name], again[name], equal_nan=True), name
    assert res["n"] == N_ROWS and tuple(res["image_shape"]) == (SIDE, SIDE)

    xs = data._rows[data.order]                                  # the evaluated order
    R = vae.reconstruct(xs)                                      # the public path: encode, decode the means
    assert np.array_equal(images.cpu().numpy(), R)               # the judged images ARE reconstruct(X)
    sv, mse_rows, _ = S.ssim(xs, R, (SIDE, SIDE))
    assert res["ssim"] == sv.mean() and res["mse"] == mse_rows.mean() and res["psnr"] == 10.0 * np.log10(1.0 / mse_rows.mean())
    want_s, want_e = SO.ssim_rows(xs, R, (1, SIDE, SIDE), W11, C1, C2)
    print("%s: ssim %.4f psnr %.2f; largest |ssim - oracle| %.3g" % (type(m).__name__, res["ssim"], res["psnr"], np.abs(sv - want_s).max()))
    assert np.abs(sv - want_s).max() <= BOUND and abs(res["ssim"] - want_s.mean()) <= BOUND
    assert abs(res["mse"] - want_e.mean() / I) <= (I + 2) * 2.0 ** -24 * want_e.mean() / I
    assert res["ssim"] < 0.9 and len(np.unique(sv)) > N_ROWS // 2                              # an untrained model: no constant

    cls = data._cls[data.order]
    count = np.bincount(cls, minlength=CLASSES)
    assert count[3] == 0 and (np.delete(count, 3) > 0).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(res["ssim_per_class"], np.bincount(cls, weights=sv, minlength=CLASSES) / count, equal_nan=True)
        assert np.array_equal(res["mse_per_class"], np.bincount(cls, weights=mse_rows, minlength=CLASSES) / count, equal_nan=True)
        oracle_pc = np.bincount(cls, weights=want_s, minlength=CLASSES) / count
    assert np.isnan(res["ssim_per_class"][3]) and np.isnan(res["mse_per_class"][3]) and np.isnan(oracle_pc[3])
    assert np.nanmax(np.abs(res["ssim_per_class"] - oracle_pc)) <= BOUND

    idx = np.argsort(sv, kind="stable")
    assert np.array_equal(res["worst"], data.order[idx[:10]]) and np.array_equal(res["worst_ssim"], sv[idx[:10]])
    full = m.get_reconstruction_quality(None, data, n_worst=N_ROWS)
    assert np.array_equal(full["worst"], data.order[idx]) and len(np.unique(sv)) < N_ROWS          # ties exist, and go to the earlier row
    pos = {int(r): i for i, r in enumerate(full["worst"])}
    where = {int(r): i for i, r in enumerate(data.order)}
    for a, b in ((3, 20), (3, 21), (20, 21), (7, 33)):
        assert (pos[a] < pos[b]) == (where[a] < where[b])
    return res


def oracle_diversity(X, n):
    comp = np.arange(n * K) % K
    ix, iy, pg = SO.group_pairs(comp, K)
    vals, _ = SO.ssim_rows(X, X, (1, SIDE, SIDE), W11, C1, C2, ix=ix, iy=iy)
    within = np.array([vals[pg == c].mean() for c in range(K)])
    pairs = [(t * K + a, t * K + b, a, b) for t in range(n) for a in range(K) for b in range(a + 1, K)]
    vb, _ = SO.ssim_rows(X, X, (1, SIDE, SIDE), W11, C1, C2, ix=[p[0] for p in pairs], iy=[p[1] for p in pairs])
    per = np.array([np.mean([v for v, p in zip(vb, pairs) if c in p[2:]]) for c in range(K)])
    return within, float(vb.mean()), per


def check_diversity(m, vae, n=5):
    rng_state = np.random.get_state()
    res = m.get_sample_diversity(None, n_per_cluster=n)
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state()))
    again = m.get_sample_diversity(None, n_per_cluster=n, counter=0)
    for name in res:
        assert np.array_equal(res[name], again[name]), name      # a second call: the same bits
    assert res["n_per_cluster"] == n and res["ssim_within"].shape == (K,) and res["ssim_between_per_cluster"].shape == (K,)
    X = vae.sample_prior_device(n * K, 0)[0].cpu().numpy()       # the draws get_sample_quality judges at the same counter
    within, between, per = oracle_diversity(X, n)
    print("%s: within %s between %.4f" % (type(m).__name__, np.round(res["ssim_within"], 4), res["ssim_between"]))
    assert np.abs(res["ssim_within"] - within).max() <= BOUND
    assert abs(res["ssim_between"] - between) <= BOUND and np.abs(res["ssim_between_per_cluster"] - per).max() <= BOUND
    assert res["collapsed"] == [c for c in range(K) if within[c] > 0.9] and (np.abs(within - 0.9) > BOUND).all()
    other = m.get_sample_diversity(None, n_per_cluster=n, counter=1)
    assert not np.array_equal(other["ssim_within"], res["ssim_within"])                          # another counter: other draws
    return res


def zero_the_decoders_last_layer(vae):
    p = vae.engine.get_parameters()
    last = [k for k, v in p.items() if k.startswith("W_") and v.ndim == 2 and v.shape[1] == I]
    assert len(last) == 1, last
    vae.engine.set_parameters({last[0]: np.zeros_like(p[last[0]])})


def check_collapse(m, vae):
    zero_the_decoders_last_layer(vae)
    res = m.get_sample_diversity(None, n_per_cluster=4, counter=2)
    X = vae.sample_prior_device(4 * K, 2)[0].cpu().numpy()
    assert (X == X[0]).all()                                     # every draw decodes to the same image
    assert res["ssim_within"].tolist() == [1.0] * K and res["ssim_between"] == 1.0               # exactly
    assert res["ssim_between_per_cluster"].tolist() == [1.0] * K and res["collapsed"] == list(range(K))
    assert m.get_sample_diversity(None, n_per_cluster=4, counter=2, collapsed_above=1.0)["collapsed"] == []


def test_dmvae_reconstruction_quality():
    m = dmvae()
    check_reconstruction(m, m, dataset())


def test_dmvae_sample_diversity_and_collapse():
    m = dmvae()
    check_diversity(m, m)
    check_collapse(m, m)


def test_vade_inherits_both():
    m = vade()
    check_reconstruction(m, m, dataset())
    check_diversity(m, m)
    check_collapse(m, m)


def test_dvmoe_forwards_both_to_its_gate():
    from includes.utils import MEDataset
    m = dvmoe()
    data = dataset(lambda X, cls: MEDataset((X, cls, np.eye(CLASSES)[cls].astype(np.float32)), batch_size=B))
    check_reconstruction(m, m.vae, data)
    check_diversity(m, m.vae)
    check_collapse(m, m.vae)


def test_arguments_outside_their_range_are_refused():
    import base_models
    m = dmvae()
    data = dataset()
    with pytest.raises(ValueError):
        m.get_reconstruction_quality(None, data, image_shape=(12, 13))
    with pytest.raises(ValueError):
        m.get_reconstruction_quality(None, data, image_shape=(16, 9))        # the 11-tap window does not fit
    with pytest.raises(ValueError):
        m.get_sample_diversity(None, n_per_cluster=1)
    res = m.get_reconstruction_quality(None, data, image_shape=(1, 12, 12), n_worst=3)
    assert tuple(res["image_shape"]) == (1, 12, 12) and len(res["worst"]) == 3
    odd = base_models.DeepMixtureVAE("odd", "binary", 150, D, K, activation="relu", initializer="xavier", batch_size=B, dtype="fp32", seed=3,
                                     eval="device", **LAYERS).build_graph()
    with pytest.raises(ValueError, match="image_shape"):
        odd.get_sample_diversity(None, n_per_cluster=2)          # 150 is no perfect square: the shape is asked for
    with pytest.raises(ValueError):
        odd.get_sample_diversity(None, n_per_cluster=2, image_shape=(15, 10))                    # 11 taps do not fit 10 columns
    assert odd.get_sample_diversity(None, n_per_cluster=2, image_shape=(15, 10), window=SO.gaussian_window(7, 1.5))["ssim_within"].shape == (K,)


def test_train_py_flags_write_their_keys_and_train_as_without_them(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    base = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--dataset", "synthetic", "--n_epochs", "2", "--eval", "device",
            "--batch_size", "1000", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    procs = []
    for name, extra in (("with", ["--recon_quality", "--sample_diversity", "4"]), ("without", [])):
        d = tmp_path / name
        d.mkdir()
        procs.append((d, subprocess.Popen(base + extra, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    outs = []
    for d, pr in procs:
        so, se = pr.communicate(timeout=900)
        assert pr.returncode == 0, (so[-2000:], se[-3000:])
        outs.append((so + se, [json.loads(l) for l in open(d / "dmvae_metrics.jsonl")]))
    (on, rec_on), (off, rec_off) = outs
    assert "ssimTest=" in on and "psnrTest=" in on and "divTest=" in on and "ssimTest" not in off and "divTest" not in off
    assert len(rec_on) == 2 and len(rec_off) == 2
    gained = {"ssimTest", "psnrTest", "mseTest", "worst_rows_test", "ssim_per_class", "mse_per_class", "divTest", "div_n", "ssim_within", "ssim_between",
              "ssim_between_per_cluster", "collapsed"}
    for a, b in zip(rec_on, rec_off):
        assert set(a) - set(b) == gained and set(b) <= set(a)
        assert all(np.isfinite(a[n]) for n in ("ssimTest", "psnrTest", "mseTest", "divTest", "ssim_between"))
        assert -1.0 <= a["ssimTest"] <= 1.0 and -1.0 <= a["divTest"] <= 1.0 and a["mseTest"] > 0.0 and a["div_n"] == 4
        assert len(a["ssim_per_class"]) == len(a["mse_per_class"]) and len(a["ssim_within"]) == len(a["ssim_between_per_cluster"])
        assert a["divTest"] == float(np.mean(a["ssim_within"]))
        assert a["loss"] == b["loss"] and a["acc_test"] == b["acc_test"] and a["acc_train"] == b["acc_train"]      # the NumPy stream is untouched
