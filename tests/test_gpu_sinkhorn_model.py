"""GPU tests of get_sample_distance (base_models.py, models.py) and of train.py --sample_distance on the tiny fp32 plan of
test_gpu_prdc_model.py -- input 32, latent 4, K = 3, batch 8 -- on 50 rows (a ragged last batch) against M = 48 generated rows.  The method
must equal dmvae_hip.sinkhorn.sinkhorn_divergence on features rebuilt from the public pieces -- dmvae_philox_normal at the documented (seed,
counter, stream id 7), the prior views, decode and encode_means_device -- exactly, and lie within the end-to-end bar of the float64 oracle
of tests/helpers/sinkhorn_oracle.py on those features."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sinkhorn_oracle as SO      # noqa: E402
from test_gpu_prdc_model import CLASSES, D, I, K, M, N_ROWS, ROOT, dataset, dmvae, dvmoe, rebuilt_features, vade      # noqa: E402

pytestmark = pytest.mark.gpu

SCALARS = ("divergence", "ot", "eps", "n_iter", "err")
VECTORS = ("per_cluster", "mean_per_cluster", "per_class", "mean_per_class")
ITERS = 30


def check_model(m, vae, data, space="latent", counter=0, n_samples=None):
    from dmvae_hip import sinkhorn
    n = (N_ROWS // K) * K if n_samples is None else n_samples
    rng_state, order = np.random.get_state(), data.order.copy()
    before = vae.engine.param.clone()
    res = m.get_sample_distance(None, data, space=space, counter=counter, n_samples=n_samples, tol=0.0, max_iter=ITERS)
    assert all(np.array_equal(a, b) for a, b in zip(rng_state, np.random.get_state()))           # nothing drawn from the NumPy stream
    assert np.array_equal(order, data.order)                                                     # no reshuffle
    assert bool((vae.engine.param == before).all())                                              # and no parameter written
    assert (res["n_real"], res["n_samples"], res["space"]) == (N_ROWS, n, space) and n == M
    again = m.get_sample_distance(None, data, space=space, counter=counter, n_samples=n_samples, tol=0.0, max_iter=ITERS)
    for name in SCALARS:
        assert res[name] == again[name], name                    # a second call: the same bits
    for name in VECTORS:
        assert np.array_equal(res[name], again[name], equal_nan=True) and res[name].shape == ((K,) if "cluster" in name else (CLASSES,))

    R, F, comp, X = rebuilt_features(vae, data, space, counter, n)
    assert R.shape == (N_ROWS, D if space == "latent" else I) and F.shape == (n, R.shape[1])
    cls = data._cls[data.order]
    want = sinkhorn.sinkhorn_divergence(R, F, eps_rel=0.05, tol=0.0, max_iter=ITERS, real_groups=cls, fake_groups=comp)
    for name in SCALARS:
        assert res[name] == want[name], name
    for name, group in zip(VECTORS, ("per_fake_group", "mean_per_fake_group", "per_real_group", "mean_per_real_group")):
        assert np.array_equal(res[name], np.array(want[group]), equal_nan=True), name
    total = res["per_cluster"].sum() + res["per_class"].sum()
    assert abs(total - res["divergence"]) <= 1e-12 * abs(res["divergence"])

    ref = SO.divergence(R, F, want["eps"], want["scale"], iters=(ITERS,) * 3, real_groups=cls, fake_groups=comp)
    print("%s %s: S_eps %.6g oracle %.6g, |difference| / bar %.2e, S / OT %.3f" % (type(m).__name__, space, res["divergence"], ref["divergence"],
                                                                                    abs(res["divergence"] - ref["divergence"]) / ref["bar"],
                                                                                    res["divergence"] / res["ot"]))
    assert abs(res["divergence"] - ref["divergence"]) <= ref["bar"] and res["divergence"] > ref["bar"]
    for name, group in zip(VECTORS, ("per_fake_group", "mean_per_fake_group", "per_real_group", "mean_per_real_group")):
        assert np.all(np.abs(res[name] - ref[group]) <= ref["bar"]), name
    return res, X


def test_dmvae_equals_sinkhorn_divergence_on_the_rebuilt_features_and_the_oracle():
    m = dmvae()
    data = dataset()
    res, X0 = check_model(m, m, data)
    check_model(m, m, data, n_samples=M)
    other, X1 = check_model(m, m, data, counter=1)
    assert not np.array_equal(X0, X1) and other["divergence"] != res["divergence"]               # another counter: other samples, another value
    # the generated rows are the bits get_sample_quality judged at the same counter
    Xq, _, _ = m.sample_prior_device(M, 0)
    assert np.array_equal(Xq.cpu().numpy(), X0)
    R, F, comp, _, _ = m._real_and_generated_features(data, M, "input", 0)
    assert np.array_equal(F.cpu().numpy(), X0)


def test_input_space_has_the_rows_width():
    m = dmvae()
    check_model(m, m, dataset(), space="input")


def test_vade_inherits_it():
    m = vade()
    check_model(m, m, dataset())


def test_dvmoe_forwards_to_its_gate():
    from includes.utils import MEDataset
    m = dvmoe()
    data = dataset(lambda X, cls: MEDataset((X, cls, np.eye(CLASSES)[cls].astype(np.float32)), batch_size=8))
    check_model(m, m.vae, data)


def test_arguments_outside_their_range_are_refused():
    m = dmvae()
    data = dataset()
    for kw in (dict(space="pixels"), dict(eps_rel=0.0), dict(tol=-1.0), dict(max_iter=0), dict(n_samples=0)):
        with pytest.raises(ValueError):
            m.get_sample_distance(None, data, **kw)


def test_train_py_sample_distance_writes_its_keys_and_trains_as_without_the_flag(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    base = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--dataset", "synthetic", "--n_epochs", "2", "--eval", "device",
            "--batch_size", "1000", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    procs = []
    for name, extra in (("with", ["--sample_distance"]), ("without", [])):
        d = tmp_path / name
        d.mkdir()
        procs.append((d, subprocess.Popen(base + extra, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    outs = []
    for d, pr in procs:
        so, se = pr.communicate(timeout=900)
        assert pr.returncode == 0, (so[-2000:], se[-3000:])
        outs.append((so + se, [json.loads(l) for l in open(d / "dmvae_metrics.jsonl")]))
    (on, rec_on), (off, rec_off) = outs
    assert "sdTest=" in on and "sdTest" not in off
    assert len(rec_on) == 2 and len(rec_off) == 2
    gained = {"sdTest", "sd_eps", "sd_iters", "sd_err", "sd_per_cluster", "sd_per_class"}
    for a, b in zip(rec_on, rec_off):
        assert set(a) - set(b) == gained and set(b) <= set(a)
        assert a["sdTest"] > 0 and a["sd_eps"] > 0 and len(a["sd_iters"]) == len(a["sd_err"]) == 3 and max(a["sd_err"]) <= 1e-4
        assert abs(sum(a["sd_per_cluster"]) + sum(a["sd_per_class"]) - a["sdTest"]) <= 1e-9 * a["sdTest"]
        assert a["loss"] == b["loss"] and a["acc_test"] == b["acc_test"] and a["acc_train"] == b["acc_train"]      # the NumPy stream is untouched
