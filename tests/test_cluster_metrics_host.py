"""CPU tests (-m "not gpu") of the cluster metrics (dmvae_hip/metrics.py, csrc/cluster_metrics.hip): the float64 silhouette oracle of
tests/helpers/cluster_metrics_oracle.py against sklearn on the GPU test's cases, scores_from_confusion against sklearn's NMI / ARI,
the error rule of silhouette_score, the three new symbols in the header / the library / the binding, and the --metrics flag."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import cluster_metrics_oracle as CO      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dmvae_argmax_labels", "dmvae_silhouette_ws_bytes", "dmvae_silhouette")


@pytest.mark.parametrize("name", CO.CASE_NAMES)
def test_oracle_equals_sklearn_on_the_gpu_cases(name):
    """1e-9: sklearn takes the distances from dot products, which leaves ~1e-8 * |z| between duplicate rows where the difference
    form gives 0"""
    skm = pytest.importorskip("sklearn.metrics")
    buf, D, labels, K, ref = CO.reference(name)
    want = skm.silhouette_samples(buf[:, :D].astype(np.float64), labels, metric="euclidean")
    err = np.abs(ref - want).max()
    print("%s: max |oracle - sklearn| = %.3g" % (name, err))
    assert ref.shape == want.shape and err <= 1e-9
    assert abs(ref.mean() - skm.silhouette_score(buf[:, :D].astype(np.float64), labels)) <= 1e-9


def test_case_list_is_the_shapes_of_the_issue():
    got = [(buf.shape[0], D, K, buf.shape[1]) for _, buf, D, _, K in CO.cases()]
    assert got == [(301, 10, 6, 10), (257, 3, 7, 5), (130, 64, 4, 64), (200, 130, 3, 130), (65, 1, 2, 1), (1030, 2, 10, 2), (66, 10, 64, 10),
                   (700, 4, 300, 4), (4097, 8, 3, 8)]
    assert [c[0] for c in CO.cases()] == CO.CASE_NAMES
    buf, D, labels, K, ref = CO.reference("N301-D10-K6")
    counts = np.bincount(labels, minlength=K)
    assert counts[3] == 0 and counts[5] == 1 and labels[7] == labels[8] and np.array_equal(buf[7], buf[8])
    assert ref[100] == 0.0                                   # the singleton
    buf, D, labels, K, ref = CO.reference("N66-D10-K64")
    assert np.count_nonzero(np.bincount(labels, minlength=K) == 1) == 62 and not ref[:62].any() and ref[62:].all()
    assert (CO.reference("N257-D3-K7-ld5")[0][:, 3:] == CO.FILLER).all()


def _expand(conf):
    """(clusters, classes) label vectors of a confusion matrix [cluster][class]"""
    i, j = np.nonzero(conf)
    reps = conf[i, j]
    return np.repeat(i, reps), np.repeat(j, reps)


def _matrices():
    rng = np.random.RandomState(0)
    out = [("random 10x10", rng.randint(0, 50, (10, 10))), ("random sparse 7x7", rng.randint(0, 3, (7, 7)) * rng.randint(0, 2, (7, 7)))]
    m = rng.randint(1, 40, (12, 12))
    m[[2, 5, 11], :] = 0                                     # clusters nobody is in
    m[:, [0, 7]] = 0                                         # classes nobody is in
    out.append(("empty rows and columns 12x12", m))
    m = np.zeros((50, 50), dtype=np.int64)                   # 50 clusters on 10 classes: rectangular in effect
    m[:, :10] = rng.randint(0, 30, (50, 10))
    out.append(("50 clusters on 10 classes", m))
    m = np.zeros((6, 6), dtype=np.int64)
    m[2] = rng.randint(1, 20, 6)
    out.append(("one cluster", m))
    m = np.zeros((6, 6), dtype=np.int64)
    m[:, 4] = rng.randint(1, 20, 6)
    out.append(("one class", m))
    m = np.zeros((5, 5), dtype=np.int64)
    m[3, 1] = 17
    out.append(("one cluster and one class", m))
    out.append(("perfect, permuted", np.diag(rng.randint(1, 30, 8))[rng.permutation(8)]))
    out.append(("rectangular 4x9", rng.randint(0, 20, (4, 9))))
    return out


@pytest.mark.parametrize("name,conf", _matrices(), ids=[n for n, _ in _matrices()])
def test_scores_from_confusion_equal_sklearn(name, conf):
    skm = pytest.importorskip("sklearn.metrics")
    from dmvae_hip.metrics import scores_from_confusion
    from includes.utils import accuracy_from_confusion
    conf = np.asarray(conf, dtype=np.int64)
    clusters, classes = _expand(conf)
    got = scores_from_confusion(conf)
    assert set(got) == {"acc", "nmi", "ari", "purity"} and all(isinstance(v, float) for v in got.values())
    assert abs(got["nmi"] - skm.normalized_mutual_info_score(classes, clusters)) <= 1e-12
    assert abs(got["ari"] - skm.adjusted_rand_score(classes, clusters)) <= 1e-12
    assert got["purity"] == conf.max(axis=1).sum() / conf.sum()
    if conf.shape[0] == conf.shape[1]:
        assert got["acc"] == accuracy_from_confusion(conf, conf.sum())
    if name.startswith("perfect"):
        assert got["acc"] == 1.0 and got["purity"] == 1.0 and abs(got["nmi"] - 1.0) <= 1e-12 and got["ari"] == 1.0
    if name == "one cluster and one class":
        assert got["nmi"] == 1.0 and got["ari"] == 1.0


def test_scores_from_confusion_does_not_import_sklearn():
    import subprocess
    code = ("import sys, numpy as np; sys.path.insert(0, %r); from dmvae_hip.metrics import scores_from_confusion; "
            "scores_from_confusion(np.array([[3, 1], [0, 4]])); assert not any(m.startswith('sklearn') for m in sys.modules)"
            % os.path.join(ROOT, "deep-mixture-vae_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_silhouette_score_refuses_one_and_n_clusters():
    """sklearn's rule, checked on the host before anything is uploaded: 2 <= non-empty clusters <= n - 1"""
    from dmvae_hip.metrics import silhouette_score
    Z = np.random.RandomState(0).randn(6, 3).astype(np.float32)
    with pytest.raises(ValueError, match="Number of labels is 1"):
        silhouette_score(Z, np.zeros(6, dtype=np.int32))
    with pytest.raises(ValueError, match="Number of labels is 1"):
        silhouette_score(Z, np.full(6, 3, dtype=np.int32), n_clusters=5)
    with pytest.raises(ValueError, match="Number of labels is 6"):
        silhouette_score(Z, np.arange(6, dtype=np.int32))
    with pytest.raises(IndexError):
        silhouette_score(Z, np.array([0, 1, 2, 0, 1, 5]), n_clusters=5)


def test_new_symbols_are_declared_exported_and_bound():
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dmvae_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).argtypes is not None
    assert _lib.lib.dmvae_silhouette_ws_bytes.restype is __import__("ctypes").c_int64
    assert _lib.lib.dmvae_abi_version() == _lib.ABI_VERSION == 5
    assert '"cluster_metrics.hip"' in open(os.path.join(ROOT, "deep-mixture-vae_amd", "build.py")).read()


def test_workspace_is_linear_in_n_and_k_and_bad_shapes_are_refused():
    """host arithmetic alone: no GPU is touched"""
    from dmvae_hip import _lib
    ws = _lib.lib.dmvae_silhouette_ws_bytes
    base = ws(1 << 10, 16)
    assert base > 0 and ws(1 << 20, 4096) <= 16 * (1 << 20) + 16 * 4096 + 4 * 256
    assert ws(1 << 11, 16) - base == 12 * (1 << 10) and ws(1 << 10, 16 + 1024) - base == 8 * 1024
    for n, K in ((1, 2), (0, 2), ((1 << 20) + 1, 2), (10, 0), (10, 4097)):
        assert ws(n, K) == -1, (n, K)
        assert b"dmvae_silhouette_ws_bytes" in _lib.lib.dmvae_last_error()


def test_train_py_parses_the_metrics_switch():
    sys.argv = ["train.py"]
    import importlib
    train = importlib.import_module("train")
    assert train.parser.parse_args([]).metrics is False and train.parser.parse_args(["--metrics"]).metrics is True
    rec = train._metrics_record(dict(acc=0.5, nmi=0.25, ari=0.125, purity=0.75, silhouette=float("nan"), n_clusters_used=1))
    assert rec == dict(nmi_test=0.25, ari_test=0.125, purity_test=0.75, silhouette_test=None, clusters_used_test=1)
