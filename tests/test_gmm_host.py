"""CPU tests of the device GMM's yardstick and host surface: the NumPy restatement (tests/helpers/gmm_oracle.py) against sklearn
itself, the C boundary of the new entries (struct layout, argument checks that need no GPU), the k-means++ seeding and the CLI."""
import ctypes as C
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import gmm_oracle as G      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("T,tol", [(1, 0.0), (10, 0.0), (200, 1e-3)])
def test_oracle_em_is_sklearn(T, tol):
    from sklearn.mixture import GaussianMixture
    N, D, K = 20000, 10, 10
    X, labels = G.overlapping(N, D, K, seed=1)
    mu0, var0 = G.init_tables(X, labels, K)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = GaussianMixture(K, covariance_type="diag", n_init=1, max_iter=T, tol=tol, weights_init=np.ones(K) / K, means_init=mu0,
                            precisions_init=1 / var0).fit(X.astype(np.float64))
    w, mu, var, lb, it, conv = G.em(X, labels, K, T, tol)
    print("T=%d tol=%g: dw %.2e dmu %.2e dvar(rel) %.2e dlb %.2e n_iter %d / %d" % (
        T, tol, np.abs(w - g.weights_).max(), np.abs(mu - g.means_).max(), np.abs(var / g.covariances_ - 1).max(), abs(lb - g.lower_bound_), it, g.n_iter_))
    assert np.abs(w - g.weights_).max() <= 1e-12
    assert np.abs(mu - g.means_).max() <= 1e-12
    assert np.abs(var - g.covariances_).max() <= 1e-12
    assert abs(lb - g.lower_bound_) <= 1e-12
    assert it == g.n_iter_ and conv == g.converged_


def test_oracle_lloyd_is_sklearn():
    from sklearn.cluster import KMeans
    X, _ = G.overlapping(3000, 6, 5, seed=3)
    c0 = X[np.random.RandomState(0).choice(len(X), 5, replace=False)].astype(np.float64)
    km = KMeans(5, init=c0, n_init=1, algorithm="lloyd", max_iter=300, tol=1e-4).fit(X.astype(np.float64))
    c, labels, it = G.lloyd(X, c0)
    assert np.array_equal(labels, km.labels_)
    assert np.abs(c - km.cluster_centers_).max() <= 1e-12
    assert it == km.n_iter_


def test_gmm_structs_match_the_header_as_a_c_compiler_lays_them_out(tmp_path):
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dmvae_hip.h"', 'int main(void) {']
    want = {}
    for cname, cls in (("dmvae_gmm_config", _lib.GmmConfig), ("dmvae_gmm_result", _lib.GmmResult)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        fields = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1)
                  for decl in body.split(";") if decl.strip() for part in decl.strip().split(",")]
        py = [f[0] for f in cls._fields_]
        assert fields == py, (cname, fields, py)
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f in fields]
        lines.append('printf("\\n");')
        want[cname] = [C.sizeof(cls)] + [getattr(cls, f).offset for f in py]
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines()}
    assert got == want


def test_gmm_workspace_size_and_limits():
    """dmvae_gmm_ws_bytes is host arithmetic: the shapes the models need are accepted, tables that do not fit LDS are refused with the limit"""
    from dmvae_hip import _lib, DmvaeError, check

    def ws(N, D, K, R=1):
        cfg = _lib.GmmConfig(N=N, D=D, K=K, n_init=R, max_iter=10, kmeans_iter=300, tol=1e-3, reg_covar=1e-6, flags=0)
        return _lib.lib.dmvae_gmm_ws_bytes(C.byref(cfg))
    for D, K in ((64, 50), (256, 10), (10, 10), (1, 1), (33, 3)):
        assert ws(65000, D, K) > 0, (D, K)
    assert ws(65000, 10, 10, 20) > ws(65000, 10, 10, 1)
    for D, K in ((512, 10), (64, 64), (8, 300)):
        n = ws(1000, D, K)
        assert n == _lib.EUNSUPPORTED
        with pytest.raises(DmvaeError, match=r"K \* D <= 3328.*65536 B of LDS"):
            check(int(n), "dmvae_gmm_ws_bytes")
    assert ws(0, 10, 10) == -1 and ws(100, 10, 10, 0) == -1


def test_kmeans_plusplus_seeding_is_a_function_of_the_seed():
    from dmvae_hip.gmm import DiagGMM, kmeans_plusplus
    X, c = G.separated(2000, 4, 6, seed=5)
    a = DiagGMM(6, n_init=3, seed=11).seed_centers(X)
    b = DiagGMM(6, n_init=3, seed=11).seed_centers(X)
    d = DiagGMM(6, n_init=3, seed=12).seed_centers(X)
    assert a.shape == (3, 6, 4) and a.dtype == np.float32
    assert np.array_equal(a, b) and not np.array_equal(a, d)
    assert not np.array_equal(a[0], a[1])                       # the restarts draw on from one stream
    # every centre is a row of X, and on clusters this far apart D^2 sampling finds all six
    s = kmeans_plusplus(X, 6, np.random.RandomState(0))
    assert all((np.abs(X.astype(np.float64) - r).max(1) == 0).any() for r in s)
    near = ((s[:, None, :] - c[None]) ** 2).sum(-1).argmin(1)
    assert sorted(near) == list(range(6))


def test_device_gmm_module_does_not_import_sklearn():
    code = "import sys; sys.path.insert(0, %r); import dmvae_hip.gmm; assert not any(m.startswith('sklearn') for m in sys.modules), 'sklearn'" % os.path.join(ROOT, "deep-mixture-vae_amd")
    subprocess.run([sys.executable, "-c", code], check=True)


def test_cli_gmm_flag_defaults_to_host_and_rejects_other_values():
    sys.argv = ["train.py"]
    import importlib
    train = importlib.import_module("train")
    assert train.parser.parse_args([]).gmm == "host"
    assert train.parser.parse_args(["--gmm", "device"]).gmm == "device"
    with pytest.raises(SystemExit):
        train.parser.parse_args(["--gmm", "sklearn"])


def test_models_take_the_gmm_option():
    import base_models
    kw = dict(activation="relu", initializer="xavier")
    assert base_models.DeepMixtureVAE("a", "binary", 40, 6, 5, **kw).gmm == "host"
    assert base_models.DeepMixtureVAE("a", "binary", 40, 6, 5, gmm="device", **kw).gmm == "device"
    assert base_models.VaDE("a", "binary", 40, 6, 5, **kw).gmm == "host"
    assert base_models.VaDE("a", "binary", 40, 6, 5, gmm="device", **kw).gmm == "device"
    with pytest.raises(ValueError):
        base_models.VaDE("a", "binary", 40, 6, 5, gmm="gpu", **kw)
