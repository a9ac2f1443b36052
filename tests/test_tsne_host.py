"""Host tests of the device t-SNE's surroundings: the float64 oracle of tests/helpers/tsne_oracle.py held to what the reference
actually calls (sklearn's joint probabilities) and to itself (its gradient is the derivative of its KL), the C ABI's struct and
entries, the CLI switch and the visualisation's dispatch.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import tsne_oracle as T      # noqa: E402

SHAPES = [(240, 10, 30.0), (97, 3, 5.0), (333, 64, 50.0)]
ENTRIES = ("dmvae_tsne_ws_bytes", "dmvae_tsne_joint_p", "dmvae_tsne_gradient", "dmvae_tsne_step", "dmvae_tsne_fit", "dmvae_tsne_p")


@pytest.mark.parametrize("N,D,perplexity", SHAPES)
def test_oracle_joint_p_matches_sklearn(N, D, perplexity):
    """sklearn's side is an f32 search that stops at |H - log u| <= 1e-5: measured 6.7e-6 * max P and 2.4e-4 relative on these inputs;
    the bars are 4x that"""
    tsne_mod = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    X, _ = T.blobs(N, D)
    d2 = T.sq_distances(X)
    P = T.joint_p(d2, perplexity)
    ref = squareform(tsne_mod._joint_probabilities(d2.astype(np.float32), perplexity, 0))
    worst_abs = np.abs(P - ref).max() / ref.max()
    big = ref > 1e-9
    worst_rel = (np.abs(P - ref)[big] / ref[big]).max()
    print("N=%d D=%d: %.3g of max P, %.3g relative" % (N, D, worst_abs, worst_rel))
    assert worst_abs <= 3e-5 and worst_rel <= 1e-3
    assert (P == P.T).all() and (np.diag(P) == 0).all() and abs(P.sum() - 1.0) <= 1e-12
    _, beta = T.conditional_p(d2, perplexity)
    assert np.abs(T.entropy(d2, beta) - np.log(perplexity)).max() <= 1e-9


def test_oracle_gradient_is_the_derivative_of_its_kl():
    X, _ = T.blobs(40, 5)
    P = T.joint_p(T.sq_distances(X), 8.0)
    Y = np.random.RandomState(2).randn(40, 2)
    g = T.gradient(P, Y, 1.0)
    fd = np.empty_like(g)
    h = 1e-5
    for i in range(40):
        for c in range(2):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, c] += h
            Ym[i, c] -= h
            fd[i, c] = (T.kl(P, Yp) - T.kl(P, Ym)) / (2 * h)
    np.testing.assert_allclose(fd, g, rtol=1e-5, atol=1e-5 * np.abs(g).max())


def test_oracle_step_is_sklearns_update():
    """gains grow where velocity and gradient disagree in sign, shrink elsewhere, floor 0.01; velocity = m U - lr G g"""
    X, _ = T.blobs(30, 4)
    P = T.joint_p(T.sq_distances(X), 5.0)
    rs = np.random.RandomState(3)
    Y, U, G = rs.randn(30, 2), rs.randn(30, 2), np.full((30, 2), 0.012)
    Y1, U1, G1, g = T.step(P, Y, U, G, 12.0, 0.5, 200.0)
    inc = U * g < 0
    assert (G1[inc] == 0.012 + 0.2).all() and (G1[~inc] == 0.01).all() and inc.any() and (~inc).any()
    np.testing.assert_array_equal(U1, 0.5 * U - 200.0 * (G1 * g))
    np.testing.assert_array_equal(Y1, Y + U1)
    assert T.auto_learning_rate(240) == 50.0 and T.auto_learning_rate(10000) == 10000 / 48.0


def test_tsne_config_layout_matches_gcc(tmp_path):
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct dmvae_tsne_config \{(.*?)\} dmvae_tsne_config;", hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            fields += [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", n.strip()).group(1) for n in decl.split(",")]
    assert fields == [f[0] for f in _lib.TsneConfig._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmvae_hip.h"\nint main(void){printf("%zu", sizeof(dmvae_tsne_config));'
                   + "".join('printf(" %%zu", offsetof(dmvae_tsne_config, %s));' % f for f in fields) + "return 0;}")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "l")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.TsneConfig)] + [getattr(_lib.TsneConfig, f).offset for f in fields]


def test_library_exports_the_tsne_entries():
    import dmvae_hip
    from dmvae_hip import _lib
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert "debug" not in name and "prof" not in name
    assert _lib.lib.dmvae_tsne_ws_bytes.restype is C.c_int64
    assert _lib.lib.dmvae_abi_version() == _lib.ABI_VERSION == 5
    assert dmvae_hip.TSNE is dmvae_hip.tsne.TSNE


def test_argument_checks_need_no_device():
    """the checks run before anything is enqueued: on a machine without a GPU they still answer, with the error text set"""
    from dmvae_hip import _lib
    from dmvae_hip.tsne import config
    lib = _lib.lib
    good = config(100, 5)
    need = lib.dmvae_tsne_ws_bytes(C.byref(good))
    assert 4 * 100 * 100 <= need <= 4 * 100 * 100 + 64 * 100 + 4096
    for bad, code in ((config(3, 5, perplexity=1.5), -1), (config(100, 0), -1),
                      (config(100, 5, perplexity=99.0), -1), (config(100, 5, perplexity=1.0), -1), (config(100, 5, n_iter=-1), -1),
                      (config(32769, 5), -2)):
        assert lib.dmvae_tsne_ws_bytes(C.byref(bad)) == code
        assert b"dmvae_tsne_ws_bytes" in lib.dmvae_last_error()
    flagged = config(100, 5)
    flagged.flags = 1
    assert lib.dmvae_tsne_ws_bytes(C.byref(flagged)) == -1
    # null pointers and a short workspace: refused before any launch (no device is touched, so this runs anywhere)
    buf = (C.c_char * 64)()
    addr = (C.addressof(buf) + 15) & ~15
    assert lib.dmvae_tsne_joint_p(None, C.byref(good), None, 5, addr, need, None) == -1
    assert lib.dmvae_tsne_joint_p(None, C.byref(good), addr, 5, addr, 32, None) == -1 and b"workspace" in lib.dmvae_last_error()
    assert lib.dmvae_tsne_fit(None, C.byref(good), addr, 5, None, addr, 32, addr, addr) == -1
    assert lib.dmvae_tsne_gradient(None, C.byref(good), addr, need, None, 1.0, addr) == -1
    assert lib.dmvae_tsne_step(None, C.byref(good), addr, need, addr, None, addr, 1.0, 0.5) == -1


def test_class_arguments():
    from dmvae_hip.tsne import TSNE, config
    with pytest.raises(ValueError):
        TSNE(n_components=3)
    with pytest.raises(ValueError):
        TSNE(init="pca")
    t = TSNE()
    assert (t.perplexity, t.early_exaggeration, t.learning_rate, t.n_iter, t.init, t.random_state) == (30.0, 12.0, "auto", 1000, "random", 0)
    assert config(240, 10).learning_rate == 50.0 and config(10000, 10).learning_rate == np.float32(10000 / 48.0)
    src = open(os.path.join(ROOT, "deep-mixture-vae_amd", "dmvae_hip", "tsne.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(sklearn|scipy)", src, flags=re.M)


def test_cli_has_the_tsne_switch():
    import train
    assert train.parser.parse_args([]).tsne == "off"
    assert train.parser.parse_args(["--tsne", "device"]).tsne == "device"
    with pytest.raises(SystemExit):
        train.parser.parse_args(["--tsne", "gpu"])


def test_cluster_scatter_dispatch(monkeypatch):
    from includes import visualization as V
    import dmvae_hip.tsne
    calls = []

    class Fake:
        def __init__(self, **kw):
            calls.append(kw)

        def fit_transform(self, Z):
            calls.append(Z.shape)
            return np.asarray(Z[:, :2], dtype=np.float32)

    monkeypatch.setattr(dmvae_hip.tsne, "TSNE", Fake)
    rng = np.random.RandomState(0)
    five = [rng.randn(40, 5) + 4 * k for k in range(2)]
    sc = V.cluster_scatter(five, side=32, tsne="device", seed=7)
    assert calls == [{"n_components": 2, "random_state": 7}, (80, 5)]
    assert sc.shape == (32, 32, 3) and len({tuple(c) for c in sc.reshape(-1, 3).astype(int).tolist()}) == 3      # white + two cluster colours
    del calls[:]
    V.cluster_scatter([rng.randn(30, 2) + 6 * k for k in range(3)], side=40, tsne="device")       # two dimensions: drawn as they are
    assert calls == []
    pytest.importorskip("sklearn")
    V.cluster_scatter(five, side=32, tsne="host")
    V.cluster_scatter(five, side=32)
    assert calls == []
    with pytest.raises(ValueError):
        V.cluster_scatter(five, side=32, tsne="gpu")
