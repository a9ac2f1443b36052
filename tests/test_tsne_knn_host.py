"""Host tests of the kNN-sparse t-SNE's surroundings: the float64 oracle of tests/helpers/tsne_knn_oracle.py held to the dense oracle
(k = N - 1 is the dense form), to sklearn's own _joint_probabilities_nn fed the same lists, and to itself (its gradient is the derivative
of its KL); the C ABI's struct, entries and argument checks; the CLI switch.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import tsne_oracle as T          # noqa: E402
import tsne_knn_oracle as K      # noqa: E402

SHAPES = [(65, 2, 30.0), (257, 10, 5.0), (261, 10, 30.0), (1030, 64, 30.0)]
ENTRIES = ("dmvae_tsne_knn_ws_bytes", "dmvae_tsne_knn_cond_p", "dmvae_tsne_knn_gradient", "dmvae_tsne_knn_step", "dmvae_tsne_knn_fit")


def test_k_equal_n_minus_one_is_the_dense_oracle():
    """N = 65, perplexity 30: k = min(64, 91) = 64, every other row is a neighbour.  Bar 1e-12 * max P; measured 3.4e-16"""
    X, _ = T.blobs(65, 2)
    assert K.n_neighbors(65, 30.0) == 64
    P, (indptr, indices, values) = K.joint_p(X, 30.0)
    want = T.joint_p(T.sq_distances(X), 30.0)
    worst = np.abs(P - want).max() / want.max()
    print("%.3g of max P" % worst)
    assert worst <= 1e-12
    assert indptr[-1] == 65 * 64 and (np.diff(indptr) == 64).all()


@pytest.mark.parametrize("N,D,perplexity", SHAPES)
def test_oracle_joint_p_matches_sklearn_nn(N, D, perplexity):
    """sklearn stops its search at 1e-5 and takes f32 distances, so relative differences reach 1.2e-3: no relative bar.
    Bar 3e-5 * max P; measured 3.7e-6 .. 7.0e-6 with sklearn 1.7.2"""
    tsne_mod = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.sparse import csr_matrix
    X, _ = T.blobs(N, D)
    k = K.n_neighbors(N, perplexity)
    idx, d2k = K.knn_lists(X, k)
    p, beta = K.conditional_p(d2k, perplexity)
    indptr, indices, values = K.joint_csr(idx, p)
    P = K.dense(indptr, indices, values)
    dist = csr_matrix((d2k.reshape(-1), idx.reshape(-1), np.arange(0, N * k + 1, k)), shape=(N, N))
    ref = np.asarray(tsne_mod._joint_probabilities_nn(dist, perplexity, 0).todense())
    worst = np.abs(P - ref).max() / ref.max()
    rows = np.diff(indptr)
    print("N=%d D=%d k=%d: %.3g of max P; %.1f entries per row, %d on the fullest" % (N, D, k, worst, rows.mean(), rows.max()))
    assert worst <= 3e-5
    assert (P == P.T).all() and (np.diag(P) == 0).all() and abs(P.sum() - 1.0) <= 1e-12
    assert ((ref > 0) <= (P > 0)).all()                                  # sklearn's pattern lies inside the union graph
    assert np.abs(K.entropy(d2k, beta) - np.log(perplexity)).max() <= 1e-9
    # sorted by (row, column), no duplicates
    r = np.repeat(np.arange(N), rows)
    key = r * N + indices
    assert (np.diff(key) > 0).all()


def test_oracle_gradient_is_the_derivative_of_its_kl():
    X, _ = T.blobs(40, 5)
    _, csr = K.joint_p(X, 4.0)                      # k = 13 of 39: a truly sparse P
    assert csr[0][-1] < 40 * 39
    Y = np.random.RandomState(2).randn(40, 2)
    g = K.gradient(csr, Y, 1.0)
    fd = np.empty_like(g)
    h = 1e-5
    for i in range(40):
        for c in range(2):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, c] += h
            Ym[i, c] -= h
            fd[i, c] = (K.kl(csr, Yp) - K.kl(csr, Ym)) / (2 * h)
    np.testing.assert_allclose(fd, g, rtol=1e-5, atol=1e-5 * np.abs(g).max())


def test_tsne_knn_config_layout_matches_gcc(tmp_path):
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct dmvae_tsne_knn_config \{(.*?)\} dmvae_tsne_knn_config;", hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        for part in decl.strip().split(","):
            if part.strip():
                fields.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1))
    assert fields == [f[0] for f in _lib.TsneKnnConfig._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmvae_hip.h"\nint main(void){printf("%zu", sizeof(dmvae_tsne_knn_config));'
                   + "".join('printf(" %%zu", offsetof(dmvae_tsne_knn_config, %s));' % f for f in fields) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.TsneKnnConfig)] + [getattr(_lib.TsneKnnConfig, f).offset for f in fields]


def test_library_exports_the_tsne_knn_entries():
    from dmvae_hip import _lib, tsne
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
    assert _lib.lib.dmvae_tsne_knn_ws_bytes.restype is C.c_int64
    for name in ("knn_joint_p", "knn_gradient", "knn_step", "knn_fit"):
        assert callable(getattr(tsne, name))
    assert tsne.n_neighbors(70000, 30.0) == K.n_neighbors(70000, 30.0) == 91 and tsne.n_neighbors(65, 30.0) == 64
    assert tsne.n_neighbors(1000, 85.0) == 256 and tsne.n_neighbors(1000, 5.0) == 16


def test_argument_checks_need_no_device():
    """the checks run before anything is enqueued: on a machine without a GPU they still answer, with the error text set"""
    from dmvae_hip import _lib
    from dmvae_hip.tsne import knn_config
    lib = _lib.lib
    good = knn_config(1000, nnz=5000)
    need = lib.dmvae_tsne_knn_ws_bytes(C.byref(good))
    assert 0 < need <= 1000 * (8 + 16 + 8 + 8 + 8 + 2 + 16) + 16 * 256
    forced = knn_config(1000, col_splits=5)
    more = lib.dmvae_tsne_knn_ws_bytes(C.byref(forced)) - need                 # S = 1 at N = 1000 (one tile): four more [N] partials of each kind
    assert 2 * 4 * 8000 <= more <= 2 * 4 * 8000 + 512
    wrong_k = knn_config(1000)
    wrong_k.k = 90
    for bad, word in ((knn_config(3, perplexity=1.5), b"N"), (knn_config(1000, perplexity=1.0), b"perplexity"), (knn_config(1000, n_iter=-1), b"n_iter"),
                      (knn_config(1000, perplexity=90.0), b"256"), (knn_config(1000, col_splits=-1), b"col_splits"), (knn_config((1 << 20) + 1), b"N"),
                      (knn_config(50, perplexity=49.0), b"perplexity"), (wrong_k, b"k=90"), (knn_config(1000, nnz=-1), b"nnz")):
        assert lib.dmvae_tsne_knn_ws_bytes(C.byref(bad)) == -1
        assert b"dmvae_tsne_knn_ws_bytes" in lib.dmvae_last_error() and word in lib.dmvae_last_error(), lib.dmvae_last_error()
    assert lib.dmvae_tsne_knn_ws_bytes(C.byref(knn_config(1 << 20))) > 0 and lib.dmvae_tsne_knn_ws_bytes(C.byref(knn_config(1000, perplexity=85.0))) > 0
    flagged = knn_config(1000)
    flagged.flags = 1
    assert lib.dmvae_tsne_knn_ws_bytes(C.byref(flagged)) == -1
    buf = (C.c_char * 64)()
    addr = (C.addressof(buf) + 15) & ~15
    assert lib.dmvae_tsne_knn_cond_p(None, C.byref(good), None, 91, addr, 91, None) == -1
    assert lib.dmvae_tsne_knn_cond_p(None, C.byref(good), addr, 90, addr, 91, None) == -1 and b"ldd" in lib.dmvae_last_error()
    assert lib.dmvae_tsne_knn_fit(None, C.byref(good), addr, addr, addr, None, addr, need - 1, addr, addr) == -1 and b"workspace" in lib.dmvae_last_error()
    assert lib.dmvae_tsne_knn_fit(None, C.byref(good), None, addr, addr, None, addr, need, addr, addr) == -1 and b"indptr" in lib.dmvae_last_error()
    assert lib.dmvae_tsne_knn_gradient(None, C.byref(good), addr, addr, addr, addr, need, None, 1.0, addr) == -1
    assert lib.dmvae_tsne_knn_step(None, C.byref(good), addr, addr, addr, addr, need, addr, None, addr, 1.0, 0.5) == -1
    assert lib.dmvae_tsne_knn_step(None, C.byref(good), addr, addr, None, addr, need, addr, addr, addr, 1.0, 0.5) == -1


def test_class_arguments():
    from dmvae_hip.tsne import TSNE
    assert TSNE().method == "exact" and TSNE(method="knn").method == "knn"
    with pytest.raises(ValueError):
        TSNE(method="barnes_hut")
    src = open(os.path.join(ROOT, "deep-mixture-vae_amd", "dmvae_hip", "tsne.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(sklearn|scipy)", src, flags=re.M)


def test_cli_has_the_latent_map_switch():
    import train
    assert train.parser.parse_args([]).latent_map == "off"
    for v in ("off", "auto", "exact", "knn"):
        assert train.parser.parse_args(["--latent_map", v]).latent_map == v
    with pytest.raises(SystemExit):
        train.parser.parse_args(["--latent_map", "gpu"])
