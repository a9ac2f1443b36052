"""Host-side tests of the k-nearest-neighbour family (csrc/knn.hip, dmvae_hip/knn.py): the entries are declared, exported and bound,
dmvae_knn_ws_bytes is host arithmetic that refuses bad shapes by name, and the float64 oracle the GPU tests lean on
(tests/helpers/knn_oracle.py) agrees with hand-worked cases and with a brute-force Python loop."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import knn_oracle as KO      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dmvae_knn", "dmvae_knn_vote", "dmvae_knn_ranks")
LINE = np.array([[0.0], [1.0], [3.0], [6.0], [10.0], [15.0]])      # gaps 1, 2, 3, 4, 5: row 2 is equally far from rows 0 and 3


def test_entries_are_declared_exported_and_bound():
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dmvae_[a-z0-9_]+)\s*\(", hdr))
    for name, nargs in zip(ENTRIES + ("dmvae_knn_ws_bytes",), (15, 11, 11, 4)):
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert len(getattr(_lib.lib, name).argtypes) == nargs, name
    assert _lib.lib.dmvae_knn_ws_bytes.restype is C.c_int64
    assert '"knn.hip"' in open(os.path.join(ROOT, "deep-mixture-vae_amd", "build.py")).read()
    import dmvae_hip.knn as K
    src = open(K.__file__).read()
    assert "import sklearn" not in src and "from sklearn" not in src
    for name in ("kneighbors", "KNeighborsClassifier", "trustworthiness"):
        assert hasattr(K, name)
    from dmvae_hip.tsne import TSNE
    assert callable(TSNE.trustworthiness)


def test_ws_bytes_is_host_arithmetic_and_refuses_bad_shapes_by_name():
    from dmvae_hip import _lib
    ws = _lib.lib.dmvae_knn_ws_bytes
    assert ws(65536, 65536, 64, 10) == 0                         # the queries alone fill the device: no split, no workspace
    few = ws(10, 55000, 10, 10)                                  # ten prior means against a data set: the database is dealt out
    assert 2 * 10 * 10 * 8 <= few <= 16 * 10 * 10 * 8 + 255          # the k best 8-byte keys of every query from 2 .. 16 parts
    assert ws(1, 1, 1, 1) == 0 and ws(1 << 20, 1 << 20, 1, 256) == 0
    for bad in ((0, 5, 1, 1), (5, 0, 1, 1), ((1 << 20) + 1, 5, 1, 1), (5, (1 << 20) + 1, 1, 1), (5, 5, 0, 1), (5, 5, 1, 0), (5, 300, 1, 257),
                (5, 5, 1, 6)):
        assert ws(*bad) == -1, bad                               # DMVAE_EINVAL
        assert b"dmvae_knn_ws_bytes" in _lib.lib.dmvae_last_error(), bad


def test_model_surface_exists():
    import base_models
    import models
    for cls in (base_models.DeepMixtureVAE, base_models.VaDE, models.DeepMoE, models.DeepVariationalMoE):
        assert callable(cls.get_knn_accuracy) and callable(cls.get_cluster_exemplars)
    from dmvae_hip.knn import KNeighborsClassifier
    with pytest.raises(ValueError):
        KNeighborsClassifier(0)
    with pytest.raises(ValueError):
        KNeighborsClassifier(257)


def test_oracle_on_the_hand_worked_line():
    idx, d2, _ = KO.knn(LINE, LINE, 2, self_first=0)
    assert idx.tolist() == [[1, 2], [0, 2], [1, 0], [2, 4], [3, 5], [4, 3]]      # row 2: rows 0 and 3 tie at 9, the lower row first
    assert d2.tolist() == [[1, 9], [1, 4], [4, 9], [9, 16], [16, 25], [25, 81]]
    idx, d2, _ = KO.knn(np.array([[3.0], [20.0]]), LINE, 3)                       # nothing left out: the point itself comes first
    assert idx.tolist() == [[2, 1, 0], [5, 4, 3]] and d2.tolist() == [[0, 4, 9], [25, 100, 196]]
    assert KO.ranks(LINE, np.array([[5], [0], [3], [2], [0], [1]])).tolist() == [[4], [0], [2], [0], [4], [3]]
    counts, pred = KO.vote(np.array([[0, 1, 2, 3, 4], [5, 5, 5, 0, 1]]), np.array([2, 2, 1, 1, 0, 3]), 4)
    assert counts.tolist() == [[1, 2, 2, 0], [0, 0, 2, 3]] and pred.tolist() == [1, 3]      # 2-2-1: the smallest class among the tied


def test_oracle_against_a_brute_force_loop():
    rng = np.random.RandomState(0)
    Q, X = rng.randint(-3, 4, (7, 2)).astype(np.float64), rng.randint(-3, 4, (40, 2)).astype(np.float64)       # many exact ties
    idx, d2, _ = KO.knn(Q, X, 9)
    for i in range(len(Q)):
        pairs = sorted((sum((Q[i][c] - X[j][c]) ** 2 for c in range(2)), j) for j in range(len(X)))
        assert [j for _, j in pairs[:9]] == idx[i].tolist() and [d for d, _ in pairs[:9]] == d2[i].tolist()
    sidx, _, _ = KO.knn(X, X, 5, self_first=0)
    rk = KO.ranks(X, sidx)
    for i in range(len(X)):
        pairs = sorted((sum((X[i][c] - X[j][c]) ** 2 for c in range(2)), j) for j in range(len(X)) if j != i)
        assert [j for _, j in pairs[:5]] == sidx[i].tolist()
        assert rk[i].tolist() == [0, 1, 2, 3, 4]                 # the rank of a row's own t-th neighbour is t
    sl, _, _ = KO.knn(X[8:12], X, 5, self_first=8)               # a slice of the queries: the same rows
    assert np.array_equal(sl, sidx[8:12])


def test_oracle_trustworthiness_of_identity_and_of_a_known_permutation():
    rng = np.random.RandomState(1)
    X = rng.randn(30, 4)
    assert KO.trustworthiness(X, X, 5) == 1.0
    assert KO.trustworthiness(X, 3.0 * X, 7) == 1.0               # the same neighbourhoods
    Y = LINE.copy()
    Y[[0, 5]] = Y[[5, 0]]                                        # the two ends change places
    # k = 1: the embedding's nearest rows are 4, 5, 1, 2, 3, 1 with ranks 3, 4, 0, 0, 0, 3 in X: T = 1 - 2 / (6 * 1 * 8) * 10 = 7 / 12
    assert abs(KO.trustworthiness(LINE, Y, 1) - 7.0 / 12.0) <= 1e-15
    with pytest.raises(ValueError):
        KO.trustworthiness(LINE, Y, 3)                           # k < n / 2
