"""CPU tests of the label-spreading oracle (tests/helpers/label_spread_oracle.py) -- the yardstick the GPU tests of csrc/label_spread.hip hold the
kernels to -- against scikit-learn's LabelSpreading on the same graph, against its own closed form, and on the graph whose second component no
label reaches; and of train.py's --few_label flag."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import label_spread_oracle as LO      # noqa: E402

ALPHA = 0.8


def some_labels(cls, every=5):
    """the class of every row of each `every`-th run of max(cls) + 1 consecutive rows (blobs: one row of every class per run), -1 elsewhere"""
    keep = (np.arange(len(cls)) // (int(cls.max()) + 1)) % every == 0
    return np.where(keep, cls, -1).astype(np.int64)


@pytest.mark.parametrize("N,C,D,k,weights", [(300, 10, 8, 7, "connectivity"), (300, 10, 8, 7, "heat"), (257, 3, 4, 5, "connectivity")])
def test_closed_form_is_sklearns_label_spreading_on_the_same_graph(N, C, D, k, weights):
    from sklearn.semi_supervised import LabelSpreading
    X, cls, (indptr, indices, values) = LO.blobs_graph(N, C, D, 0, k, weights)
    W = LO.dense_from_csr(indptr, indices, values)
    assert np.array_equal(W, W.T) and not np.any(np.diag(W)) and np.all(np.diff(indptr) >= k)
    for a, b in zip(indptr[:-1], indptr[1:]):
        assert np.all(np.diff(indices[a:b]) > 0)                      # columns ascend within a row
    y = some_labels(cls)
    s, _ = LO.normalize(indptr, indices, values)
    ours = LO.row_normalize(LO.closed_form(indptr, indices, s, y, C, ALPHA))
    sk = LabelSpreading(kernel=lambda A, B: W, alpha=ALPHA, max_iter=5000, tol=1e-12).fit(X.astype(np.float64), y)
    assert sk.label_distributions_.shape == ours.shape
    assert np.max(np.abs(sk.label_distributions_ - ours)) <= 1e-9
    assert np.array_equal(sk.transduction_, LO.predict(ours))


def test_iteration_approaches_the_closed_form_at_the_rate_alpha():
    """F^t - F* = -(alpha S)^t F* from F^0 = 0 (subtract the fixed-point equation from the update).  S = D^1/2 P D^-1/2 with P = D^-1 W row-
    stochastic, so S^t = D^1/2 P^t D^-1/2 and |S^t|_inf <= sqrt(d_max / d_min), hence
        |F^t - F*|_inf <= alpha^t |F*|_inf sqrt(d_max / d_min).
    On the connectivity graph every weight is 1/2 or 1 and every row has at least k = 7 entries: d_min >= 3.5 >= 1 and d_max <= the largest
    number of entries in a row, so the bound alpha^t |F*|_inf sqrt(max degree) follows."""
    _, cls, (indptr, indices, values) = LO.blobs_graph(300, 10, 8, 0, 7)
    y = some_labels(cls)
    s, r = LO.normalize(indptr, indices, values)
    star = LO.closed_form(indptr, indices, s, y, 10, ALPHA)
    t = 57
    F, change = LO.iterate(indptr, indices, s, y, 10, ALPHA, t)
    err = np.max(np.abs(F - star))
    d = r ** -2.0
    exact = ALPHA ** t * np.max(np.abs(star)) * np.sqrt(d.max() / d.min())
    assert d.min() >= 1.0 and d.max() <= np.max(np.diff(indptr))
    assert err <= ALPHA ** t * np.max(np.abs(star)) * np.sqrt(np.max(np.diff(indptr)))
    assert err <= exact
    assert change[0] == pytest.approx(1.0 - ALPHA) and change[-1] <= 2.0 * exact / ALPHA
    F32, _ = LO.iterate_f32(indptr, indices, s, y, 10, ALPHA, t)
    assert F32.dtype == np.float32 and np.max(np.abs(F32 - F)) <= 1e-5


def test_islands_no_label_reaches_the_second_component_or_the_edgeless_rows():
    (indptr, indices, values), y, C = LO.islands()
    s, r = LO.normalize(indptr, indices, values)
    assert r[11] == 0.0 and r[12] == 0.0 and np.all(r[:11] > 0)
    for F in (LO.iterate(indptr, indices, s, y, C, ALPHA, 57)[0], LO.closed_form(indptr, indices, s, y, C, ALPHA)):
        assert not np.any(F[6:12]) and np.all(F[:6].sum(axis=1) > 0)
        assert np.array_equal(F[12], [0.0, 1.0 - ALPHA, 0.0])
        pred = LO.predict(F)
        assert np.array_equal(pred[6:12], np.full(6, -1)) and pred[12] == 1 and pred[0] == 0 and pred[3] == 2 and np.all(pred[:6] >= 0)


def test_sparse_product_is_the_dense_one_with_empty_rows_anywhere():
    rng = np.random.RandomState(0)
    W = np.zeros((9, 9))
    W[1, 3] = W[3, 1] = 1.0
    W[3, 6] = W[6, 3] = 0.5                                           # rows 0, 2, 4, 5, 7, 8 are empty: first, middle and last
    for indptr, indices, values in (LO.islands()[0], LO.star_and_ring(40), LO.csr_from_dense(W), LO.blobs_graph(65, 10, 10, 4, 7)[2]):
        N = len(indptr) - 1
        for dtype, bar in ((np.float64, 1e-13), (np.float32, 1e-5)):
            F, s = rng.rand(N, 5).astype(dtype), rng.rand(len(values)).astype(dtype)
            got = LO.spmm(indptr, indices, s, F)
            assert got.dtype == dtype and np.max(np.abs(got - LO.dense_from_csr(indptr, indices, s) @ F.astype(np.float64))) <= bar


def test_star_and_ring_has_one_hub():
    indptr, indices, values = LO.star_and_ring(300)
    deg = np.diff(indptr)
    assert deg[0] == 299 and np.all(deg[1:] == 3) and len(values) == 299 * 4


def test_knn_lists_are_knn_oracles():
    import knn_oracle as KO
    X, _ = LO.blobs(65, 10, 10, 3)
    X[7] = X[3]                                                       # an exact tie: two rows at the same place
    idx, d2 = LO.knn_lists(X, 7)
    ref_idx, ref_d2, _ = KO.knn(X, X, 7, self_first=0)
    assert np.array_equal(idx, ref_idx) and np.array_equal(d2, ref_d2)


def test_train_py_knows_few_label_and_defaults_it_to_off():
    import train
    args = train.parser.parse_args([])
    assert args.few_label == 0 and args.few_label_seed == 0 == args.label_seed
    args = train.parser.parse_args(["--few_label", "100", "--few_label_seed", "3"])
    assert args.few_label == 100 and args.few_label_seed == 3
    rec = train._few_label_record(dict(accuracy=0.5, accuracy_unlabeled_train=0.25, knn1=0.125, probe=0.75, n_unreached=2, n_iter=16, n_labeled=20,
                                       change=1e-7, per_class=[0.5]))
    assert rec == dict(few_label_test=0.5, few_label_unlabeled_train=0.25, few_label_knn1=0.125, few_label_probe=0.75, few_label_unreached=2,
                       few_label_iters=16, few_label_n=20)
