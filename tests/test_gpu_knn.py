"""GPU tests of the k-nearest-neighbour kernels (csrc/knn.hip) against the float64 oracle of tests/helpers/knn_oracle.py.

Exact cases: integer-valued rows whose differences, squares and sums are exact in f32, so idx and d2 must equal the oracle bit for
bit, ties included -- lattices with many duplicates and equidistant rows, and database orders that are the select's worst and best.
Real-valued cases, with u = (D + 3) 2^-24 (knn_oracle.u_bar): per query (a) the indices are in range and distinct, (b) the returned
(d2, index) ascend, (c) a returned d2 is within u of the oracle's d2 of that row, (d) and within u of the oracle's t-th smallest,
(e) every row the oracle puts below (1 - 2u) x its k-th smallest is returned.  Votes, ranks, reproducibility, refusals: exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import knn_oracle as KO      # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1
IDX_SENTINEL, D2_SENTINEL = -7, -3.0


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def padded(A, pad):
    """the f32 rows A inside a buffer of ld = D + pad with 1e30 between the rows; (the buffer on the device, its [:, :D] view)"""
    buf = np.full((A.shape[0], A.shape[1] + pad), 1e30, dtype=np.float32)
    buf[:, :A.shape[1]] = A
    t = dev(buf)
    return t, t[:, :A.shape[1]]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(M, N, D, k):
    from dmvae_hip import _lib
    nbytes = _lib.lib.dmvae_knn_ws_bytes(M, N, D, k)
    assert nbytes >= 0
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device="cuda"), int(nbytes)


def raw_knn(Q, X, k, self_first=-1, pads=(3, 2, 2)):
    """one dmvae_knn call on padded rows into sentinel-filled outputs of ldo = k + pads[2]: (idx [M][k], d2 [M][k]) on the host"""
    from dmvae_hip import _lib
    Q, X = np.asarray(Q, dtype=np.float32), np.asarray(X, dtype=np.float32)
    (M, D), N = Q.shape, X.shape[0]
    qb, _ = padded(Q, pads[0])
    xb, _ = padded(X, pads[1])
    ldo = k + pads[2]
    idx = torch.full((M, ldo), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    d2 = torch.full((M, ldo), D2_SENTINEL, dtype=torch.float32, device="cuda")
    ws, nbytes = workspace(M, N, D, k)
    rc = _lib.lib.dmvae_knn(stream(), qb.data_ptr(), qb.stride(0), M, xb.data_ptr(), xb.stride(0), N, D, k, self_first, ws.data_ptr(), nbytes,
                            idx.data_ptr(), d2.data_ptr(), ldo)
    assert rc == 0, _lib.lib.dmvae_last_error()
    ih, dh = idx.cpu().numpy(), d2.cpu().numpy()
    assert (ih[:, k:] == IDX_SENTINEL).all() and (dh[:, k:] == D2_SENTINEL).all()        # nothing outside the k columns is written
    return ih[:, :k], dh[:, :k]


def assert_exact(Q, X, k, self_first=-1, what=""):
    ref_idx, ref_d2, _ = KO.knn(Q, X, k, self_first)
    idx, d2 = raw_knn(Q, X, k, self_first)
    assert idx.dtype == np.int32 and np.array_equal(idx, ref_idx), (what, np.argwhere(idx != ref_idx)[:5].tolist())
    assert d2.tobytes() == ref_d2.astype(np.float32).tobytes(), what
    assert np.array_equal(ref_d2.astype(np.float32).astype(np.float64), ref_d2)          # what the case promises: exact in f32
    return idx, d2


def grid7(repeat_to, seed):
    """the 7 x 7 x 7 lattice, its points repeated in a shuffled order up to repeat_to rows: duplicates and equidistant rows everywhere"""
    g = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    rng = np.random.RandomState(seed)
    rows = np.concatenate([rng.permutation(len(g)) for _ in range((repeat_to + len(g) - 1) // len(g))])[:repeat_to]
    return g[rows], g


def exact_case(name):
    rng = np.random.RandomState(len(name))
    if name == "1x1":
        return np.array([[3.0]]), np.array([[5.0]]), 1, -1
    if name == "17x255-D1-k1":
        return rng.randint(-64, 65, (17, 1)), rng.randint(-64, 65, (255, 1)), 1, -1
    if name == "16x256-D3-k256":                                 # k = N: the whole database in order
        return rng.randint(-4, 5, (16, 3)), rng.randint(-4, 5, (256, 3)), 256, -1
    if name == "33x257-D33-k10":
        return rng.randint(-2, 3, (33, 33)), rng.randint(-2, 3, (257, 33)), 10, -1
    if name == "257x1003-D3-k64-grid":                           # the lattice queried from its own points
        X, g = grid7(1003, 1)
        return g[rng.randint(0, len(g), 257)], X, 64, -1
    if name == "5x2000-identical-k37":                           # every index is decided by the tie rule
        return rng.randint(-64, 65, (5, 3)), np.tile(np.array([[7.0, -64.0, 64.0]]), (2000, 1)), 37, -1
    if name == "self-100-k99":                                   # every other row once
        X = rng.randint(-6, 7, (100, 2))
        return X, X, 99, 0
    if name == "slice-40-of-300":
        X, _ = grid7(300, 2)
        return X[40:56], X, 12, 40
    if name == "D64-64x600-k20":                                 # the widest exact rows: |coordinate| <= 64, D = 64, two chunks of columns
        return rng.randint(-64, 65, (64, 64)), rng.randint(-64, 65, (600, 64)), 20, -1
    if name == "4100x600-D3-k20-grid":                           # enough queries that one workgroup walks the whole database
        X, g = grid7(600, 3)
        return g[rng.randint(0, len(g), 4100)], X, 20, -1
    raise KeyError(name)


EXACT = ["1x1", "17x255-D1-k1", "16x256-D3-k256", "33x257-D33-k10", "257x1003-D3-k64-grid", "5x2000-identical-k37", "self-100-k99", "slice-40-of-300",
         "D64-64x600-k20", "4100x600-D3-k20-grid"]


@pytest.mark.parametrize("name", EXACT)
def test_exact_cases_equal_the_oracle_bit_for_bit(name):
    Q, X, k, self_first = exact_case(name)
    idx, _ = assert_exact(np.asarray(Q, dtype=np.float32), np.asarray(X, dtype=np.float32), k, self_first, name)
    if name == "5x2000-identical-k37":
        assert np.array_equal(idx, np.tile(np.arange(37), (5, 1)))
    if name == "self-100-k99":
        assert all(sorted(idx[i].tolist()) == [j for j in range(100) if j != i] for i in range(100))
    if name == "slice-40-of-300":
        assert not (idx == 40 + np.arange(16)[:, None]).any()


def ladder(M):
    """4 099 rows at strictly increasing distance from the queries (0, 0) and (-1, 0): (s, 0), (s, 1), (s + 1, 0), ... -- d2 = s^2, s^2 + 1,
    (s + 1)^2, ... below 2^23, exact in f32.  M queries, the two in turn."""
    s = np.arange(4099) // 2 + 1
    X = np.stack([s, np.arange(4099) % 2], axis=1).astype(np.float32)
    return np.array([[0.0, 0.0], [-1.0, 0.0]], dtype=np.float32)[np.arange(M) % 2], X


@pytest.mark.parametrize("M", [3, 4100], ids=["database-split", "one-walk"])       # few queries share the database out; many walk all of it
@pytest.mark.parametrize("k", [1, 37, 256])
@pytest.mark.parametrize("order", ["decreasing", "increasing", "nearest-last"])
def test_adversarial_orders_for_the_select(order, k, M):
    Q, X = ladder(M)
    d = KO.pair_d2(Q[:1], X)[0]
    assert np.all(np.diff(d) > 0)
    if order == "decreasing":                                    # every column is an insertion
        X = X[::-1]
    elif order == "nearest-last":
        X = np.concatenate([X[k:][np.random.RandomState(k).permutation(4099 - k)], X[:k]])
    X = np.ascontiguousarray(X)
    ref_idx, ref_d2, _ = KO.knn(Q[:2], X, k)                     # the oracle of the two distinct queries, shared by the M rows
    idx, d2 = raw_knn(Q, X, k)
    assert np.array_equal(idx, ref_idx[np.arange(M) % 2]), (order, k, M)
    assert d2.tobytes() == ref_d2.astype(np.float32)[np.arange(M) % 2].tobytes()
    assert np.array_equal(ref_d2.astype(np.float32).astype(np.float64), ref_d2)
    if order == "increasing":                                   # no insertion after the first k
        assert np.array_equal(idx, np.tile(np.arange(k), (M, 1)))
    if order == "decreasing":
        assert np.array_equal(idx, np.tile(4098 - np.arange(k), (M, 1)))


REAL_SHAPES = [(257, 1003, 3, 10), (64, 4097, 10, 64), (100, 2000, 64, 50), (33, 1500, 300, 128), (50, 1000, 70, 256)]


@pytest.mark.parametrize("kind", ["normal", "near"])
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_real_valued_rows_against_the_float64_oracle(shape, kind):
    M, N, D, k = shape
    rng = np.random.RandomState(M + N + D + k)
    if kind == "normal":
        Q, X = rng.randn(M, D), rng.randn(N, D)
    else:                                                        # near rows: a norm expansion would cancel
        Q, X = 5.0 + 0.01 * rng.randn(M, D), 5.0 + 0.01 * rng.randn(N, D)
    Q, X = Q.astype(np.float32), X.astype(np.float32)
    idx, d2 = raw_knn(Q, X, k)
    ref = KO.pair_d2(Q, X)                                       # float64, from the f32 inputs
    u = KO.u_bar(D)
    assert idx.min() >= 0 and idx.max() < N                                                               # (a)
    assert all(len(set(row.tolist())) == k for row in idx)
    assert np.all((np.diff(d2, axis=1) > 0) | ((np.diff(d2, axis=1) == 0) & (np.diff(idx, axis=1) > 0)))  # (b)
    of_idx = np.take_along_axis(ref, idx.astype(np.int64), axis=1)
    smallest = np.sort(ref, axis=1)[:, :k]
    err_c = np.abs(d2 - of_idx) / of_idx
    err_d = np.abs(d2 - smallest) / smallest
    print("%s %s: max |d2 - oracle of the index| = %.3f u, max |d2 - oracle's t-th| = %.3f u" % (shape, kind, err_c.max() / u, err_d.max() / u))
    assert err_c.max() <= u and err_d.max() <= u                                                          # (c), (d)
    got = np.zeros((M, N), dtype=bool)
    np.put_along_axis(got, idx.astype(np.int64), True, axis=1)
    required = ref < (1.0 - 2.0 * u) * smallest[:, -1:]
    assert not (required & ~got).any()                                                                    # (e)


def raw_vote(idx, classes, N, Cn, pads=(3, 2)):
    from dmvae_hip import _lib
    M, k = idx.shape
    ib = torch.full((M, k + pads[0]), 1 << 30, dtype=torch.int32, device="cuda")      # what lies between the rows would flag
    ib[:, :k] = dev(idx, torch.int32)
    counts = torch.full((M, Cn + pads[1]), -3.0, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _lib.lib.dmvae_knn_vote(stream(), ib.data_ptr(), ib.stride(0), M, k, dev(classes, torch.int32).data_ptr(), N, Cn, counts.data_ptr(),
                                 counts.stride(0), flag.data_ptr())
    assert rc == 0, _lib.lib.dmvae_last_error()
    ch = counts.cpu().numpy()
    assert (ch[:, Cn:] == -3.0).all()
    return counts[:, :Cn], ch[:, :Cn], int(flag.item())


@pytest.mark.parametrize("k", [1, 5, 256])
@pytest.mark.parametrize("Cn", [2, 10, 4096])
def test_vote_counts_equal_bincount_and_ties_go_to_the_smallest_class(Cn, k):
    from dmvae_hip import metrics
    rng = np.random.RandomState(Cn + k)
    M, N = 37, 500
    classes = rng.randint(0, Cn, N)
    idx = rng.randint(0, N, (M, k))
    if k == 5 and Cn >= 4:                                       # 2 - 2 - 1 among 5: the smaller of the two tied classes
        classes[:5] = [3, 1, 3, 1, 0]
        idx[0] = [0, 1, 2, 3, 4]
    view, counts, flag = raw_vote(idx, classes, N, Cn)
    ref, pred = KO.vote(idx, classes, Cn)
    assert flag == 0 and np.array_equal(counts, ref.astype(np.float32)) and (counts.sum(axis=1) == k).all()
    labels = metrics.argmax_labels(view).cpu().numpy()           # the strided counts where they lie
    assert np.array_equal(labels, pred)
    if k == 5 and Cn >= 4:
        assert counts[0, :4].tolist() == [1, 2, 0, 2] and labels[0] == 1


def test_vote_flags_a_class_or_an_index_out_of_range_and_counts_it_nowhere():
    rng = np.random.RandomState(0)
    N, Cn, k = 50, 6, 4
    classes = rng.randint(0, Cn, N)
    idx = rng.randint(0, N, (9, k))
    for bad_index in (N, -1, 1 << 30):
        broken = idx.copy()
        broken[4, 2] = bad_index
        _, counts, flag = raw_vote(broken, classes, N, Cn)
        ref, _ = KO.vote(np.delete(idx[4], 2)[None], classes, Cn)
        assert flag == 1 and np.array_equal(counts[4], ref[0]) and counts[4].sum() == k - 1
        assert np.array_equal(np.delete(counts, 4, axis=0), np.delete(KO.vote(idx, classes, Cn)[0], 4, axis=0))
    for bad_class in (Cn, -2):
        cl = classes.copy()
        cl[idx[3, 1]] = bad_class
        _, counts, flag = raw_vote(idx, cl, N, Cn)
        keep = cl[idx] != bad_class
        assert flag == 1 and np.array_equal(counts.sum(axis=1), keep.sum(axis=1))
        assert all(np.array_equal(counts[i], np.bincount(cl[idx[i]][keep[i]], minlength=Cn)) for i in range(len(idx)))


def raw_ranks(X, idx, pads=(2, 1, 3)):
    from dmvae_hip import _lib
    N, D = X.shape
    k = idx.shape[1]
    xb, _ = padded(np.asarray(X, dtype=np.float32), pads[0])
    ib = torch.full((N, k + pads[1]), 1 << 30, dtype=torch.int32, device="cuda")
    ib[:, :k] = dev(idx, torch.int32)
    ranks = torch.full((N, k + pads[2]), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _lib.lib.dmvae_knn_ranks(stream(), xb.data_ptr(), xb.stride(0), N, D, ib.data_ptr(), ib.stride(0), k, ranks.data_ptr(), ranks.stride(0),
                                  flag.data_ptr())
    assert rc == 0, _lib.lib.dmvae_last_error()
    rh = ranks.cpu().numpy()
    assert (rh[:, k:] == IDX_SENTINEL).all()
    return rh[:, :k], int(flag.item())


def other_rows(N, k, seed):
    """idx [N][k] of arbitrary rows != i"""
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, N - 1, (N, k))
    return idx + (idx >= np.arange(N)[:, None])


def test_ranks_equal_the_oracle_on_integer_lattices():
    X, _ = grid7(400, 3)                                         # every point at least once, 57 twice: ties and duplicates in every row
    X[[17, 250, 399]] = X[0]                                     # copies of ROW 0: the pair (d2 = +0, row 0) is the smallest key there is
    near, _, _ = KO.knn(X, X, 7, self_first=0)
    assert near[17, 0] == 0 and near[250, 0] == 0 and near[399, 0] == 0 and near[0, 0] == 17
    got, flag = raw_ranks(X, near)
    assert flag == 0 and np.array_equal(got, np.tile(np.arange(7), (400, 1)))        # a row's own t-th neighbour has rank t
    far = other_rows(400, 5, 1)
    far[17, 3] = far[250, 0] = far[399, 4] = far[5, 2] = 0       # row 0 asked for from its copies (rank 0) and from another row
    far[0, 1] = 399                                              # and the last copy from row 0: rows 17 and 250 come before it
    got, flag = raw_ranks(X, far)
    assert flag == 0 and np.array_equal(got, KO.ranks(X, far))
    assert got[17, 3] == 0 and got[250, 0] == 0 and got[399, 4] == 0 and got[0, 1] == 2
    Y = np.random.RandomState(4).randint(-64, 65, (257, 64)).astype(np.float32)      # two chunks of columns, a ragged last workgroup
    far = other_rows(257, 256, 2)                                                    # the largest k
    got, flag = raw_ranks(Y, far)
    assert flag == 0 and np.array_equal(got, KO.ranks(Y, far))


@pytest.mark.parametrize("N,D", [(300, 3), (1003, 64)])
def test_ranks_of_real_valued_rows_differ_only_inside_near_ties(N, D):
    X = np.random.RandomState(N).randn(N, D).astype(np.float32)
    idx = other_rows(N, 6, N)
    got, flag = raw_ranks(X, idx)
    ref, d2, u = KO.ranks(X, idx), KO.pair_d2(X, X), KO.u_bar(D)
    assert flag == 0
    pivot = np.take_along_axis(d2, idx, axis=1)                  # [N][k]
    near = (np.abs(d2[:, None, :] - pivot[:, :, None]) <= 2.0 * u * pivot[:, :, None]).sum(axis=2) - 1      # rows the oracle cannot tell from j (j itself aside)
    print("ranks N=%d D=%d: %d of %d differ from the oracle, %d pairs have a near tie" % (N, D, (got != ref).sum(), got.size, (near > 0).sum()))
    assert np.all(np.abs(got - ref) <= near)


def test_ranks_flag_an_index_out_of_range_or_equal_to_the_row():
    X, _ = grid7(60, 5)
    X[40] = X[0]
    idx = other_rows(60, 3, 0)
    idx[40, 0] = 0                                               # a real pair at d2 = 0 with row 0 beside the refused ones: rank 0, not -1
    ref = KO.ranks(X, idx)
    for i, bad in ((7, 60), (20, -1), (33, 33)):
        broken = idx.copy()
        broken[i, 1] = bad
        got, flag = raw_ranks(X, broken)
        assert flag == 1 and got[i, 1] == -1
        keep = np.ones_like(idx, dtype=bool)
        keep[i, 1] = False
        assert np.array_equal(got[keep], ref[keep]) and got[40, 0] == 0


def test_trustworthiness_equals_the_oracle_and_is_one_for_the_identity():
    from dmvae_hip import knn
    from dmvae_hip.tsne import TSNE
    X, _ = grid7(300, 6)
    rng = np.random.RandomState(6)
    Y = (X[:, :2] * 3 + rng.randint(-2, 3, (300, 2))).astype(np.float32)             # an integer-valued embedding: exact
    for k in (1, 5, 40):
        t = knn.trustworthiness(X, Y, n_neighbors=k)
        assert isinstance(t, float) and abs(t - KO.trustworthiness(X, Y, k)) <= 1e-12 and 0.0 < t < 1.0
    assert knn.trustworthiness(dev(X), dev(X), 5) == 1.0
    Z = rng.randn(257, 9).astype(np.float32)
    assert knn.trustworthiness(Z, Z, 12) == 1.0
    ts = TSNE()
    ts.embedding_device_ = dev(Y)
    assert ts.trustworthiness(X, n_neighbors=5) == knn.trustworthiness(X, Y, 5)
    for k in (150, 151, 299):
        with pytest.raises(ValueError):
            knn.trustworthiness(X, Y, n_neighbors=k)             # k < n / 2


def test_python_surface_takes_arrays_and_strided_views_and_votes_like_the_oracle():
    from dmvae_hip import knn
    rng = np.random.RandomState(9)
    X, Q = rng.randint(-5, 6, (700, 4)).astype(np.float32), rng.randint(-5, 6, (90, 4)).astype(np.float32)
    y = rng.randint(0, 7, 700) * 10 + 3                           # class values 3, 13, .., 63
    ref_idx, ref_d2, _ = KO.knn(Q, X, 5)
    idx, d2 = knn.kneighbors(Q, X, 5)                            # arrays that are uploaded
    assert idx.is_cuda and idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (90, 5)
    assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(d2.cpu().numpy(), ref_d2.astype(np.float32))
    _, xv = padded(X, 3)
    _, qv = padded(Q, 5)
    idx2, d22 = knn.kneighbors(qv, xv, 5)                        # row-strided views, where they lie
    assert torch.equal(idx, idx2) and torch.equal(d2, d22)
    sl, _ = knn.kneighbors(xv[100:140], xv, 5, self_first=100)
    assert np.array_equal(sl.cpu().numpy(), KO.knn(X, X, 5, self_first=0)[0][100:140])
    clf = knn.KNeighborsClassifier(n_neighbors=5).fit(X, y)
    _, pred = KO.vote(ref_idx, (y - 3) // 10, 7)
    got = clf.predict(Q)
    assert np.array_equal(clf.classes_, np.arange(7) * 10 + 3) and np.array_equal(got, pred * 10 + 3)
    assert clf.score(Q, got) == 1.0 and clf.score(qv, y[:90]) == float(np.mean(got == y[:90]))
    assert torch.equal(clf.kneighbors(qv)[0], idx)


def test_a_second_call_returns_the_same_bytes():
    rng = np.random.RandomState(3)
    Q, X = rng.randn(40, 20).astype(np.float32), rng.randn(3000, 20).astype(np.float32)       # few queries: the database is split
    a, b = raw_knn(Q, X, 30), raw_knn(Q, X, 30)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    Q2 = rng.randn(4200, 5).astype(np.float32)                   # many queries: one workgroup walks the whole database
    a, b = raw_knn(Q2, Q2, 9, 0), raw_knn(Q2, Q2, 9, 0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    ref_idx, _, _ = KO.knn(Q2[:64], Q2, 9, self_first=0)
    assert (a[0][:64] == ref_idx).mean() > 0.999                 # (real-valued: the test above holds it to the bar)
    idx = other_rows(3000, 4, 0)
    r1, r2 = raw_ranks(X, idx), raw_ranks(X, idx)
    assert r1[0].tobytes() == r2[0].tobytes()
    cls = rng.randint(0, 10, 3000)
    v1, v2 = raw_vote(idx, cls, 3000, 10), raw_vote(idx, cls, 3000, 10)
    assert v1[1].tobytes() == v2[1].tobytes()


def test_refused_arguments_return_einval_and_write_nothing():
    from dmvae_hip import _lib
    M, N, D, k = 4, 2000, 3, 8                                   # few queries: this shape needs a workspace
    rng = np.random.RandomState(0)
    qb, _ = padded(rng.randn(M, D).astype(np.float32), 2)
    xb, _ = padded(rng.randn(N, D).astype(np.float32), 1)
    need = _lib.lib.dmvae_knn_ws_bytes(M, N, D, k)
    assert need > 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    idx = torch.full((M, 300), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    d2 = torch.full((M, 300), D2_SENTINEL, dtype=torch.float32, device="cuda")
    good = dict(Q=qb.data_ptr(), ldq=qb.stride(0), M=M, X=xb.data_ptr(), ldx=xb.stride(0), N=N, D=D, k=k, self_first=-1, ws=ws.data_ptr(), ws_bytes=need,
                idx=idx.data_ptr(), d2=d2.data_ptr(), ldo=300)

    def call(**change):
        a = dict(good, **change)
        return _lib.lib.dmvae_knn(stream(), a["Q"], a["ldq"], a["M"], a["X"], a["ldx"], a["N"], a["D"], a["k"], a["self_first"], a["ws"], a["ws_bytes"],
                                  a["idx"], a["d2"], a["ldo"])

    bad = [dict(k=0), dict(k=257), dict(N=8, self_first=0), dict(ldo=k - 1), dict(ldq=D - 1), dict(ldx=D - 1), dict(Q=None), dict(X=None),
           dict(idx=None), dict(d2=None), dict(ws=None), dict(ws_bytes=need - 1), dict(ws=ws.data_ptr() + 4), dict(M=0), dict(N=0), dict(D=0),
           dict(M=(1 << 20) + 1)]
    for change in bad:
        assert call(**change) == EINVAL, change
        assert b"dmvae_knn" in _lib.lib.dmvae_last_error(), change
    torch.cuda.synchronize()
    assert (idx == IDX_SENTINEL).all() and (d2 == D2_SENTINEL).all()
    assert call() == 0                                           # and the same arguments unchanged are accepted
    assert call(N=9, self_first=0) == 0                          # k = N - 1 with the row itself left out
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    counts = torch.full((M, 16), -3.0, dtype=torch.float32, device="cuda")
    cls = torch.zeros(N, dtype=torch.int32, device="cuda")
    vote = _lib.lib.dmvae_knn_vote
    for args in ((None, 300, M, k, cls.data_ptr(), N, 10, counts.data_ptr(), 16, flag.data_ptr()),
                 (idx.data_ptr(), 300, M, k, cls.data_ptr(), N, 4097, counts.data_ptr(), 4097, flag.data_ptr()),
                 (idx.data_ptr(), 300, M, k, cls.data_ptr(), N, 0, counts.data_ptr(), 16, flag.data_ptr()),
                 (idx.data_ptr(), 300, M, k, cls.data_ptr(), N, 10, counts.data_ptr(), 9, flag.data_ptr()),
                 (idx.data_ptr(), k - 1, M, k, cls.data_ptr(), N, 10, counts.data_ptr(), 16, flag.data_ptr()),
                 (idx.data_ptr(), 300, M, k, cls.data_ptr(), N, 10, counts.data_ptr(), 16, None)):
        assert vote(stream(), *args) == EINVAL and b"dmvae_knn_vote" in _lib.lib.dmvae_last_error(), args
    ranks = torch.full((N, 12), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    ridx = torch.zeros((N, 12), dtype=torch.int32, device="cuda")
    rk = _lib.lib.dmvae_knn_ranks
    for args in ((None, 4, N, D, ridx.data_ptr(), 12, 8, ranks.data_ptr(), 12, flag.data_ptr()),
                 (xb.data_ptr(), D - 1, N, D, ridx.data_ptr(), 12, 8, ranks.data_ptr(), 12, flag.data_ptr()),
                 (xb.data_ptr(), 4, 1, D, ridx.data_ptr(), 12, 1, ranks.data_ptr(), 12, flag.data_ptr()),
                 (xb.data_ptr(), 4, 8, D, ridx.data_ptr(), 12, 8, ranks.data_ptr(), 12, flag.data_ptr()),
                 (xb.data_ptr(), 4, N, D, ridx.data_ptr(), 12, 257, ranks.data_ptr(), 300, flag.data_ptr()),
                 (xb.data_ptr(), 4, N, D, ridx.data_ptr(), 7, 8, ranks.data_ptr(), 12, flag.data_ptr()),
                 (xb.data_ptr(), 4, N, D, ridx.data_ptr(), 12, 8, ranks.data_ptr(), 7, flag.data_ptr()),
                 (xb.data_ptr(), 4, N, D, ridx.data_ptr(), 12, 8, ranks.data_ptr(), 12, None)):
        assert rk(stream(), *args) == EINVAL and b"dmvae_knn_ranks" in _lib.lib.dmvae_last_error(), args
    torch.cuda.synchronize()
    assert (counts == -3.0).all() and (ranks == IDX_SENTINEL).all() and int(flag.item()) == 0
