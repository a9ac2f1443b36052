"""GPU tests of dmvae_prdc_counts (csrc/prdc.hip) and dmvae_hip.prdc against the float64 oracle of tests/helpers/prdc_oracle.py.

Exact cases: integer-valued rows (|coordinate| <= 64, D <= 64) make every difference, square and sum exact in f32, so every output equals
the oracle EXACTLY, pairs that lie on a radius (closed balls) and tied minima (the lowest j) included.

Real-valued cases, with u = (D + 3) 2^-24 (knn_oracle.u_bar) and the oracle's own k-th-neighbour radii rounded to f32 handed in: a pair
is DECIDED when |d2 - r2| > 2 u max(d2, r2) in float64.  Each device count lies between the decided-inside pairs of its row or column
and that number plus the undecided ones; real_min_d2 is within u of the oracle's minimum.  The cases themselves are held to two
conditions on the oracle: undecided pairs are at most 1e-3 of all pairs, and each of the four metrics lies strictly inside (0.05, 0.95) in
at least one case, so that a constant 0 or 1 cannot pass."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import prdc_oracle as PO      # noqa: E402

pytestmark = pytest.mark.gpu

METRICS = ("precision", "recall", "density", "coverage")


def stream():
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def padded(a, pad):
    """a [n][D] on the device at row stride D + pad, NaN between the rows: reading there would poison a distance"""
    a = np.asarray(a, dtype=np.float32)
    t = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device="cuda")
    t[:, :a.shape[1]] = torch.as_tensor(a).cuda()
    return t


def raw_counts(R, F, rR2, rF2, out=None, pads=(3, 1), min_j=True):
    """dmvae_prdc_counts through the C entry on row-padded inputs; out: the four device buffers of an earlier call, written again"""
    from dmvae_hip import _lib
    (N, D), M = np.shape(R), len(F)
    Rd, Fd = padded(R, pads[0]), padded(F, pads[1])
    r1, r2 = torch.as_tensor(np.asarray(rR2, dtype=np.float32)).cuda(), torch.as_tensor(np.asarray(rF2, dtype=np.float32)).cuda()
    if out is None:                                              # garbage to start with, guard words behind every vector
        out = (torch.full((M + 2,), 12345, dtype=torch.int32, device="cuda"), torch.full((N + 2,), -7, dtype=torch.int32, device="cuda"),
               torch.full((N + 2,), -3.0, dtype=torch.float32, device="cuda"), torch.full((N + 2,), -9, dtype=torch.int32, device="cuda"))
    guards = [o[-2:].clone() for o in out]
    rc = _lib.lib.dmvae_prdc_counts(stream(), Rd.data_ptr(), Rd.stride(0), N, Fd.data_ptr(), Fd.stride(0), M, D, r1.data_ptr(), r2.data_ptr(),
                                    out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr() if min_j else None)
    assert rc == 0, _lib.lib.dmvae_last_error()
    torch.cuda.synchronize()
    for o, g in zip(out, guards):
        assert torch.equal(o[-2:], g)                            # nothing behind the vectors is written
    host = dict(fake_in_real=out[0][:M].cpu().numpy(), real_in_fake=out[1][:N].cpu().numpy(), real_min_d2=out[2][:N].cpu().numpy(),
                real_min_j=out[3][:N].cpu().numpy())
    return host, out


def assert_exact(got, R, F, rR2, rF2, min_j=True):
    ref = PO.counts(R, F, rR2, rF2)
    assert np.array_equal(got["fake_in_real"], ref["fake_in_real"])
    assert np.array_equal(got["real_in_fake"], ref["real_in_fake"])
    assert np.array_equal(got["real_min_d2"].astype(np.float64), ref["real_min_d2"])
    if min_j:
        assert np.array_equal(got["real_min_j"], ref["real_min_j"])
    return ref


def lattice():
    g = np.arange(7)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)        # 343 rows


@pytest.mark.parametrize("shift", [0, 1], ids=["itself", "shifted"])
@pytest.mark.parametrize("k", [1, 6, 10])
def test_lattice_pairs_on_a_radius_and_tied_minima(shift, k):
    R = lattice()
    F = R + np.array([float(shift), 0.0, 0.0])
    if shift:                                                    # the shifted copy in another order, 60 of its rows twice: min_j is no
        F = F[np.random.RandomState(k).permutation(len(F))]      # identity, and a minimum is reached at two j
        F = np.concatenate([F, F[:60]])
    rR2, rF2 = PO.radii(R, k), PO.radii(F, k)
    got, _ = raw_counts(R, F, rR2, rF2)
    ref = assert_exact(got, R, F, rR2, rF2)
    on_radius = np.count_nonzero(ref["d2"] == rR2[:, None])
    assert on_radius > len(R)                                    # what this test is for: many pairs lie exactly ON a ball
    assert np.count_nonzero(ref["d2"] < rR2[:, None]) < ref["fake_in_real"].sum()      # the open rule would count fewer
    if shift:                                                    # the real rows off the x = 0 face coincide with a generated row: d2 = 0
        assert (ref["real_min_d2"] == 0).sum() == 6 * 49 and (ref["real_min_d2"] == 1).sum() == 49
        tied = np.sum(ref["d2"] == ref["real_min_d2"][:, None], axis=1)
        assert (tied > 1).sum() >= 40                            # the rows nearest a doubled generated row: the lowest j wins
    from dmvae_hip import prdc
    m, want = prdc.prdc(R, F, k), PO.prdc(R, F, k)               # end to end, the radii from dmvae_knn: exact as well
    assert {n: m[n] for n in METRICS} == {n: want[n] for n in METRICS} and m["k"] == k
    if not shift:
        assert m["precision"] == m["recall"] == m["coverage"] == 1.0 and m["density"] > 1.0


def test_identical_rows_radii_zero_every_pair_inside():
    R = np.tile(np.array([[3.0, -2.0, 7.0, 1.0, 0.0]]), (200, 1))
    z = np.zeros(200)
    got, _ = raw_counts(R, R, z, z)
    assert_exact(got, R, R, z, z)
    assert (got["fake_in_real"] == 200).all() and (got["real_in_fake"] == 200).all() and (got["real_min_d2"] == 0).all() and (got["real_min_j"] == 0).all()
    from dmvae_hip import prdc
    m = prdc.prdc(R, R, 5)                                       # the k-th neighbour is at distance 0
    assert (m["precision"], m["recall"], m["coverage"], m["density"]) == (1.0, 1.0, 1.0, 200 / 5)


def int_rows(rng, n, D, lo=-4, hi=5):
    return rng.randint(lo, hi, (n, D)).astype(np.float64)


def test_infinite_radii_give_full_counts_and_zero_radii_none():
    rng = np.random.RandomState(3)
    R, F = int_rows(rng, 37, 4, -64, 65), int_rows(rng, 300, 4, -64, 64) + 0.5      # never coincident: every d2 > 0, halves are exact
    inf_r, inf_f = np.full(37, np.inf), np.full(300, np.inf)
    got, _ = raw_counts(R, F, inf_r, inf_f)
    assert_exact(got, R, F, inf_r, inf_f)
    assert (got["fake_in_real"] == 37).all() and (got["real_in_fake"] == 300).all()
    got, _ = raw_counts(R, F, np.zeros(37), np.zeros(300))
    assert_exact(got, R, F, np.zeros(37), np.zeros(300))
    assert (got["fake_in_real"] == 0).all() and (got["real_in_fake"] == 0).all() and (got["real_min_d2"] > 0).all()
    mixed = np.where(np.arange(37) % 2 == 0, np.inf, 0.0)        # every other real ball holds everything
    got, _ = raw_counts(R, F, mixed, np.zeros(300))
    assert_exact(got, R, F, mixed, np.zeros(300))
    assert (got["fake_in_real"] == 19).all()


EXACT_SHAPES = [(1, 1, 1), (2, 2, 1), (17, 257, 5), (16, 256, 32), (300, 1000, 33), (33, 513, 64)]


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_rows_equal_the_oracle_exactly(shape):
    N, M, D = shape
    rng = np.random.RandomState(N + M + D)
    span = 64 if D <= 5 else 3                                   # |coordinate| <= 64; small spans in wide rows keep exact ties frequent
    R, F = int_rows(rng, N, D, -span, span + 1), int_rows(rng, M, D, -span, span + 1)
    d2 = PO.pair_d2(R, F)
    assert d2.max() < 2 ** 24
    rR2 = d2[np.arange(N), rng.randint(0, M, N)]                 # radii that ARE distances of pairs: every row and column has a pair ON its ball
    rF2 = d2[rng.randint(0, N, M), np.arange(M)]
    got, out = raw_counts(R, F, rR2, rF2)
    ref = assert_exact(got, R, F, rR2, rF2)
    assert ref["fake_in_real"].sum() > 0 and ref["real_in_fake"].sum() > 0
    # the same buffers again: fake_in_real is zeroed by the entry, not added into twice, and two calls give the same bits
    again, _ = raw_counts(R, F, rR2, rF2, out=out)
    for name in got:
        assert np.array_equal(got[name], again[name]), name
    # other radii into the same buffers: nothing of the first call is left
    got3, _ = raw_counts(R, F, np.zeros(N), np.zeros(M), out=out)
    assert_exact(got3, R, F, np.zeros(N), np.zeros(M))
    nomin, _ = raw_counts(R, F, rR2, rF2, min_j=False)           # real_min_j may be NULL: its buffer keeps its fill
    assert_exact(nomin, R, F, rR2, rF2, min_j=False)
    assert (nomin["real_min_j"] == -9).all()


# ---------------------------------------------------------------------------------------------------------------- real-valued rows
REAL_SHAPES = [(257, 1003, 3, 5), (100, 300, 33, 3), (1000, 517, 70, 10), (33, 1500, 300, 5)]
_cases = {}


def real_case(shape, kind):
    """(R, F f32; the oracle's radii rounded to f32; the oracle's counts and metrics on them; the undecided pairs), computed once"""
    key = (shape, kind)
    if key not in _cases:
        N, M, D, k = shape
        rng = np.random.RandomState(0)
        shift, scale = (0.5, 0.8) if D < 33 else (0.0, 1.0)      # wide rows: a 0.8 scale drives recall to about 0
        loc, sc = (0.0, 1.0) if kind == "normal" else (5.0, 0.01)
        R = (loc + sc * rng.randn(N, D)).astype(np.float32)
        F = (loc + sc * (shift + scale * rng.randn(M, D))).astype(np.float32)
        rR2 = PO.radii(R, k).astype(np.float32).astype(np.float64)
        rF2 = PO.radii(F, k).astype(np.float32).astype(np.float64)
        ref = PO.counts(R, F, rR2, rF2)
        u = PO.u_bar(D)
        und_r, und_f = PO.undecided(ref["d2"], rR2[:, None], u), PO.undecided(ref["d2"], rF2[None, :], u)
        _cases[key] = dict(R=R, F=F, rR2=rR2, rF2=rF2, ref=ref, u=u, und_r=und_r, und_f=und_f, k=k, metrics=PO.metrics_from_counts(ref, rR2, k))
    return _cases[key]


def test_the_real_valued_cases_are_fit_to_test_with():
    interior = {m: [] for m in METRICS}
    for shape in REAL_SHAPES:
        for kind in ("normal", "near"):
            c = real_case(shape, kind)
            pairs = c["ref"]["d2"].size
            print("%s %s: undecided %d (real radii) + %d (generated radii) of %d pairs; %s" % (
                shape, kind, c["und_r"].sum(), c["und_f"].sum(), pairs, {m: round(v, 4) for m, v in c["metrics"].items()}))
            assert c["und_r"].sum() + c["und_f"].sum() <= 1e-3 * pairs
            for m in METRICS:
                if 0.05 < c["metrics"][m] < 0.95:
                    interior[m].append((shape, kind))
    assert all(interior[m] for m in METRICS), interior


@pytest.mark.parametrize("kind", ["normal", "near"])
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_real_valued_rows_against_the_float64_oracle(shape, kind):
    c = real_case(shape, kind)
    ref, u = c["ref"], c["u"]
    got, _ = raw_counts(c["R"], c["F"], c["rR2"], c["rF2"])
    in_r, in_f = (ref["d2"] <= c["rR2"][:, None]) & ~c["und_r"], (ref["d2"] <= c["rF2"][None, :]) & ~c["und_f"]
    lo, hi = in_r.sum(axis=0), in_r.sum(axis=0) + c["und_r"].sum(axis=0)
    assert np.all((lo <= got["fake_in_real"]) & (got["fake_in_real"] <= hi))
    lo, hi = in_f.sum(axis=1), in_f.sum(axis=1) + c["und_f"].sum(axis=1)
    assert np.all((lo <= got["real_in_fake"]) & (got["real_in_fake"] <= hi))
    err = np.abs(got["real_min_d2"].astype(np.float64) - ref["real_min_d2"]) / ref["real_min_d2"]
    print("%s %s: max |min d2 - oracle| = %.3f u" % (shape, kind, err.max() / u))
    assert err.max() <= u
    j = got["real_min_j"].astype(np.int64)
    assert j.min() >= 0 and j.max() < len(c["F"])
    assert np.all(ref["d2"][np.arange(len(j)), j] <= ref["real_min_d2"] * (1.0 + 2.0 * u))      # the row it names is a nearest one
    again, _ = raw_counts(c["R"], c["F"], c["rR2"], c["rF2"])
    for name in got:
        assert np.array_equal(got[name], again[name]), name      # two calls: the same bits

    # end to end, the radii from dmvae_knn: off by at most the pairs and rows the f32 distance cannot decide
    from dmvae_hip import prdc
    N, M, k = len(c["R"]), len(c["F"]), c["k"]
    rng = np.random.RandomState(1)
    g_r, g_f = rng.randint(0, 4, N), rng.randint(0, 3, M)
    m = prdc.prdc(torch.as_tensor(c["R"]).cuda(), c["F"], k, real_groups=g_r, fake_groups=torch.as_tensor(g_f.astype(np.int32)).cuda())
    near = 0
    for X in (c["R"], c["F"]):
        srt = np.sort(PO.pair_d2(X, X), axis=1)[:, 1:]           # (column 0: the row itself)
        near += int(np.count_nonzero(srt[:, k] - srt[:, k - 1] <= 2.0 * u * srt[:, k])) if srt.shape[1] > k else 0
    slack = int(c["und_r"].sum() + c["und_f"].sum()) + near
    for name, den in (("precision", M), ("recall", N), ("density", k * M), ("coverage", N)):
        print("%s %s: %s device %.6f oracle %.6f (slack %d / %d)" % (shape, kind, name, m[name], c["metrics"][name], slack, den))
        assert abs(m[name] - c["metrics"][name]) <= slack / den + 1e-12
    if slack == 0:                                               # nothing to decide: the group vectors equal the np.bincount oracle
        want = PO.prdc(c["R"], c["F"], k, c["rR2"], c["rF2"], real_groups=g_r, fake_groups=g_f)
        for name in ("coverage_per_group", "recall_per_group", "precision_per_group", "density_per_group"):
            assert np.array_equal(np.array(m[name]), want[name]), name


def test_group_vectors_equal_the_bincount_oracle_on_integer_rows():
    from dmvae_hip import prdc
    rng = np.random.RandomState(7)
    R, F = int_rows(rng, 150, 3), int_rows(rng, 420, 3)
    g_r, g_f = rng.randint(0, 5, 150), rng.randint(0, 7, 420)
    g_f[g_f == 4] = 5                                            # a group without rows: nan on both sides
    for k in (1, 5):
        m, want = prdc.prdc(R, F, k, real_groups=g_r, fake_groups=g_f), PO.prdc(R, F, k, real_groups=g_r, fake_groups=g_f)
        assert {n: m[n] for n in METRICS} == {n: want[n] for n in METRICS}
        for name in ("coverage_per_group", "recall_per_group", "precision_per_group", "density_per_group"):
            assert np.array_equal(np.array(m[name]), want[name], equal_nan=True), name
        assert np.isnan(m["precision_per_group"][4]) and len(m["precision_per_group"]) == 7 and len(m["recall_per_group"]) == 5
    with pytest.raises(ValueError):
        prdc.prdc(R, F, 0)
    with pytest.raises(ValueError):
        prdc.prdc(R[:4], F, 4)
    with pytest.raises(ValueError):
        prdc.prdc(R, F, 3, real_groups=g_r[:-1])
