"""GPU tests of the label-spreading kernels (csrc/label_spread.hip) through the C ABI, on caller buffers pre-filled with known bits, against the
float64 oracle of tests/helpers/label_spread_oracle.py running the SAME number of iterations on the SAME float32 inputs.

Bars.  Normalisation: relative 4 * 2^-24 -- one rounding of r_i, one of r_j, two multiplies.  Iteration: tolerance("pred", oracle, yardstick) of
tests/helpers/moe_cases.py, the project's forward bar with its absolute part raised to twice the error of the float32 yardstick (the same
iteration in np.float32) where that is larger; each change_t is held to the same rule.  Everything the entries must not touch -- the columns
>= C of the caller's F (ldf = C + 3), the entries of `change` past n_iter, the tails of s -- is compared by bits, and so are determinism,
chunking through F_in and the refusals."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import label_spread_oracle as LO      # noqa: E402
import moe_cases as MC                # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1
F_SENTINEL, CH_SENTINEL, S_SENTINEL = -7.0, -3.0, -5.0
ALPHAS, STEPS = (0.2, 0.8, 0.99), (1, 8, 57)
PATTERNS = ("none", "all", "mixed", "class0", "classC-1")
U = 2.0 ** -24

BLOB_N = (1, 2, 63, 64, 65, 257)
BLOB_C = (2, 17, 64, 65, 257)                                         # N = 65: one chunk per row .. two passes of the 64 lanes
GRAPHS = (["blobs-N%d" % n for n in BLOB_N] + ["blobs-C%d" % c for c in BLOB_C] + ["star300", "islands", "blobs-5000"])
BLOBS = [g for g in GRAPHS if g.startswith("blobs")]


@functools.lru_cache(maxsize=None)
def graph(name):
    """(csr = (indptr, indices, values f32), classes int64 [N], C)"""
    if name == "star300":
        return LO.star_and_ring(300), np.arange(300) % 10, 10
    if name == "islands":
        csr, y, Cn = LO.islands()
        return csr, np.arange(13) % Cn, Cn
    if name == "blobs-5000":
        _, cls, csr = LO.blobs_graph(5000, 10, 10, 4, 10)
        return csr, cls, 10
    kind, v = name.split("-")[1][0], int(name.split("-")[1][1:])
    N, Cn = (v, 10) if kind == "N" else (65, v)
    _, cls, csr = LO.blobs_graph(N, Cn, 10, 4, min(7, N - 1))
    return csr, cls, Cn


@functools.lru_cache(maxsize=None)
def normalized(name):
    """(s float32 [nnz]: the oracle's S rounded once -- the input both the kernel and the oracle iterate on; s float64; r float64)"""
    (indptr, indices, values), _, _ = graph(name)
    s, r = LO.normalize(indptr, indices, values)
    return s.astype(np.float32), s, r


def labels(name, pattern):
    (csr, cls, Cn) = graph(name)
    N, rows = len(cls), np.arange(len(cls))
    if pattern == "none":
        y = np.full(N, -1)
    elif pattern == "all":
        y = cls.copy()
    elif pattern == "mixed":
        y = LO.islands()[1].copy() if name == "islands" else np.where(rows % 3 == 0, cls, -1)
    else:
        y = np.where(rows % 4 == 0, 0 if pattern == "class0" else Cn - 1, -1)
    return y.astype(np.int32)


@functools.lru_cache(maxsize=None)
def references(name, alpha):
    """{T: (F oracle [P][N][C], change oracle [P][T], F yardstick, change yardstick)} for T in STEPS and the P label patterns, computed
    once, all patterns in one pass over the graph; alpha as the float32 the entry receives"""
    (indptr, indices, _), _, Cn = graph(name)
    s32 = normalized(name)[0]
    ys, a = np.stack([labels(name, p) for p in PATTERNS]), float(np.float32(alpha))
    out, prev = {}, 0
    Fo = Fy = None
    co, cy = np.zeros((len(PATTERNS), 0)), np.zeros((len(PATTERNS), 0), dtype=np.float32)
    for T in STEPS:
        Fo, c1 = LO.iterate(indptr, indices, s32.astype(np.float64), ys, Cn, a, T - prev, Fo)
        Fy, c2 = LO.iterate_f32(indptr, indices, s32, ys, Cn, a, T - prev, Fy)
        co, cy, prev = np.concatenate([co, c1], axis=1), np.concatenate([cy, c2], axis=1), T
        out[T] = (Fo, co, Fy, cy)
    return out


def reference(name, pattern, alpha):
    """{T: (F oracle [N][C], change oracle [T], F yardstick, change yardstick)} of one pattern"""
    p = PATTERNS.index(pattern)
    return {T: tuple(v[p] for v in vals) for T, vals in references(name, alpha).items()}


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def raw_normalize(csr, expect_flag=0):
    """one dmvae_graph_sym_normalize call into sentinel-filled outputs: (s [nnz], r [N]) on the host"""
    from dmvae_hip import _lib
    indptr, indices, values = csr
    N, nnz = len(indptr) - 1, len(indices)
    s = torch.full((nnz + 3,), S_SENTINEL, dtype=torch.float32, device="cuda")
    r = torch.full((N + 3,), S_SENTINEL, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ip, ix, w = dev(indptr, torch.int64), dev(indices, torch.int32), dev(values, torch.float32)
    rc = _lib.lib.dmvae_graph_sym_normalize(stream(), ip.data_ptr(), ptr(ix), ptr(w), N, nnz, s.data_ptr(), r.data_ptr(), flag.data_ptr())
    assert rc == 0, _lib.lib.dmvae_last_error()
    sh, rh = s.cpu().numpy(), r.cpu().numpy()
    assert int(flag.item()) == expect_flag
    assert (sh[nnz:] == S_SENTINEL).all() and (rh[N:] == S_SENTINEL).all()
    return sh[:nnz], rh[:N]


class Spreader:
    """the device copies of one graph and the workspace, for many dmvae_label_spread calls"""

    def __init__(self, csr_s, Cn):
        from dmvae_hip import _lib
        self.lib = _lib.lib
        indptr, indices, s = csr_s
        self.N, self.nnz, self.C = len(indptr) - 1, len(indices), Cn
        self.ip, self.ix, self.s = dev(indptr, torch.int64), dev(indices, torch.int32), dev(s, torch.float32)
        self.nbytes = int(self.lib.dmvae_label_spread_ws_bytes(self.N, Cn))
        assert self.nbytes > 0
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def fresh(self, pad=3):
        return torch.full((self.N, self.C + pad), F_SENTINEL, dtype=torch.float32, device="cuda")

    def call(self, y, alpha, T, F_in=None, F=None, expect_flag=0, rc_only=False, ldf=None, ws_bytes=None):
        """-> (F [N][C], change [T]) on the host, after the untouched bits were checked; F_in / F: device buffers [N][C + 3] (F: a fresh one)"""
        F = self.fresh() if F is None else F
        before = F.cpu().numpy().copy()
        change = torch.full((T + 2,), CH_SENTINEL, dtype=torch.float32, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        yd = dev(y, torch.int32)
        rc = self.lib.dmvae_label_spread(stream(), self.ip.data_ptr(), ptr(self.ix), ptr(self.s), self.N, self.nnz, yd.data_ptr(), self.C, float(alpha),
                                         int(T), None if F_in is None else F_in.data_ptr(), 0 if F_in is None else F_in.stride(0), F.data_ptr(),
                                         F.stride(0) if ldf is None else ldf, change.data_ptr(), self.ws.data_ptr(),
                                         self.nbytes if ws_bytes is None else ws_bytes, flag.data_ptr())
        if rc_only:
            torch.cuda.synchronize()
            assert np.array_equal(bits(F.cpu().numpy()), bits(before))             # a refused call enqueues nothing
            return rc
        assert rc == 0, self.lib.dmvae_last_error()
        Fh, ch = F.cpu().numpy(), change.cpu().numpy()
        assert int(flag.item()) == expect_flag
        assert np.array_equal(bits(Fh[:, self.C:]), bits(before[:, self.C:]))      # the columns >= C keep their bits
        assert (ch[T:] == CH_SENTINEL).all()                                       # nothing past n_iter entries
        return Fh[:, :self.C].copy(), ch[:T].copy()


@functools.lru_cache(maxsize=None)
def spreader(name):
    (indptr, indices, _), _, Cn = graph(name)
    return Spreader((indptr, indices, normalized(name)[0]), Cn)


# ------------------------------------------------------------------------------------------------------------------ the normalisation
@pytest.mark.parametrize("name", GRAPHS)
def test_normalize_against_the_oracle(name):
    csr, _, _ = graph(name)
    _, s64, r64 = normalized(name)
    s, r = raw_normalize(csr)
    assert np.all(np.abs(r - r64) <= U * r64) and np.array_equal(r == 0, r64 == 0)          # one rounding; exactly 0 without edges
    assert np.all(np.abs(s - s64) <= 4 * U * s64)
    if name == "islands":
        assert r[11] == 0.0 and r[12] == 0.0
    if name == "blobs-N1":
        assert len(s) == 0 and r[0] == 0.0


def without(indptr, keep):
    """the row pointers of the CSR that keeps the entries `keep` (bool [nnz])"""
    return indptr - np.concatenate([[0], np.cumsum(~keep)])[indptr]


def test_normalize_skips_an_index_out_of_range():
    (indptr, indices, values), _, _ = graph("blobs-N65")
    bad = [int(indptr[5]) + 1, int(indptr[40])]
    broken = indices.copy()
    broken[bad[0]], broken[bad[1]] = 65, -1
    s, r = raw_normalize((indptr, broken, values), expect_flag=1)
    keep = np.ones(len(indices), dtype=bool)
    keep[bad] = False
    s0, r0 = raw_normalize((without(indptr, keep), indices[keep], values[keep]))
    assert np.array_equal(bits(r), bits(r0)) and np.array_equal(bits(s[keep]), bits(s0)) and np.all(s[bad] == 0.0)


# ------------------------------------------------------------------------------------------------------------------ the iteration
@pytest.mark.parametrize("name", GRAPHS)
def test_spread_against_the_oracle_running_the_same_iterations(name):
    sp = spreader(name)
    worst = {}
    for pattern in PATTERNS:
        y = labels(name, pattern)
        for alpha in ALPHAS:
            ref = reference(name, pattern, alpha)
            for T in STEPS:
                Fo, co, Fy, cy = ref[T]
                F, ch = sp.call(y, alpha, T)
                ok, err, yard = MC.within("pred", F, Fo, Fy)
                okc, errc, yardc = MC.within("pred", ch, co, cy)
                worst[(pattern, alpha, T)] = (err, yard, errc, yardc)
                assert ok and okc, (name, pattern, alpha, T, err, yard, errc, yardc)
                if pattern == "none":
                    assert not F.any() and not ch.any() and np.array_equal(LO.predict(F), np.full(sp.N, -1))
    print(name, "max |F - oracle| %.3g (yardstick %.3g), max |change - oracle| %.3g (yardstick %.3g)"
          % tuple(max(v[i] for v in worst.values()) for i in range(4)))


@pytest.mark.parametrize("name", BLOBS)
def test_argmax_is_the_oracles_on_every_row(name):
    """mixed labels (every third row), alpha = 0.8, 57 iterations: every row is reached, the oracle's top-two gap exceeds four times the
    yardstick's error in EVERY row -- an unclear row fails the test -- and the kernel's arg-max is the oracle's"""
    sp = spreader(name)
    Fo, _, Fy, _ = reference(name, "mixed", 0.8)[57]
    F, _ = sp.call(labels(name, "mixed"), 0.8, 57)
    want = LO.predict(Fo)
    print(name, "smallest top-two gap %.3g, yardstick error %.3g" % (MC.top_two_gap(Fo).min(), MC.yard_error(Fo, Fy)))
    assert np.all(want >= 0)
    assert np.all(MC.clear_rows(Fo, Fy))
    assert np.array_equal(LO.predict(F), want)


@pytest.mark.parametrize("name", ["islands", "star300"])
def test_unreached_rows_stay_zero(name):
    sp = spreader(name)
    y = labels(name, "mixed")
    F, _ = sp.call(y, 0.8, 57)
    want = LO.predict(reference(name, "mixed", 0.8)[57][0])
    assert np.array_equal(LO.predict(F), want)
    if name == "islands":
        assert not F[6:12].any() and np.array_equal(want[6:12], np.full(6, -1)) and want[12] == 1 and np.all(want[:6] >= 0)


# ------------------------------------------------------------------------------------------------------------------ determinism and chunking
@pytest.mark.parametrize("name", ["blobs-N257", "star300", "blobs-C257", "blobs-5000"])
def test_two_runs_and_chunked_runs_give_the_same_bits(name):
    sp = spreader(name)
    y = labels(name, "mixed")
    F16, c16 = sp.call(y, 0.8, 16)
    again, cagain = sp.call(y, 0.8, 16)
    assert np.array_equal(bits(F16), bits(again)) and np.array_equal(bits(c16), bits(cagain))
    first = sp.fresh()
    _, c8a = sp.call(y, 0.8, 8, F=first)
    F8b, c8b = sp.call(y, 0.8, 8, F_in=first)                                      # into another buffer
    assert np.array_equal(bits(F8b), bits(F16)) and np.array_equal(bits(np.concatenate([c8a, c8b])), bits(c16))
    F8c, c8c = sp.call(y, 0.8, 8, F_in=first, F=first)                             # in place
    assert np.array_equal(bits(F8c), bits(F16)) and np.array_equal(bits(c8c), bits(c8b))
    zeros = torch.zeros((sp.N, sp.C + 3), dtype=torch.float32, device="cuda")
    Fz, cz = sp.call(y, 0.8, 16, F_in=zeros)
    assert np.array_equal(bits(Fz), bits(F16)) and np.array_equal(bits(cz), bits(c16))
    # one iteration in place (the launch may not write the rows others still read), and a 16-byte-aligned F_in with ld = a multiple of 4
    F9, c9 = sp.call(y, 0.8, 9)
    buf = sp.fresh()
    sp.call(y, 0.8, 8, F=buf)
    F1, c1 = sp.call(y, 0.8, 1, F_in=buf, F=buf)
    assert np.array_equal(bits(F1), bits(F9)) and bits(c1)[0] == bits(c9)[8]
    pad = (-sp.C) % 4 or 4
    wide = sp.fresh(pad)
    sp.call(y, 0.8, 8, F=wide)
    assert wide.stride(0) % 4 == 0 and wide.data_ptr() % 16 == 0
    Fw, cw = sp.call(y, 0.8, 8, F_in=wide)
    assert np.array_equal(bits(Fw), bits(F16)) and np.array_equal(bits(cw), bits(c8b))


# ------------------------------------------------------------------------------------------------------------------ labels, indices, refusals
def test_a_label_out_of_range_sets_bit_1_and_counts_as_unlabelled():
    name = "blobs-N65"
    sp = spreader(name)
    y = labels(name, "mixed")
    broken = y.copy()
    assert y[1] == -1 and y[2] == -1
    broken[1], broken[2] = sp.C, -2
    F, ch = sp.call(broken, 0.8, 8, expect_flag=2)
    F0, ch0 = sp.call(y, 0.8, 8)
    assert np.array_equal(bits(F), bits(F0)) and np.array_equal(bits(ch), bits(ch0))


def test_spread_skips_an_index_out_of_range():
    name = "blobs-N65"
    (indptr, indices, _), _, Cn = graph(name)
    s32 = normalized(name)[0]
    bad = [int(indptr[5]) + 1, int(indptr[40])]
    broken = indices.copy()
    broken[bad[0]], broken[bad[1]] = 65, -1
    keep = np.ones(len(indices), dtype=bool)
    keep[bad] = False
    y = labels(name, "mixed")
    F, ch = Spreader((indptr, broken, s32), Cn).call(y, 0.8, 8, expect_flag=1)
    F0, ch0 = Spreader((without(indptr, keep), indices[keep], s32[keep]), Cn).call(y, 0.8, 8)
    assert np.array_equal(bits(F), bits(F0)) and np.array_equal(bits(ch), bits(ch0))


def test_arguments_outside_the_domain_are_refused():
    from dmvae_hip import _lib
    sp = spreader("blobs-N65")
    y = labels("blobs-N65", "mixed")
    assert sp.call(y, 0.0, 8, rc_only=True) == EINVAL and sp.call(y, 1.0, 8, rc_only=True) == EINVAL
    assert sp.call(y, 0.8, 0, rc_only=True) == EINVAL
    assert sp.call(y, 0.8, 8, ldf=sp.C - 1, rc_only=True) == EINVAL
    assert sp.call(y, 0.8, 8, ws_bytes=sp.nbytes - 1, rc_only=True) == EINVAL
    assert b"dmvae_label_spread" in _lib.lib.dmvae_last_error()
    for N, Cn in ((0, 10), (2 ** 20 + 1, 10), (65, 1), (65, 1025)):
        assert _lib.lib.dmvae_label_spread_ws_bytes(N, Cn) == EINVAL
    assert _lib.lib.dmvae_label_spread_ws_bytes(2 ** 20, 1024) > 0
