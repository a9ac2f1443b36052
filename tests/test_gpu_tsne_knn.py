"""GPU tests of the kNN-sparse t-SNE on the device (csrc/tsne_knn.hip behind dmvae_hip.tsne) against the float64 oracle of
tests/helpers/tsne_knn_oracle.py, which tests/test_tsne_knn_host.py holds to sklearn's _joint_probabilities_nn, to the dense oracle and to
a finite difference of its KL.

The oracle is always evaluated on the neighbour lists the DEVICE returned: dmvae_knn has its own tests (tests/test_gpu_knn.py), and a
near-tie at the k-th place, which f32 and f64 distances may order differently, must not decide these.

Bars, those of tests/test_gpu_tsne.py.  Joint P: 3e-5 * max P absolute and 1e-3 relative above 1e-9, the row entropies at the device's
beta within 1e-4 of log(perplexity), |sum P - 1| <= 1e-5.  Gradient: 1e-4 of the largest oracle value.  KL of a short fit: 1e-5 relative
to the oracle's KL of the device's own P and Y.  The whole run: 5 % of the float64 oracle's KL from the same start (the float64
restatement's f32-state run differs from its f64 run by 1.9 % at this shape)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import tsne_oracle as T         # noqa: E402
import tsne_knn_oracle as K     # noqa: E402

pytestmark = pytest.mark.gpu

# (N, D, perplexity, ldx, rows made identical).  65: k = N - 1 = 64, one slot per lane; 257 / perplexity 5: k = 16, a quarter of the lanes
# idle; 261 and 1030: k = 91, two slots per lane and a ragged second one; 1030 has a fullest row of some 300 entries (five trips of
# the attraction's wave) and is past one 1024-column tile by six columns.  ldx 13: a row-strided X.  Eight identical rows: d2 = 0 ties.
CASES = [(65, 2, 30.0, 2, None), (257, 10, 5.0, 10, None), (261, 10, 30.0, 10, None), (1030, 64, 30.0, 64, None), (261, 10, 30.0, 13, None),
         (261, 10, 30.0, 10, (3, 40, 41, 77, 120, 200, 201, 260))]


def device_joint_p(N, D, perplexity, ldx=None, same=None, **kw):
    from dmvae_hip import tsne
    X, lab = T.blobs(N, D)
    if same is not None:
        X[list(same[1:])] = X[same[0]]
    ldx = D if ldx is None else ldx
    buf = torch.full((N, ldx), 1e30, dtype=torch.float32, device="cuda")        # what lies between the rows must not be read
    buf[:, :D] = torch.as_tensor(X)
    Xd = buf[:, :D]
    cfg = tsne.knn_config(N, perplexity=perplexity, **kw)
    P = tsne.knn_joint_p(Xd, cfg)
    torch.cuda.synchronize()
    return dict(X=X, lab=lab, Xd=Xd, cfg=cfg, P=P)


def oracle_csr_of(P, perplexity):
    """the oracle's conditional p and CSR on the device's lists (its f32 squared distances, read as f64)"""
    p, beta = K.conditional_p(P.d2.cpu().numpy().astype(np.float64), perplexity)
    return K.joint_csr(P.idx.cpu().numpy(), p), p, beta


def dense64(P):
    return K.dense(P.indptr.cpu().numpy(), P.indices.cpu().numpy(), P.values.cpu().numpy())


@pytest.fixture(scope="module")
def run240():
    r = device_joint_p(240, 10, 30.0)
    r["P64"] = dense64(r["P"])
    return r


@pytest.fixture(scope="module")
def run1030():
    r = device_joint_p(1030, 64, 30.0)
    r["P64"] = dense64(r["P"])
    return r


@pytest.mark.parametrize("N,D,perplexity,ldx,same", CASES)
def test_joint_p_against_the_oracle(N, D, perplexity, ldx, same):
    from dmvae_hip import tsne
    r = device_joint_p(N, D, perplexity, ldx, same)
    P, k = r["P"], r["cfg"].k
    assert k == K.n_neighbors(N, perplexity) == tsne.n_neighbors(N, perplexity) and tuple(P.idx.shape) == (N, k)
    assert P.indptr.dtype == torch.int64 and P.indices.dtype == torch.int32 and P.values.dtype == torch.float32 and r["cfg"].nnz == P.nnz
    (indptr, indices, want), _, _ = oracle_csr_of(P, perplexity)
    assert np.array_equal(P.indptr.cpu().numpy(), indptr) and np.array_equal(P.indices.cpu().numpy(), indices)
    got = P.values.cpu().numpy()
    worst_abs = np.abs(got - want).max() / want.max()
    big = want > 1e-9
    worst_rel = (np.abs(got - want)[big] / want[big]).max()
    H = K.entropy(P.d2.cpu().numpy().astype(np.float64), P.beta.cpu().numpy().astype(np.float64))
    worst_H = np.abs(H - np.log(perplexity)).max()
    total = got.astype(np.float64).sum()
    rows = np.diff(indptr)
    print("N=%d D=%d k=%d: %.3g of max P, %.3g relative, entropy off by %.3g, sum P - 1 = %.3g; %.1f entries per row, %d on the fullest" % (
        N, D, k, worst_abs, worst_rel, worst_H, total - 1.0, rows.mean(), rows.max()))
    assert np.isfinite(got).all() and abs(total - 1.0) <= 1e-5
    assert worst_abs <= 3e-5 and worst_rel <= 1e-3
    assert worst_H <= 1e-4
    Pd = P.dense().cpu().numpy()
    assert np.array_equal(Pd.view(np.uint32), Pd.T.view(np.uint32)) and (np.diag(Pd) == 0).all()        # P_ij == P_ji in bits
    if N == 65:
        assert (rows == 64).all()
    if N == 1030:
        assert rows.max() > 256                                                                          # more than four trips of a wave
    if same is not None:
        d2 = P.d2.cpu().numpy()
        assert (d2[list(same), :7] == 0).all() and np.isfinite(P.beta.cpu().numpy()).all()
        # ties go to the lower row: the seven other copies, ascending
        assert np.array_equal(P.idx.cpu().numpy()[same[0], :7], np.array(same[1:]))


@pytest.mark.parametrize("splits", [0, 1, 2, 5])
@pytest.mark.parametrize("scale", [1e-4, 10.0])
@pytest.mark.parametrize("e", [12.0, 1.0])
@pytest.mark.parametrize("N", [240, 1030])
def test_gradient_against_the_oracle(run240, run1030, N, scale, e, splits):
    """col_splits 2 and 5 at N = 1030: two column tiles (1024 + 6) dealt to more splits than tiles, so some are empty, and five row
    blocks of 256 of which the last holds six rows"""
    from dmvae_hip import tsne
    r = run240 if N == 240 else run1030
    cfg = tsne.knn_config(N, perplexity=30.0, col_splits=splits, nnz=r["P"].nnz)
    ws = tsne.knn_workspace(cfg, "cuda")
    Y = (scale * np.random.RandomState(5).randn(N, 2)).astype(np.float32)
    g = tsne.knn_gradient(cfg, r["P"], ws, torch.as_tensor(Y).cuda(), e).cpu().numpy()
    want = T.gradient(r["P64"], Y.astype(np.float64), e)
    worst = np.abs(g - want).max() / np.abs(want).max()
    print("N %d scale %g e %g splits %d: %.3g of max |g|" % (N, scale, e, splits, worst))
    assert np.isfinite(g).all() and worst <= 1e-4


def test_fit_is_the_steps(run240):
    from dmvae_hip import tsne
    X, P = run240["Xd"], run240["P"]
    cfg = tsne.knn_config(240, perplexity=30.0, n_iter=7, exaggeration_iters=3)
    Y0 = torch.as_tensor((1e-4 * np.random.RandomState(8).randn(240, 2)).astype(np.float32)).cuda()
    ws = tsne.knn_workspace(cfg, X.device)
    Y, kl = tsne.knn_fit(X, cfg, ws, Y0)                      # builds its own P
    torch.cuda.synchronize()
    assert cfg.nnz == P.nnz
    ws2 = tsne.knn_workspace(cfg, X.device)
    P2 = tsne.knn_joint_p(X, cfg)
    assert torch.equal(P2.indptr, P.indptr) and torch.equal(P2.indices, P.indices) and torch.equal(P2.values, P.values)
    Ys, U, G = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
    for it in range(7):
        tsne.knn_step(cfg, P2, ws2, Ys, U, G, 12.0 if it < 3 else 1.0, 0.5 if it < 3 else 0.8)
    torch.cuda.synchronize()
    assert torch.equal(Y, Ys) and not torch.equal(Y, Y0)
    want = T.kl(run240["P64"], Y.cpu().numpy().astype(np.float64))
    print("KL %.9g oracle %.9g" % (kl.item(), want))
    assert abs(kl.item() - want) <= 1e-5 * abs(want)


def test_whole_run(run240):
    from dmvae_hip import TSNE
    X, lab = run240["X"], run240["lab"]
    a = TSNE(method="knn")
    Y = a.fit_transform(X)
    assert Y.shape == (240, 2) and Y.dtype == np.float32 and a.n_iter_ == 1000 and a.learning_rate_ == 50.0
    assert a.n_neighbors_ == 91 and a.nnz_ == run240["P"].nnz
    d = ((Y[:, None, :].astype(np.float64) - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    assert (lab[d.argmin(1)] == lab).all()
    from dmvae_hip import tsne
    cfg0 = tsne.knn_config(240, n_iter=0)
    Y0, _ = tsne.knn_fit(run240["Xd"], cfg0, tsne.knn_workspace(cfg0, "cuda"), None, run240["P"])        # the Philox start of random_state 0
    _, want = T.fit(run240["P64"], Y0.cpu().numpy().astype(np.float64))
    print("KL %.6g float64 oracle %.6g" % (a.kl_divergence_, want))
    assert abs(a.kl_divergence_ - want) <= 0.05 * want
    b = TSNE(method="knn").fit(X)
    assert np.array_equal(b.embedding_, Y) and b.kl_divergence_ == a.kl_divergence_


def _kl64_chunked(P, Y, chunk=4096):
    """float64 torch composition on the device: Z over all pairs in row chunks, then the CSR sum"""
    N = Y.shape[0]
    Yd = Y.double()
    Z = torch.zeros((), dtype=torch.float64, device=Y.device)
    for s in range(0, N, chunk):
        q = 1.0 / (1.0 + torch.cdist(Yd[s:s + chunk], Yd) ** 2)
        Z += q.sum() - q[torch.arange(q.shape[0]), torch.arange(s, s + q.shape[0])].sum()
    rows = torch.repeat_interleave(torch.arange(N, device=Y.device), P.indptr[1:] - P.indptr[:-1])
    d2 = ((Yd[rows] - Yd[P.indices.long()]) ** 2).sum(1)
    v = P.values.double()
    m = v > 0
    return float((v[m] * torch.log(v[m] * Z * (1.0 + d2[m]))).sum().item())


def test_beyond_the_dense_cap():
    from dmvae_hip import TSNE, tsne
    X = torch.as_tensor(T.blobs(40000, 10)[0]).cuda()
    with pytest.raises(Exception, match="32768") as err:
        TSNE(n_iter=20).fit(X)
    assert 'method="knn"' in str(err.value)
    a = TSNE(n_iter=20, method="knn").fit(X)
    assert np.isfinite(a.embedding_).all() and a.n_neighbors_ == 91 and a.nnz_ >= 40000 * 91
    cfg = tsne.knn_config(40000, n_iter=20)
    P = tsne.knn_joint_p(X, cfg)
    assert P.nnz == a.nnz_
    want = _kl64_chunked(P, a.embedding_device_)
    print("KL %.9g float64 composition %.9g; nnz %d" % (a.kl_divergence_, want, P.nnz))
    assert abs(a.kl_divergence_ - want) <= 1e-5 * abs(want)
    b = TSNE(n_iter=20, method="knn").fit(X)
    assert np.array_equal(b.embedding_, a.embedding_) and b.kl_divergence_ == a.kl_divergence_


def test_limits_fail_loudly(run240):
    from dmvae_hip import tsne
    from dmvae_hip._lib import lib
    P = run240["P"]
    good = tsne.knn_config(240, nnz=P.nnz)
    ws = tsne.knn_workspace(good, "cuda")
    ws.fill_(0x5A)
    Y = torch.full((240, 2), 7.0, device="cuda")
    kl = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fit(cfg, nbytes=None, indptr=P.indptr.data_ptr(), y=Y.data_ptr()):
        return lib.dmvae_tsne_knn_fit(s, C.byref(cfg), indptr, P.indices.data_ptr(), P.values.data_ptr(), None, ws.data_ptr(),
                                      ws.numel() if nbytes is None else nbytes, y, kl.data_ptr())

    for kw, word in ((dict(cfg=tsne.knn_config(300, perplexity=90.0)), b"256"), (dict(cfg=good, nbytes=ws.numel() - 1), b"workspace"),
                     (dict(cfg=good, indptr=None), b"indptr"), (dict(cfg=good, y=None), b"Y"),
                     (dict(cfg=tsne.knn_config(240, col_splits=-1, nnz=P.nnz)), b"col_splits")):
        assert fit(**kw) == -1
        assert word in lib.dmvae_last_error(), lib.dmvae_last_error()
    bad = tsne.knn_config(300, perplexity=90.0)                 # k = min(299, 271) = 271; at 240 rows k = 239 would pass
    assert bad.k == 271
    assert fit(bad) == -1 and b"perplexity above 85" in lib.dmvae_last_error()
    p = torch.full((240, 91), 7.0, device="cuda")
    assert lib.dmvae_tsne_knn_cond_p(s, C.byref(bad), P.d2.data_ptr(), 91, p.data_ptr(), 91, None) == -1
    assert lib.dmvae_tsne_knn_cond_p(s, C.byref(good), None, 91, p.data_ptr(), 91, None) == -1
    assert lib.dmvae_tsne_knn_ws_bytes(C.byref(bad)) == -1
    torch.cuda.synchronize()
    assert (ws == 0x5A).all() and (Y == 7.0).all() and kl.item() == 7.0 and (p == 7.0).all()           # nothing was enqueued
    with pytest.raises(Exception, match="256"):
        tsne.TSNE(perplexity=90.0, method="knn").fit(T.blobs(300, 4)[0])
