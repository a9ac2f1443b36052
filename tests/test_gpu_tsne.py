"""GPU tests of the exact t-SNE on the device (csrc/tsne.hip behind dmvae_hip.tsne) against the float64 oracle of
tests/helpers/tsne_oracle.py, which tests/test_tsne_host.py holds to sklearn's joint probabilities and to a finite difference of its KL.

Bars.  Joint P: 3e-5 * max P absolute and 1e-3 relative above 1e-9 -- the bars the oracle itself is held to against sklearn.  Gradient and
step: 1e-4 of the largest oracle value, the project's fp32 gradient bar (tests/test_gpu_moe.py).  KL of a short fit: 1e-5 relative to the
oracle's KL of the device's own P and Y (f64 terms on both sides).  The whole run: 5 % of the float64 oracle's KL from the same start --
long trajectories are chaotic: f32 and f64 runs of the oracle from one start differ by 1.1 - 1.7 % over four seeds.

The Philox start: Y equals float32(1e-4) * dmvae_philox_normal's stream (seed, step 0, stream id 5) bit for bit, and that stream is the
oracle's (tests/helpers/philox_oracle.py) to atol 1e-3 per normal -- the device's Box-Muller goes through __logf / __sinf / __cosf, which is
the bar tests/test_gpu_philox.py holds every normal of the project to; the words under it are exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import philox_oracle as PH      # noqa: E402
import tsne_oracle as T         # noqa: E402

pytestmark = pytest.mark.gpu

# (N, D, perplexity, ldx, rows made identical).  A wave takes a row 256 elements (64 float4) per trip: 261 and 1030 are just past one and
# four trips, with odd N every row starts at another alignment; 1030 is also past the 256-column / 16-row distance tiles and the 64 x 64
# tiles of the symmetrisation by a few.
CASES = [(240, 10, 30.0, 10, None), (97, 3, 5.0, 3, None), (333, 64, 50.0, 64, None), (65, 2, 20.0, 2, None), (1030, 7, 30.0, 7, None),
         (261, 4, 10.0, 4, None), (130, 6, 12.0, 9, None), (100, 5, 10.0, 5, (3, 7))]


def device_joint_p(N, D, perplexity, ldx=None, same=None, **kw):
    from dmvae_hip import tsne
    X, lab = T.blobs(N, D)
    if same is not None:
        X[same[1]] = X[same[0]]
    ldx = D if ldx is None else ldx
    buf = torch.full((N, ldx), 1e30, dtype=torch.float32, device="cuda")        # what lies between the rows must not be read
    buf[:, :D] = torch.as_tensor(X)
    Xd = buf[:, :D]
    cfg = tsne.config(N, D, perplexity=perplexity, **kw)
    ws = tsne.workspace(cfg, Xd.device)
    P, beta = tsne.joint_p(Xd, cfg, ws)
    torch.cuda.synchronize()
    return dict(X=X, lab=lab, Xd=Xd, cfg=cfg, ws=ws, P=P, beta=beta.cpu().numpy())


@pytest.fixture(scope="module")
def run240():
    r = device_joint_p(240, 10, 30.0)
    r["P64"] = r["P"].cpu().numpy().astype(np.float64)
    return r


@pytest.mark.parametrize("N,D,perplexity,ldx,same", CASES)
def test_joint_p_against_the_oracle(N, D, perplexity, ldx, same):
    r = device_joint_p(N, D, perplexity, ldx, same)
    P = r["P"].cpu().numpy()
    d2 = T.sq_distances(r["X"])
    want = T.joint_p(d2, perplexity)
    worst_abs = np.abs(P - want).max() / want.max()
    big = want > 1e-9
    worst_rel = (np.abs(P - want)[big] / want[big]).max()
    H = T.entropy(d2, r["beta"].astype(np.float64))
    worst_H = np.abs(H - np.log(perplexity)).max()
    print("N=%d D=%d: %.3g of max P, %.3g relative, entropy off by %.3g, sum P - 1 = %.3g" % (N, D, worst_abs, worst_rel, worst_H,
                                                                                          P.astype(np.float64).sum() - 1.0))
    assert np.isfinite(P).all() and np.array_equal(P, P.T) and (np.diag(P) == 0).all()
    assert abs(P.astype(np.float64).sum() - 1.0) <= 1e-5
    assert worst_abs <= 3e-5 and worst_rel <= 1e-3
    assert worst_H <= 1e-4
    if same is not None:
        assert P[same[0], same[1]] > 0 and np.isfinite(r["beta"]).all()


def _Y(scale, seed=5):
    return (scale * np.random.RandomState(seed).randn(240, 2)).astype(np.float32)


@pytest.mark.parametrize("scale", [1e-4, 10.0])
@pytest.mark.parametrize("e", [12.0, 1.0])
def test_gradient_against_the_oracle(run240, scale, e):
    from dmvae_hip import tsne
    Y = _Y(scale)
    g = tsne.gradient(run240["cfg"], run240["ws"], torch.as_tensor(Y).cuda(), e).cpu().numpy()
    want = T.gradient(run240["P64"], Y.astype(np.float64), e)
    worst = np.abs(g - want).max() / np.abs(want).max()
    print("scale %g e %g: %.3g of max |g|" % (scale, e, worst))
    assert worst <= 1e-4


@pytest.mark.parametrize("scale", [1e-4, 10.0])
@pytest.mark.parametrize("e,m", [(12.0, 0.5), (1.0, 0.8)])
def test_one_step_against_the_oracle(run240, scale, e, m):
    from dmvae_hip import tsne
    rs = np.random.RandomState(6)
    Y = _Y(scale)
    U = (0.1 * scale * rs.randn(240, 2)).astype(np.float32)
    G = rs.uniform(0.01, 2.0, (240, 2)).astype(np.float32)
    assert (U != 0).all()
    lr = float(run240["cfg"].learning_rate)
    assert lr == 50.0
    Yd, Ud, Gd = (torch.as_tensor(a).cuda() for a in (Y, U, G))
    tsne.step(run240["cfg"], run240["ws"], Yd, Ud, Gd, e, m)
    torch.cuda.synchronize()
    Y1, U1, G1, g = T.step(run240["P64"], Y.astype(np.float64), U.astype(np.float64), G.astype(np.float64), e, m, lr)
    assert np.abs(Yd.cpu().numpy() - Y1).max() <= 1e-4 * np.abs(Y1).max()
    assert np.abs(Ud.cpu().numpy() - U1).max() <= 1e-4 * np.abs(U1).max()
    # the gains: the rule in f32 arithmetic on the oracle's sign decisions, exact; gradients too small to carry a sign are left out
    inc = U.astype(np.float64) * g < 0
    G32 = np.maximum(np.where(inc, G + np.float32(0.2), G * np.float32(0.8)), np.float32(0.01)).astype(np.float32)
    np.testing.assert_allclose(G32, G1, rtol=1e-6)
    keep = np.abs(g) >= 1e-4 * np.abs(g).max()
    assert (~keep).sum() <= 0.01 * keep.size
    assert np.array_equal(Gd.cpu().numpy()[keep], G32[keep])


def test_fit_is_the_steps(run240):
    from dmvae_hip import tsne
    X = run240["Xd"]
    cfg = tsne.config(240, 10, perplexity=30.0, n_iter=7, exaggeration_iters=3)
    Y0 = torch.as_tensor(_Y(1e-4, seed=8)).cuda()
    ws = tsne.workspace(cfg, X.device)
    Y, kl = tsne.fit(X, cfg, ws, Y0)
    torch.cuda.synchronize()
    assert torch.equal(ws[:240 * 240 * 4].view(torch.float32).reshape(240, 240), run240["P"])
    ws2 = tsne.workspace(cfg, X.device)
    tsne.joint_p(X, cfg, ws2)
    Ys, U, G = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
    for it in range(7):
        tsne.step(cfg, ws2, Ys, U, G, 12.0 if it < 3 else 1.0, 0.5 if it < 3 else 0.8)
    torch.cuda.synchronize()
    assert torch.equal(Y, Ys) and not torch.equal(Y, Y0)
    want = T.kl(run240["P64"], Y.cpu().numpy().astype(np.float64))
    print("KL %.9g oracle %.9g" % (kl.item(), want))
    assert abs(kl.item() - want) <= 1e-5 * abs(want)


def test_whole_run(run240):
    from dmvae_hip import TSNE
    X, lab = run240["X"], run240["lab"]
    Y0 = (1e-4 * np.random.RandomState(0).randn(240, 2)).astype(np.float32)
    a = TSNE(init=Y0)
    Y = a.fit_transform(X)
    assert Y.shape == (240, 2) and Y.dtype == np.float32 and a.n_iter_ == 1000 and a.learning_rate_ == 50.0
    d = ((Y[:, None, :].astype(np.float64) - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    assert (lab[d.argmin(1)] == lab).all()
    _, want = T.fit(T.joint_p(T.sq_distances(X), 30.0), Y0.astype(np.float64))
    print("KL %.6g float64 oracle %.6g" % (a.kl_divergence_, want))
    assert abs(a.kl_divergence_ - want) <= 0.05 * want
    b = TSNE(init=Y0).fit(X)
    assert np.array_equal(b.embedding_, Y) and b.kl_divergence_ == a.kl_divergence_


def test_philox_start(run240):
    from dmvae_hip import tsne
    from dmvae_hip._lib import lib, check
    X, seed, n = run240["Xd"], 1234567, 480
    cfg = tsne.config(240, 10, n_iter=0, seed=seed)
    Y, kl = tsne.fit(X, cfg, tsne.workspace(cfg, X.device), None)
    normals = torch.empty(n, dtype=torch.float32, device="cuda")
    check(lib.dmvae_philox_normal(C.c_void_p(torch.cuda.current_stream().cuda_stream), normals.data_ptr(), n, seed, 0, 5), "dmvae_philox_normal")
    torch.cuda.synchronize()
    got = Y.cpu().numpy().reshape(-1)
    assert np.array_equal(got, np.float32(1e-4) * normals.cpu().numpy())
    np.testing.assert_allclose(got, 1e-4 * PH.normal_at(seed, 0, 5, np.arange(n, dtype=np.uint64)), rtol=0, atol=1e-4 * 1e-3)
    assert np.isfinite(kl.item()) and abs(kl.item() - T.kl(run240["P64"], got.reshape(240, 2).astype(np.float64))) <= 1e-5 * abs(kl.item())
    other = tsne.config(240, 10, n_iter=0, seed=seed + 1)
    Y2, _ = tsne.fit(X, other, tsne.workspace(other, X.device), None)
    assert not torch.equal(Y, Y2)


def test_class_surface(run240, tmp_path, monkeypatch):
    from dmvae_hip import TSNE
    X = run240["X"]
    a = TSNE(n_iter=60, random_state=3).fit_transform(torch.as_tensor(X).cuda())
    b = TSNE(n_iter=60, random_state=3)
    assert np.array_equal(a, b.fit_transform(X)) and np.isfinite(a).all() and b.kl_divergence_ > 0
    assert not np.array_equal(a, TSNE(n_iter=60, random_state=4).fit_transform(X))
    big = TSNE(n_iter=2).fit(T.blobs(2500, 5)[0])
    assert big.learning_rate_ == np.float32(2500 / 48.0) and big.embedding_device_.is_cuda

    import base_models
    from includes import visualization as V
    monkeypatch.chdir(tmp_path)
    m = base_models.DeepMixtureVAE("tsne_plot", "binary", 196, 5, 3, activation="relu", initializer="xavier", batch_size=16, dtype="fp32", noise="host",
                                   seed=3, enc_layers=(70, 50), head_dim=90, dec_layers=(90, 50, 30)).build_graph()
    fig = V.mnist_sample_plot(m, None, tsne=True, tsne_backend="device")
    blob = open(str(tmp_path / "plots" / "tsne_plot" / "mnist" / "sampled.png"), "rb").read()
    import struct
    import zlib
    w, h, depth, ctype = struct.unpack(">IIBB", blob[16:26])
    assert (h, depth, ctype) == (fig.shape[0], 8, 2) and w == fig.shape[1] + 14 + h
    pos, idat = 8, b""
    while pos < len(blob):
        n, tag = struct.unpack(">I", blob[pos:pos + 4])[0], blob[pos + 4:pos + 8]
        if tag == b"IDAT":
            idat += blob[pos + 8:pos + 8 + n]
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3)
    panel = rows[:, fig.shape[1] + 14:]
    seen = {tuple(c) for c in panel.reshape(-1, 3).tolist()}
    assert seen - {(255, 255, 255)} and seen <= {(255, 255, 255)} | {tuple(c) for c in V._COLORS[:3].astype(int).tolist()}      # dots, in the clusters' colours


def test_limits_fail_loudly():
    from dmvae_hip import tsne
    from dmvae_hip._lib import lib
    X = torch.as_tensor(T.blobs(64, 4)[0]).cuda()
    good = tsne.config(64, 4, perplexity=10.0)
    ws = tsne.workspace(good, X.device)
    ws.fill_(0x5A)
    Y = torch.full((64, 2), 7.0, device="cuda")
    kl = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fit(cfg, nbytes=None, n_rows=64):
        return lib.dmvae_tsne_fit(s, C.byref(cfg), X.data_ptr(), 4, None, ws.data_ptr(), ws.numel() if nbytes is None else nbytes, Y.data_ptr(),
                                  kl.data_ptr())

    for cfg, nbytes, code, word in ((tsne.config(64, 4, perplexity=63.0), None, -1, b"perplexity"), (tsne.config(64, 4, perplexity=70.0), None, -1, b"perplexity"),
                                    (tsne.config(3, 4, perplexity=1.5), None, -1, b"N >= 4"), (good, ws.numel() - 1, -1, b"workspace"),
                                    (tsne.config(32769, 4), None, -2, b"32768")):
        assert fit(cfg, nbytes) == code
        assert word in lib.dmvae_last_error(), lib.dmvae_last_error()
        assert lib.dmvae_tsne_joint_p(s, C.byref(cfg), X.data_ptr(), 4, ws.data_ptr(), ws.numel() if nbytes is None else nbytes, None) == code
    assert lib.dmvae_tsne_ws_bytes(C.byref(tsne.config(32769, 4))) == -2 and lib.dmvae_tsne_ws_bytes(C.byref(tsne.config(32768, 4))) >= 4 * 32768 ** 2
    torch.cuda.synchronize()
    assert (ws == 0x5A).all() and (Y == 7.0).all() and kl.item() == 7.0           # nothing was enqueued
    with pytest.raises(Exception, match="perplexity"):
        tsne.TSNE(perplexity=63.0).fit(X)
