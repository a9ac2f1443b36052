"""GPU tests of the clustering evaluation kernels (csrc/eval_clusters.hip) through the C ABI: dmvae_confusion_add exactly
against np.argmax + np.add.at, and dmvae_plan_eval_clusters on VaDE plans against the float64 oracle (fed noise) and against
itself (Philox noise fed back).  Counts are integers: no tolerance.  The averaged responsibilities are held to the bar of the
engine's own `weights` view on an fp32 VaDE plan (tests/test_gpu_vade.py: atol 2e-5); the arg-max may differ from the
oracle's only where the oracle's two largest entries are closer than 10 x that bar."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dmvae_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import philox_oracle as PH      # noqa: E402

W_ATOL = 2e-5             # tests/test_gpu_vade.py:131
GAP = 10 * W_ATOL


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def confusion(clusters, classes, R):
    d = np.zeros((R, R), dtype=np.int64)
    np.add.at(d, (np.asarray(clusters, dtype=np.int64), np.asarray(classes, dtype=np.int64)), 1)
    return d


def add(L, scores, first, n, K, classes, perm, conf, R):
    flag = C.c_void_p(conf.data_ptr() + 4 * R * R)
    sub = scores[first:]
    L.check(L.lib.dmvae_confusion_add(stream(), C.c_void_p(sub.data_ptr()), scores.stride(0), n, K, L.ptr(classes), classes.numel(),
                                      L.ptr(perm), first, L.ptr(conf), R, flag), "dmvae_confusion_add")


@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("K", [1, 5, 10, 50, 256])
def test_confusion_add_equals_numpy_exactly(K, with_perm):
    from dmvae_hip import _lib as L
    rng = np.random.RandomState(K + 7 * with_perm)
    n, R, ld = 1000 + 7, K + 3, K + 5
    s = rng.randint(0, 4, (n, K)).astype(np.float32)              # four values: nearly every row has exact ties for the largest
    s[::3] += rng.randn(*s[::3].shape).astype(np.float32)         # and a third of the rows none
    s[5] = -np.inf                                                # all equal, all -inf: index 0
    assert K == 1 or ((s == s.max(1, keepdims=True)).sum(1) > 1).mean() > 0.25
    sd = torch.full((n, ld), 9.0e9, device="cuda")                # (columns >= K must not be read)
    sd[:, :K] = dev(s, torch.float32)
    cls = rng.randint(0, R, n)
    order = rng.permutation(n) if with_perm else np.arange(n)
    cd, pd = dev(cls, torch.int32), (dev(order, torch.int32) if with_perm else None)
    conf = torch.zeros(R * R + 1, dtype=torch.int32, device="cuda")
    cuts = [0, 16, 16 + 333, n]                                   # three ragged batches: `first` moves through the set
    for a, b in zip(cuts[:-1], cuts[1:]):
        add(L, sd, a, b - a, K, cd, pd, conf, R)
    want = confusion(np.argmax(s, axis=1), cls[order], R)
    got = conf.cpu().numpy()
    assert got[-1] == 0
    assert np.array_equal(got[:-1].reshape(R, R), want) and want.sum() == n
    for a, b in zip(cuts[:-1], cuts[1:]):                         # it ADDS: a second pass doubles the matrix
        add(L, sd, a, b - a, K, cd, pd, conf, R)
    assert np.array_equal(conf.cpu().numpy()[:-1].reshape(R, R), 2 * want)


def test_confusion_add_flags_what_it_cannot_count():
    from dmvae_hip import _lib as L
    rng = np.random.RandomState(3)
    n, K, R = 200, 6, 8
    s = rng.randn(n, K).astype(np.float32)
    cls = rng.randint(0, R, n)
    bad = np.array([3, 50, 51, 199])
    cls_bad = cls.copy()
    cls_bad[bad] = [R, -1, R + 100, 2 ** 31 - 1]
    sd, conf = dev(s, torch.float32), torch.zeros(R * R + 1, dtype=torch.int32, device="cuda")
    add(L, sd, 0, n, K, dev(cls_bad, torch.int32), None, conf, R)
    got = conf.cpu().numpy()
    keep = np.setdiff1d(np.arange(n), bad)
    assert got[-1] == 1 and np.array_equal(got[:-1].reshape(R, R), confusion(np.argmax(s, 1)[keep], cls[keep], R))
    # a permutation entry outside the data set: bit 1, nothing counted for that row
    perm = np.arange(n)
    perm[[7, 8]] = [n, -5]
    conf.zero_()
    add(L, sd, 0, n, K, dev(cls, torch.int32), dev(perm, torch.int32), conf, R)
    got = conf.cpu().numpy()
    keep = np.setdiff1d(np.arange(n), [7, 8])
    assert got[-1] == 2 and np.array_equal(got[:-1].reshape(R, R), confusion(np.argmax(s, 1)[keep], cls[keep], R))
    # argument errors enqueue nothing
    conf.zero_()
    cd = dev(cls, torch.int32)
    with pytest.raises(L.DmvaeError, match="K=6, R=5"):
        add(L, sd, 0, n, K, cd, None, conf, 5)
    with pytest.raises(L.DmvaeError, match="not inside"):
        add(L, sd, 1, n, K, cd, None, conf, R)
    torch.cuda.synchronize()
    assert not conf.any()
    from dmvae_hip import StepEngine
    with pytest.raises(IndexError, match="class outside"):
        c2 = StepEngine.confusion_buffer(R, "cuda")
        add(L, sd, 0, n, K, dev(cls_bad, torch.int32), None, c2, R)
        StepEngine.read_confusion(c2)


# ---------------------------------------------------------------------------------------------------------------- VaDE plans
def vade_engine(D, K, B, dtype="fp32"):
    from dmvae_hip import StepEngine
    kw = dict(input_dim=40, latent_dim=D, n_classes=K, enc_layers=(70, 50), dec_layers=(50, 30, 60))
    eng = StepEngine(dtype=dtype, max_batch=B, deterministic=True, model="vade", head_dim=64, seed=11, **kw)
    eng.init_parameters(2)
    rng = np.random.RandomState(D + K)
    p = eng.get_parameters()
    p["prior_means"] = (0.3 * rng.randn(K, D)).astype(np.float32)        # unscaled N(0, 1) means saturate the gate at D = 64
    p["prior_log_vars"] = np.zeros((K, D), np.float32)
    eng.set_parameters(p)
    cfg = O.VadeConfig(40, D, K, kw["enc_layers"], kw["dec_layers"])
    return eng, cfg, {k: v.astype(np.float64) for k, v in eng.get_parameters().items()}


def vade_inputs(N, seed):
    rng = np.random.RandomState(seed)
    X = (rng.rand(N, 40) * (rng.rand(N, 40) < 0.4)).astype(np.float32)
    return X, rng


@pytest.mark.parametrize("D,K", [(8, 5), (10, 10), (64, 10)])
def test_vade_eval_against_the_oracle_with_fed_noise(D, K):
    # enough rows that the 1 % cap on near-tie rows (an oracle property, asserted below) is not decided by a single row: with
    # the gap 2e-4 against top-two gaps of order 0.1 the oracle expects about one such row in several hundred
    B, N, first, n, k, R = 1024, 1100, 9, 1003, 10, K + 2
    eng, cfg, p = vade_engine(D, K, B)
    X, rng = vade_inputs(N, 1)
    cls = rng.randint(0, R, N)
    order = rng.permutation(N)
    eps = rng.randn(k, n, D).astype(np.float32)
    Xd, cd, pd = dev(X, torch.float32), dev(cls, torch.int32), dev(order, torch.int32)
    conf = eng.confusion_buffer(R, "cuda")
    eng.load_batch(Xd, pd, first, n)
    eng.eval_clusters(conf, cd, pd, first, n, draws=k, eps=dev(eps, torch.float32))
    w = eng.view("eval_w", n).cpu().numpy()
    got = eng.read_confusion(conf)
    rows = order[first:first + n]
    a = O.vade_forward(p, cfg, X[rows].astype(np.float64), np.zeros((n, D)))
    gam = np.stack([O.cluster_probs(O.gaussian_reparam(a["mean"], a["logvar"], eps[j].astype(np.float64)), p["prior_means"], p["prior_log_vars"])
                    for j in range(k)])
    assert (gam.max(-1) > 0.99).mean() < 0.10                     # the gate is not saturated: the comparison below means something
    want = gam.mean(0)
    err = np.abs(w - want).max()
    print("D=%d K=%d: max |w - oracle| = %.3g" % (D, K, err))
    np.testing.assert_allclose(w, want, rtol=0, atol=W_ATOL)
    top = np.sort(want, axis=1)
    clear = (top[:, -1] - top[:, -2]) > GAP if K > 1 else np.ones(n, bool)
    print("rows inside the gap: %d of %d" % ((~clear).sum(), n))
    assert (~clear).mean() <= 0.01
    mine = confusion(np.argmax(want, 1)[clear], cls[rows][clear], R) + confusion(np.argmax(w, 1)[~clear], cls[rows][~clear], R)
    assert np.array_equal(got, mine) and got.sum() == n


def test_vade_eval_philox_noise_fed_back_is_bit_identical():
    from dmvae_hip import _lib as L
    D, K, B, N, first, n, k = 10, 10, 96, 120, 9, 83, 4
    eng, cfg, p = vade_engine(D, K, B)
    X, rng = vade_inputs(N, 2)
    Xd, cd = dev(X, torch.float32), dev(rng.randint(0, K, N), torch.int32)
    eng.load_batch(Xd, None, first, n)

    def run(counter, eps=None):
        conf = eng.confusion_buffer(K, "cuda")
        eng.eval_clusters(conf, cd, None, first, n, draws=k, eps=eps, counter=counter)
        return eng.view("eval_w", n).clone(), eng.read_confusion(conf)
    w7, c7 = run(7)
    w7b, c7b = run(7)
    w8, _ = run(8)
    assert torch.equal(w7, w7b) and np.array_equal(c7, c7b) and not torch.equal(w7, w8)
    assert c7.sum() == n and abs(float(w7.sum(1).mean()) - 1.0) < 1e-5
    # the documented keying: element ((j * n_rows + first + r) * D + d) of stream (plan seed, step = counter, stream id 2)
    z = torch.zeros(k * N * D, device="cuda")
    L.check(L.lib.dmvae_philox_normal(stream(), L.ptr(z), z.numel(), int(eng._cfg.seed), 7, 2), "dmvae_philox_normal")
    eps = z.view(k, N, D)[:, first:first + n].contiguous()
    assert abs(float(eps.mean())) < 0.1 and abs(float(eps.std()) - 1.0) < 0.1
    # ... and that buffer is what the exact Philox oracle says stream (seed, counter, 2) holds (atol as in tests/test_gpu_philox.py)
    np.testing.assert_allclose(z.view(k, N, D).cpu().numpy(), PH.eps_eval(int(eng._cfg.seed), 7, k, N, D), rtol=0, atol=1e-3)
    wf, cf = run(99, eps)
    assert torch.equal(wf, w7) and np.array_equal(cf, c7)


def test_eval_clusters_argument_errors_and_limits():
    from dmvae_hip import _lib as L, StepEngine
    eng, _, _ = vade_engine(6, 5, 32)
    X, rng = vade_inputs(40, 3)
    Xd, cd = dev(X, torch.float32), dev(rng.randint(0, 5, 40), torch.int32)
    eng.load_batch(Xd, None, 0, 32)
    conf = eng.confusion_buffer(5, "cuda")
    with pytest.raises(L.DmvaeError, match="draws=0"):
        eng.eval_clusters(conf, cd, None, 0, 32, draws=0)
    with pytest.raises(L.DmvaeError, match="not inside"):
        eng.eval_clusters(conf, cd, None, 20, 32, draws=2)
    with pytest.raises(L.DmvaeError, match="exceeds max_batch"):
        eng.eval_clusters(conf, cd, None, 0, 33, draws=2)
    torch.cuda.synchronize()
    assert not conf.any()
    # a DMVAE plan has no "eval_w"
    e2 = StepEngine(40, 6, 5, enc_layers=(70, 50), head_dim=90, dec_layers=(90, 50, 30), dtype="fp32", max_batch=32)
    with pytest.raises(L.DmvaeError, match="unknown view"):
        e2.view("eval_w")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_whole_set_loop_synchronises_once_and_replays_from_a_graph(dtype):
    from dmvae_hip import StepEngine
    B, N, K = 64, 64 * 5 + 17, 5
    eng = StepEngine(40, 6, K, enc_layers=(70, 50), head_dim=90, dec_layers=(90, 50, 30), dtype=dtype, max_batch=B)
    eng.init_parameters(1)
    X, rng = vade_inputs(N, 4)
    cls, order = rng.randint(0, K, N), rng.permutation(N)
    Xd, cd, pd = dev(X, torch.float32), dev(cls, torch.int32), dev(order, torch.int32)
    conf = eng.confusion_buffer(K, "cuda")
    logits = torch.empty((N, K), device="cuda")
    for s in range(0, N, B):                                      # nothing in this loop waits for the device
        n = min(B, N - s)
        eng.load_batch(Xd, pd, s, n)
        eng.eval_clusters(conf, cd, pd, s, n)
        logits[s:s + n].copy_(eng.view("logits", n))
    d = eng.read_confusion(conf)                                  # the one synchronisation
    assert d.sum() == N
    assert np.array_equal(d, confusion(np.argmax(logits.cpu().numpy(), 1), cls[order], K))
    # one batch's gather + encoder + count under stream capture: three replays count that batch three times
    one = eng.confusion_buffer(K, "cuda")
    eng.load_batch(Xd, pd, 0, B)
    eng.eval_clusters(one, cd, pd, 0, B)
    single = eng.read_confusion(one)
    rep = eng.confusion_buffer(K, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        eng.load_batch(Xd, pd, 0, B)
        eng.eval_clusters(rep, cd, pd, 0, B)
    torch.cuda.synchronize()
    assert not rep.any()                                          # capture enqueued nothing
    for _ in range(3):
        g.replay()
    assert np.array_equal(eng.read_confusion(rep), 3 * single)
