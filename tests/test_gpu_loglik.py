"""GPU tests of the held-out log-likelihood on the device (csrc/eval_loglik.hip, dmvae_plan_eval_loglik): the importance-weighted
bound per row against the float64 oracle of tests/helpers/loglik_oracle.py.

Bars.  fp32 plans: every row's L to 1e-3 * max(1, |reference|), the bar the project holds fp32 losses to (DESIGN section 5,
tests/test_gpu_moe.py).  bf16 against fp32 on the same inputs: the mean within 2e-3 relative, the project's bf16 loss bar (DESIGN
section 5).  acc against the sum of row_ll: 1e-9 relative (a float64 tree over float32 values).  Properties (reproducibility, no side
effects, plan sizes): bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import dmvae_oracle as O        # noqa: E402
import loglik_oracle as LO      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENC, HEAD, DEC = (72,), 40, (48, 36)
BUILT = []                      # (Config copy, sizes as dmvae_plan_sizes returned them at creation) of every plan built in this file


def sizes_tuple(sz):
    return (sz.param_elems, sz.work_bytes, sz.batch_pad, sz.input_pad, sz.n_tensors)


def engine(model, input_type, I, D, K, B, dtype="fp32", enc=ENC, head=HEAD, dec=DEC, cnn=False, seed=11):
    """a small engine with prior tables, posterior widths and output biases away from their symmetric initial values, its oracle
    config and its parameters in float64"""
    from dmvae_hip import StepEngine, _lib
    eng = StepEngine(I, D, K, enc_layers=enc, head_dim=head, dec_layers=dec, input_type=input_type, dtype=dtype, max_batch=B,
                     deterministic=True, model=model, cnn=cnn, seed=seed)
    eng.init_parameters(2)
    rng = np.random.RandomState(D + K)
    eng.set_parameters({"prior_means": 0.5 * rng.randn(K, D), "prior_log_vars": 0.3 * rng.randn(K, D),
                        "b_logvar": 0.2 * rng.randn(D) - 0.5, "b_out": 0.3 * rng.randn(I)})
    if model == "vade":
        cfg = O.VadeConfig(I, D, K, enc, dec, input_type, cnn=cnn)
    else:
        cfg = O.Config(I, D, K, enc, head, dec, input_type, cnn=cnn)
    c2 = _lib.Config()
    C.memmove(C.byref(c2), C.byref(eng._cfg), C.sizeof(c2))
    BUILT.append((c2, sizes_tuple(eng.sizes)))
    assert eng.work.numel() == eng.sizes.work_bytes
    return eng, cfg


def params64(eng):
    return {k: v.astype(np.float64) for k, v in eng.get_parameters().items()}


def inputs(N, I, input_type, seed):
    rng = np.random.RandomState(seed)
    X = (rng.rand(N, I) < 0.4).astype(np.float32) if input_type == "binary" else (0.7 * rng.randn(N, I)).astype(np.float32)
    return X, rng


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def run(eng, Xd, pd, n_rows, first, n, S, eps=None, counter=0, acc=None):
    """one batch through the engine: (row_ll [n] float32 on the host, acc float64 [2] on the host, the device acc)"""
    acc = eng.loglik_buffer() if acc is None else acc
    rl = torch.full((n,), float("nan"), device="cuda")
    eng.load_batch(Xd, pd, first, n)
    eng.eval_loglik(acc, n, n_rows, first, S, eps=None if eps is None else dev(eps), counter=counter, row_ll=rl)
    return rl.cpu().numpy(), acc.cpu().numpy(), acc


def assert_rows(got, ref, what=""):
    bar = 1e-3 * np.maximum(1.0, np.abs(ref))
    err = np.abs(got.astype(np.float64) - ref)
    print("%s max |L - oracle| = %.3g (bar %.3g, |L| up to %.4g)" % (what, err.max(), bar[np.argmax(err / bar)], np.abs(ref).max()))
    assert np.all(np.isfinite(got)) and np.all(err <= bar), (what, float(err.max()), int(np.argmax(err / bar)))


def assert_acc(acc, row_ll, n):
    tot = row_ll.astype(np.float64).sum()
    assert acc[1] == n and abs(acc[0] - tot) <= 1e-9 * abs(tot), (acc, tot)


# (input_dim, D, K): pad columns in I and D | more clusters than lanes, D past one pad | 80 KiB of tables, past one LDS chunk |
# a row of z wider than the kernel keeps in LDS (the read-back form of loglik_draw_kernel)
SHAPES = [(70, 5, 3), (64, 70, 17), (64, 256, 40), (64, 800, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "I%d-D%d-K%d" % s)
@pytest.mark.parametrize("input_type", ["binary", "real"])
@pytest.mark.parametrize("model", ["dmvae", "vade"])
def test_rows_against_the_oracle_with_fed_noise(model, input_type, shape):
    I, D, K = shape
    N, B, first, n = 90, 40, 11, 37
    eng, cfg = engine(model, input_type, I, D, K, B)
    p = params64(eng)
    X, rng = inputs(N, I, input_type, 1)
    order = rng.permutation(N)
    Xd, pd = dev(X), dev(order, torch.int32)
    Xb = X[order[first:first + n]].astype(np.float64)
    for S in (1, 2, 7):
        eps = rng.randn(S, n, D).astype(np.float32)
        got, acc, _ = run(eng, Xd, pd, N, first, n, S, eps)
        assert_rows(got, LO.row_ll(p, cfg, Xb, eps), "%s %s %s S=%d" % (model, input_type, shape, S))
        assert_acc(acc, got, n)


@pytest.mark.parametrize("model", ["dmvae", "vade"])
def test_tables_of_the_largest_configured_shape(model):
    """K = 256 clusters of D = 512 columns (1 MiB of tables: 16 cluster tiles of 8 column chunks each, the large-table form of VaDE's step)"""
    I, D, K = 64, 512, 256
    N, B, first, n, S = 90, 40, 11, 37, 2
    eng, cfg = engine(model, "binary", I, D, K, B)
    X, rng = inputs(N, I, "binary", 9)
    order = rng.permutation(N)
    eps = rng.randn(S, n, D).astype(np.float32)
    got, acc, _ = run(eng, dev(X), dev(order, torch.int32), N, first, n, S, eps)
    assert_rows(got, LO.row_ll(params64(eng), cfg, X[order[first:first + n]].astype(np.float64), eps), "%s K=256 D=512" % model)
    assert_acc(acc, got, n)


def test_stable_softplus_under_saturated_output_biases():
    I, D, K = 70, 5, 3
    N, B, first, n, S = 90, 40, 11, 37, 2
    eng, cfg = engine("dmvae", "binary", I, D, K, B)
    b = eng.get_parameters()["b_out"]
    b[::7], b[3::7] = 40.0, -40.0
    eng.set_parameters({"b_out": b})
    p = params64(eng)
    X, rng = inputs(N, I, "binary", 2)
    order = rng.permutation(N)
    eps = rng.randn(S, n, D).astype(np.float32)
    got, acc, _ = run(eng, dev(X), dev(order, torch.int32), N, first, n, S, eps)
    ref = LO.row_ll(p, cfg, X[order[first:first + n]].astype(np.float64), eps)
    assert np.abs(ref).max() > 100.0                             # rows that pay 40 nats per saturated pixel they contradict
    assert_rows(got, ref, "b_out = +-40")
    assert_acc(acc, got, n)


@pytest.mark.parametrize("model", ["dmvae", "vade"])
def test_pad_columns_of_the_logits_are_not_summed(model):
    I, D, K = 70, 5, 3                                           # input_pad = 128: 58 pad columns of logit 0, -log 2 each if summed
    N, B, first, n, S = 90, 40, 11, 37, 2
    eng, cfg = engine(model, "binary", I, D, K, B)
    eng.set_parameters({"b_out": np.zeros(I), "W_out": np.zeros((DEC[-1], I))})
    assert eng.input_pad - I == 58
    p = params64(eng)
    X, rng = inputs(N, I, "binary", 3)
    order = rng.permutation(N)
    eps = rng.randn(S, n, D).astype(np.float32)
    got, _, _ = run(eng, dev(X), dev(order, torch.int32), N, first, n, S, eps)
    Xb = X[order[first:first + n]].astype(np.float64)
    mean, lv = LO.posterior(p, cfg, Xb)
    lat = np.stack([np.subtract(*LO.draw_terms(p, cfg, Xb, mean, lv, e.astype(np.float64))[1:]) for e in eps])      # log p(z_s) - log q_s
    want = -70.0 * np.log(2.0) + LO.bound(lat)
    np.testing.assert_allclose(LO.row_ll(p, cfg, Xb, eps), want, rtol=1e-12)
    assert_rows(got, want, "zero logits")
    assert np.all(np.abs(got - (want - 58.0 * np.log(2.0))) > 30.0)


@pytest.mark.parametrize("input_type", ["binary", "real"])
@pytest.mark.parametrize("model", ["dmvae", "vade"])
def test_closed_form_with_device_noise(model, input_type):
    I, D, K = 70, 5, 3
    N, B = 40, 40
    eng, cfg = engine(model, input_type, I, D, K, B)
    rng = np.random.RandomState(8)
    q = LO.closed_form_parameters(params64(eng), rng.randn(D), 0.4 * rng.randn(D))
    eng.set_parameters(q)
    p = params64(eng)
    X, _ = inputs(N, I, input_type, 4)
    want = LO.bias_only_log_px(p, cfg, X.astype(np.float64))
    Xd = dev(X)
    for S in (1, 9):
        for counter in (0, 12345):
            got, acc, _ = run(eng, Xd, None, N, 0, N, S, None, counter)
            assert_rows(got, want, "closed form %s %s S=%d counter=%d" % (model, input_type, S, counter))
            assert_acc(acc, got, N)


@pytest.mark.parametrize("shape", [(70, 5, 3), (64, 70, 17)], ids=lambda s: "I%d-D%d-K%d" % s)
def test_device_noise_is_stream_four_keyed_by_position(shape):
    I, D, K = shape
    N, B, first, n, S = 90, 40, 11, 37, 3
    eng, cfg = engine("vade", "binary", I, D, K, B, seed=23)
    X, rng = inputs(N, I, "binary", 5)
    order = rng.permutation(N)
    Xd, pd = dev(X), dev(order, torch.int32)
    g7, _, _ = run(eng, Xd, pd, N, first, n, S, None, 7)
    g7b, _, _ = run(eng, Xd, pd, N, first, n, S, None, 7)
    g8, _, _ = run(eng, Xd, pd, N, first, n, S, None, 8)
    assert np.array_equal(g7, g7b) and not np.array_equal(g7, g8)
    eps = LO.device_eps(int(eng._cfg.seed), 7, S, N, D, first, n).astype(np.float32)
    assert abs(eps.mean()) < 0.1 and abs(eps.std() - 1.0) < 0.1
    fed, _, _ = run(eng, Xd, pd, N, first, n, S, eps, 99)
    assert_rows(g7, fed.astype(np.float64), "device noise against the fed oracle noise")
    assert_rows(g7, LO.row_ll(params64(eng), cfg, X[order[first:first + n]].astype(np.float64), eps), "device noise against the oracle")


def test_two_batches_accumulate_into_the_mean_of_the_set():
    I, D, K = 70, 5, 3
    N, B, S, counter = 63, 40, 4, 3
    eng, cfg = engine("dmvae", "binary", I, D, K, B, seed=5)
    X, rng = inputs(N, I, "binary", 6)
    order = rng.permutation(N)
    Xd, pd = dev(X), dev(order, torch.int32)
    acc = eng.loglik_buffer()
    r0, _, _ = run(eng, Xd, pd, N, 0, 40, S, None, counter, acc)
    r1, a, _ = run(eng, Xd, pd, N, 40, 23, S, None, counter, acc)
    eps = LO.device_eps(int(eng._cfg.seed), counter, S, N, D)                # the noise index follows `first`
    ref = LO.row_ll(params64(eng), cfg, X[order].astype(np.float64), eps)
    assert_rows(np.concatenate([r0, r1]), ref, "two batches")
    mean, rows = eng.read_loglik(acc)
    assert rows == 63 and a[1] == 63 and abs(mean - ref.mean()) <= 1e-3 * max(1.0, abs(ref.mean())), (mean, ref.mean())
    assert_acc(a, np.concatenate([r0, r1]), 63)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("model", ["dmvae", "vade"])
def test_an_evaluation_leaves_the_training_state_alone(model, dtype):
    from dmvae_hip import _lib
    I, D, K, B, N = 64, 6, 5, 40, 90
    X, rng = inputs(N, I, "binary", 7)
    order = rng.permutation(N)
    Xd, pd = dev(X), dev(order, torch.int32)
    out = []
    for evaluate in (False, True):
        eng, _ = engine(model, "binary", I, D, K, B, dtype=dtype)
        eng.write_state(lr=0.002, kl_ratio=0.8)
        eng.train_step(Xd, pd, B, first=0)                       # non-zero moments and gradients to keep
        eng.load_batch(Xd, pd, 0, B)
        eng.forward_backward(B)                                  # (the fused step does not write the gradient arena; this pass does)
        torch.cuda.synchronize()
        if evaluate:
            arenas = [t.clone() for t in (eng.param, eng.m, eng.v, eng.grad)] + ([eng.param_bf16.clone()] if eng.param_bf16 is not None else [])
            state = bytes(eng.read_state())
            for first, n, S, eps in ((0, 40, 3, None), (40, 37, 2, rng.randn(2, 37, D).astype(np.float32))):
                got, _, _ = run(eng, Xd, pd, N, first, n, S, eps, 4)
                assert np.all(np.isfinite(got))
            now = [eng.param, eng.m, eng.v, eng.grad] + ([eng.param_bf16] if eng.param_bf16 is not None else [])
            assert all(torch.equal(a, b) for a, b in zip(arenas, now)) and bytes(eng.read_state()) == state
            sz = _lib.Sizes()
            _lib.check(_lib.lib.dmvae_plan_sizes(eng._plan, C.byref(sz)), "dmvae_plan_sizes")
            assert sizes_tuple(sz) == sizes_tuple(eng.sizes)
        eng.train_step(Xd, pd, B, first=40)
        torch.cuda.synchronize()
        out.append((eng.param.clone(), eng.m.clone(), eng.v.clone(), bytes(eng.read_state())))
    assert all(torch.equal(out[0][i], out[1][i]) for i in range(3)) and out[0][3] == out[1][3]


def test_bf16_plan_against_the_fp32_plan_at_reference_sized_layers():
    I, D, K, B, S = 784, 64, 10, 256, 4
    ref = dict(enc=(500, 500), head=2000, dec=(2000, 500, 500))
    X = O.synthetic_images(B, I, seed=3)
    eps = np.random.RandomState(9).randn(S, B, D).astype(np.float32)
    means = {}
    for dtype in ("fp32", "bf16"):
        eng, _ = engine("dmvae", "binary", I, D, K, B, dtype=dtype, **ref)
        got, acc, dacc = run(eng, dev(X), None, B, 0, B, S, eps)
        assert_acc(acc, got, B)
        means[dtype] = eng.read_loglik(dacc)[0]
    gap = abs(means["bf16"] - means["fp32"]) / abs(means["fp32"])
    print("mean L: fp32 %.6f, bf16 %.6f, relative gap %.3g" % (means["fp32"], means["bf16"], gap))
    assert gap <= 2e-3, (means, gap)


def test_conv_trunk_against_the_oracle():
    I, D, K, B, S = 784, 8, 5, 8, 2
    eng, cfg = engine("dmvae", "binary", I, D, K, B, enc=(96,), head=64, dec=(64, 48), cnn=True)
    X = O.synthetic_images(B, I, seed=9)
    eps = np.random.RandomState(4).randn(S, B, D).astype(np.float32)
    got, acc, _ = run(eng, dev(X), None, B, 0, B, S, eps)
    assert_rows(got, LO.row_ll(params64(eng), cfg, X.astype(np.float64), eps), "conv trunk")
    assert_acc(acc, got, B)


def test_argument_errors_enqueue_nothing():
    from dmvae_hip import _lib as L
    I, D, K, B, N = 64, 6, 5, 40, 90
    eng, _ = engine("dmvae", "binary", I, D, K, B, dtype="bf16")
    X, _ = inputs(N, I, "binary", 8)
    Xd = dev(X)
    acc = eng.loglik_buffer()
    eng.load_batch(Xd, None, 0, B)
    with pytest.raises(L.DmvaeError, match="draws=0"):
        eng.eval_loglik(acc, B, N, 0, 0)
    with pytest.raises(L.DmvaeError, match="draws=1025"):
        eng.eval_loglik(acc, B, N, 0, 1025)
    with pytest.raises(L.DmvaeError, match="not inside"):
        eng.eval_loglik(acc, B, N, N - B + 1, 2)
    with pytest.raises(L.DmvaeError, match="not inside"):
        eng.eval_loglik(acc, B, N, -1, 2)
    with pytest.raises(L.DmvaeError, match="max_batch"):
        eng.eval_loglik(acc, B + 1, N, 0, 2)
    need = int(L.lib.dmvae_plan_eval_loglik_ws_bytes(eng._plan))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda ws_ptr, nbytes, acc_ptr: L.lib.dmvae_plan_eval_loglik(eng._plan, stream, B, N, 0, 2, None, D, 0, ws_ptr, nbytes, None, acc_ptr)
    with pytest.raises(L.DmvaeError, match="%d are needed" % need):
        L.check(call(L.ptr(ws), need - 1, L.ptr(acc)), "dmvae_plan_eval_loglik")
    with pytest.raises(L.DmvaeError, match="are needed"):
        L.check(call(None, need, L.ptr(acc)), "dmvae_plan_eval_loglik")
    with pytest.raises(L.DmvaeError, match="null acc"):
        L.check(call(L.ptr(ws), need, None), "dmvae_plan_eval_loglik")
    eng._load_batch_for_step(Xd, None, 0, B)                     # bf16, input_dim % 4 == 0: no f32 copy of this batch exists
    with pytest.raises(L.DmvaeError, match="dmvae_plan_load_batch"):
        eng.eval_loglik(acc, B, N, 0, 2)
    torch.cuda.synchronize()
    assert not acc.cpu().numpy().any() and not ws.any()
    eng.load_batch(Xd, None, 0, B)                               # and the plan still evaluates
    L.check(call(L.ptr(ws), need, L.ptr(acc)), "dmvae_plan_eval_loglik")
    mean, rows = eng.read_loglik(acc)
    assert rows == B and np.isfinite(mean)


@pytest.mark.parametrize("model", ["dmvae", "vade"])
def test_get_log_likelihood_equals_the_engine_level_loop(model):
    import base_models
    from includes.utils import Dataset
    rng = np.random.RandomState(12)
    X, cls = (rng.rand(300, 40) * (rng.rand(300, 40) < 0.4)).astype(np.float32), rng.randint(0, 5, 300)
    kw = dict(activation="relu", initializer="xavier", batch_size=100, dtype="bf16", seed=3)
    if model == "vade":
        m = base_models.VaDE("vade", "binary", 40, 6, 5, enc_layers=(70, 50, 30), dec_layers=(30, 50, 70), **kw).build_graph()
    else:
        m = base_models.DeepMixtureVAE("dmvae", "binary", 40, 6, 5, enc_layers=(70, 50), head_dim=90, dec_layers=(90, 50, 30), **kw).build_graph()
    np.random.seed(5)
    data = Dataset((X, cls), batch_size=100)
    state = np.random.get_state()
    ll = m.get_log_likelihood(None, data, k=3, counter=2)
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))      # nothing is drawn from NumPy, the order is kept
    assert isinstance(ll, float) and np.isfinite(ll) and ll < 0.0
    assert ll == m.get_log_likelihood(None, data, k=3, counter=2) and ll != m.get_log_likelihood(None, data, k=3, counter=3)
    eng = m.engine
    acc = eng.loglik_buffer()
    rows, pd = data.device_rows(eng.device), dev(data.order, torch.int32)
    for s in range(0, 300, 100):
        eng.load_batch(rows, pd, s, 100)
        eng.eval_loglik(acc, 100, 300, s, 3, counter=2)
    assert eng.read_loglik(acc) == (ll, 300)


def test_train_py_loglik_prints_lltest_and_is_silent_without_the_flag(tmp_path):
    env = dict(os.environ, DMVAE_DATA=str(tmp_path / "nodata"))
    base = [sys.executable, os.path.join(ROOT, "deep-mixture-vae_amd", "train.py"), "--dataset", "synthetic", "--n_epochs", "1", "--eval", "device",
            "--batch_size", "1000", "--enc_layers", "128", "--head_dim", "128", "--dec_layers", "128"]
    procs = []
    for name, extra in (("with", ["--loglik", "2"]), ("without", [])):
        d = tmp_path / name
        d.mkdir()
        procs.append((d, subprocess.Popen(base + extra, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    outs = []
    for d, pr in procs:
        so, se = pr.communicate(timeout=900)
        assert pr.returncode == 0, (so[-2000:], se[-3000:])
        outs.append((so + se, [__import__("json").loads(l) for l in open(d / "dmvae_metrics.jsonl")]))
    (on, rec_on), (off, rec_off) = outs
    assert "llTest=-" in on and "llTest" not in off and "accTest=" in off
    assert len(rec_on) == 1 and rec_on[0]["loglik_draws"] == 2 and np.isfinite(rec_on[0]["ll_test"]) and rec_on[0]["ll_test"] < 0.0
    assert len(rec_off) == 1 and "ll_test" not in rec_off[0] and set(rec_on[0]) - set(rec_off[0]) == {"ll_test", "loglik_draws"}
    assert rec_on[0]["loss"] == rec_off[0]["loss"] and rec_on[0]["acc_test"] == rec_off[0]["acc_test"]      # the evaluation changes nothing it follows


def test_plan_sizes_of_every_plan_built_here_do_not_know_the_evaluation():
    """dmvae_plan_sizes is what it was: the scratch is the caller's.  Every configuration this file built -- recorded with the sizes the
    public call returned when its engine was created -- gives the same sizes on a fresh plan that never saw an evaluation, and the
    workspace the engine allocated is exactly work_bytes."""
    from dmvae_hip import _lib
    engine("dmvae", "real", 70, 5, 3, 40)                        # (so that the list is not empty when this test runs alone)
    engine("vade", "binary", 64, 256, 40, 200, dtype="bf16")
    for cfg, want in BUILT:
        h = C.c_void_p()
        _lib.check(_lib.lib.dmvae_plan_create(C.byref(cfg), C.byref(h)), "dmvae_plan_create")
        sz = _lib.Sizes()
        _lib.check(_lib.lib.dmvae_plan_sizes(h, C.byref(sz)), "dmvae_plan_sizes")
        ws = int(_lib.lib.dmvae_plan_eval_loglik_ws_bytes(h))
        _lib.lib.dmvae_plan_destroy(h)
        assert sizes_tuple(sz) == want and ws == (12 * want[2] + 255) // 256 * 256
