"""GPU parity tests, step level: the plan's forward/loss/backward/Adam against
the float64 oracle on identical parameters, batches and noise.

Tolerances (stated per BASELINE.json's north star):
  fp32 (parity) mode : per-step loss |delta| <= 1e-3 nats, gradients <= 1e-4
                       relative (to the tensor's max |g|, oracle backward taking the
                       GPU's ReLU masks, see dmvae_oracle.backward),
                       parameters after 3 Adam steps <= 2e-4 absolute.
  bf16 mode          : loss within 2e-3 relative, gradients within 8e-2
                       relative Frobenius error per tensor.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import dmvae_oracle as O


@pytest.fixture(scope="module")
def hip():
    from dmvae_hip import _lib
    torch.cuda.set_device(0)
    return _lib


def make(cfg_kw, dtype, B, mode="exact", deterministic=True, seed=0):
    from dmvae_hip import StepEngine
    eng = StepEngine(dtype=dtype, max_batch=B, mode=mode, temperature=0.5, deterministic=deterministic, **cfg_kw)
    eng.init_parameters(seed)
    return eng


def oracle_cfg(kw):
    return O.Config(kw["input_dim"], kw["latent_dim"], kw["n_classes"], kw.get("enc_layers", (500, 500)),
                    kw.get("head_dim", 2000), kw.get("dec_layers", (2000, 500, 500)), kw.get("input_type", "binary"))


SMALL = dict(input_dim=40, latent_dim=6, n_classes=5, enc_layers=(70, 50), head_dim=90, dec_layers=(90, 50, 30))
REF = dict(input_dim=784, latent_dim=10, n_classes=10)


def test_init_matches_reference_rules_and_oracle_stream():
    eng = make(REF, "fp32", 100)
    p = eng.get_parameters()
    o = O.init_params(oracle_cfg(REF), 0)
    assert set(p) == set(o)
    for k in o:
        np.testing.assert_allclose(p[k], o[k].astype(np.float32), rtol=0, atol=0, err_msg=k)
    assert eng.param.numel() >= oracle_cfg(REF).n_params()


# cfg4's latent geometry (D=256, K=50: the prior tables go through LDS in four D-chunks) on small layers
WIDE = dict(input_dim=100, latent_dim=256, n_classes=50, enc_layers=(70, 50), head_dim=90, dec_layers=(90, 50, 30))


@pytest.mark.parametrize("cfg_kw,B", [(SMALL, 37), (REF, 100), (WIDE, 48)])
@pytest.mark.parametrize("mode", ["exact", "relaxed"])
@pytest.mark.parametrize("input_type", ["binary", "real"])
def test_fp32_step_matches_oracle(cfg_kw, B, mode, input_type):
    kw = dict(cfg_kw, input_type=input_type)
    if cfg_kw is REF and (mode == "relaxed" or input_type == "real"):
        pytest.skip("reference-size case runs once (exact, binary)")
    if cfg_kw is WIDE and input_type == "real":
        pytest.skip("wide-latent case runs with the binary loss only")
    eng = make(kw, "fp32", B, mode)
    cfg = oracle_cfg(kw)
    rng = np.random.RandomState(1)
    p = {k: v.astype(np.float64) for k, v in eng.get_parameters().items()}
    p["prior_log_vars"] = (rng.randn(*p["prior_log_vars"].shape) * 0.3).astype(np.float32).astype(np.float64)
    for k in p:
        if k.startswith("b_"):
            p[k] = (rng.randn(*p[k].shape) * 0.05).astype(np.float32).astype(np.float64)
    eng.set_parameters(p)
    X = (rng.rand(B, cfg.input_dim) * (rng.rand(B, cfg.input_dim) < 0.3)).astype(np.float32)
    eps = rng.randn(B, cfg.latent_dim).astype(np.float32)
    gum = O.sample_gumbel((B, cfg.n_classes), rng).astype(np.float32)
    Xd, ed, gd = (torch.as_tensor(a).cuda() for a in (X, eps, gum))
    eng.write_state(kl_ratio=0.8, lr=0.002)
    eng.load_batch(Xd, None, 0, B)
    eng.forward_backward(B, ed, gd if mode == "relaxed" else None)
    torch.cuda.synchronize()
    a = O.forward(p, cfg, X.astype(np.float64), eps.astype(np.float64), 0.8, mode, gum.astype(np.float64), 0.5)
    # the oracle's backward takes the GPU's ReLU masks: a pre-activation within f32 rounding of
    # zero can fall on the other side in float64 (see dmvae_oracle.backward); count them
    masks = {k: (v > 0).cpu().numpy() for k, v in eng.hidden_activations(B).items()}
    flips = sum(int((masks[k] != (a[k] > 0)).sum()) for k in masks)
    assert flips <= 1e-4 * sum(mk.size for mk in masks.values()), flips
    for k in masks:      # forward activations agree to f32 rounding everywhere
        np.testing.assert_allclose(eng.hidden_activations(B)[k].cpu().numpy(), a[k], atol=3e-5, err_msg=k)
    g = O.backward(p, cfg, a, masks)
    st = eng.read_state()
    assert abs(st.last_loss - a["loss"]) <= 1e-3, (st.last_loss, a["loss"])
    assert abs(st.last_recon - a["recon"]) <= 1e-3
    assert abs(st.last_klz - a["kl_z"]) <= 1e-4 * max(1.0, abs(a["kl_z"]))
    assert abs(st.last_klc - a["kl_c"]) <= 1e-5
    np.testing.assert_allclose(eng.view("mean", B).cpu().numpy(), a["mean"], atol=2e-5)
    np.testing.assert_allclose(eng.view("logits", B).cpu().numpy(), a["logits"], atol=2e-5)
    np.testing.assert_allclose(eng.view("weights", B).cpu().numpy(), a["w"], atol=1e-5)
    gg = eng.get_gradients()
    for k in g:
        scale = np.abs(g[k]).max() + 1e-12
        assert np.abs(gg[k] - g[k]).max() <= 1e-4 * scale, (k, np.abs(gg[k] - g[k]).max(), scale)
    # pad rows/cols of the arena carry no gradient
    total = sum(float(np.abs(v).sum()) for v in gg.values())
    assert abs(eng.grad.abs().sum().item() - total) <= 1e-4 * total
    # three Adam steps on the same batch
    m, v = O.adam_tf_init(p)
    O.adam_tf(p, g, m, v, 1, 0.002)
    eng.update(1.0)
    for t in (2, 3):
        eng.forward_backward(B, ed, gd if mode == "relaxed" else None)
        eng.update(1.0)
        a2, _ = O.train_step(p, m, v, t, cfg, X.astype(np.float64), eps.astype(np.float64), 0.8, 0.002, mode,
                             gum.astype(np.float64), 0.5)
        torch.cuda.synchronize()
        assert abs(eng.read_state().last_loss - a2["loss"]) <= 2e-3
    assert eng.read_state().adam_t == 3
    pg = eng.get_parameters()
    for k in p:       # Adam moves a parameter by ~lr per step whatever |g|: compare the bulk
        d = np.abs(pg[k] - p[k])
        assert np.percentile(d, 99.0) <= 2e-4, (k, np.percentile(d, 99.0))
        assert d.max() <= 3 * 3 * 0.002, (k, d.max())


@pytest.mark.parametrize("deterministic", [True, False])
def test_bf16_step_close_to_oracle(deterministic):
    kw, B = dict(input_dim=784, latent_dim=64, n_classes=10), 512
    eng = make(kw, "bf16", B, deterministic=deterministic)
    cfg = oracle_cfg(kw)
    rng = np.random.RandomState(2)
    p = {k: v.astype(np.float64) for k, v in eng.get_parameters().items()}
    X = O.synthetic_images(B, 784, seed=3)
    eps = rng.randn(B, 64).astype(np.float32)
    Xd, ed = torch.as_tensor(X).cuda(), torch.as_tensor(eps).cuda()
    eng.load_batch(Xd, None, 0, B)
    eng.forward_backward(B, ed)
    torch.cuda.synchronize()
    a = O.forward(p, cfg, X.astype(np.float64), eps.astype(np.float64))
    g = O.backward(p, cfg, a)
    st = eng.read_state()
    assert abs(st.last_loss - a["loss"]) <= 2e-3 * abs(a["loss"]), (st.last_loss, a["loss"])
    gg = eng.get_gradients()
    for k in g:       # bf16 operands: per-tensor relative Frobenius error (measured 2e-4 .. 5e-2)
        rel = np.linalg.norm(gg[k] - g[k]) / (np.linalg.norm(g[k]) + 1e-30)
        assert rel <= 8e-2, (k, rel)
    eng.update(1.0)
    torch.cuda.synchronize()
    assert eng.read_state().adam_t == 1
    assert torch.equal(eng.param_bf16, eng.param.to(torch.bfloat16))


@pytest.mark.parametrize("mode", ["exact", "relaxed"])
def test_fused_update_equals_backward_then_adam(mode):
    """dmvae_plan_train_step (Adam in the epilogue of the dW launch, gradients never stored) must
    leave exactly the bits that forward_backward + update leave: parameters, m, v, bf16 shadow,
    step state -- over several steps, with a ragged batch among them."""
    kw, B = dict(input_dim=784, latent_dim=64, n_classes=10), 256
    rng = np.random.RandomState(11)
    X = O.synthetic_images(B, 784, seed=5)
    Xd = torch.as_tensor(X).cuda()
    engs = [make(kw, "bf16", B, deterministic=True, seed=9, mode=mode) for _ in range(2)]
    for step, n in enumerate((B, B, 200, B)):
        ed = torch.as_tensor(rng.randn(n, 64).astype(np.float32)).cuda()
        gd = torch.as_tensor(rng.gumbel(size=(n, 10)).astype(np.float32)).cuda() if mode == "relaxed" else None
        for fused, eng in zip((False, True), engs):
            eng.load_batch(Xd, None, 0, n)
            if fused:
                eng.forward_backward_update(n, ed, gd)
            else:
                eng.forward_backward(n, ed, gd)
                eng.update(1.0)
        torch.cuda.synchronize()
        a, b = engs
        assert a.read_state().adam_t == b.read_state().adam_t == step + 1
        assert a.read_state().last_loss == b.read_state().last_loss
        for name in ("param", "m", "v", "param_bf16"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (step, name)
    assert engs[0].param.abs().sum().item() > 0


@pytest.mark.parametrize("B", [256, 4096])
def test_step_path_without_the_f32_batch_copy_equals_plain_load(B):
    """train_step assembles its batch with dmvae_plan_load_batch_step: only the bf16 copy is written and the output layer's
    reconstruction epilogue reads its targets from the dataset through the permutation.  It must leave the bits of
    load_batch (bf16 + f32 copies) + the same step: loss, parameters, moments -- shuffled rows, a ragged last batch, several
    steps, eager and replayed from a graph with the cursor in the device state."""
    kw = dict(input_dim=784, latent_dim=64, n_classes=10)
    N = 3 * B + 77
    X = torch.as_tensor(O.synthetic_images(N, 784, seed=8)).cuda()
    perm = torch.randperm(N, device="cuda").to(torch.int32)
    plain, stepp = make(kw, "bf16", B, seed=4), make(kw, "bf16", B, seed=4)
    rng = np.random.RandomState(2)
    for step, (first, n) in enumerate(((0, B), (B, B), (2 * B, B), (3 * B, 77))):
        ed = torch.as_tensor(rng.randn(n, 64).astype(np.float32)).cuda()
        plain.load_batch(X, perm, first, n)                  # writes the f32 copy: the epilogue reads its targets there
        plain.forward_backward_update(n, ed)
        stepp.train_step(X, perm, n, ed, None, first, False)  # dmvae_plan_load_batch_step
        torch.cuda.synchronize()
        assert plain.read_state().last_loss == stepp.read_state().last_loss, step
        assert plain.read_state().last_recon == stepp.read_state().last_recon, step
        for name in ("param", "m", "v", "param_bf16"):
            assert torch.equal(getattr(plain, name), getattr(stepp, name)), (step, name)
    # device-side cursor + graph replay (the bench's form) against eager plain loads
    for eng in (plain, stepp):
        eng.reset_epoch(3)
    rp = stepp.capture_step(X, perm)
    for i in range(3):
        plain.load_batch(X, perm, 0, B, use_state_cursor=True)
        plain.forward_backward_update(B)
        rp()
    torch.cuda.synchronize()
    assert plain.read_state().last_loss == stepp.read_state().last_loss
    assert torch.equal(plain.param, stepp.param)
    # fp32 plans keep the copy (nothing changes there), and an n_valid that disagrees with the assembled batch is refused
    f = make(kw, "fp32", 256, seed=4)
    f.train_step(X, perm, 200, torch.zeros((200, 64), device="cuda"), None, 0, False)
    np.testing.assert_array_equal(f.view("x", 200, 784).cpu().numpy(), X[perm[:200].long()].cpu().numpy())
    stepp._load_batch_for_step(X, perm, 0, 77)
    with pytest.raises(Exception, match="assembled 77 rows"):
        stepp.forward_backward_update(B)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_staged_backward_equals_whole_and_buckets_cover_the_arena(dtype):
    """dmvae_plan_forward_backward_stage 0, 1, 2 (the data-parallel form: one dW launch and one
    finished gradient bucket per segment) leaves the bits dmvae_plan_forward_backward leaves, and
    after segment k its bucket no longer changes."""
    kw, B = dict(input_dim=784, latent_dim=64, n_classes=10), 256
    rng = np.random.RandomState(13)
    Xd = torch.as_tensor(O.synthetic_images(B, 784, seed=6)).cuda()
    ed = torch.as_tensor(rng.randn(B, 64).astype(np.float32)).cuda()
    whole, staged = make(kw, dtype, B, seed=2), make(kw, dtype, B, seed=2)
    whole.load_batch(Xd, None, 0, B)
    whole.forward_backward(B, ed)
    buckets, (tlo, thi) = staged.grad_buckets()
    assert buckets[2][0] == 0 and buckets[0][1] == tlo and tlo % 4096 == 0      # trunk weights first in the arena, decoder weights last, then the tail
    assert buckets[2][1] == buckets[1][0] and buckets[1][1] == buckets[0][0]    # contiguous, no gap
    assert thi == staged.sizes.param_elems <= staged.grad.numel()
    names = staged.tensors
    assert all((names[k][0] >= tlo) == (k.startswith("b_") or k.startswith("prior")) for k in names)     # the tail = every bias + the prior tables
    staged.load_batch(Xd, None, 0, B)
    done = []
    for stage, (lo, hi) in enumerate(buckets):
        staged.forward_backward_stage(stage, B, ed)
        torch.cuda.synchronize()
        done.append((lo, hi))
        for dlo, dhi in done:      # finished buckets equal the whole-pass gradient already
            assert torch.equal(staged.grad[dlo:dhi], whole.grad[dlo:dhi]), (stage, dlo, dhi)
    assert torch.equal(staged.grad[tlo:thi], whole.grad[tlo:thi])               # the tail is complete behind the last segment
    assert staged.read_state().last_loss == whole.read_state().last_loss
    # two weight-gradient launches instead of three (dmvae_plan_set_stage_groups(2), the two-bucket exchange): segment 0's problems go
    # out with segment 1's, so decoder + heads are complete behind segment 1 -- and not a bit differs
    two = make(kw, dtype, B, seed=2)
    two.set_stage_groups(2)
    two.load_batch(Xd, None, 0, B)
    two.forward_backward_stage(0, B, ed)
    two.forward_backward_stage(1, B, ed)
    torch.cuda.synchronize()
    lo, hi = buckets[1][0], buckets[0][1]
    assert torch.equal(two.grad[lo:hi], whole.grad[lo:hi])
    if dtype == "bf16":       # (bf16 queues the problems; the f32 path launches each GEMM where it is issued)
        assert not torch.equal(two.grad[:lo], whole.grad[:lo])                  # the trunk is still to come
    two.forward_backward_stage(2, B, ed)
    torch.cuda.synchronize()
    assert torch.equal(two.grad, whole.grad)
    whole.update(0.5)
    staged.update(0.5)
    torch.cuda.synchronize()
    assert torch.equal(whole.param, staged.param)


def test_ragged_batch_and_determinism():
    """n_valid < max_batch (the short last batch of an epoch, utils.py:462-463):
    same result as an engine sized exactly; deterministic mode is bit-reproducible."""
    kw = SMALL
    rng = np.random.RandomState(5)
    X = rng.rand(64, 40).astype(np.float32)
    eps = rng.randn(64, 6).astype(np.float32)
    res = []
    for B in (37, 64, 37):
        eng = make(kw, "fp32", B if len(res) != 1 else 64)
        eng.load_batch(torch.as_tensor(X).cuda(), None, 0, 37)
        eng.forward_backward(37, torch.as_tensor(eps[:37]).cuda())
        torch.cuda.synchronize()
        res.append((eng.read_state().last_loss, eng.get_gradients()))
    assert res[0][0] == res[2][0]
    for k in res[0][1]:
        np.testing.assert_array_equal(res[0][1][k], res[2][1][k])
        np.testing.assert_allclose(res[0][1][k], res[1][1][k], rtol=1e-5, atol=1e-7)
    assert res[0][0] == pytest.approx(res[1][0], rel=1e-6)


def test_graph_replay_matches_eager_and_epoch_accounting():
    """HIP-graph replay of the step == the same steps issued eagerly (device
    Philox noise and batch cursor come from the device state)."""
    kw, B, N = dict(input_dim=784, latent_dim=10, n_classes=10), 256, 1024
    data = torch.as_tensor(O.synthetic_images(N, 784, seed=1)).cuda()
    perm = torch.randperm(N, device="cuda", dtype=torch.int64).to(torch.int32)
    out = []
    for use_graph in (False, True):
        eng = make(kw, "bf16", B, deterministic=True, seed=4)
        eng.reset_epoch(N // B, kl_ratio=1.0)
        if use_graph:
            replay = eng.capture_step(data, perm)
            for _ in range(N // B):
                replay()
        else:
            for _ in range(N // B):
                eng.train_step(data, perm, use_state_cursor=True)
        torch.cuda.synchronize()
        st = eng.read_state()
        out.append((st.epoch_loss, st.adam_t, st.batch_cursor, st.noise_step, eng.param.clone()))
    assert out[0][1] == out[1][1] == N // B and out[0][2] == out[1][2] == 0
    assert out[0][3] == out[1][3] == N // B
    assert out[0][0] == out[1][0]
    assert torch.equal(out[0][4], out[1][4])
    assert 100 < out[0][0] < 600          # epoch-mean loss in nats, 784*ln2 = 543 at init


_FIN_FIELDS = ("last_loss", "last_recon", "last_klz", "last_klc", "epoch_loss", "epoch_recon", "epoch_klz", "epoch_klc", "lr_t", "adam_t", "noise_step", "batch_cursor")


def _profiled_rows(L, fn):
    """{profiler row: launches} of the library calls fn makes"""
    rows = (L.ProfRow * 64)()
    L.lib.dmvae_prof_collect(rows, 64)          # drop whatever was recorded before
    L.lib.dmvae_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.lib.dmvae_prof_enable(0)
        n = L.lib.dmvae_prof_collect(rows, 64)
    return {rows[i].name.decode(): int(rows[i].launches) for i in range(n)}


@pytest.mark.parametrize("B", [256, 4096])
def test_step_finalize_placements_leave_the_same_bits(hip, B):
    """step_finalize_block is compiled into five kernels and knob 16 says which one a step runs it in (csrc/step.hip place_riders): 0 a launch
    of its own, 1 the dZ GEMM where its tile carries it, else the output layer's dX, 2 the heads' dX (the streaming kernel), 3 the output
    layer's dX.  Two train steps under each setting, the batch addressed through the device cursor: the state (loss scalars, epoch sums,
    lr_t, the counters, the cursor), the gradient arena (the fused step writes the prior-table sums there), parameters, moments and the bf16
    shadow are bit-identical -- a multiply-add of block 0 contracted in one kernel and not in another would show in last_loss / epoch_*.
    The profiler's step_finalize row: one launch per step with knob 16 = 0, none otherwise.  The same with the 64-row dZ tiles (knob 18 = 0),
    where setting 1 rides in the dZ GEMM itself."""
    kw = dict(input_dim=784, latent_dim=64, n_classes=10)
    X = torch.as_tensor(O.synthetic_images(2 * B, 784, seed=21)).cuda()
    perm = torch.randperm(2 * B, device="cuda").to(torch.int32)
    rng = np.random.RandomState(B)
    eps = [torch.as_tensor(rng.randn(B, 64).astype(np.float32)).cuda() for _ in range(2)]

    def run(knob16):
        hip.check(hip.lib.dmvae_debug_set_knob(16, knob16))
        e = make(kw, "bf16", B, seed=3)
        e.reset_epoch(2, kl_ratio=0.37)

        def steps():
            for ed in eps:
                e.train_step(X, perm, B, ed, None, 0, True)
        rows = _profiled_rows(hip, steps)
        assert rows.get("step_finalize", 0) == (2 if knob16 == 0 else 0), (knob16, rows)
        st = e.read_state()
        assert (st.adam_t, st.noise_step, st.batch_cursor) == (2, 2, 0)
        assert e.grad_view("prior_means").abs().sum().item() > 0          # (written by the step_finalize blocks)
        return {k: getattr(st, k) for k in _FIN_FIELDS}, [getattr(e, n).clone() for n in ("grad", "param", "m", "v", "param_bf16")]

    try:
        for knob18, settings in ((2, (0, 1, 2, 3)), (0, (0, 1))):
            hip.check(hip.lib.dmvae_debug_set_knob(18, knob18))
            ref = None
            for knob16 in settings:
                state, arenas = run(knob16)
                if ref is None:
                    ref = (state, arenas)
                    assert 100 < state["last_loss"] < 700
                    continue
                assert state == ref[0], (B, knob18, knob16, {k: (state[k], ref[0][k]) for k in state if state[k] != ref[0][k]})
                for name, a, b in zip(("grad", "param", "m", "v", "param_bf16"), arenas, ref[1]):
                    assert torch.equal(a, b), (B, knob18, knob16, name, int((a != b).sum().item()))
    finally:
        hip.check(hip.lib.dmvae_debug_set_knob(16, 1))
        hip.check(hip.lib.dmvae_debug_set_knob(18, 2))


_KNOB_DEFAULTS = {1: 1, 17: 1, 18: 2}


@pytest.mark.parametrize("B,knobs", [(256, ()), (4096, ()), (4096, ((17, 0),)), (256, ((1, 0),)), (16384, ()),
                                     (4096, ((18, 0),)), (4096, ((18, 1),)), (4096, ((18, 0), (17, 2))), (4096, ((18, 1), (17, 3))), (1024, ((18, 0), (17, 3)))])
def test_pipelined_capture_equals_the_plain_graph(hip, B, knobs):
    """capture_step's pipelined form (two graphs, each assembling the NEXT batch under its own backward pass: dmvae_plan_prefetch_batch /
    dmvae_plan_swap_batch) against the plain captured step (the gather in front): same loss, parameters, moments, cursor -- over an epoch
    wrap, a reset_epoch in between, an eager step in between, an encode in between (each of which makes the callable assemble the
    cursor's batch itself).  Placements of the prefetched gather: at 256 rows it rides in the dZ GEMM (knob 1 = 0: on the four-wave tiles).
    At 4096 rows with the default THIN dZ tiles (knob 18 = 2: 256 two-wave workgroups of 16 rows) that launch has no room for riders
    (gemm_bf16_riders_room = 0), so the gather is a launch of its own whatever knob 17 says ((4096, ()) and (4096, ((17, 0),)) are the same
    placement); the rider forms of gemm_bf16_dx_riders_kernel on the LATENT tiles are reached with knob 18 = 0 (64-row tiles) / 1 (32-row
    tiles) and knob 17 = 1 (last ids), 2 (first ids), 3 (two blocks per idle CU) -- ADVICE r4.  16 384 rows: the dZ launch is full, the
    gather is a launch of its own in front of the trunk's backward pass."""
    kw = dict(input_dim=784, latent_dim=64, n_classes=10)
    N = 5 * B
    X = torch.as_tensor(O.synthetic_images(min(N, 8192), 784, seed=18)).cuda()
    if N > X.shape[0]: X = X.repeat((N + X.shape[0] - 1) // X.shape[0], 1)[:N].contiguous()
    perm = torch.randperm(N, device="cuda").to(torch.int32)
    try:
        for k, v in knobs:
            hip.check(hip.lib.dmvae_debug_set_knob(k, v))
        plain, pipe = make(kw, "bf16", B, seed=6), make(kw, "bf16", B, seed=6)
        for e in (plain, pipe):
            e.reset_epoch(5)
        rp, rq = plain.capture_step(X, perm, pipelined=False), pipe.capture_step(X, perm, pipelined=True)
        assert len(plain._graph) == 1 and len(pipe._graph) == 2, "the pipelined form was not taken"

        def both(n):
            for _ in range(n):
                rp(); rq()
            torch.cuda.synchronize()
            a, b = plain.read_state(), pipe.read_state()
            assert (a.last_loss, a.epoch_loss, a.batch_cursor, a.adam_t, a.noise_step) == (b.last_loss, b.epoch_loss, b.batch_cursor, b.adam_t, b.noise_step)
            for name in ("param", "m", "v", "param_bf16"):
                assert torch.equal(getattr(plain, name), getattr(pipe, name)), name
        both(7)                                   # wraps the 5-batch epoch: batches 0 1 2 3 4 0 1
        for e in (plain, pipe):
            e.reset_epoch(3)                      # cursor back to 0, another epoch length: the prefetched batch (2) is not the next one
        both(4)
        for e in (plain, pipe):
            e.train_step(X, perm, use_state_cursor=True)     # an eager step between replays
        both(3)
        for e in (plain, pipe):                   # something else uses the batch buffer
            e.load_batch(X[:B].contiguous(), None, 0, B); e.encode(B)
        both(2)
        assert plain.param.abs().sum().item() > 0
    finally:
        for k, v in knobs:
            hip.check(hip.lib.dmvae_debug_set_knob(k, _KNOB_DEFAULTS[k]))


def test_a_batch_loaded_by_explicit_first_takes_repeat_passes(hip):
    """the consumed-batch guard of dmvae_plan_load_batch_step concerns batches addressed by the DEVICE cursor (step_finalize
    advances it under them).  With an explicit `first` a second forward_backward over the same batch is valid -- gradient checks, repeat
    passes -- and gives the same gradients; with the cursor it is refused."""
    kw, B = dict(input_dim=784, latent_dim=64, n_classes=10), 256
    X = torch.as_tensor(O.synthetic_images(2 * B, 784, seed=5)).cuda()
    perm = torch.randperm(2 * B, device="cuda").to(torch.int32)
    eps = torch.randn((B, 64), device="cuda")
    e = make(kw, "bf16", B, seed=2)
    e._load_batch_for_step(X, perm, B, B, False)
    e.forward_backward(B, eps)
    g0, l0 = e.grad.clone(), e.read_state().last_loss
    e.forward_backward(B, eps)                     # same batch, same noise: same bits
    torch.cuda.synchronize()
    assert torch.equal(e.grad, g0) and e.read_state().last_loss == l0
    e.reset_epoch(2)
    e._load_batch_for_step(X, perm, 0, B, True)
    e.forward_backward(B, eps)
    with pytest.raises(Exception, match="consumed by an earlier pass"):
        e.forward_backward(B, eps)


def test_k_slices_of_the_thin_launches_at_small_batches(hip):
    """at <= 256 rows the dense launches with K >= 1024 (here: the 2000 -> 500 decoder layer, 4 slices; the dX of the 500 -> 2 x 2000 head
    hidden layer, K = 4096, 8 slices) are cut into K slices whose partial tiles the last workgroup to arrive adds in a fixed order before the fused
    epilogue (GemmArgs::tick, csrc/gemm_bf16.hip).  Against the unsliced launches (knob 21 = 0): same step up to the f32 summation order -- loss to
    1e-5 relative, gradients to 2e-3 of each tensor's max; two sliced runs bit-identical (no atomics in the sum); HIP-graph replay == eager; the tickets
    are back at zero after every launch (three steps in a row work)."""
    kw, B = dict(input_dim=784, latent_dim=10, n_classes=10), 100
    X = torch.as_tensor(O.synthetic_images(B, 784, seed=2)).cuda()
    eps = torch.as_tensor(np.random.RandomState(3).randn(B, 10).astype(np.float32)).cuda()
    res = {}
    try:
        for name, knob in (("off", 0), ("on", 1), ("on2", 1)):
            hip.check(hip.lib.dmvae_debug_set_knob(21, knob))
            e = make(kw, "bf16", B, seed=9)
            for _ in range(3):
                e.load_batch(X, None, 0, B)
                e.forward_backward(B, eps)
            torch.cuda.synchronize()
            res[name] = (e.read_state().last_loss, e.grad.clone(), {k: v.float().clone() for k, v in e.hidden_activations(B).items()}, e)
        assert res["on"][0] == res["on2"][0] and torch.equal(res["on"][1], res["on2"][1])            # deterministic
        assert abs(res["on"][0] - res["off"][0]) <= 1e-5 * abs(res["off"][0])
        for k in res["off"][2]:
            a, b = res["off"][2][k], res["on"][2][k]
            assert (a - b).abs().max().item() <= 2e-2 * max(1e-6, a.abs().max().item()), k        # bf16 activations: a unit in the last place
        e_off, e_on = res["off"][3], res["on"][3]
        for k in e_off.tensors:
            a, b = e_off.grad_view(k), e_on.grad_view(k)
            assert (a - b).abs().max().item() <= 2e-3 * max(1e-12, a.abs().max().item()), k
        # the captured step replays the same sliced launches (tickets reset inside the graph)
        data = torch.as_tensor(O.synthetic_images(4 * B, 784, seed=5)).cuda()
        perm = torch.randperm(4 * B, device="cuda").to(torch.int32)
        g, h = make(kw, "bf16", B, seed=4), make(kw, "bf16", B, seed=4)
        g.reset_epoch(4); h.reset_epoch(4)
        rp = g.capture_step(data, perm, pipelined=False)
        for _ in range(4):
            rp(); h.train_step(data, perm, use_state_cursor=True)
        torch.cuda.synchronize()
        assert g.read_state().epoch_loss == h.read_state().epoch_loss and torch.equal(g.param, h.param)
    finally:
        hip.check(hip.lib.dmvae_debug_set_knob(21, 1))


def test_k_slices_repeated_passes_stay_identical(hip):
    """The K slices hand partial tiles from one XCD to another inside a kernel (agent-scope stores, a ticket, agent-scope loads: csrc/gemm_bf16.hip,
    csrc/heads_latent.hip).  A visibility fault there -- a slab read before it is complete, a stale line -- would show as a RARE difference: 400 passes over
    the same batch (each running the sliced dense launches, the sliced dZ GEMM and the fused heads + latent launch in eight slices) must give the bits
    of the first one, and so must 200 replays of a captured pass at 256 rows."""
    kw = dict(input_dim=784, latent_dim=10, n_classes=10)
    for B, reps in ((100, 400), (256, 200)):
        X = torch.as_tensor(O.synthetic_images(B, 784, seed=7)).cuda()
        eps = torch.as_tensor(np.random.RandomState(8).randn(B, 10).astype(np.float32)).cuda()
        e = make(kw, "bf16", B, seed=5)
        e.load_batch(X, None, 0, B)
        e.forward_backward(B, eps)
        torch.cuda.synchronize()
        g0, l0, m0 = e.grad.clone(), e.read_state().last_loss, e.view("mean").clone()
        bad = 0
        for i in range(reps):
            e.forward_backward(B, eps)
            if i % 20 == 19 or i == reps - 1:
                torch.cuda.synchronize()
                bad += int(not torch.equal(e.grad, g0)) + int(e.read_state().last_loss != l0) + int(not torch.equal(e.view("mean"), m0))
        assert bad == 0, (B, bad)
    # ... and with the inputs CHANGING from pass to pass (identical passes cannot tell a stale slab from a fresh one): 60 different batches through a
    # sliced and an unsliced engine in turn; a slab line left over from the pass before would be off by far more than a summation order
    B = 100
    try:
        hip.check(hip.lib.dmvae_debug_set_knob(21, 1)); on = make(kw, "bf16", B, seed=5)
        hip.check(hip.lib.dmvae_debug_set_knob(21, 0)); off = make(kw, "bf16", B, seed=5)
        rng = np.random.RandomState(12)
        for i in range(60):
            X = torch.as_tensor((rng.rand(B, 784) * (rng.rand(B, 784) < 0.1 + 0.4 * rng.rand())).astype(np.float32)).cuda()
            eps = torch.as_tensor(rng.randn(B, 10).astype(np.float32)).cuda()
            out = []
            for knob, e in ((1, on), (0, off)):
                hip.check(hip.lib.dmvae_debug_set_knob(21, knob))
                e.load_batch(X, None, 0, B)
                e.forward_backward(B, eps)
                torch.cuda.synchronize()
                out.append((e.read_state().last_loss, e.view("mean").clone(), e.grad_view("W_enc0").clone(), e.grad_view("W_dec1").clone()))
            assert abs(out[0][0] - out[1][0]) <= 1e-5 * abs(out[1][0]), (i, out[0][0], out[1][0])
            for a, b in zip(out[0][1:], out[1][1:]):      # (bf16 activations downstream of another f32 summation order differ by a unit in the last place here and there:
                assert (a - b).abs().max().item() <= 1e-2 * max(1e-9, b.abs().max().item()), i      #  2.5e-3 of a tensor's max seen; a stale slab is off by O(1))
    finally:
        hip.check(hip.lib.dmvae_debug_set_knob(21, 1))


def test_pipelined_capture_is_the_default_for_small_batches_only(monkeypatch):
    """capture_step's default: pipelined up to PIPELINE_MAX_BATCH rows (measured: -2.7 % at 100 rows, -1.7 % at 2048, nothing at 4096), DMVAE_PREFETCH=0 / 1 forces"""
    from dmvae_hip import runtime
    kw = dict(input_dim=784, latent_dim=64, n_classes=10)
    monkeypatch.delenv("DMVAE_PREFETCH", raising=False)
    for B, want in ((256, 2), (runtime.PIPELINE_MAX_BATCH, 2), (4096, 1)):
        X = torch.rand((2 * B, 784), device="cuda")
        perm = torch.randperm(2 * B, device="cuda").to(torch.int32)
        e = make(kw, "bf16", B, seed=1); e.reset_epoch(2)
        e.capture_step(X, perm)
        assert len(e._graph) == want, B
    monkeypatch.setenv("DMVAE_PREFETCH", "0")
    e = make(kw, "bf16", 256, seed=1); e.reset_epoch(2)
    X = torch.rand((512, 784), device="cuda"); perm = torch.randperm(512, device="cuda").to(torch.int32)
    e.capture_step(X, perm)
    assert len(e._graph) == 1
    monkeypatch.setenv("DMVAE_PREFETCH", "1")
    e = make(kw, "bf16", 4096, seed=1); e.reset_epoch(2)
    X = torch.rand((8192, 784), device="cuda"); perm = torch.randperm(8192, device="cuda").to(torch.int32)
    e.capture_step(X, perm)
    assert len(e._graph) == 2


def test_prefetch_refused_where_the_plan_cannot(hip):
    """fp32 plans keep the f32 copy of the batch (dmvae_plan_load_batch): no prefetch; a swap without a pass behind the prefetch is refused"""
    kw = dict(input_dim=784, latent_dim=64, n_classes=10)
    X = torch.as_tensor(O.synthetic_images(512, 784, seed=3)).cuda()
    f = make(kw, "fp32", 256, seed=1)
    f._load_batch_for_step(X, None, 0, 256)
    assert hip.lib.dmvae_plan_prefetch_batch(f._plan, hip.ptr(X), 512, None, 256, 256, 0) == hip.EUNSUPPORTED
    rp = f.capture_step(X, None)                  # falls back to the plain graph
    assert len(f._graph) == 1
    b = make(kw, "bf16", 256, seed=1)
    with pytest.raises(Exception, match="no current batch"):
        b._prefetch_batch(X, None, 256, 256, False)
    b._load_batch_for_step(X, None, 0, 256)
    b._prefetch_batch(X, None, 256, 256, False)
    assert hip.lib.dmvae_plan_swap_batch(b._plan) != 0        # nothing has run since
    # explicit `first` (no device cursor), eager: prefetch -> step -> swap -> step == load -> step -> load -> step
    ref = make(kw, "bf16", 256, seed=1)
    b.forward_backward_update(256); hip.check(hip.lib.dmvae_plan_swap_batch(b._plan)); b.forward_backward_update(256)
    ref.train_step(X, None, 256, None, None, 0, False); ref.train_step(X, None, 256, None, None, 256, False)
    torch.cuda.synchronize()
    assert b.read_state().last_loss == ref.read_state().last_loss and torch.equal(b.param, ref.param)


def test_encode_decode_views():
    kw, B = dict(input_dim=784, latent_dim=10, n_classes=10), 100
    eng = make(kw, "fp32", B)
    cfg = oracle_cfg(kw)
    p = {k: v.astype(np.float64) for k, v in eng.get_parameters().items()}
    X = O.synthetic_images(B, 784, seed=2)
    eng.load_batch(torch.as_tensor(X).cuda(), None, 0, B)
    eng.encode(B)
    a = O.encode(p, cfg, X.astype(np.float64))
    np.testing.assert_allclose(eng.view("mean", B).cpu().numpy(), a["mean"], atol=2e-5)
    np.testing.assert_allclose(eng.view("log_var", B).cpu().numpy(), a["logvar"], atol=2e-5)
    np.testing.assert_allclose(eng.view("logits", B).cpu().numpy(), a["logits"], atol=2e-5)
    Z = np.random.RandomState(0).randn(B, 10).astype(np.float32)
    eng.decode(torch.as_tensor(Z).cuda())
    xl = O.decode(p, cfg, Z.astype(np.float64))["xlogits"]
    np.testing.assert_allclose(eng.view("recon", B).cpu().numpy(), 1 / (1 + np.exp(-xl)), atol=2e-5)


def _dp_rank(rank, world, port, overlap, out, mode="allreduce", dtype="fp32"):
    """one data-parallel rank on the shared GPU (gloo carries the collectives in this rehearsal)"""
    import torch.distributed as dist
    for p in (os.path.join(ROOT, "deep-mixture-vae_amd"), os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      DMVAE_DP_OVERLAP="1" if overlap else "0", DMVAE_DP_MODE=mode, DMVAE_DP_BUCKETS="2" if overlap == 2 else "3")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import dmvae_oracle as Or
    from dmvae_hip import StepEngine, make_exchange, shard_range
    kw, B = dict(input_dim=784, latent_dim=64, n_classes=10), 256
    rng = np.random.RandomState(21)
    X = Or.synthetic_images(B, 784, seed=8)
    lo, hi = shard_range(B, rank, world)
    eng = StepEngine(dtype=dtype, max_batch=hi - lo, mode="exact", **kw)
    eng.init_parameters(3)
    ex = make_exchange()
    assert ex.enabled and ex.overlap == bool(overlap) and ex.sharded == (mode == "sharded") and ex.n_buckets == (2 if overlap == 2 else 3)
    Xd = torch.as_tensor(X[lo:hi]).cuda()
    for step in range(2):
        eps = rng.randn(B, 64).astype(np.float32)
        ed = torch.as_tensor(eps[lo:hi]).cuda()
        eng.train_step(Xd, None, hi - lo, ed, None, grad_sync=ex, grad_scale=ex.grad_scale, inv_B=world / float(B))
    torch.cuda.synchronize()
    if dtype == "bf16":      # bf16 plans: the sharded exchange gathers the bf16 SHADOW; the fp32 weights outside the owned slice are stale until sync_master
        before = eng.param.cpu().numpy()
        stale = bool(getattr(eng, "_master_stale", False))
        eng.sync_master(ex)                  # collective
        out.put((rank, eng.param.cpu().numpy(), eng.read_state().adam_t, eng.m.cpu().numpy(), eng.param_bf16.float().cpu().numpy(), before, stale,
                 eng.grad_buckets()[1][0]))
    else:
        out.put((rank, eng.param.cpu().numpy(), eng.read_state().adam_t, eng.m.cpu().numpy()))
    dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [True, 2, False])      # three buckets / two buckets (decoder + heads | trunk) / one collective pair
def test_sharded_exchange_equals_allreduce_bit_for_bit(overlap):
    """reduce-scatter -> Adam on the owned slice -> all-gather leaves, on every rank, exactly the parameters that
    all-reduce + replicated Adam leaves (two ranks: a + b is the same float either way); the Adam moments are
    maintained on the owned slice only and equal the replicated ones there."""
    import socket
    import torch.multiprocessing as mp
    res = {}
    for mode in ("allreduce", "sharded"):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        ctx = mp.get_context("spawn")
        out = ctx.Queue()
        procs = [ctx.Process(target=_dp_rank, args=(r, 2, port, overlap, out, mode)) for r in range(2)]
        for p in procs:
            p.start()
        res[mode] = sorted([out.get(timeout=300) for _ in procs], key=lambda t: t[0])
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    ar, sh = res["allreduce"], res["sharded"]
    np.testing.assert_array_equal(sh[0][1], sh[1][1])            # replicas identical after the all-gather
    np.testing.assert_array_equal(sh[0][1], ar[0][1])            # and equal to the replicated update
    n = ar[0][3].size
    owned_somewhere = np.zeros(n, bool)
    for r in range(2):
        touched = sh[r][3] != 0
        np.testing.assert_array_equal(sh[r][3][touched], ar[r][3][touched])    # m on the slices this rank updated
        owned_somewhere |= touched
    assert (owned_somewhere | (ar[0][3] == 0)).all()             # every parameter with a gradient is owned by some rank
    assert (sh[0][3] != 0).sum() < 0.75 * (ar[0][3] != 0).sum()  # ... and a rank does not maintain the others' moments


@pytest.mark.parametrize("overlap", [True, 2, False])      # three buckets / two buckets (decoder + heads | trunk) / one collective pair
def test_sharded_exchange_gathers_the_bf16_shadow(overlap):
    """bf16 plans (VERDICT r2 next #5 iv): reduce-scatter -> Adam on the owned weight slice -> all-gather of the bf16
    SHADOW (2 B per parameter), the tail (biases, prior tables) all-reduced and updated on every rank.  After two steps on two ranks:
    every bit a step READS -- the shadow of the weights, the fp32 tail -- is identical on both ranks and equal to what all-reduce +
    replicated Adam leaves; a rank's fp32 weights outside its slice are stale (that is what proves the fp32 master was not sent) until
    sync_master(), after which the fp32 arenas are those of the replicated run too."""
    import socket
    import torch.multiprocessing as mp
    res = {}
    for mode in ("allreduce", "sharded"):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        ctx = mp.get_context("spawn")
        out = ctx.Queue()
        procs = [ctx.Process(target=_dp_rank, args=(r, 2, port, overlap, out, mode, "bf16")) for r in range(2)]
        for p in procs:
            p.start()
        res[mode] = sorted([out.get(timeout=300) for _ in procs], key=lambda t: t[0])
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    ar, sh = res["allreduce"], res["sharded"]
    tlo = sh[0][7]
    for r in range(2):
        np.testing.assert_array_equal(sh[r][4], ar[0][4])            # the shadow the GEMMs read: same bits as the replicated run, on both ranks
        np.testing.assert_array_equal(sh[r][5][tlo:], ar[0][1][tlo:])  # the fp32 tail (biases, prior tables), before any sync
        np.testing.assert_array_equal(sh[r][1], ar[0][1])            # after sync_master: the whole fp32 arena
        assert sh[r][6] and not ar[r][6]                             # the sharded bf16 step marked the master stale; the replicated one never does
    final = ar[0][1][:tlo]
    cur = [sh[r][5][:tlo] == final for r in range(2)]                 # before the sync: where a rank's fp32 weights are current
    assert (cur[0] | cur[1]).all()                                   # every weight is current on the rank that owns it ...
    for r in range(2):
        assert 0.3 < 1.0 - cur[r].mean() < 0.55, cur[r].mean()       # ... and a rank's copy of the other's slices was NOT refreshed (two Adam steps
                                                                     # move nearly every real weight; pad elements stay 0 everywhere)


@pytest.mark.parametrize("overlap", [True, 2, False])      # three buckets / two buckets (decoder + heads | trunk) / one collective pair
def test_two_ranks_equal_one_rank_to_fp32_roundoff(overlap):
    """N ranks x B/N == 1 rank x B.  Two processes share the GPU (gloo carries the
    all-reduce here; RCCL on the multi-GPU box), each runs the real kernels on its half of the batch
    with local mean and the bucketed / single exchange; parameters after two steps match the
    single-process full-batch run to fp32 round-off."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_dp_rank, args=(r, 2, port, overlap, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([out.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[0][2] == res[1][2] == 2
    np.testing.assert_array_equal(res[0][1], res[1][1])          # replicas stay identical
    kw, B = dict(input_dim=784, latent_dim=64, n_classes=10), 256
    rng = np.random.RandomState(21)
    X = O.synthetic_images(B, 784, seed=8)
    one = make(kw, "fp32", B, seed=3)
    Xd = torch.as_tensor(X).cuda()
    for step in range(2):
        ed = torch.as_tensor(rng.randn(B, 64).astype(np.float32)).cuda()
        one.train_step(Xd, None, B, ed, None)
    torch.cuda.synchronize()
    ref = one.param.cpu().numpy()
    d = np.abs(res[0][1][:ref.size] - ref)          # (the two-rank arenas are padded to 64 * world elements)
    # Adam moves every parameter by ~lr = 2e-3 per step; a round-off difference in a gradient near zero
    # can flip a sign of m/sqrt(v) only where |g| ~ 1e-9, so compare the bulk tightly and the tail loosely
    assert np.percentile(d, 99.9) <= 2e-6, np.percentile(d, 99.9)
    assert d.max() <= 4.1e-3


def _rccl_rank(port, overlap, out, mode="allreduce"):
    """a world of ONE rank on RCCL: every collective of the data-parallel step is the real library
    call (an identity), on the streams and buffers the N > 1 job uses"""
    import torch.distributed as dist
    p = os.path.join(ROOT, "deep-mixture-vae_amd")
    if p not in sys.path:
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
                      DMVAE_DP_FORCE="1", DMVAE_DP_OVERLAP="1" if overlap else "0", DMVAE_DP_MODE=mode, DMVAE_DP_BUCKETS="2" if overlap == 2 else "3")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from dmvae_hip import StepEngine, make_exchange
    kw, B = dict(input_dim=784, latent_dim=64, n_classes=10), 512
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    data = torch.rand((4 * B, 784), device="cuda", generator=g)
    perm = torch.randperm(4 * B, device="cuda", generator=g).to(torch.int32)
    ex = make_exchange()
    assert ex.enabled and ex.world == 1 and ex.overlap == bool(overlap) and ex.sharded == (mode == "sharded")
    res = []
    for sync in (ex, None):
        eng = StepEngine(dtype="bf16", max_batch=B, mode="exact", seed=77, **kw)
        eng.init_parameters(3)
        ex.broadcast_(eng.param)
        eng.refresh_shadow()
        eng.reset_epoch(4, kl_ratio=1.0)
        step = eng.capture_step(data, perm, grad_sync=sync, grad_scale=1.0)
        for _ in range(4):
            step()
        torch.cuda.synchronize()
        res.append((eng.param.cpu().numpy(), eng.read_state().adam_t, eng.read_state().epoch_loss))
    out.put(res)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["sharded", "allreduce"])
@pytest.mark.parametrize("overlap", [True, 2, False])      # three buckets / two buckets (decoder + heads | trunk) / one collective pair
def test_rccl_exchange_on_one_rank_is_the_identity(overlap, mode):
    """The N > 1 step sequence (staged backward, bucketed asynchronous collectives on RCCL's stream -- reduce-scatter /
    all-gather or all-reduce --, per-bucket Adam) with a one-rank communicator must reproduce the single-process
    fused step bit for bit: the collectives are identities, so any difference is a stream-ordering or
    bucket-coverage fault in the data-parallel path."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    proc = ctx.Process(target=_rccl_rank, args=(port, overlap, out, mode))
    proc.start()
    (p_dp, t_dp, l_dp), (p_one, t_one, l_one) = out.get(timeout=300)
    proc.join(60)
    assert proc.exitcode == 0
    assert t_dp == t_one == 4
    assert l_dp == l_one
    np.testing.assert_array_equal(p_dp, p_one)


def test_deep_stack_more_than_sixteen_weight_gradients():
    """8 + 8 layers give 20 dW problems: more than one grouped launch holds (16).  The queue is then
    launched early; fused, plain and staged backward must still agree bit for bit, and the bf16
    gradients must track the fp32 engine."""
    kw = dict(input_dim=96, latent_dim=8, n_classes=4, enc_layers=(64,) * 8, head_dim=64, dec_layers=(64,) * 8)
    B = 128
    rng = np.random.RandomState(31)
    Xd = torch.as_tensor((rng.rand(B, 96) * (rng.rand(B, 96) < 0.4)).astype(np.float32)).cuda()
    ed = torch.as_tensor(rng.randn(B, 8).astype(np.float32)).cuda()
    plain, fused, staged, ref = (make(kw, dt, B, seed=5) for dt in ("bf16", "bf16", "bf16", "fp32"))
    for eng in (plain, staged, ref, fused):
        eng.load_batch(Xd, None, 0, B)
    plain.forward_backward(B, ed)
    ref.forward_backward(B, ed)
    for stage in range(3):
        staged.forward_backward_stage(stage, B, ed)
    torch.cuda.synchronize()
    assert torch.equal(plain.grad, staged.grad)
    gp, gr = plain.get_gradients(), ref.get_gradients()
    assert len([k for k in gp if k.startswith("W_")]) == 8 + 5 + 8 + 1     # 20 GEMM problems: [zh|ch] and [mean|log_var] are fused pairs
    for k in gp:
        rel = np.linalg.norm(gp[k] - gr[k]) / (np.linalg.norm(gr[k]) + 1e-30)
        assert rel <= 0.15, (k, rel)          # bf16 through 18 layers
    plain.update(1.0)
    fused.forward_backward_update(B, ed)
    torch.cuda.synchronize()
    for name in ("param", "m", "v", "param_bf16"):
        assert torch.equal(getattr(plain, name), getattr(fused, name)), name


def _captured_dp_rank(rank, world, port, out):
    """bench.py's and train_op's multi-rank form: capture_step (warm-up steps, state restored, then the eager data-parallel step callable)
    under the sharded bf16 exchange, device noise, batch cursor in the device state"""
    import torch.distributed as dist
    for p in (os.path.join(ROOT, "deep-mixture-vae_amd"), os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), DMVAE_DP_MODE="sharded", DMVAE_DP_OVERLAP="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dmvae_hip import StepEngine, make_exchange
    kw, B = dict(input_dim=784, latent_dim=64, n_classes=10), 256
    g = torch.Generator(device="cuda"); g.manual_seed(5 + rank)
    data = torch.rand((4 * B, 784), device="cuda", generator=g)
    perm = torch.randperm(4 * B, device="cuda", generator=g).to(torch.int32)
    eng = StepEngine(dtype="bf16", max_batch=B, mode="exact", seed=77 + rank, **kw)
    eng.init_parameters(3)
    ex = make_exchange(4 * eng.param.numel())
    assert ex.enabled and ex.sharded and ex.world == world
    p0 = eng.param.clone()
    eng.reset_epoch(4, kl_ratio=1.0)
    step = eng.capture_step(data, perm, grad_sync=ex, grad_scale=ex.grad_scale)      # (raised in refresh_shadow before the fix)
    assert torch.equal(eng.param, p0) and not eng._master_stale                           # the warm-up steps left no trace
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    stale = bool(eng._master_stale)
    refused = False
    try:
        eng.get_parameters()
    except RuntimeError:
        refused = True
    eng.sync_master(ex)                        # collective
    params = eng.get_parameters()
    out.put((rank, stale, refused, eng.param.cpu().numpy(), eng.param_bf16.float().cpu().numpy(), eng.read_state().adam_t,
             bool(all(np.isfinite(v).all() for v in params.values()))))
    dist.destroy_process_group()


def test_captured_step_under_the_sharded_exchange_two_ranks():
    """capture_step + sharded bf16 exchange + world 2 -- the path `bench.py --gpus N` and `train_op` take on a node.  Round 4's stale-master
    guard made capture_step's own refresh_shadow refuse after its warm-up steps, so every multi-rank run died before its
    first step; no test took this path (the one-rank RCCL test has nothing stale, the two-rank tests step without capture).  Here: it
    captures, three steps run, the replicas agree in every bit a step reads and -- after sync_master -- in the fp32 master; before the
    sync the master IS stale and get_parameters refuses."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_captured_dp_rank, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([out.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in res:
        assert r[1] and r[2] and r[5] == 3 and r[6], r[:3] + r[5:]      # stale before the sync, get_parameters refused, three Adam steps, finite
    np.testing.assert_array_equal(res[0][4], res[1][4])                  # the bf16 shadow: identical on both ranks
    np.testing.assert_array_equal(res[0][3], res[1][3])                  # the fp32 master after sync_master
