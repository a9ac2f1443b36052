"""GPU tests of the semi-supervised label stage inside the step plan (dmvae_plan_attach_labels; csrc/step.hip: label_stage), on a small
stack: I = 20, one 16-wide trunk layer, head 8, D = 3, K = 4, batches of up to 8 rows, host-supplied eps so that passes are comparable.

  a. attached at w = 0 against an un-attached plan (f32): the gradient arenas are bit-identical, and the profiling entry shows the attached
     pass as the un-attached one plus the one "label_xent" launch.
  b. w > 0 against w = 0 on the same batch (f32 exact and relaxed, bf16): every tensor the term has no path to -- decoder, output layer, z-head,
     prior tables -- is bit-identical; the difference of the c-head bias gradient is sum_r w inv_B (q_r - onehot) of the oracle on the "logits"
     view under the f32 bar of test_gpu_moe_head.py (bf16: dlogits itself within one bf16 ulp on top of it); the accumulators match the oracle.
  c. labels read through the device cursor are the labels of an explicit offset (test_gpu_moe_head.py's case e).
  d. a short batch behind a full one leaves nothing of the full one.
  e. three captured replays equal three eager steps in every parameter's bits (f32: the plain graph; bf16: the pipelined pair of graphs
     with prefetched batches), and writing w = 0 into "label_ctl" between replays takes effect without recapture.
  f. the conv trunk takes the attachment; VaDE plans and plans with a MoE attachment return DMVAE_EUNSUPPORTED."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import label_xent_oracle as LO      # noqa: E402
import moe_cases as MC              # noqa: E402

pytestmark = pytest.mark.gpu

f64 = np.float64
SMALL = dict(input_dim=20, enc_layers=(16,), head_dim=8, dec_layers=(16,), latent_dim=3, n_classes=4)
I, D, K, B, N_DATA = 20, 3, 4, 8, 24
NO_PATH = ("W_dec", "b_dec", "W_out", "b_out", "W_mean", "b_mean", "W_logvar", "b_logvar", "W_zh", "b_zh", "prior_")


@pytest.fixture(scope="module")
def data():
    rng = np.random.RandomState(3)
    X = (rng.rand(N_DATA, I) * (rng.rand(N_DATA, I) < 0.5)).astype(np.float32)
    labels = np.where(rng.rand(N_DATA) < 0.6, rng.randint(0, K, N_DATA), -1).astype(np.int32)
    perm = rng.permutation(N_DATA).astype(np.int32)
    labels[perm[:2]] = (0, K - 1)                        # the first batch holds labels whatever the draw
    eps = rng.randn(B, D).astype(np.float32)
    gum = -np.log(-np.log(rng.uniform(1e-6, 1.0 - 1e-6, (B, K)))).astype(np.float32)
    return dict(X=X, labels=labels, perm=perm, eps=eps, gum=gum,
                Xd=torch.as_tensor(X).cuda(), permd=torch.as_tensor(perm).cuda(), labd=torch.as_tensor(labels).cuda())


def make(data, dtype="fp32", mode="exact", attached=True, **kw):
    from dmvae_hip import StepEngine
    eng = StepEngine(dtype=dtype, max_batch=B, mode=mode, deterministic=True, labels=data["labd"] if attached else None, **dict(SMALL, **kw))
    eng.init_parameters(5)
    eng.write_state(lr=0.002, kl_ratio=0.7)
    pr = eng.get_parameters()
    pr["b_logits"] = (np.random.RandomState(8).randn(*pr["b_logits"].shape) * 0.5).astype(np.float32)     # q away from uniform
    eng.set_parameters(pr)
    return eng


def one_pass(eng, data, n, first=0, w=None):
    if w is not None:
        eng.set_label_weight(w)
        eng.zero_label_acc()
    eng.load_batch(data["Xd"], data["permd"], first, n)
    gum = torch.as_tensor(data["gum"][:n]).cuda().contiguous() if eng.mode == 1 else None
    eng.forward_backward(n, torch.as_tensor(data["eps"][:n]).cuda().contiguous(), gum)
    torch.cuda.synchronize()


def host(t):
    return t.float().cpu().numpy().astype(f64)


def test_attached_at_zero_weight_is_the_unattached_plan(data):
    from dmvae_hip import runtime
    plain, att = make(data, attached=False), make(data)
    assert att.sizes.param_elems == plain.sizes.param_elems and att.sizes.work_bytes > plain.sizes.work_bytes
    rows = []
    try:
        runtime.prof_enable(True)
        runtime.prof_collect(256)
        for eng in (plain, att):
            one_pass(eng, data, 6, w=0.0 if eng is att else None)
            rows.append([(r["name"], r["launches"], r["kernel_launches"]) for r in runtime.prof_collect(256)])
    finally:
        runtime.prof_enable(False)
        runtime.prof_collect(256)
    assert torch.equal(plain.grad, att.grad) and bool(plain.grad.any())
    assert plain.read_state().last_loss == att.read_state().last_loss
    extra = [r for r in rows[1] if r[0] == "label_xent"]
    assert extra == [("label_xent", 1, 1)] and [r for r in rows[1] if r[0] != "label_xent"] == rows[0]
    acc = att.label_acc()
    n_lab = int((data["labels"][data["perm"][:6]] >= 0).sum())
    assert acc[4] == n_lab >= 2 and acc[3] > 0 and att.label_err() == 0          # the loss is measured at w = 0 too


@pytest.mark.parametrize("dtype,mode", [("fp32", "exact"), ("fp32", "relaxed"), ("bf16", "exact"), ("bf16", "relaxed")])
def test_weighted_against_unweighted_on_the_same_batch(data, dtype, mode):
    n, w = 6, 2.5
    eng = make(data, dtype, mode)
    one_pass(eng, data, n, w=0.0)
    g0, dl0, lg0 = eng.get_gradients(), eng.view("dlogits", eng.batch_pad, 1 << 30).clone(), host(eng.view("logits", n))
    one_pass(eng, data, n, w=w)
    g1, dl1, lg1 = eng.get_gradients(), eng.view("dlogits", eng.batch_pad, 1 << 30).clone(), host(eng.view("logits", n))
    assert np.array_equal(lg0, lg1)
    y = LO.batch_labels(data["labels"], data["perm"], 0, n)
    coef = LO.coefficient(w, np.float32(1.0 / n))
    o, y32 = LO.term(lg1, y, coef), LO.term_f32(lg1, y, coef)
    lab = o["labelled"]
    assert lab.sum() >= 2
    # no path leads there
    for k in g0:
        if k.startswith(NO_PATH):
            assert np.array_equal(g0[k], g1[k]), k
    assert not np.array_equal(g0["b_logits"], g1["b_logits"]) and not np.array_equal(g0["W_enc0"], g1["W_enc0"])
    # dlogits: untouched outside the labelled rows' K columns, the term inside
    keep = torch.ones_like(dl0, dtype=torch.bool)
    keep[:n, :K] = torch.as_tensor(~lab).cuda()[:, None]
    assert torch.equal(dl0[keep], dl1[keep])
    want = host(dl0[:n, :K]) + o["d"]
    yard = (host(dl0[:n, :K]).astype(np.float32) + y32["d"]).astype(f64)
    rtol, atol = MC.tolerance("dlogits", want[lab], yard[lab])
    e = np.abs(host(dl1[:n, :K]) - want)[lab]
    lim = atol + rtol * np.abs(want[lab]) + (MC.bf16_ulp(want[lab]) if dtype == "bf16" else 0.0)
    assert np.all(e <= lim), (float(e.max()), float(lim.min()))
    if dtype == "fp32":
        # the c-head's bias gradient is the column sum of dlogits: its difference is the column sum of the term
        ref, yref = o["d"].sum(0), y32["d"].astype(f64).sum(0)
        rtol, atol = MC.tolerance("dlogits", ref, yref)
        got = g1["b_logits"].astype(f64) - g0["b_logits"].astype(f64)
        print("label step %s b_logits difference error %.3e atol %.3e max|ref| %.3e" % (mode, np.abs(got - ref).max(), atol, np.abs(ref).max()))
        assert np.all(np.abs(got - ref) <= atol + rtol * np.abs(ref)), (got, ref)
    acc = eng.label_acc()
    rtol, atol = MC.tolerance("loss", o["loss"], float(y32["loss_rows"].astype(f64).sum()))
    assert abs(acc[3] - o["loss"]) <= atol + rtol * abs(o["loss"]) and (acc[4], acc[5]) == (o["n_labelled"], o["n_correct"])
    assert np.array_equal(acc[:3], acc[3:]) and eng.label_err() == 0


def test_labels_through_the_device_cursor(data):
    nb = N_DATA // B
    A, E = make(data), make(data)
    for eng in (A, E):
        eng.reset_epoch(nb)
        eng.set_label_weight(1.5)
        eng.zero_label_acc()
    rng = np.random.RandomState(10)
    seen = 0
    for step in range(nb):
        eps = torch.as_tensor(rng.randn(B, D).astype(np.float32)).cuda()
        A.train_step(data["Xd"], data["permd"], None, eps, first=0, use_state_cursor=True)
        E.train_step(data["Xd"], data["permd"], B, eps, first=step * B)
        torch.cuda.synchronize()
        seen += int((LO.batch_labels(data["labels"], data["perm"], step * B, B) >= 0).sum())
        assert A.label_acc().tobytes() == E.label_acc().tobytes(), step
        assert A.label_acc()[1] == seen and torch.equal(A.param, E.param), step
    assert seen == int((data["labels"] >= 0).sum()) and A.label_err() == 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_short_batch_behind_a_full_one(data, dtype):
    out = []
    for passes in ((8, 5), (5,)):
        eng = make(data, dtype)
        eng.set_label_weight(2.0)
        for m in passes:
            one_pass(eng, data, m)
        out.append((eng.grad.clone(), eng.label_acc()[3:], eng.view("dlogits", eng.batch_pad, 1 << 30).clone()))
    (ga, aa, da), (gb, ab, db) = out
    assert torch.equal(ga, gb) and np.array_equal(aa, ab) and torch.equal(da, db) and not bool(da[5:].any())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_captured_replays_equal_eager_steps_and_follow_the_weight(data, dtype):
    nb = N_DATA // B
    schedule = (2.0, 2.0, 2.0, 0.0, 2.0, 0.0)
    out = []
    for use_graph in (False, True):
        eng = make(data, dtype)
        eng.reset_epoch(nb, kl_ratio=1.0)
        eng.set_label_weight(schedule[0])
        replay = eng.capture_step(data["Xd"], data["permd"]) if use_graph else None
        eng.reset_epoch(nb, kl_ratio=1.0)
        eng.zero_label_acc()
        snaps = []
        for w in schedule:
            eng.set_label_weight(w)
            if use_graph:
                replay()
            else:
                eng.train_step(data["Xd"], data["permd"], use_state_cursor=True)
            torch.cuda.synchronize()
            snaps.append((eng.param.clone(), eng.label_acc().copy()))
        out.append(snaps)
        assert eng.label_err() == 0
    for step, ((pa, aa), (pb, ab)) in enumerate(zip(*out)):
        assert torch.equal(pa, pb), step                 # three replays = three eager steps, then the w = 0 steps without recapture
        assert aa.tobytes() == ab.tobytes(), step
    # the weight is read, not baked in: the same six steps at a constant weight end elsewhere
    eng = make(data, dtype)
    eng.reset_epoch(nb, kl_ratio=1.0)
    eng.set_label_weight(2.0)
    for _ in schedule:
        eng.train_step(data["Xd"], data["permd"], use_state_cursor=True)
    torch.cuda.synchronize()
    assert not torch.equal(eng.param, out[0][-1][0])


def test_staged_backward_equals_the_whole_pass(data):
    whole, staged = make(data), make(data)
    for eng in (whole, staged):
        eng.set_label_weight(2.0)
        eng.zero_label_acc()
        eng.load_batch(data["Xd"], data["permd"], 0, 6)
    eps = torch.as_tensor(data["eps"][:6]).cuda().contiguous()
    whole.forward_backward(6, eps)
    for stage in (0, 1, 2):
        staged.forward_backward_stage(stage, 6, eps)
    torch.cuda.synchronize()
    assert torch.equal(whole.grad, staged.grad) and whole.label_acc().tobytes() == staged.label_acc().tobytes()


def test_conv_trunk_takes_the_attachment():
    from dmvae_hip import StepEngine
    rng = np.random.RandomState(4)
    n = 5
    X = torch.as_tensor(rng.rand(16, 784).astype(np.float32)).cuda()
    labels = torch.as_tensor(rng.randint(0, 10, 16).astype(np.int32)).cuda()
    eps = torch.as_tensor(rng.randn(n, 10).astype(np.float32)).cuda()
    grads = []
    for w in (0.0, 3.0):
        eng = StepEngine(784, 10, 10, enc_layers=(500,), dtype="fp32", max_batch=8, deterministic=True, cnn=True, labels=labels)
        eng.init_parameters(2)
        eng.set_label_weight(w)
        eng.load_batch(X, None, 3, n)
        eng.forward_backward(n, eps)
        torch.cuda.synchronize()
        grads.append(eng.get_gradients())
        acc = eng.label_acc()
        assert acc[4] == n and eng.label_err() == 0
    lg = host(eng.view("logits", n))
    o = LO.term(lg, labels.cpu().numpy()[3:3 + n], LO.coefficient(3.0, np.float32(1.0 / n)))
    y32 = LO.term_f32(lg, labels.cpu().numpy()[3:3 + n], LO.coefficient(3.0, np.float32(1.0 / n)))
    ref = o["d"].sum(0)
    rtol, atol = MC.tolerance("dlogits", ref, y32["d"].astype(f64).sum(0))
    got = grads[1]["b_logits"].astype(f64) - grads[0]["b_logits"].astype(f64)
    assert np.all(np.abs(got - ref) <= atol + rtol * np.abs(ref)), (got, ref)
    assert np.array_equal(grads[0]["W_out"], grads[1]["W_out"]) and not np.array_equal(grads[0]["W_enc0"], grads[1]["W_enc0"])
    changed = [k for k in grads[0] if not np.array_equal(grads[0][k], grads[1][k])]
    assert any("conv" in k for k in changed), changed   # the term reaches the convolutions through the trunk's backward


def test_vade_and_moe_plans_refuse(data):
    from dmvae_hip import StepEngine
    from dmvae_hip._lib import DmvaeError
    with pytest.raises(DmvaeError, match=r"dmvae_plan_attach_labels failed \(code -2\).*VaDE"):
        StepEngine(I, D, K, enc_layers=(16,), head_dim=64, dec_layers=(16,), dtype="fp32", max_batch=B, model="vade", labels=data["labd"])
    Y = torch.zeros((N_DATA, 2), dtype=torch.float32, device="cuda")
    moe = dict(n_experts=K, output_dim=2, featLearn=0, classification=1, lossVAE=1, labels=Y)
    with pytest.raises(DmvaeError, match=r"dmvae_plan_attach_labels failed \(code -2\).*MoE"):
        StepEngine(dtype="fp32", max_batch=B, moe=moe, labels=data["labd"], **SMALL)
    plain = make(data, attached=False)
    with pytest.raises(RuntimeError):
        plain.set_label_weight(1.0)
