"""GPU tests of the mixture-of-experts row stage (csrc/moe_head.hip: moe_head_kernel), forward AND backward, at every width at which the kernel
takes another path, in the mild and in the trained regime (tests/helpers/moe_cases.py), per element:

  a. fp32, lossVAE = 0 (the VAE's share of dlogits and gmu is then exactly zero: the "dlogits" and "gmu" views hold the head's terms alone): the
     head's real inputs -- the "logits", "mean" and "moe_P" views -- are read back and given to the float64 oracle and to the float32 yardstick
     (moe_oracle.head_f32); prediction, dP, dlogits, gmu, loss and error against the oracle under tolerance(): the project's bars, the absolute
     part raised to twice the yardstick's own error where that is larger.  Prints error / yardstick error per output (pytest -s).
  b. bf16: the weight-gradient operand "moe_dP" is the round-to-nearest-even of the f32 dP bit for bit, zero in the padding; dlogits within one
     bf16 ulp; the W_moe / b_moe gradients are the float64 product / column sum of the plan's own bf16 operands up to f32 accumulation.
  c. a short batch behind a full one leaves nothing of the full one in any gradient.
  d. lossVAE = 0 on trained inputs (dq ~ 1e21 next to gate weights that are 0.0f): exact zeros where the VAE alone would act, no NaN anywhere.
  e. labels read through the device cursor are the labels of an explicit offset.

CPU side of the same cases: tests/test_moe_host.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import dmvae_oracle as O      # noqa: E402
import moe_cases as MC        # noqa: E402
import moe_oracle as MO       # noqa: E402
from test_gpu_moe import make     # noqa: E402

pytestmark = pytest.mark.gpu

f64 = np.float64
CASES_A = [(s, k, c, f) for s in MC.SHAPES for k in MC.KINDS for c in (1, 0) for f in (0, 1)]
BF16_SHAPES = ((40, 17, 33), (16, 64, 24), (256, 4, 4))
CASES_B = [(s, k, c, f) for s in BF16_SHAPES for k in MC.KINDS for c in (1, 0) for f in (0, 1)]
VAE_ONLY = ("W_dec", "b_dec", "W_out", "b_out", "W_logvar", "b_logvar", "prior_")       # no path from the MoE loss, featLearn or not
Z_HEAD = ("W_mean", "b_mean", "W_zh", "b_zh")                                          # reached through relu(mean) with featLearn only


def engine(c, dtype="fp32", lossVAE=0, mode="exact"):
    """make() of tests/test_gpu_moe.py at the case's shape, then the case's parameters and labels in place of make()'s"""
    E, Od, D = c["shape"]
    eng, _, _, _ = make(E, Od, c["featLearn"], c["classification"], lossVAE, MC.MAX_BATCH, latent=D, mode=mode, dtype=dtype, n_data=MC.N_DATA)
    eng.moe_set_labels(torch.as_tensor(c["Y"]).cuda())
    assert set(eng.parameter_names()) == set(c["params"])
    eng.set_parameters(c["params"])
    return eng


def host(t):
    return t.float().cpu().numpy().astype(f64)


def run_head(eng, c, n, seed=1):
    """predict (P survives: the training pass overwrites it with dP), then one forward + backward pass on the same batch.
    -> the head's inputs as the GPU had them (float64 copies of the f32 views)"""
    E, Od, D = c["shape"]
    Xd, permd = torch.as_tensor(c["X"]).cuda(), torch.as_tensor(c["perm"]).cuda()
    eng.load_batch(Xd, permd, 0, n)
    eng.moe_predict(n)
    torch.cuda.synchronize()
    seen = dict(logits=host(eng.view("logits", n)), mean=host(eng.view("mean", n)), P=host(eng.view("moe_P", n)).reshape(n, E, Od))
    eps = torch.as_tensor(np.random.RandomState(seed).randn(n, D).astype(np.float32)).cuda()
    eng.moe_zero_acc()
    eng.forward_backward(n, eps)
    torch.cuda.synchronize()
    after = dict(logits=host(eng.view("logits", n)), mean=host(eng.view("mean", n)))
    if eng.dtype_name == "fp32":
        # the training pass saw the same inputs (P itself is gone: it is dP now)
        assert np.array_equal(seen["logits"], after["logits"]) and np.array_equal(seen["mean"], after["mean"])
    else:
        # bf16: the training pass runs the heads inside the latent launch (csrc/heads_latent.hip), whose logits and mean are not the encoder's
        # bit for bit: the head's inputs are the views the pass left.  P = x . W_moe + b_moe is the same GEMM in both; the featLearn P
        # is a function of mean and is restated from it (references: P = None)
        seen.update(after)
        if c["featLearn"]:
            seen["P"] = None
    seen["Y"] = c["Y"][c["perm"][:n]].astype(f64)
    return seen


def references(c, seen, n):
    kw = dict(mean=seen["mean"], W=c["params"]["W_moe"], bias=c["params"]["b_moe"]) if c["featLearn"] else {}
    inv_B = float(np.float32(1.0 / n))
    if seen["P"] is None:
        E, Od, D = c["shape"]
        P64 = (np.maximum(seen["mean"], 0.0) @ c["params"]["W_moe"] + c["params"]["b_moe"][None]).reshape(n, E, Od)
        return MC.oracle(seen["logits"], P64, seen["Y"], c["classification"], inv_B, **kw), MC.yardstick(seen["logits"], None, seen["Y"], c["classification"], inv_B, **kw)
    o = MC.oracle(seen["logits"], seen["P"], seen["Y"], c["classification"], inv_B, **kw)
    y = MC.yardstick(seen["logits"], seen["P"], seen["Y"], c["classification"], inv_B, **kw)
    return o, y


@pytest.mark.parametrize("case", CASES_A, ids=[MC.case_id(*c) for c in CASES_A])
def test_row_stage_against_the_oracle_on_its_own_inputs(case):
    """Every shape of moe_cases.SHAPES as the plan takes it (none had to be replaced).  On (5, 7, 8) mild the bars are the project's own, without
    the yardstick's help."""
    shape, kind, classification, featLearn = case
    E, Od, D = shape
    n = MC.N
    c = MC.get_case(*case)
    eng = engine(c)
    seen = run_head(eng, c, n)
    o, y = references(c, seen, n)
    acc = eng.moe_acc()
    got = dict(pred=host(eng.view("moe_pred", n)), dP=host(eng.view("moe_P", n)).reshape(n, E, Od), dlogits=host(eng.view("dlogits", n)),
               loss=acc[2], err=acc[3])
    if featLearn:
        got.update(P_fl=seen["P"], gmu=host(eng.view("gmu", n)))
        assert not np.any(seen["mean"][:, D - 1]) and np.any(c["params"]["W_moe"][D - 1])      # the edge of the gate [mean > 0]: a >= would add here
    alone = shape == (5, 7, 8) and kind == "mild"
    bad = []
    for k, v in got.items():
        tol = MC.project_bar(k, o[k]) if alone else MC.tolerance(k, o[k], y[k])
        ok, err, yerr = MC.within(k, v, o[k], y[k], tol=tol)
        print("moe_head %s %-7s error %.3e yardstick %.3e ratio %s atol %.3e max|ref| %.3e" % (
            MC.case_id(*case), k, err, yerr, "%.2f" % (err / yerr) if yerr > 0 else ("0" if err == 0 else "inf"), tol[1], np.max(np.abs(o[k]))))
        if not ok:
            where = np.unravel_index(np.argmax(np.abs(np.asarray(v, f64) - o[k])), np.shape(o[k])) if np.ndim(o[k]) else ()
            bad.append((k, err, tol, tuple(int(i) for i in where)))
    assert not bad, bad          # (output, max error, (rtol, atol), (row, expert, output) of the worst entry)
    assert acc[0] == acc[2] and acc[1] == acc[3] and np.all(np.isfinite(acc))
    if classification:
        clear = MC.clear_rows(o["pred"], y["pred"])
        assert clear.mean() >= 0.95
        top = np.argmax(got["pred"], axis=1)
        rows = np.sum(np.abs(seen["Y"] - np.eye(Od)[top]), axis=1) / 2
        assert np.array_equal(rows[clear], o["err_rows"][clear])                       # exact over the clear rows
        count, unclear = o["err_rows"].sum(), int((~clear).sum())
        assert count - unclear <= acc[3] <= count + unclear, (acc[3], count, unclear)   # the kernel's own arg-max merge


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("case", CASES_B, ids=[MC.case_id(*c) for c in CASES_B])
def test_bf16_operands_and_expert_gradients(case):
    """The f32-accumulation bar of the weight gradient: the operands are bf16, their products exact in float32, and K = 128 rows are added in float32
    in some order: |error| <= K 2^-24 sum_k |x_k dP_k| (Higham, gamma_{K-1} to first order).  The bf16 copy of the batch is not a view of its own:
    it is the round-to-nearest-even of the f32 "x" view."""
    shape, kind, classification, featLearn = case
    E, Od, D = shape
    n, EO = MC.N, E * Od
    c = MC.get_case(*case)
    eng = engine(c, dtype="bf16")
    seen = run_head(eng, c, n)
    o, y = references(c, seen, n)
    Bp = eng.batch_pad
    dPb, dP32 = eng.view("moe_dP", Bp, 1 << 30), eng.view("moe_P", n)
    assert dPb.dtype == torch.bfloat16 and dP32.dtype == torch.float32 and dPb.shape[0] == Bp == 128 and dPb.shape[1] % 64 == 0
    assert torch.equal(_bits(dPb[:n, :EO]), _bits(dP32.to(torch.bfloat16)))             # round to nearest even, bit for bit
    assert not dPb[n:].any() and not dPb[:, EO:].any()
    # dlogits: the VAE's share is 0, so the bf16 buffer holds the rounding of the head's f32 term
    dl = eng.view("dlogits", n)
    assert dl.dtype == torch.bfloat16
    rtol, atol = MC.tolerance("dlogits", o["dlogits"], y["dlogits"])
    err = np.abs(host(dl) - o["dlogits"])
    lim = MC.bf16_ulp(o["dlogits"]) + atol + rtol * np.abs(o["dlogits"])
    assert np.all(np.isfinite(host(dl))) and np.all(err <= lim), (float(err.max()), np.unravel_index(np.argmax(err - lim), err.shape))
    # the expert layer's gradients from the plan's own operands
    if featLearn:
        xin = host(torch.relu(eng.view("mean", n)).to(torch.bfloat16))
    else:
        xin = host(eng.view("x", n).to(torch.bfloat16))
    d = host(dPb[:n, :EO])
    g = eng.get_gradients()
    unit = 128 * 2.0 ** -24
    for name, ref, mag in (("W_moe", xin.T @ d, np.abs(xin).T @ np.abs(d)), ("b_moe", d.sum(0), np.abs(d).sum(0))):
        gg = g[name].astype(f64).reshape(ref.shape)
        e = np.abs(gg - ref)
        assert np.all(np.isfinite(gg)) and np.all(e <= unit * mag + 2.0 ** -126), (name, float(e.max()), np.unravel_index(np.argmax(e - unit * mag), e.shape))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("featLearn", [0, 1])
def test_short_batch_behind_a_full_one(dtype, featLearn):
    """the product's last batch of an epoch: rows >= n of the MoE buffers hold the previous batch's dP until the kernel's zero stores"""
    c = MC.get_case((40, 17, 33), "mild", 1, featLearn)
    Xd, permd = torch.as_tensor(c["X"]).cuda(), torch.as_tensor(c["perm"]).cuda()
    rng = np.random.RandomState(4)
    eps = [torch.as_tensor(rng.randn(m, 33).astype(np.float32)).cuda() for m in (100, 37)]
    out = []
    for passes in ((100, 37), (37,)):
        eng = engine(c, dtype=dtype, lossVAE=1)
        for m in passes:
            eng.load_batch(Xd, permd, 0, m)
            eng.forward_backward(m, eps[0] if m == 100 else eps[1])
        torch.cuda.synchronize()
        Bp = eng.batch_pad
        out.append((eng.get_gradients(), eng.moe_acc()[2:4], [eng.view(v, Bp).clone() for v in ("moe_dP", "dlogits", "gmu")]))
    (ga, aa, va), (gb, ab, vb) = out
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert np.array_equal(aa, ab)
    for name, a, b in zip(("moe_dP", "dlogits", "gmu"), va, vb):
        assert torch.equal(a, b), name
        assert not a[37:].any(), name


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("featLearn", [0, 1])
@pytest.mark.parametrize("shape", [(40, 17, 33), (256, 4, 4)], ids=lambda s: "%dx%dx%d" % s)
def test_no_vae_loss_on_trained_inputs(shape, featLearn, dtype):
    """lossVAE = 0 scales the VAE's gradients by inv_B = 0: one infinity there would be a NaN"""
    c = MC.get_case(shape, "trained", 1, featLearn)
    eng = engine(c, dtype=dtype)
    n = MC.N
    run_head(eng, c, n)
    g = eng.get_gradients()
    for k, v in g.items():
        assert np.all(np.isfinite(v)), k
        if k.startswith(VAE_ONLY) or (not featLearn and k.startswith(Z_HEAD)):
            assert not np.any(v), k
    assert np.any(g["W_moe"]) and np.any(g["W_logits"])
    Xd, permd = torch.as_tensor(c["X"]).cuda(), torch.as_tensor(c["perm"]).cuda()
    for _ in range(3):
        eng.train_step(Xd, permd, n, first=0)
    torch.cuda.synchronize()
    for name, t in (("param", eng.param), ("m", eng.m), ("v", eng.v)):
        assert bool(torch.isfinite(t).all()), name


def test_labels_through_the_device_cursor():
    """one epoch of four 64-row batches: A reads batch and labels through state->batch_cursor, B through an explicit offset.  Regression labels:
    N(0, 1) draws, distinct in every row, so that no offset can cancel."""
    B, nb, E, Od, D = 64, 4, 5, 7, 8
    engs = []
    for _ in range(2):
        eng, X, Y, _ = make(E, Od, 0, 0, 1, B, latent=D, n_data=nb * B)
        eng.reset_epoch(nb)
        eng.moe_zero_acc()
        engs.append(eng)
    A, Bn = engs
    assert len(np.unique(Y[:, 0])) == nb * B
    perm = np.random.RandomState(9).permutation(nb * B).astype(np.int32)
    Xd, permd = torch.as_tensor(X).cuda(), torch.as_tensor(perm).cuda()
    rng = np.random.RandomState(10)
    cfg = O.Config(64, D, E, (128,), 128, (128,), "binary")
    loss = err = 0.0
    for step in range(nb):
        p = {k: v.astype(f64) for k, v in Bn.get_parameters().items()}
        idx = perm[step * B:(step + 1) * B]
        a = O.encode(p, cfg, X[idx].astype(f64))
        r = MO.head_forward(MO.expert_outputs(p, X[idx].astype(f64), E, Od), O.softmax(a["logits"]), Y[idx].astype(f64), 0)
        loss += r["loss_rows"].sum() / B
        err += r["err_rows"].sum() / B
        eps = torch.as_tensor(rng.randn(B, D).astype(np.float32)).cuda()
        A.train_step(Xd, permd, None, eps, first=0, use_state_cursor=True)
        Bn.train_step(Xd, permd, B, eps, first=step * B)
        torch.cuda.synchronize()
        assert np.array_equal(A.moe_acc(), Bn.moe_acc()), (step, A.moe_acc(), Bn.moe_acc())
        assert torch.equal(A.param, Bn.param), step
    acc = A.moe_acc()
    for got, ref in ((acc[0], loss), (acc[1], err)):
        assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)) * 10, (got, ref)
