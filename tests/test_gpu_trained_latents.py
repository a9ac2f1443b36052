"""GPU tests of every form of the latent stage on trained-regime inputs (tests/helpers/trained_latents.py: prior tables of a Gaussian-mixture
fit with small variances, posterior means on a cluster mean, one-hot q and gamma, a quarter of the rows decided by a few nats, dead
dimensions and a collapsed cluster at variance 1e-6, vanished probabilities) against the float64 oracle.  The tolerance of every output is
tolerance(name, oracle, yardstick): the bars of test_gpu_kernels.py::test_latent_fwd_matches_oracle, the absolute one raised to twice the
error of a float32 restatement of the form's own algebra computed on the CPU (direct differences for the one-kernel forms, expanded
squares for the MFMA forms).  tests/test_trained_latents_host.py holds the inputs and the yardsticks to their conditions without a GPU.
Each case is one launch; it prints error / yardstick error per output (the figures of DESIGN.md's section on trained tables)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import trained_latents as TL                        # noqa: E402
from test_gpu_kernels import hip, run_latent        # noqa: E402,F401
from test_gpu_vade_large import run_stage           # noqa: E402

MODE = dict(exact=0, relaxed=1)


def launch(L, form, shape, kind, tau):
    """one launch of the form on the case -> dict of float64 arrays cut to [B, D] / [B, K], plus the uncut ones for the pad checks"""
    mode = TL.FORMS[form][0]
    c = TL.get_case(shape, kind)
    B, D, K = shape
    if mode == "vade":
        cc = dict(c, kl_ratio=TL.KL_RATIO)
        o = run_stage(cc, forced=form == "vade_mfma_forced")
        assert (o["ws_bytes"] > 0) == (form != "vade"), "the shape did not take the form under test"
        raw = {k: o[k].cpu().numpy() for k in ("Z", "w", "gmu", "glv", "clv")}
        dp = o["dpri"].double().sum(0).cpu().numpy()
        got = dict(Z=raw["Z"][:B, :D], clv=raw["clv"][:B, :D], w=raw["w"][:B], gmu=raw["gmu"][:B, :D], glv=raw["glv"][:B, :D],
                   dpm=dp[:K * D].reshape(K, D), dplv=dp[K * D:].reshape(K, D),
                   klz=o["lp"][:, 0].double().sum().item() / B, klc=o["lp"][:, 1].double().sum().item() / B)
        return got, raw
    raw = run_latent(L, c["mean"], c["lv"], c["logits"], c["eps"], c["gumbel"] if mode == "relaxed" else None, c["pm"], c["plv"], MODE[mode], tau,
                     TL.KL_RATIO, 0, ldpad=4, mfma=form == "dmvae_mfma")
    got = dict(Z=raw["Z"][:B, :D], clv=raw["clv"][:B, :D], w=raw["w"][:B], gmu=raw["gmu"][:B, :D], glv=raw["glv"][:B, :D], dlogits=raw["dlogits"][:B, :K],
               dpm=raw["dpm"], dplv=raw["dplv"], klz=raw["klz"], klc=raw["klc"])
    np.testing.assert_array_equal(raw["Zf"][:B], got["Z"])
    return got, raw


def check_pads(raw, shape, mode):
    B, D, K = shape
    assert not raw["Z"][:, D:].any() and not raw["Z"][B:].any()
    assert not raw["gmu"][B:, :D].any()
    if mode == "vade":
        assert not raw["gmu"][:, D:].any() and not raw["gmu"][B:].any() and not raw["glv"][:, D:].any() and not raw["glv"][B:].any()
    else:
        assert not raw["dlogits"][:, K:].any() and not raw["dlogits"][B:].any()


def check_outputs(tag, names, got, o, y):
    """every output finite and within tolerance(...); prints error / yardstick error of each"""
    line, missed = [], []
    for n in names:
        ok, err, yerr = TL.within(n, got[n], o[n], y[n])
        rtol, atol = TL.tolerance(n, o[n], y[n])
        line.append("%s %.2e / %.2e = %.2f" % (n, err, yerr, err / max(yerr, 1e-300)))
        if not ok:
            missed.append((n, err, "atol %.3e rtol %.1e" % (atol, rtol)))
    print("trained latents | %s | error / yardstick error | %s" % (tag, " | ".join(line)))
    for n in names:
        assert np.all(np.isfinite(got[n])), n
    assert not missed, missed


def check_argmax(got_w, o, y):
    clear = TL.clear_rows(o["u"], y["u"])
    assert np.array_equal(np.argmax(got_w, 1)[clear], np.argmax(o["w"], 1)[clear])
    return clear


@pytest.mark.parametrize("case", TL.CASES, ids=[TL.case_id(*c) for c in TL.CASES])
def test_latent_form_on_trained_tables_matches_oracle(hip, case):
    form, shape, kind, tau = case
    mode, which = TL.FORMS[form][:2]
    c, o, y = TL.get_case(shape, kind), TL.get_oracle(shape, kind, mode, tau), TL.get_yard(shape, kind, mode, which, tau)
    got, raw = launch(hip, form, shape, kind, tau)
    check_pads(raw, shape, mode)
    check_outputs(TL.case_id(*case), TL.outputs_of(form, shape, kind), got, o, y)
    if mode == "vade":
        clear = check_argmax(got["w"], o, y)
        print("trained latents | %s | rows held to the oracle's arg-max: %d of %d" % (TL.case_id(*case), clear.sum(), len(clear)))
    if kind == "vanishing":
        # wherever q is 0.0 in float32: dlogits is the oracle's with q = 0 there -- r / B (log 1e-20 + log K) through the softmax Jacobian
        gone = y["q"] == 0.0
        assert gone.any()
        o0 = TL.oracle(c, mode, tau, q=np.where(gone, 0.0, o["q"]))
        rtol, atol = TL.tolerance("dlogits", o["dlogits"], y["dlogits"])
        np.testing.assert_allclose(got["dlogits"][gone], o0["dlogits"][gone], rtol=rtol, atol=atol)
        if mode == "exact":
            assert not got["w"][gone].any() and not got["dlogits"][gone].any()


@pytest.mark.parametrize("mode,shape", TL.BOTH_FORMS, ids=["%s-%dx%dx%d" % ((m,) + s) for m, s in TL.BOTH_FORMS])
@pytest.mark.parametrize("kind", TL.KINDS[:3])
def test_cost_of_the_expansion_is_printed(hip, mode, shape, kind):
    """both forms of one mode at one shape: each output's error over max |direct_f32 - oracle|.  Printed, not asserted: the ratio of the
    MFMA form's line to the one-kernel form's is what expanding the squares costs (DESIGN.md records the figures)."""
    forms = ("dmvae_exact", "dmvae_mfma") if mode == "exact" else ("vade", "vade_mfma_forced")
    o, y = TL.get_oracle(shape, kind, mode, 1.0), TL.get_yard(shape, kind, mode, "direct", 1.0)
    for form in forms:
        got, _ = launch(hip, form, shape, kind, 1.0)
        names = [n for n in TL.OUTPUTS if n in got]
        for n in names:
            assert np.all(np.isfinite(got[n])), (form, n)
        print("trained latents | cost of the expansion | %s %dx%dx%d %s | error / direct_f32 error | %s" % ((form,) + shape + (kind, " | ".join(
            "%s %.2f" % (n, TL.yard_error(o[n], got[n]) / max(TL.yard_error(o[n], y[n]), 1e-300)) for n in names))))


# ---------------------------------------------------------------------------------------------------------------- the product surface
def identity_encoder(eng, mean, lv):
    """parameters under which the plan's encoder returns exactly (mean, lv) for the one-hot batch X = I: the first layer's row i holds
    [mean+ | mean- | lv+ | lv-] of row i (non-negative: the ReLU passes them), the heads subtract the halves; biases zero.
    Every product is a number times 1 or 0: exact in the fp32 GEMMs."""
    n, D = mean.shape
    p = {k: np.zeros_like(v) for k, v in eng.get_parameters().items()}
    pos = lambda a: np.maximum(a, 0.0)
    assert p["W_enc0"].shape == (n, 4 * D) and p["W_mean"].shape == (4 * D, D) and p["W_logvar"].shape == (4 * D, D)
    p["W_enc0"][:] = np.concatenate([pos(mean), pos(-mean), pos(lv), pos(-lv)], axis=1)
    eye, zero = np.eye(D), np.zeros((D, D))
    p["W_mean"][:] = np.concatenate([eye, -eye, zero, zero], axis=0)
    p["W_logvar"][:] = np.concatenate([zero, zero, eye, -eye], axis=0)
    return p


@pytest.mark.parametrize("shape", [(100, 10, 10), (64, 256, 12)], ids=["one-kernel", "large-table"])
@pytest.mark.parametrize("kind", ["competing", "floor"])
def test_responsibilities_through_the_product_surface(hip, shape, kind):
    """latent_eval(mode="vade") and dmvae_plan_eval_clusters (draws = 1, the caller's eps) on the case's tables and posteriors: the w rule and
    the arg-max rule of the stage's own test"""
    from dmvae_hip import StepEngine, latent_eval
    B, D, K = shape
    which = "direct" if D == 10 else "expanded"
    c, o, y = TL.get_case(shape, kind), TL.get_oracle(shape, kind, "vade", 1.0), TL.get_yard(shape, kind, "vade", which, 1.0)
    le = latent_eval(c["mean"], c["lv"], np.zeros((B, K)), c["pm"], c["plv"], eps=c["eps"], mode="vade", kl_ratio=TL.KL_RATIO)
    tag = "%dx%dx%d-%s" % (shape + (kind,))
    check_outputs("latent_eval " + tag, ["w"], dict(w=np.asarray(le["weights"], np.float64)), o, y)
    check_argmax(np.asarray(le["weights"]), o, y)

    Bmax = (B + 63) // 64 * 64
    eng = StepEngine(dtype="fp32", max_batch=Bmax, deterministic=True, model="vade", head_dim=64, seed=11, input_dim=B, latent_dim=D, n_classes=K,
                     enc_layers=(4 * D,), dec_layers=(8,))
    eng.init_parameters(0)
    p = identity_encoder(eng, c["mean"], c["lv"])
    p["prior_means"], p["prior_log_vars"] = c["pm"], c["plv"]
    eng.set_parameters(p)
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(torch.int32).cuda()
    Xd, cls, order = torch.eye(B, device="cuda"), i32(np.argmax(o["w"], 1)), i32(np.arange(B))
    conf = eng.confusion_buffer(K, "cuda")
    eng.load_batch(Xd, order, 0, B)
    eng.eval_clusters(conf, cls, order, 0, B, draws=1, eps=torch.as_tensor(c["eps"][None].astype(np.float32)).cuda().contiguous())
    w = eng.view("eval_w", B).cpu().numpy().astype(np.float64)
    conf = eng.read_confusion(conf)
    assert np.array_equal(eng.view("mean", B, D).cpu().numpy(), c["mean"].astype(np.float32))           # the encoder handed the case over, bit for bit
    assert np.array_equal(eng.view("log_var", B, D).cpu().numpy(), c["lv"].astype(np.float32))
    check_outputs("eval_clusters " + tag, ["w"], dict(w=w), o, y)
    clear = check_argmax(w, o, y)
    assert conf.sum() == B and np.trace(conf) >= clear.sum()          # classes = the oracle's arg-max: every clear row lands on the diagonal
