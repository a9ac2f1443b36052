"""GPU tests of the mixture-of-experts head (dmvae_plan_attach_moe; models.py:10-163 of the reference) against the float64
restatement in tests/helpers/moe_oracle.py.  Bars as in tests/test_gpu_configs.py: fp32 gradients <= 1e-4 of each tensor's max,
loss terms <= 1e-3; properties bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import dmvae_oracle as O      # noqa: E402
import moe_oracle as MO       # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = dict(input_dim=64, enc_layers=(128,), head_dim=128, dec_layers=(128,))


def make(E, Od, featLearn, classification, lossVAE, B, latent=8, mode="exact", dtype="fp32", n_data=None, seed=3, layers=SMALL):
    from dmvae_hip import StepEngine
    rng = np.random.RandomState(seed)
    n_data = n_data or B + 37
    I = layers["input_dim"]
    X = (rng.rand(n_data, I) * (rng.rand(n_data, I) < 0.4)).astype(np.float32)
    if classification:
        Y = MO.classification_labels(rng.randint(0, Od, n_data), Od).astype(np.float32)
    else:
        Y = rng.randn(n_data, Od).astype(np.float32)
    Yd = torch.as_tensor(Y).cuda()
    moe = dict(n_experts=E, output_dim=Od, featLearn=featLearn, classification=classification, lossVAE=lossVAE, labels=Yd)
    eng = StepEngine(latent_dim=latent, n_classes=E, dtype=dtype, max_batch=B, mode=mode, deterministic=True, moe=moe, **layers)
    eng.init_parameters(5)
    eng.write_state(lr=0.002, kl_ratio=0.7)
    # O(1) gate logits and expert outputs, so that every softmax of the head is exercised away from saturation
    pr = eng.get_parameters()
    pr["W_moe"] = pr["W_moe"] * 0.05
    pr["b_moe"] = rng.randn(*pr["b_moe"].shape).astype(np.float32) * 0.1
    pr["b_logits"] = rng.randn(*pr["b_logits"].shape).astype(np.float32) * 0.5
    eng.set_parameters(pr)
    return eng, X, Y, rng


def ocfg(latent, E, layers=SMALL):
    return O.Config(layers["input_dim"], latent, E, layers["enc_layers"], layers["head_dim"], layers["dec_layers"], "binary")


def run_step(eng, X, Y, rng, n, latent, E, mode):
    perm = rng.permutation(X.shape[0]).astype(np.int32)
    eps = rng.randn(n, latent).astype(np.float32)
    gum = O.sample_gumbel((n, E), rng).astype(np.float32) if mode == "relaxed" else None
    eng.moe_zero_acc()
    eng.load_batch(torch.as_tensor(X).cuda(), torch.as_tensor(perm).cuda(), 0, n)
    eng.forward_backward(n, torch.as_tensor(eps).cuda(), None if gum is None else torch.as_tensor(gum).cuda())
    torch.cuda.synchronize()
    idx = perm[:n]
    return X[idx].astype(np.float64), Y[idx].astype(np.float64), eps.astype(np.float64), None if gum is None else gum.astype(np.float64)


@pytest.mark.parametrize("model", ["dvmoe", "dmoe"])
@pytest.mark.parametrize("classification", [1, 0])
@pytest.mark.parametrize("featLearn", [0, 1])
@pytest.mark.parametrize("mode", ["exact", "relaxed"])
def test_fp32_step_against_the_oracle(model, classification, featLearn, mode):
    step_against_the_oracle(model, classification, featLearn, mode)


# the widths at which moe_head_kernel takes another path (tests/helpers/moe_cases.py): one output in the second slot of a lane with E no multiple
# of 16 and D > 32; all four slots full; sixteen experts per lane.  dvmoe, both modes; not the full cross product
@pytest.mark.parametrize("classification,featLearn", [(1, 1), (0, 0)])
@pytest.mark.parametrize("mode", ["exact", "relaxed"])
@pytest.mark.parametrize("shape", [(40, 17, 33), (16, 64, 24), (256, 4, 4)], ids=lambda s: "%dx%dx%d" % s)
def test_fp32_step_against_the_oracle_at_shape(shape, mode, classification, featLearn):
    step_against_the_oracle("dvmoe", classification, featLearn, mode, shape)


def step_against_the_oracle(model, classification, featLearn, mode, shape=(5, 7, 8)):
    E, Od, n = shape[0], shape[1], 93        # ragged: 93 real rows of a 128-row plan
    latent = 1 if model == "dmoe" else shape[2]     # DeepMoE gates with a latent_dim = 1 DMVAE (models.py:240-243)
    lossVAE = 1 if model == "dvmoe" else 0
    eng, X, Y, rng = make(E, Od, featLearn, classification, lossVAE, 100, latent=latent, mode=mode)
    p = {k: v.astype(np.float64) for k, v in eng.get_parameters().items()}
    Xb, Yb, eps, gum = run_step(eng, X, Y, rng, n, latent, E, mode)
    cfg = ocfg(latent, E)
    a = MO.forward(p, cfg, Xb, eps, Yb, E, Od, featLearn, classification, lossVAE, kl_ratio=0.7, mode=mode, gumbel=gum)
    acc = eng.moe_acc()
    assert abs(acc[2] - a["loss_moe"]) <= 1e-3 * max(1.0, abs(a["loss_moe"])), (acc[2], a["loss_moe"])
    assert abs(acc[3] - a["error"]) <= 1e-3 * max(1.0, abs(a["error"])), (acc[3], a["error"])
    assert acc[0] == acc[2] and acc[1] == acc[3]
    st = eng.read_state()
    assert abs(st.last_loss - a["loss"]) <= 1e-3                   # the VAE loss is reported in both models
    g = MO.backward(p, cfg, a, E, Od, featLearn, classification, lossVAE)
    got = eng.get_gradients()
    for k, ref in g.items():
        ref = np.asarray(ref).reshape(got[k].shape)
        bar = 1e-4 * max(np.abs(ref).max(), 1e-30)
        err = np.abs(got[k] - ref).max()
        assert err <= bar or (np.abs(ref).max() == 0 and err == 0), (k, err, np.abs(ref).max())
    if model == "dmoe" and not featLearn:
        # no VAE term: the decoder, the z-head and the prior tables get exactly zero
        for k in got:
            if k.startswith(("W_dec", "b_dec", "W_out", "b_out", "W_mean", "b_mean", "W_logvar", "b_logvar", "W_zh", "b_zh", "prior_")):
                assert not np.any(got[k]), k


def test_dmoe_leaves_decoder_and_z_head_bit_identical():
    eng, X, Y, rng = make(5, 10, 0, 1, 0, 100, latent=1)
    names = [k for k in eng.parameter_names() if k.startswith(("W_dec", "b_dec", "W_out", "b_out", "W_mean", "b_mean", "W_logvar", "b_logvar", "W_zh", "b_zh"))]
    before = {k: (eng.param_view(k).clone(), eng._strided(eng.m, k).clone(), eng._strided(eng.v, k).clone()) for k in names}
    w0 = eng.param_view("W_moe").clone()
    perm = torch.as_tensor(rng.permutation(X.shape[0]).astype(np.int32)).cuda()
    Xd = torch.as_tensor(X).cuda()
    for _ in range(3):
        eng.train_step(Xd, perm, 100, first=0)
    torch.cuda.synchronize()
    for k, (p0, m0, v0) in before.items():
        assert torch.equal(eng.param_view(k), p0) and torch.equal(eng._strided(eng.m, k), m0) and torch.equal(eng._strided(eng.v, k), v0), k
    assert not torch.equal(eng.param_view("W_moe"), w0)          # the experts did train


@pytest.mark.parametrize("E,Od", [(5, 1), (5, 64), (10, 10), (256, 1), (256, 4)])
@pytest.mark.parametrize("classification", [1, 0])
def test_row_kernel_predict_against_the_oracle(E, Od, classification):
    n = 77
    eng, X, Y, rng = make(E, Od, 0, classification, 1, 80, latent=4)
    p = {k: v.astype(np.float64) for k, v in eng.get_parameters().items()}
    perm = rng.permutation(X.shape[0]).astype(np.int32)
    eng.moe_zero_acc()
    eng.load_batch(torch.as_tensor(X).cuda(), torch.as_tensor(perm).cuda(), 0, n)
    eng.moe_predict(n)
    torch.cuda.synchronize()
    Xb, Yb = X[perm[:n]].astype(np.float64), Y[perm[:n]].astype(np.float64)
    cfg = ocfg(4, E)
    a = O.encode(p, cfg, Xb)
    q = O.softmax(a["logits"])
    P = MO.expert_outputs(p, Xb, E, Od)
    r = MO.head_forward(P, q, Yb, classification)
    pred = eng.view("moe_pred", n).cpu().numpy()
    np.testing.assert_allclose(pred, r["pred"], rtol=1e-5, atol=1e-5 * max(1.0, np.abs(r["pred"]).max()))
    acc = eng.moe_acc()
    loss = r["loss_rows"].sum() / n
    err = r["err_rows"].sum() if classification else r["err_rows"].sum() / n
    assert abs(acc[2] - loss) <= 1e-5 * max(1.0, abs(loss)) * 10, (acc[2], loss)
    if classification:
        ties = np.sort(r["pred"], axis=1)
        if Od == 1 or np.all(ties[:, -1] - ties[:, -2] > 1e-5):
            assert acc[3] == err, (acc[3], err)
    else:
        assert abs(acc[3] - err) <= 1e-5 * max(1.0, abs(err)) * 10


@pytest.mark.parametrize("featLearn", [0, 1])
def test_captured_replay_matches_eager_bit_for_bit(featLearn):
    B = 64
    engs = []
    for _ in range(2):
        eng, X, Y, rng = make(10, 10, featLearn, 1, 1, B, latent=8, dtype="bf16", n_data=4 * B)
        eng.reset_epoch(4)
        eng.moe_zero_acc()
        engs.append(eng)
    Xd = torch.as_tensor(X).cuda()
    perm = torch.as_tensor(np.random.RandomState(9).permutation(4 * B).astype(np.int32)).cuda()
    replay = engs[0].capture_step(Xd, perm)
    engs[0].moe_zero_acc()
    for _ in range(5):
        replay()
        engs[1].train_step(Xd, perm, None, first=0, use_state_cursor=True)
    torch.cuda.synchronize()
    assert torch.equal(engs[0].param, engs[1].param) and torch.equal(engs[0].m, engs[1].m) and torch.equal(engs[0].v, engs[1].v)
    assert np.array_equal(engs[0].moe_acc(), engs[1].moe_acc())
    assert engs[0].read_state().adam_t == engs[1].read_state().adam_t == 5


def test_bf16_step_at_4096_rows_against_fp32():
    B = 4096
    layers = dict(input_dim=784, enc_layers=(500, 500), head_dim=2000, dec_layers=(2000, 500, 500))
    out = {}
    for dt in ("fp32", "bf16"):
        eng, X, Y, rng = make(10, 10, 0, 1, 1, B, latent=64, dtype=dt, n_data=B, layers=layers)
        perm = torch.as_tensor(np.arange(B, dtype=np.int32)).cuda()
        eps = torch.as_tensor(np.random.RandomState(2).randn(B, 64).astype(np.float32)).cuda()
        eng.moe_zero_acc()
        eng.load_batch(torch.as_tensor(X).cuda(), perm, 0, B)
        eng.forward_backward(B, eps)
        torch.cuda.synchronize()
        out[dt] = (eng.moe_acc(), eng.get_gradients(), eng.read_state().last_loss)
    (a32, g32, l32), (a16, g16, l16) = out["fp32"], out["bf16"]
    assert abs(a16[2] - a32[2]) <= 2e-3 * abs(a32[2]), (a16[2], a32[2])
    assert abs(l16 - l32) <= 2e-3 * abs(l32)
    for k in ("W_moe", "b_moe", "W_logits", "b_logits", "W_enc0"):
        rel = np.linalg.norm(g16[k] - g32[k]) / max(np.linalg.norm(g32[k]), 1e-30)
        assert rel <= 8e-2, (k, rel)


def test_attach_limits_fail_loudly():
    from dmvae_hip import StepEngine
    from dmvae_hip._lib import DmvaeError
    Yd = torch.zeros(8, 64).cuda()
    with pytest.raises(DmvaeError):
        StepEngine(latent_dim=4, n_classes=20, dtype="fp32", max_batch=8,
                   moe=dict(n_experts=20, output_dim=64, featLearn=0, classification=1, lossVAE=1, labels=Yd), **SMALL)
