"""GPU tests of VaDE past the LDS limit of its one-kernel latent stage: the large-table form (csrc/latent_vade_mfma.hip) alone
through dmvae_latent_fwd mode 2 against the float64 oracle, against the one-kernel form where both run (debug knob 22), in the
whole fp32 and bf16 steps, in the evaluation (get_cluster_probs, latent_eval, dmvae_plan_eval_clusters) and through the class
surface.  Bars: those of tests/test_gpu_vade.py.  Inputs: prior tables scaled so that the responsibilities stay soft at these
widths (tests/helpers/vade_large.py; the condition is asserted on the oracle before anything runs on the GPU)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dmvae_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import vade_large as V      # noqa: E402

KNOB_FORCE_LARGE = 22


def run_stage(c, forced=False, scratch=True, noise=None, act_dtype=None, ldZ=None):
    """dmvae_latent_fwd mode 2 exactly as tests/test_gpu_vade.py::test_vade_latent_stage_matches_oracle drives it, every output
    requested, plus the scratch of the large-table form where the shape (or the knob) asks for it.  noise = (seed, step): the
    device draws eps instead of taking c["eps"].  act_dtype (default: f32 and no f32 copy): Z in that dtype and the f32 copy Zf
    beside it; ldZ (default: D padded to 64): the leading dimension of Z"""
    from dmvae_hip import lib, _lib
    B, D, K = c["B"], c["D"], c["K"]
    Bp, ldD = (B + 63) // 64 * 64, (D + 63) // 64 * 64
    dev = lambda x, ld: torch.nn.functional.pad(torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)), (0, ld - x.shape[1], 0, Bp - x.shape[0])).cuda().contiguous()
    md, lvd = dev(c["mean"], ldD), dev(c["lv"], ldD)
    epsd = torch.as_tensor(c["eps"].astype(np.float32)).cuda()
    pmd, plvd = torch.as_tensor(c["pm"].astype(np.float32)).cuda(), torch.as_tensor(c["plv"].astype(np.float32)).cuda()
    ldZ = ldZ or ldD
    Z = torch.full((Bp, ldZ), 9.0, device="cuda", dtype=torch.bfloat16 if act_dtype == _lib.BF16 else torch.float32); w = torch.zeros((Bp, K), device="cuda")
    Zf = torch.zeros((Bp, D), device="cuda") if act_dtype is not None else None
    gmu, glv, clv = (torch.zeros((Bp, ldD), device="cuda") for _ in range(3))
    nblk = lib.dmvae_latent_nblocks_vade(Bp)
    dpri, lp = torch.zeros((nblk, 2 * K * D), device="cuda"), torch.zeros((nblk, 2), device="cuda")
    la = _lib.LatentArgs()
    la.B, la.B_pad, la.D, la.K, la.mode, la.act_dtype = B, Bp, D, K, 2, _lib.F32 if act_dtype is None else act_dtype
    if Zf is not None:
        la.Z_f32, la.ld_Zf = Zf.data_ptr(), D
    la.kl_ratio, la.temperature, la.inv_B = c["kl_ratio"], 1.0, 1.0 / B
    la.mean, la.ld_mean, la.log_var, la.ld_log_var = md.data_ptr(), ldD, lvd.data_ptr(), ldD
    if noise is None:
        la.eps, la.ld_eps = epsd.data_ptr(), D
    else:
        la.seed, la.noise_step = noise
    la.prior_means, la.prior_log_vars = pmd.data_ptr(), plvd.data_ptr()
    la.Z_act, la.ld_Z, la.weights, la.ld_w = Z.data_ptr(), ldZ, w.data_ptr(), K
    la.gmu, la.glv, la.clv, la.ld_g = gmu.data_ptr(), glv.data_ptr(), clv.data_ptr(), ldD
    la.dprior_partials, la.loss_partials = dpri.data_ptr(), lp.data_ptr()
    nb = int(lib.dmvae_latent_vade_ws_bytes(Bp, D, K, 1 if forced else 0, None)) if scratch else 0
    ws = torch.full((max(nb // 4, 1),), float("nan"), device="cuda")          # (the kernels must not read what they have not written)
    if nb:
        la.mfma_ws, la.mfma_ws_bytes = ws.data_ptr(), nb
    if forced:
        _lib.check(lib.dmvae_debug_set_knob(KNOB_FORCE_LARGE, 1), "knob")
    try:
        _lib.check(lib.dmvae_latent_fwd(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(la)), "dmvae_latent_fwd")
        torch.cuda.synchronize()
    finally:
        if forced:
            _lib.check(lib.dmvae_debug_set_knob(KNOB_FORCE_LARGE, 0), "knob")
    return dict(Z=Z, Zf=Zf, w=w, gmu=gmu, glv=glv, clv=clv, dpri=dpri, lp=lp, ws_bytes=nb)


def check_stage(o, c, want):
    """the bars of test_vade_latent_stage_matches_oracle; want: dict(Z, w, kl_z, kl_c, gmu, glv, dpm, dplv)"""
    B, D, K = c["B"], c["D"], c["K"]
    Z, w, gmu, glv, dpri, lp = o["Z"], o["w"], o["gmu"], o["glv"], o["dpri"], o["lp"]
    klz, klc = lp[:, 0].double().sum().item() / B, lp[:, 1].double().sum().item() / B
    dp = dpri.double().sum(0).cpu().numpy()
    rel = lambda got, ref: float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300))
    print("B=%d D=%d K=%d: Z %.2e  gamma (rel to entry) %.2e  KL_Z %.2e KL_C %.2e  gmu %.2e glv %.2e dpm %.2e dplv %.2e (rel to max)" % (
        B, D, K, np.abs(Z[:B, :D].cpu().numpy() - want["Z"]).max(), float(np.max(np.abs(w[:B].cpu().numpy() - want["w"]) / (want["w"] + 1e-7 / 2e-4))),
        abs(klz - want["kl_z"]) / abs(want["kl_z"]), abs(klc - want["kl_c"]) / abs(want["kl_c"]), rel(gmu[:B, :D].cpu().numpy(), want["gmu"]),
        rel(glv[:B, :D].cpu().numpy(), want["glv"]), rel(dp[:K * D].reshape(K, D), want["dpm"]), rel(dp[K * D:].reshape(K, D), want["dplv"])))
    np.testing.assert_allclose(Z[:B, :D].cpu().numpy(), want["Z"], rtol=2e-6, atol=2e-6)
    assert not Z[:, D:].any() and not Z[B:].any()
    assert not gmu[:, D:].any() and not gmu[B:].any() and not glv[:, D:].any() and not glv[B:].any()
    np.testing.assert_allclose(w[:B].cpu().numpy(), want["w"], rtol=2e-4, atol=1e-7)
    assert klz == pytest.approx(want["kl_z"], rel=3e-5, abs=1e-5)
    assert klc == pytest.approx(want["kl_c"], rel=3e-5, abs=1e-6)
    sc = 1.0 / B
    np.testing.assert_allclose(gmu[:B, :D].cpu().numpy(), want["gmu"], rtol=5e-4, atol=5e-5 * sc)
    np.testing.assert_allclose(glv[:B, :D].cpu().numpy(), want["glv"], rtol=5e-4, atol=5e-5 * sc)
    np.testing.assert_allclose(dp[:K * D].reshape(K, D), want["dpm"], rtol=5e-4, atol=2e-5)
    np.testing.assert_allclose(dp[K * D:].reshape(K, D), want["dplv"], rtol=5e-4, atol=2e-5)


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("shape", [(93, 256, 10), (70, 128, 50), (130, 200, 37), (64, 512, 256), (64, 64, 460)])
def test_large_table_latent_stage_matches_oracle(shape):
    """(130, 200, 37): nothing a multiple of 64; (64, 512, 256): the configs[4] table at one row block; (64, 64, 460): more clusters
    than the DMVAE kernel's LDS takes at any chunk width (4 (83 K + 608) bytes > 150 KiB from K = 456 on) -- a limit VaDE never had
    a reason to inherit.  Each of these shapes was DMVAE_EUNSUPPORTED before the large-table form existed."""
    c = V.latent_case(*shape)
    V.assert_gamma_is_soft(c["mean"], c["lv"], c["eps"], c["pm"], c["plv"], c["kl_ratio"])
    o = run_stage(c)
    assert o["ws_bytes"] > 0
    check_stage(o, c, c)
    assert not o["dpri"][1:].any()                # one partial set: the prior-table gradient is complete in row 0


def test_large_table_shape_without_scratch_is_an_argument_error():
    from dmvae_hip import _lib
    with pytest.raises(_lib.DmvaeError, match="dmvae_latent_vade_ws_bytes"):
        run_stage(V.latent_case(20, 256, 4), scratch=False)


def test_forcing_knob_without_scratch_is_an_argument_error_not_the_other_kernel():
    from dmvae_hip import _lib
    with pytest.raises(_lib.DmvaeError, match="dmvae_latent_vade_ws_bytes"):
        run_stage(V.latent_case(70, 33, 3, scaled=False), forced=True, scratch=False)


@pytest.mark.parametrize("shape,forced", [((93, 256, 10), False), ((130, 200, 37), False), ((70, 30, 200), False), ((70, 33, 3), True)])
def test_large_table_form_draws_what_the_table_says(shape, forced):
    """Device noise of the large-table form against the exact Philox oracle (tests/helpers/philox_oracle.py), as tests/test_gpu_philox.py
    holds every other kernel: block b (Dp / 4) + d / 4, normal d & 3 -- csrc/latent_mfma.hip's keying.  mean = log_var = 0: Z is eps.
    D = 200: quads past D inside the padded row draw nothing; D = 30, 33: the scalar column path, a quad that straddles D."""
    import philox_oracle as P
    B, D, K = shape
    c = V.latent_case(B, D, K, scaled=not forced)
    c["mean"], c["lv"] = np.zeros((B, D)), np.zeros((B, D))
    seed, got = 0xDEADBEEF12345678, {}
    for step in (7, 2 ** 32 + 5):
        o = run_stage(c, forced=forced, noise=(seed, step))
        assert o["ws_bytes"] > 0
        Z = o["Z"].cpu().numpy()
        want = P.eps_mfma(seed, step, B, D)
        print("philox deviation | eps VaDE large-table form (%d, %d, %d) step %x | max |device - oracle| = %.3e" % (B, D, K, step, np.abs(Z[:B, :D] - want).max()))
        np.testing.assert_allclose(Z[:B, :D], want, rtol=0, atol=1e-3)          # the bar of tests/test_gpu_philox.py (fast-math log / sin / cos)
        assert not Z[:, D:].any() and not Z[B:].any()
        np.testing.assert_allclose(o["clv"].cpu().numpy()[:B, :D], 0.5 * want, rtol=0, atol=1e-3)
        assert np.isfinite(o["gmu"].cpu().numpy()).all() and np.isfinite(o["w"].cpu().numpy()).all()
        got[step] = Z[:B, :D]
    assert (np.abs(got[7] - got[2 ** 32 + 5]) > 1e-3).mean() > 0.99


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("shape,forced", [((93, 256, 10), False), ((70, 33, 3), True)])
@pytest.mark.parametrize("noise", [None, (1234, 7)])
def test_large_table_form_bf16_Z_is_the_rounded_f32_Z(shape, forced, noise):
    """Z[:B, :D] in bf16 is Z_f32 rounded to nearest even, bit for bit (csrc/common.h's f2bf / pack2bf are the hardware convert: that
    rounding); every other element of Z is zero.  D = 256: the packed store; D = 33: element by element, a quad that straddles D."""
    from dmvae_hip import _lib
    B, D, K = shape
    o = run_stage(V.latent_case(B, D, K, scaled=not forced), forced=forced, noise=noise, act_dtype=_lib.BF16)
    assert o["ws_bytes"] > 0 and o["Zf"][:B].abs().max() > 1.0
    assert torch.equal(o["Z"][:B, :D], o["Zf"][:B].bfloat16())
    assert not o["Z"][:, D:].any() and not o["Z"][B:].any()


@pytest.mark.parametrize("act", ["F32", "BF16"])
def test_large_table_form_Z_buffer_wider_than_padded_D(act):
    """ld_Z = Dp + 64: columns [D, ld_Z) of every row come back zero, Z[:B, :D] is what the ld_Z = Dp run writes"""
    from dmvae_hip import _lib
    B, D, K = 64, 33, 3
    c = V.latent_case(B, D, K, scaled=False)
    narrow = run_stage(c, forced=True, act_dtype=getattr(_lib, act))
    wide = run_stage(c, forced=True, act_dtype=getattr(_lib, act), ldZ=64 + 64)
    assert wide["ws_bytes"] > 0 and wide["Z"].shape == (64, 128) and narrow["Z"][:B, :D].float().abs().max() > 1.0
    assert not wide["Z"][:, D:].any()
    assert torch.equal(wide["Z"][:B, :D], narrow["Z"][:B, :D])


@pytest.mark.parametrize("shape", [(100, 64, 20), (70, 33, 3)])
def test_both_forms_agree_where_both_run(shape):
    c = V.latent_case(*shape, scaled=False)
    small, again = run_stage(c), run_stage(c)
    assert small["ws_bytes"] == 0
    for k in ("Z", "w", "gmu", "glv", "clv", "dpri", "lp"):                 # knob off: the one-kernel form, untouched and deterministic
        assert torch.equal(small[k], again[k]), k
    check_stage(small, c, c)
    large = run_stage(c, forced=True)
    assert large["ws_bytes"] > 0 and not large["dpri"][1:].any() and small["dpri"][1:].any()      # (it did take the other form)
    B, D, K = shape
    dp = small["dpri"].double().sum(0).cpu().numpy()
    want = dict(Z=small["Z"][:B, :D].double().cpu().numpy(), w=small["w"][:B].double().cpu().numpy(),
                kl_z=small["lp"][:, 0].double().sum().item() / B, kl_c=small["lp"][:, 1].double().sum().item() / B,
                gmu=small["gmu"][:B, :D].double().cpu().numpy(), glv=small["glv"][:B, :D].double().cpu().numpy(),
                dpm=dp[:K * D].reshape(K, D), dplv=dp[K * D:].reshape(K, D))
    check_stage(large, c, want)
    check_stage(large, c, c)
    assert torch.equal(large["clv"], small["clv"])


# ---------------------------------------------------------------------------------------------------------------- (c)
def make(kw, dtype, B, seed=0):
    from dmvae_hip import StepEngine
    eng = StepEngine(dtype=dtype, max_batch=B, deterministic=True, model="vade", head_dim=64, **kw)
    eng.init_parameters(seed)
    return eng


def ocfg(kw):
    return O.VadeConfig(kw["input_dim"], kw["latent_dim"], kw["n_classes"], kw["enc_layers"], kw["dec_layers"])


def test_vade_fp32_step_at_latent_256_matches_oracle():
    kw, B, Bmax = V.STEP_KW, 93, 128
    eng, cfg = make(kw, "fp32", Bmax), ocfg(kw)
    X, eps, pm, plv = V.step_inputs(B)
    p = {k: v.astype(np.float64) for k, v in eng.get_parameters().items()}
    p["prior_means"], p["prior_log_vars"] = pm, plv
    a = O.vade_forward(p, cfg, X.astype(np.float64), eps.astype(np.float64), 0.8)
    V.assert_gamma_is_soft(a["mean"], a["logvar"], eps.astype(np.float64), pm, plv, 0.8)
    eng.set_parameters(p)
    eng.write_state(kl_ratio=0.8, lr=0.002)
    eng.load_batch(torch.as_tensor(X).cuda(), None, 0, B)
    eng.forward_backward(B, torch.as_tensor(eps).cuda())
    torch.cuda.synchronize()
    masks = {k: (v > 0).cpu().numpy() for k, v in eng.hidden_activations(B).items()}
    flips = sum(int((masks[k] != (a[k] > 0)).sum()) for k in masks)
    assert flips <= 1e-4 * sum(mk.size for mk in masks.values()), flips
    g = O.vade_backward(p, cfg, a, masks)
    st = eng.read_state()
    print("loss %.6f / %.6f  kl_z %.6f / %.6f  kl_c %.6f / %.6f" % (st.last_loss, a["loss"], st.last_klz, a["kl_z"], st.last_klc, a["kl_c"]))
    assert abs(st.last_loss - a["loss"]) <= 1e-3, (st.last_loss, a["loss"])
    assert abs(st.last_klz - a["kl_z"]) <= 1e-3 and abs(st.last_klc - a["kl_c"]) <= 1e-3
    np.testing.assert_allclose(eng.view("weights", B).cpu().numpy(), a["w"], atol=2e-5)
    gg = eng.get_gradients()
    assert set(gg) == set(g)
    for k in g:
        scale = np.abs(g[k]).max() + 1e-12
        print("%-16s max err / max %.2e" % (k, np.abs(gg[k] - g[k]).max() / scale))
        assert np.abs(gg[k] - g[k]).max() <= 1e-4 * scale, (k, np.abs(gg[k] - g[k]).max(), scale)


# ---------------------------------------------------------------------------------------------------------------- (d)
def test_vade_bf16_step_at_latent_256_fused_update_and_graph_replay():
    kw, B, steps = V.STEP_KW, 256, 3
    N = B * steps
    rng = np.random.RandomState(2)
    data = torch.as_tensor((rng.rand(N, kw["input_dim"]) * (rng.rand(N, kw["input_dim"]) < 0.3)).astype(np.float32)).cuda()
    perm = torch.as_tensor(rng.permutation(N).astype(np.int32)).cuda()
    out = []
    for _ in range(2):
        eng = make(kw, "bf16", B, seed=4)
        eng.reset_epoch(steps, kl_ratio=1.0)
        step = eng.capture_step(data, perm)
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        out.append((eng.read_state().epoch_loss, eng.param.clone(), eng.m.clone(), eng.v.clone()))
    assert np.isfinite(out[0][0]) and out[0][0] == out[1][0]
    for i, name in ((1, "param"), (2, "m"), (3, "v")):
        assert torch.equal(out[0][i], out[1][i]), name
    assert torch.isfinite(out[0][1]).all() and out[0][2].abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------- (e)
def test_cluster_probs_and_latent_eval_at_large_width():
    import priors
    from dmvae_hip import latent_eval
    B, D, K = 93, 256, 10
    c = V.latent_case(B, D, K)
    mix = priors.NormalMixtureFactorial("representation", D, K)
    mix.means, mix.log_vars = c["pm"].astype(np.float32), c["plv"].astype(np.float32)
    want = O.cluster_probs(c["Z"].astype(np.float32).astype(np.float64), c["pm"], c["plv"])
    np.testing.assert_allclose(mix.get_cluster_probs(c["Z"]), want, rtol=2e-4, atol=1e-7)
    le = latent_eval(c["mean"], c["lv"], np.zeros((B, K)), c["pm"], c["plv"], eps=c["eps"], mode="vade", kl_ratio=0.6)
    np.testing.assert_allclose(le["weights"], c["w"], rtol=2e-4, atol=1e-7)
    assert le["kl_z"] == pytest.approx(c["kl_z"], rel=3e-5) and le["kl_c"] == pytest.approx(c["kl_c"], rel=3e-5)


def confusion(clusters, classes, R):
    d = np.zeros((R, R), dtype=np.int64)
    np.add.at(d, (np.asarray(clusters, dtype=np.int64), np.asarray(classes, dtype=np.int64)), 1)
    return d


def test_plan_eval_clusters_at_large_width():
    from dmvae_hip import StepEngine
    kw, Bmax, N, first, n, k = V.EVAL_KW, 128, 120, 9, 93, 3
    K, R = kw["n_classes"], kw["n_classes"] + 2
    eng = StepEngine(dtype="fp32", max_batch=Bmax, deterministic=True, model="vade", head_dim=64, seed=11, **kw)
    eng.init_parameters(2)
    X, cls, order, eps, pm, plv = V.eval_inputs(N, n, k)
    p = {a: v.astype(np.float64) for a, v in eng.get_parameters().items()}
    p["prior_means"], p["prior_log_vars"] = pm, plv
    rows = order[first:first + n]
    want, clear = V.eval_oracle(p, kw, X[rows], eps)
    assert (~clear).mean() <= 0.02                                # near ties of the oracle's top two: excluded, and few
    assert np.median(want.max(1)) <= 0.9
    eng.set_parameters(p)
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(torch.int32).cuda()
    Xd, cd, pd = torch.as_tensor(X).cuda(), i32(cls), i32(order)
    conf = eng.confusion_buffer(R, "cuda")
    eng.load_batch(Xd, pd, first, n)
    eng.eval_clusters(conf, cd, pd, first, n, draws=k, eps=torch.as_tensor(eps).cuda())
    w = eng.view("eval_w", n).cpu().numpy()
    got = eng.read_confusion(conf)
    np.testing.assert_allclose(w, want, rtol=2e-4, atol=2e-5)
    mine = confusion(np.argmax(want, 1)[clear], cls[rows][clear], R) + confusion(np.argmax(w, 1)[~clear], cls[rows][~clear], R)
    assert np.array_equal(got, mine) and got.sum() == n
    # Philox draws: reproducible, and another estimate than the fed one
    def run(counter):
        c2 = eng.confusion_buffer(R, "cuda")
        eng.eval_clusters(c2, cd, pd, first, n, draws=k, counter=counter)
        return eng.view("eval_w", n).clone(), eng.read_confusion(c2)
    w7, c7 = run(7)
    w7b, c7b = run(7)
    assert torch.equal(w7, w7b) and np.array_equal(c7, c7b) and c7.sum() == n
    assert abs(float(w7.sum(1).mean()) - 1.0) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- (f)
def test_vade_class_surface_at_latent_256(tmp_path):
    import base_models
    from includes.utils import Dataset
    np.random.seed(0)
    rng = np.random.RandomState(0)
    N, K, I = 600, 12, 196
    cls = rng.randint(0, K, N)
    X = np.clip(O.synthetic_images(N, I, seed=2) * 0.3 + (np.arange(I)[None, :] % K == cls[:, None]) * 0.7, 0, 1).astype(np.float32)
    data = Dataset((X, cls), batch_size=128)
    model = base_models.VaDE("vade_l", "binary", I, 256, K, activation="relu", initializer="xavier", batch_size=128, dtype="fp32", noise="host",
                             enc_layers=(128, 64), dec_layers=(64, 128)).build_graph()
    pm, plv = V.scaled_tables(rng, 256, K)                   # soft responsibilities at this width (tests/helpers/vade_large.py)
    model.engine.set_parameters({"prior_means": pm.astype(np.float32), "prior_log_vars": plv.astype(np.float32)})
    model.path = str(tmp_path / "vade_l")
    model.define_train_step(0.002, 100)
    losses = [model.train_op(None, data, 1.0) for _ in range(2)]
    assert all(np.isfinite(l) for l in losses) and losses[0] > losses[1], losses
    state = np.random.get_state()
    model.eval = "host"
    acc_h = model.get_accuracy(None, data, k=2)
    np.random.set_state(state)
    model.eval = "device"
    acc_d = model.get_accuracy(None, data, k=2)
    print("accuracy host %.6f device %.6f" % (acc_h, acc_d))
    assert 0.0 <= acc_h <= 1.0 and acc_h == acc_d
