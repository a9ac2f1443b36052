"""GPU tests of the device noise (csrc/common.h) against the exact NumPy oracle of tests/helpers/philox_oracle.py, through the C ABI:
the uniform stream bit for bit, the normal and Gumbel transforms against float64 on the same words, and every kernel that draws in
its own counter layout -- the "noise streams" table of DESIGN.md section 4 -- against what that table says it draws.

Tolerances.  Philox is integer arithmetic and the uniform transform is exact: those comparisons are assert_array_equal.  The normal
and Gumbel transforms go through __logf / __sinf / __cosf, whose error on this hardware is stated nowhere in the project: atol = 1e-3
there is a SEPARATING bound, not an accuracy claim.  Every other term rounds below 3e-6 of the radius (1-ulp log and sqrt, exact u01,
float32 2 pi off by 1.75e-7); a wrong word gives an independent N(0, 1) draw, within 1e-3 of the right one with probability below
1e-3 per element, and the smallest case compares 12 elements.  The largest deviation seen per transform is printed (pytest -s) and
recorded in profiles/philox_oracle.txt; it is not asserted."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import philox_oracle as P                                   # noqa: E402
from test_gpu_kernels import run_latent                     # noqa: E402
from test_gpu_heads_latent import run_heads_latent          # noqa: E402

ATOL = 1e-3
SEED, STEP = 1234, 7            # run_latent's defaults
STREAM_PARAMS = [(42, 3), (0, 0), (0xDEADBEEF12345678, 2 ** 32 + 5), (2 ** 64 - 1, 2 ** 64 - 1)]


@pytest.fixture(scope="module")
def hip():
    import dmvae_hip  # noqa: F401
    from dmvae_hip import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(L, what, n, seed, step, sid):
    out = torch.full((n,), float("nan"), device="cuda")
    fn = getattr(L.lib, "dmvae_philox_" + what)
    L.check(fn(stream(), L.ptr(out), n, seed, step, sid), "dmvae_philox_" + what)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def report(what, got, want):
    dev = float(np.abs(got.astype(np.float64) - want).max())
    print("philox deviation | %-44s | n = %9d | max |device - oracle| = %.3e" % (what, got.size, dev))
    return dev


# ------------------------------------------------------------------------------------------------------------ the element streams
@pytest.mark.parametrize("seed,step", STREAM_PARAMS)
@pytest.mark.parametrize("sid", [0, 1, 2, 3])
def test_uniform_stream_is_bit_equal_to_the_oracle(hip, sid, seed, step):
    """(word >> 8) * 2^-24 of every word, 24 bits of each observable: a wrong round constant, key schedule or counter packing, a
    dropped stream id, a seed or step cut to 32 bits on its way through ctypes or the launch -- each changes every value"""
    n = 2 ** 20 + 3
    got = launch(hip, "uniform", n, seed, step, sid)
    want = P.uniform(P.words_flat(seed, step, sid, n)).astype(np.float32)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("seed,step", STREAM_PARAMS)
@pytest.mark.parametrize("sid", [0, 1, 2, 3])
def test_normal_and_gumbel_streams_match_the_float64_oracle(hip, sid, seed, step):
    n = 2 ** 20 + 3
    idx = np.arange(n, dtype=np.uint64)
    got = launch(hip, "normal", n, seed, step, sid)
    want = P.normal_at(seed, step, sid, idx)
    report("normal stream %d seed %x step %x" % (sid, seed, step), got, want)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    got = launch(hip, "gumbel", n, seed, step, sid)
    want = P.gumbel_at(seed, step, sid, idx)
    report("gumbel stream %d seed %x step %x" % (sid, seed, step), got, want)
    assert np.isfinite(got).all()
    atom = P.u01(P.words_flat(seed, step, sid, n)) == 1.0
    np.testing.assert_allclose(got[~atom], want[~atom], rtol=0, atol=ATOL)
    np.testing.assert_allclose(got[atom], want[atom], rtol=1e-6, atol=0)


def test_gumbel_at_the_ends_of_the_u01_grid(hip):
    """Words at the two ends of the (0, 1] grid of u01, found by the oracle in stream (seed 42, step 3, stream 1): word 12 300 443 is
    >= 0xFFFFFF00 (U = 1) and word 5 262 247 is < 0x100 (U = 2^-24).

    PINNED, not changed here: the reference draws its Gumbel noise from U on [0, 1) (sample_gumbel: -log(-log(U + eps) + eps)), so its
    largest value is near 16.  The device draws U on (0, 1], where log never sees 0 -- and where U = 1 gives -log(1e-20f) = 46.05: an
    atom of probability 2^-24 per draw.  The float64 formula on the same U agrees with the kernel, so this is a property of the grid
    and not a kernel error."""
    seed, step, sid = 42, 3, 1
    top = P.find_edge_word(seed, step, sid, "top")
    bot = P.find_edge_word(seed, step, sid, "bottom")
    assert (top, bot) == (12300443, 5262247)
    n = max(top, bot) + 1 + 5
    got = launch(hip, "gumbel", n, seed, step, sid)
    assert np.isfinite(got).all()
    assert float(got[top]) == pytest.approx(-math.log(float(np.float32(1e-20))), rel=1e-6) == pytest.approx(46.0517, abs=1e-4)
    assert float(got[bot]) == pytest.approx(-math.log(24 * math.log(2)), abs=ATOL) == pytest.approx(-2.8116, abs=1e-4)
    assert got.max() == got[top] and got.min() >= got[bot] - ATOL
    # the whole launch against the oracle, in pieces (the oracle takes ~0.25 us per word)
    dev = 0.0
    for lo in range(0, n, 1 << 22):
        hi = min(n, lo + (1 << 22))
        w = P.words_flat(seed, step, sid, hi - lo, first_block=lo // 4)
        want, atom = P.gumbel(w), P.u01(w) == 1.0
        dev = max(dev, float(np.abs(got[lo:hi][~atom] - want[~atom]).max()))
        np.testing.assert_allclose(got[lo:hi][~atom], want[~atom], rtol=0, atol=ATOL)
        np.testing.assert_allclose(got[lo:hi][atom], want[atom], rtol=1e-6, atol=0)
    print("philox deviation | %-44s | n = %9d | max |device - oracle| = %.3e" % ("gumbel stream 1 seed 2a step 3, edge launch", n, dev))


def test_normals_at_the_ends_of_the_u01_grid(hip):
    """philox_normal_at takes its radius from word 0 of a block.  Within the first 2^24 blocks of (seed 42, step 3) the oracle finds a
    word 0 >= 0xFFFFFF00 in stream 1 (block 7 237 770: u01 = 1, radius exactly 0) and a word 0 < 0x100 in stream 2 (block 2 208 432:
    u01 = 2^-24, the largest radius there is, sqrt(48 ln 2) = 5.768)."""
    seed, step = 42, 3
    top = P.find_edge_word(seed, step, 1, "top", words=(0,))
    bot = P.find_edge_word(seed, step, 2, "bottom", words=(0,))
    assert (top, bot) == (4 * 7237770, 4 * 2208432)
    for sid, blk, edge in ((1, top // 4, "top"), (2, bot // 4, "bottom")):
        n = 2 * blk + 2 + 5
        got = launch(hip, "normal", n, seed, step, sid)
        assert np.isfinite(got).all()
        pair = got[2 * blk: 2 * blk + 2]
        want = P.normal_at(seed, step, sid, np.arange(2 * blk, 2 * blk + 2, dtype=np.uint64))
        np.testing.assert_allclose(pair, want, rtol=0, atol=ATOL)
        if edge == "top":
            assert pair[0] == 0.0 and pair[1] == 0.0
        else:
            rmax = math.sqrt(48 * math.log(2))
            assert np.abs(pair).max() <= rmax and math.hypot(*pair) == pytest.approx(rmax, abs=ATOL)
            assert np.abs(got).max() <= rmax
        tail = np.arange(n - 4096, n, dtype=np.uint64)
        np.testing.assert_allclose(got[n - 4096:], P.normal_at(seed, step, sid, tail), rtol=0, atol=ATOL)


# ------------------------------------------------------------------------------------------------------------ the consumers
def zero_inputs(B, D, K, seed=0):
    rng = np.random.RandomState(seed)
    return np.zeros((B, D)), np.zeros((B, D)), np.zeros((B, K)), rng.randn(K, D), rng.randn(K, D) * 0.4


# ... and three shapes on the wide chunks (128 and 256 columns: two and four blocks per lane and chunk), which the LDS budget allows at small K only
ONE_KERNEL_SHAPES = [(4, 3, 5), (100, 10, 10), (37, 30, 7), (200, 64, 10), (70, 96, 130), (130, 300, 50), (64, 512, 256),
                     (100, 128, 10), (50, 256, 10), (33, 200, 7)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", ONE_KERNEL_SHAPES)
def test_one_kernel_latent_draws_what_the_table_says(hip, mode, shape):
    """mean = log_var = 0: Z is eps.  D < 16, D = 300 in chunks, columns per lane not a multiple of four (D = 3, 10, 30, 96 ...), K > 64.
    Mode 1 with logits = 0, temperature 1: the weights are softmax(g), so log w_k - log w_0 = g_k - g_0 of stream 1."""
    L = hip
    B, D, K = shape
    mean, lv, logits, pm, plv = zero_inputs(B, D, K)
    B_pad = (B + 63) // 64 * 64
    assert L.lib.dmvae_latent_nblocks(B_pad, D, K) == -(-B_pad // P.one_kernel_geometry(B_pad, D, K)[0])
    got = {}
    for step in (STEP, STEP + 1):
        g = run_latent(L, mean, lv, logits, None, None, pm, plv, mode, 1.0, 0.6, 0, ldpad=4, seed=SEED, noise_step=step)
        eps = g["Zf"][:B]
        want = P.eps_one_kernel(SEED, step, B, D, K, B_pad)
        report("eps one-kernel mode %d (%d, %d, %d) step %d" % (mode, B, D, K, step), eps, want)
        np.testing.assert_allclose(eps, want, rtol=0, atol=ATOL)
        np.testing.assert_array_equal(g["Z"][:B, :D], eps)
        assert not g["Z"][:, D:].any() and not g["Z"][B:].any() and not g["Zf"][B:].any()
        np.testing.assert_allclose(g["clv"][:B, :D], 0.5 * want, rtol=0, atol=ATOL)
        if mode == 1:
            gum = P.gumbel_latent(SEED, step, B, K)
            lw = np.log(g["w"][:B].astype(np.float64))
            report("gumbel differences (%d, %d, %d) step %d" % (B, D, K, step), lw[:, 1:] - lw[:, :1], gum[:, 1:] - gum[:, :1])
            np.testing.assert_allclose(lw[:, 1:] - lw[:, :1], gum[:, 1:] - gum[:, :1], rtol=0, atol=ATOL)
        else:
            np.testing.assert_allclose(g["w"][:B], 1.0 / K, rtol=1e-6)
        got[step] = eps
    assert (np.abs(got[STEP] - got[STEP + 1]) > ATOL).mean() > 0.99
    # the 64-bit seed and step reach the kernel whole
    big_seed, big_step = 0xDEADBEEF12345678, 2 ** 32 + 5
    g = run_latent(L, mean, lv, logits, None, None, pm, plv, mode, 1.0, 0.6, 0, ldpad=4, seed=big_seed, noise_step=big_step)
    np.testing.assert_allclose(g["Zf"][:B], P.eps_one_kernel(big_seed, big_step, B, D, K, B_pad), rtol=0, atol=ATOL)


@pytest.mark.parametrize("shape", [(130, 300, 50), (70, 96, 130), (128, 256, 50), (64, 512, 256), (1000, 64, 64), (333, 30, 200)])
def test_mfma_latent_draws_what_the_table_says(hip, shape):
    """the shapes of test_latent_mfma_form_matches_oracle: block b * (Dp / 4) + d / 4, normal d & 3 (D = 30: the scalar column loop)"""
    L = hip
    B, D, K = shape
    mean, lv, logits, pm, plv = zero_inputs(B, D, K)
    got = {}
    for step in (STEP, STEP + 1):
        g = run_latent(L, mean, lv, logits, None, None, pm, plv, 0, 1.0, 0.6, 0, ldpad=4, mfma=True, seed=SEED, noise_step=step)
        eps = g["Zf"][:B]
        want = P.eps_mfma(SEED, step, B, D)
        report("eps MFMA form (%d, %d, %d) step %d" % (B, D, K, step), eps, want)
        np.testing.assert_allclose(eps, want, rtol=0, atol=ATOL)
        np.testing.assert_array_equal(g["Z"][:B, :D], eps)
        assert not g["Z"][:, D:].any() and not g["Z"][B:].any() and not g["Zf"][B:].any()
        got[step] = eps
    assert (np.abs(got[STEP] - got[STEP + 1]) > ATOL).mean() > 0.99
    # the one-kernel form on the same arguments draws ANOTHER eps: the oracle's two layouts, each held to its kernel
    one = run_latent(L, mean, lv, logits, None, None, pm, plv, 0, 1.0, 0.6, 0, ldpad=4, seed=SEED, noise_step=STEP)["Zf"][:B]
    np.testing.assert_allclose(one, P.eps_one_kernel(SEED, STEP, B, D, K), rtol=0, atol=ATOL)
    assert (np.abs(one - got[STEP]) > ATOL).mean() > 0.9


def run_vade_latent(L, B, D, K, seed, step):
    """dmvae_latent_fwd mode 2 (csrc/latent_vade.hip) as tests/test_gpu_vade.py calls it, with mean = log_var = 0 and no caller noise"""
    Bp, ldD = (B + 63) // 64 * 64, (D + 63) // 64 * 64
    rng = np.random.RandomState(B + D + K)
    md, lvd = torch.zeros((Bp, ldD), device="cuda"), torch.zeros((Bp, ldD), device="cuda")
    pmd = torch.as_tensor(rng.randn(K, D).astype(np.float32)).cuda()
    plvd = torch.as_tensor((rng.randn(K, D) * 0.4).astype(np.float32)).cuda()
    Z = torch.full((Bp, ldD), 9.0, device="cuda"); w = torch.zeros((Bp, K), device="cuda")
    gmu, glv, clv = (torch.zeros((Bp, ldD), device="cuda") for _ in range(3))
    nblk = L.lib.dmvae_latent_nblocks_vade(Bp)
    dpri, lp = torch.zeros((nblk, 2 * K * D), device="cuda"), torch.zeros((nblk, 2), device="cuda")
    la = L.LatentArgs()
    la.B, la.B_pad, la.D, la.K, la.mode, la.act_dtype = B, Bp, D, K, 2, L.F32
    la.kl_ratio, la.temperature, la.inv_B, la.seed, la.noise_step = 0.6, 1.0, 1.0 / B, seed, step
    la.mean, la.ld_mean, la.log_var, la.ld_log_var = md.data_ptr(), ldD, lvd.data_ptr(), ldD
    la.prior_means, la.prior_log_vars = pmd.data_ptr(), plvd.data_ptr()
    la.Z_act, la.ld_Z, la.weights, la.ld_w = Z.data_ptr(), ldD, w.data_ptr(), K
    la.gmu, la.glv, la.clv, la.ld_g = gmu.data_ptr(), glv.data_ptr(), clv.data_ptr(), ldD
    la.dprior_partials, la.loss_partials = dpri.data_ptr(), lp.data_ptr()
    L.check(L.lib.dmvae_latent_fwd(stream(), C.byref(la)), "dmvae_latent_fwd")
    torch.cuda.synchronize()
    return Z.cpu().numpy()


@pytest.mark.parametrize("shape", [(100, 10, 10), (37, 6, 5), (200, 64, 20), (70, 33, 3)])
def test_vade_latent_draws_what_the_table_says(hip, shape):
    B, D, K = shape
    got = {}
    for step in (STEP, STEP + 1):
        Z = run_vade_latent(hip, B, D, K, SEED, step)
        want = P.eps_vade(SEED, step, B, D)
        report("eps VaDE (%d, %d, %d) step %d" % (B, D, K, step), Z[:B, :D], want)
        np.testing.assert_allclose(Z[:B, :D], want, rtol=0, atol=ATOL)
        assert not Z[:, D:].any() and not Z[B:].any()
        got[step] = Z[:B, :D]
    assert (np.abs(got[STEP] - got[STEP + 1]) > ATOL).mean() > 0.99


@pytest.mark.parametrize("B,D,K,Hp", [(100, 10, 10, 128), (200, 100, 16, 192)])
def test_fused_heads_latent_draws_the_one_kernel_streams(hip, B, D, K, Hp):
    """csrc/heads_latent.hip must reproduce the draws of latent_fwd_kernel, eps and Gumbel: zero head kernels and biases make
    mean = log_var = logits = 0, so Z is eps and (mode 1, temperature 1) the weights are softmax(g)"""
    L = hip
    B_pad, Dp, Kp = (B + 63) // 64 * 64, (D + 63) // 64 * 64, 64
    rng = np.random.RandomState(B + D)
    hzc = torch.as_tensor(np.maximum(rng.randn(B_pad, 2 * Hp), 0.0)).to(torch.bfloat16).cuda()
    Wmv, Wlg = torch.zeros((Hp, 2 * Dp), dtype=torch.bfloat16, device="cuda"), torch.zeros((Hp, Kp), dtype=torch.bfloat16, device="cuda")
    bmv, blg = torch.zeros(2 * Dp, device="cuda"), torch.zeros(Kp, device="cuda")
    pm, plv = rng.randn(K, D), rng.randn(K, D) * 0.4
    got = {}
    for step in (STEP, STEP + 1):
        o = run_heads_latent(L, hzc, Wmv, Wlg, bmv, blg, None, None, pm, plv, 1, 1.0, 0.8, B, D, K, fused=True, seed=SEED, step=step)
        assert not o["mv"].any().item() and not o["logits"].any().item()
        Zf = o["Zf"].cpu().numpy()
        want = P.eps_one_kernel(SEED, step, B, D, K, B_pad)
        report("eps fused heads + latent (%d, %d, %d) step %d" % (B, D, K, step), Zf[:B, :D], want)
        np.testing.assert_allclose(Zf[:B, :D], want, rtol=0, atol=ATOL)
        assert not Zf[B:].any() and not Zf[:, D:].any() and not o["Z"][:, D:].any().item() and not o["Z"][B:].any().item()
        gum = P.gumbel_latent(SEED, step, B, K)
        lw = np.log(o["w"].cpu().numpy()[:B, :K].astype(np.float64))
        np.testing.assert_allclose(lw[:, 1:] - lw[:, :1], gum[:, 1:] - gum[:, :1], rtol=0, atol=ATOL)
        got[step] = Zf[:B, :D]
    assert (np.abs(got[STEP] - got[STEP + 1]) > ATOL).mean() > 0.99


# ------------------------------------------------------------------------------------------------------------ the step state
def test_noise_step_advances_through_the_device_state():
    """fp32 plan, device noise, learning rate 0 (the parameters stay put): three eager steps, then three replays of the captured graph.
    After each, eps recovered from the plan's mean / log_var / Z views is the oracle's draw at the noise_step the state held for that
    step (the captured graph reads it from the device state: a replay does not redraw the captured step's noise)."""
    from dmvae_hip import StepEngine
    kw = dict(input_dim=40, latent_dim=6, n_classes=5, enc_layers=(70, 50), head_dim=90, dec_layers=(90, 50, 30))       # test_gpu_step.py SMALL
    B, N, seed = 37, 4 * 37, 0xDEADBEEF12345678
    eng = StepEngine(dtype="fp32", max_batch=B, deterministic=True, seed=seed, **kw)
    eng.init_parameters(0)
    rng = np.random.RandomState(5)
    data = torch.as_tensor((rng.rand(N, 40) * (rng.rand(N, 40) < 0.3)).astype(np.float32)).cuda()
    perm = torch.as_tensor(rng.permutation(N).astype(np.int32)).cuda()
    eng.reset_epoch(N // B, kl_ratio=1.0)
    eng.write_state(lr=0.0, noise_step=2 ** 32 - 2)             # the steps below cross the 32-bit boundary of the counter
    p0 = eng.param.clone()
    D, K = kw["latent_dim"], kw["n_classes"]

    def check(held):
        torch.cuda.synchronize()
        st = eng.read_state()
        assert st.noise_step == held + 1
        mean, lv, Z = (eng.view(n, B).double().cpu().numpy() for n in ("mean", "log_var", "Z"))
        eps = (Z - mean) / np.exp(lv / 2)
        want = P.eps_one_kernel(seed, held, B, D, K, eng.batch_pad)
        report("eps of the step, noise_step %x" % held, eps, want)
        np.testing.assert_allclose(eps, want, rtol=0, atol=ATOL)
        return eps

    draws = []
    for _ in range(3):
        held = eng.read_state().noise_step
        eng.train_step(data, perm, use_state_cursor=True)
        draws.append(check(held))
    replay = eng.capture_step(data, perm)
    assert eng.read_state().noise_step == 2 ** 32 + 1          # capture_step restores the state its warm-up steps moved
    for _ in range(3):
        held = eng.read_state().noise_step
        replay()
        draws.append(check(held))
    assert eng.read_state().noise_step == 2 ** 32 + 4
    for a, b in zip(draws[:-1], draws[1:]):
        assert (np.abs(a - b) > ATOL).mean() > 0.9
    assert torch.equal(eng.param, p0)
