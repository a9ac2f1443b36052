"""Host-side tests of the linear probe (csrc/probe.hip, dmvae_hip/probe.py): the entries are declared, exported and bound,
dmvae_softmax_xent_ws_bytes is host arithmetic that refuses every shape outside the domain by name, and the oracles the GPU tests lean
on (tests/helpers/probe_oracle.py) agree with central differences, with the closed form at W = 0 and with their own optimality."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import probe_oracle as PO      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def problem(n=40, D=5, Cn=4, seed=0):
    rng = np.random.RandomState(seed)
    Z = rng.randn(n, D).astype(np.float32)
    y = rng.randint(0, Cn, n)
    return Z, y, 0.5 * rng.randn(D, Cn), 0.5 * rng.randn(Cn), rng.randn(D).astype(np.float32), (0.5 + rng.rand(D)).astype(np.float32)


def test_entries_are_declared_exported_and_bound():
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dmvae_[a-z0-9_]+)\s*\(", hdr))
    for name, nargs in (("dmvae_softmax_xent", 16), ("dmvae_linear_scores", 13), ("dmvae_softmax_xent_ws_bytes", 3)):
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert len(getattr(_lib.lib, name).argtypes) == nargs, name
    assert _lib.lib.dmvae_softmax_xent_ws_bytes.restype is C.c_int64
    assert _lib.ABI_VERSION == 5 and _lib.lib.dmvae_abi_version() == 5          # entries were only added
    assert '"probe.hip"' in open(os.path.join(ROOT, "deep-mixture-vae_amd", "build.py")).read()
    import dmvae_hip.probe as P
    src = open(P.__file__).read()
    assert "sklearn" not in re.sub(r'""".*?"""', "", src, flags=re.S)            # (the docstrings name what it reproduces)
    assert "import sklearn" not in src and "from sklearn" not in src
    for name in ("softmax_xent", "LogisticRegression", "scores_enqueue"):
        assert hasattr(P, name)


def test_ws_bytes_is_host_arithmetic_and_refuses_bad_shapes_by_name():
    from dmvae_hip import _lib
    ws = _lib.lib.dmvae_softmax_xent_ws_bytes
    for good in ((1, 1, 2), (1 << 22, 512, 32), (1 << 22, 64, 256), (55000, 64, 10), (5, 128, 128)):
        got = ws(*good)
        assert got >= 8 + 8 * (good[1] + 1) * good[2], good                    # at least one workgroup's partials
        assert got == ws(*good)
    for bad in ((0, 4, 3), ((1 << 22) + 1, 4, 3), (5, 0, 3), (5, 513, 3), (5, 4, 1), (5, 4, 257), (5, 65, 253), (5, 129, 128)):
        assert ws(*bad) == -1, bad                                               # DMVAE_EINVAL
        assert b"dmvae_softmax_xent_ws_bytes" in _lib.lib.dmvae_last_error(), bad


def test_oracle_gradient_agrees_with_central_differences():
    for shifted in (False, True):
        Z, y, W, b, sh, sc = problem()
        sh, sc = (sh, sc) if shifted else (None, None)
        _, gW, gb = PO.xent(Z, y, W, b, sh, sc)
        h = 1e-6
        for (d, c) in ((0, 0), (2, 3), (4, 1)):
            Wp, Wm = W.copy(), W.copy()
            Wp[d, c] += h
            Wm[d, c] -= h
            num = (PO.xent(Z, y, Wp, b, sh, sc)[0] - PO.xent(Z, y, Wm, b, sh, sc)[0]) / (2 * h)
            assert abs(num - gW[d, c]) <= 1e-6 * max(abs(gW[d, c]), np.abs(gW).max()), (d, c)
        for c in range(4):
            bp, bm = b.copy(), b.copy()
            bp[c] += h
            bm[c] -= h
            num = (PO.xent(Z, y, W, bp, sh, sc)[0] - PO.xent(Z, y, W, bm, sh, sc)[0]) / (2 * h)
            assert abs(num - gb[c]) <= 1e-6 * np.abs(gb).max(), c
        f, oW, ob = PO.objective(Z, y, W, b, 0.5, sh, sc)                        # the penalty: ||W||^2 / (2 C n), the bias unpenalised
        assert abs(f - PO.xent(Z, y, W, b, sh, sc)[0] - (W * W).sum() / (2 * 0.5 * 40)) <= 1e-15
        assert np.allclose(oW - gW, W / (0.5 * 40), rtol=0, atol=1e-15) and np.array_equal(ob, gb)


def test_oracle_loss_at_zero_is_log_c_and_refused_rows_add_nothing():
    Z, y, W, b, _, _ = problem(Cn=7)
    loss, gW, gb = PO.xent(Z, y, np.zeros_like(W), np.zeros_like(b))
    assert abs(loss - np.log(7)) <= 1e-15 and abs(gb.sum()) <= 1e-15
    l32, gW32, gb32, sc = PO.xent_f32(Z, y, np.zeros_like(W), np.zeros_like(b))
    assert abs(l32 - np.log(7)) <= 1e-6 and np.abs(gW32 - gW).max() <= 1e-6 and not sc.any()
    yb = y.copy()
    yb[[3, 17]] = (-1, 7)
    keep = np.ones(len(y), bool)
    keep[[3, 17]] = False
    got, want = PO.xent(Z, yb, W, b), PO.xent(Z[keep], y[keep], W, b)
    for a, w in zip(got, want):
        assert np.allclose(a, np.asarray(w) * keep.sum() / len(y), rtol=1e-14, atol=0)
    got32 = PO.xent_f32(Z, yb, W, b)
    assert abs(got32[0] - got[0]) <= 1e-5 and got32[3].shape == (len(y), 7)


def test_oracle_yardstick_is_close_and_finite_where_the_true_class_underflows():
    Z, y, W, b, sh, sc = problem()
    ref, f32 = PO.xent(Z, y, W, b, sh, sc), PO.xent_f32(Z, y, W, b, sh, sc)
    assert abs(f32[0] - ref[0]) <= 1e-5 and np.abs(f32[1] - ref[1]).max() <= 1e-6 and np.abs(f32[2] - ref[2]).max() <= 1e-6
    assert np.abs(f32[3] - PO.scores(Z, W, b, sh, sc)).max() <= 1e-5
    big = 200.0 * np.array([[1.0, -1.0]])                                        # p(true class) = exp(-400): zero in f32
    loss = PO.xent_f32(np.ones((1, 1), np.float32), [1], big, np.zeros(2))[0]
    assert np.isfinite(loss) and abs(loss - 400.0) <= 1e-4


def test_optimum_is_a_stationary_point():
    Z, y, _, _, sh, sc = problem(n=200, D=6, Cn=3, seed=3)
    W, b = PO.optimum(Z, y, 3, C_reg=0.2, shift=sh, scale=sc)
    _, gW, gb = PO.objective(Z, y, W, b, 0.2, sh, sc)
    assert max(np.abs(gW).max(), np.abs(gb).max()) <= 1e-9
    assert np.allclose(PO.xent(Z, y, W, b, sh, sc)[1], -W / (0.2 * 200), rtol=0, atol=1e-9)      # the data gradient balances the penalty


def test_model_surface_and_parser():
    import base_models
    import models
    for cls in (base_models.DeepMixtureVAE, base_models.VaDE, models.DeepMoE, models.DeepVariationalMoE):
        assert callable(cls.get_linear_probe_accuracy)
    from dmvae_hip.probe import LogisticRegression
    with pytest.raises(ValueError):
        LogisticRegression(C=0.0)
    with pytest.raises(ValueError):
        LogisticRegression(n_classes=257)
    src = open(os.path.join(ROOT, "deep-mixture-vae_amd", "train.py")).read()
    assert re.search(r'add_argument\("--probe", action="store_true", default=False', src)
    assert re.search(r'add_argument\("--probe_C", type=float, default=1.0', src)
