"""CPU tests of the large-table form of VaDE's latent stage (csrc/latent_vade_mfma.hip): the algebra of its contractions against the
float64 oracle, and the host arithmetic of its workspace."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import dmvae_oracle as O      # noqa: E402
import vade_large as V        # noqa: E402


def test_expanded_squares_are_the_oracle():
    """every matrix-product formula of the kernel, in float64, against O.vade_latent_backward / O.vade_forward's KL terms: 1e-10 relative"""
    B, D, K, r = 9, 70, 7, 0.6
    c = V.latent_case(B, D, K, scaled=False, kl_ratio=r)
    x = V.expanded(c["mean"], c["lv"], c["eps"], c["pm"], c["plv"], r)
    rel = lambda got, want: np.abs(got - want).max() / np.abs(want).max()
    for k in ("Z", "w", "gmu", "glv", "dpm", "dplv"):
        assert rel(x[k], c[k]) <= 1e-10, (k, rel(x[k], c[k]))
    assert abs(x["kl_z"] - c["kl_z"]) <= 1e-10 * abs(c["kl_z"])
    assert abs(x["kl_c"] - c["kl_c"]) <= 1e-10 * abs(c["kl_c"])
    # the same two KL terms as O.vade_forward computes them (its latent block)
    cfg = O.VadeConfig(4, D, K, (4,), (4,))
    p = O.init_params(cfg, 0)
    p = {k: v.astype(np.float64) for k, v in p.items()}
    p["prior_means"], p["prior_log_vars"] = c["pm"], c["plv"]
    X = np.random.RandomState(0).rand(B, 4)
    a = O.vade_forward(p, cfg, X, c["eps"], r)
    y = V.expanded(a["mean"], a["logvar"], c["eps"], c["pm"], c["plv"], r)
    assert abs(y["kl_z"] - a["kl_z"]) <= 1e-10 * abs(a["kl_z"]) and abs(y["kl_c"] - a["kl_c"]) <= 1e-10 * abs(a["kl_c"])


@pytest.mark.parametrize("shape", [(93, 256, 10), (70, 128, 50), (130, 200, 37), (64, 512, 256)])
def test_scaled_tables_keep_gamma_soft(shape):
    """the inputs of tests/test_gpu_vade_large.py (a): under them the path through gamma is exercised"""
    B, D, K = shape
    c = V.latent_case(B, D, K)
    V.assert_gamma_is_soft(c["mean"], c["lv"], c["eps"], c["pm"], c["plv"], c["kl_ratio"])


def test_workspace_size_is_host_arithmetic_and_linear():
    from dmvae_hip import _lib
    ws = lambda B, D, K, forced=0: int(_lib.lib.dmvae_latent_vade_ws_bytes(B, D, K, forced, None))
    for B, D, K in ((100, 10, 10), (37, 6, 5), (200, 64, 20), (70, 33, 3)):          # the shapes of tests/test_gpu_vade.py: the one-kernel form
        Bp = (B + 63) // 64 * 64
        assert ws(Bp, D, K) == 0 and _lib.lib.dmvae_latent_ws_bytes(Bp, D, K, 2) == 0
        assert ws(Bp, D, K, 1) > 0                                                   # (debug knob 22: what the other form would need)
    assert ws(128, 128, 10) == 0                                                     # the last shape inside the LDS limit
    for B, D, K in ((128, 256, 10), (128, 128, 50), (8192, 512, 256)):
        assert ws(B, D, K) > 0 and ws(B, D, K) == ws(B, D, K, 1) == _lib.lib.dmvae_latent_ws_bytes(B, D, K, 2)
    assert ws(100, 256, 10) == 0 and ws(0, 256, 10) == 0                             # not a padded batch: no size
    slabs = C.c_int(0)
    B, D, K = 8192, 512, 256
    n = int(_lib.lib.dmvae_latent_vade_ws_bytes(B, D, K, 0, C.byref(slabs)))
    assert slabs.value >= 2 and slabs.value % 2 == 0
    assert n < 2 * 4 * (B * (4 * D + 4 * K) + slabs.value * K * (2 * D + 64))        # linear in B D + B K + K D, never B K D
    assert n < 4 * B * K * D // 8
