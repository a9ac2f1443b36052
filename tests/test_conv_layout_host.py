"""Host checks of tests/helpers/conv_layout.py: the layout helper is itself right, and the inputs of tests/test_gpu_conv_kernels.py
have the properties that make a wrong kernel visible (ties at a positive maximum, all-zero windows, sums below 2^24, a launch
geometry with empty trailing blocks).  No GPU."""
import os
import sys

import numpy as np
import pytest

import dmvae_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import conv_layout as CL      # noqa: E402


@pytest.mark.parametrize("H", [4, 7, 14, 28])         # P = 6, 9 (odd), 16, 30
@pytest.mark.parametrize("Cn,ld", [(32, 32), (32, 64), (5, 32)])
def test_pack_unpack_round_trip(H, Cn, ld):
    rng = np.random.RandomState(H + Cn + ld)
    B, P = 3, H + 2
    x = rng.randint(1, 4, size=(B, H, H, Cn)).astype(np.float64)       # never zero: whatever is zero afterwards is padding
    rows, off = CL.pack(x, ld, guard_fill=7.0)
    assert rows.shape == (2 * (P + 1) + B * P * P, ld) and off == (P + 1) * ld
    np.testing.assert_array_equal(CL.unpack(rows, off, B, H, Cn), x)
    assert (rows[:P + 1] == 7.0).all() and (rows[-(P + 1):] == 7.0).all()
    img = CL.images(rows, B, P)
    assert (img[:, CL.border_mask(P)] == 0).all() and (img[..., Cn:] == 0).all()
    assert CL.border_mask(P).sum() == 4 * P - 4
    assert np.count_nonzero(rows[P + 1:-(P + 1)]) == B * H * H * Cn
    # row m + (ky-1)*P + (kx-1) of the packed array IS tap (ky,kx) of the patch matrix: the identity the conv-mode GEMMs rest on
    flat = rows.reshape(-1)
    col = O.im2col3x3(x)
    b, y, xx = B - 1, H - 1, 0
    m = (b * P + y + 1) * P + xx + 1
    for tap in range(9):
        r = m + (tap // 3 - 1) * P + (tap % 3 - 1)
        np.testing.assert_array_equal(flat[off + r * ld: off + r * ld + Cn], col[b, y, xx, tap * Cn:(tap + 1) * Cn])


def test_wflip_reference_is_the_adjoint_of_im2col():
    """conv(dy, flipped / transposed kernel) == col2im3x3(dy @ W.T): the two ways to write the input gradient agree"""
    rng = np.random.RandomState(0)
    B, H, cin, cout = 2, 5, 3, 4
    W = CL.ints(rng, (9 * cin, cout))
    dy = CL.ints(rng, (B, H, H, cout))
    Kt, cin_ld = CL.pad64(9 * cout), 8
    Wt = CL.wflip_reference(W, cin, cin_ld, cout, Kt)
    assert (Wt[cin:] == 0).all() and (Wt[:, 9 * cout:] == 0).all()
    via_flip = (O.im2col3x3(dy) @ Wt[:, :9 * cout].T)[..., :cin]
    np.testing.assert_array_equal(via_flip, O.col2im3x3(dy @ W.T, cin))
    # and it is not the unflipped kernel
    W_noflip = np.concatenate([W.reshape(9, cin, cout)[t] for t in range(9)], axis=1)
    assert not np.array_equal(O.im2col3x3(dy) @ W_noflip.T, via_flip)


@pytest.mark.parametrize("H", [28, 14, 7])
@pytest.mark.parametrize("n_img", [1, 5])
def test_pool_inputs_tie_at_a_positive_maximum_and_have_dead_windows(H, n_img):
    x = CL.pool_input(np.random.RandomState(100 * H + n_img), n_img, H, 32)
    tied, dead = CL.window_stats(x)
    assert tied >= 0.25, tied            # full windows of four: 1 - P(unique max) - P(all zero) = 0.43; fewer live cells at the odd edge
    assert dead > 0.0, dead
    out, route = O.maxpool2_same(x)
    assert route.sum() == out.size       # one pixel per window takes the gradient ...
    first = route & (x > 0)
    assert first.sum() < route.sum()     # ... unless the window is dead: the `> 0` gate is observable


def test_pool_side_one_has_a_single_live_cell():
    x = CL.pool_input(np.random.RandomState(3), 5, 1, 32)
    out, route = O.maxpool2_same(x)
    np.testing.assert_array_equal(out, x)
    assert route.all()


def test_integer_operands_stay_exact_in_fp32():
    """every sum the kernels form is an integer below 2^24, so fp32 accumulation in any order is exact"""
    rng = np.random.RandomState(1)
    v = CL.ints(rng, (4096,))
    assert v.min() == -3 and v.max() == 3
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    import torch
    assert torch.equal(torch.as_tensor(v).to(torch.bfloat16).double(), torch.as_tensor(v))
    assert CL.max_abs_sum(9 * 128) < 2 ** 24                   # forward / input gradient: 9 taps x 128 channels
    assert CL.max_abs_sum(512 * 9 * 9, 0) < 2 ** 24           # weight gradient: 512 images of 9 x 9 padded pixels
    assert CL.max_abs_sum(4 * 16 * 16, 0) < 2 ** 24
    for H, n in CL.FIRST_DW_CASES:                             # first layer's weight gradient: every pixel of every image
        assert CL.max_abs_sum(n * H * H, 0) < 2 ** 24
    assert CL.max_abs_sum(9) < 2 ** 8                          # first layer forward: exact in bf16 as well


def test_first_layer_grid_geometries():
    assert [CL.first_fwd_grid(H, n) for H, n in CL.FIRST_FWD_CASES] == [(1, 1), (2, 1), (4096, 2)]
    assert CL.first_units(4, 3) == 12                          # one partly filled block
    assert CL.first_units(28, 1400) > 4096 * 64                # the grid-stride loop runs
    got = [CL.first_dw_grid(H, n) for H, n in CL.FIRST_DW_CASES]
    assert [g[0] for g in got] == [1, 33, 65, 512, 512]
    assert CL.first_units(4, 8208) == 32832 and got[3] == (512, 65, 506)      # blocks from 506 on start past the end
    assert got[4][1] == 77 and got[4][2] == 510                # the long loop: two passes of the 64 unit lanes per block (and two empty blocks)
    assert all(g[2] is None for g in got[:3])


def test_first_dw_block_count_is_the_library_s():
    """the geometry above is not a copy that can drift: the size query of dmvae_debug_conv_first_dw (no launch, no GPU) gives the same counts"""
    import ctypes as C
    from dmvae_hip import _lib
    for H, n in CL.FIRST_DW_CASES + [(28, 4096), (8, 5)]:
        nb = C.c_int(-1)
        _lib.check(_lib.lib.dmvae_debug_conv_first_dw(None, _lib.BF16, None, H * H, H, n, None, 32, None, 64, None, None, 0, C.byref(nb)), "blocks")
        assert nb.value == CL.first_dw_grid(H, n)[0], (H, n)
    # and the entries refuse what they cannot run, before any launch
    assert _lib.lib.dmvae_debug_conv_dw(None, _lib.BF16, 1000, 16, 32, None, 32, None, 32, 64, 32, 1, None, None, None) != 0
    assert _lib.lib.dmvae_debug_conv_gemm(None, _lib.BF16, _lib.GEMM_FWD, 64, 64, 320, None, 32, None, 64, None, 1, 0, 32) != 0
