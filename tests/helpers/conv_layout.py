"""Memory layout of the CNN trunk's activations (csrc/conv.hip), and the inputs of tests/test_gpu_conv_kernels.py.

An activation lives in memory as [B][P][P][ld], P = H + 2: every image carries a zero border (the SAME padding of the 3x3
convolution), channels beyond the real ones are zero, and P + 1 guard rows stand in front of the first image and behind the last
one -- the conv-mode GEMMs run over ALL padded pixel rows and read a row's eight neighbours at fixed row offsets, so the first and
last border pixels reach (P + 1) rows outside the images.

The float64 references are oracle/dmvae_oracle.py's (im2col3x3, col2im3x3, maxpool2_same, maxpool2_same_backward); nothing of them
is repeated here.  What is here is only layout, and the integer inputs whose stated properties tests/test_conv_layout_host.py
asserts without a GPU.
"""
import numpy as np


def pad64(n):
    return (n + 63) // 64 * 64


def pack(x_nhwc, ld, guard_fill=0.0):
    """[B,H,H,C] -> (rows [(P+1) + B*P*P + (P+1), ld] float64, element offset of padded pixel 0 of image 0)."""
    B, H, W, Cn = x_nhwc.shape
    assert H == W and Cn <= ld
    P = H + 2
    buf = np.zeros((2 * (P + 1) + B * P * P, ld), np.float64)
    buf[:P + 1] = guard_fill
    buf[P + 1 + B * P * P:] = guard_fill
    img = buf[P + 1:P + 1 + B * P * P].reshape(B, P, P, ld)
    img[:, 1:-1, 1:-1, :Cn] = x_nhwc
    return buf, (P + 1) * ld


def unpack(rows, offset, B, H, Cn):
    """inverse of pack: the interior pixels and real channels, [B,H,H,C]"""
    ld = rows.shape[1]
    P = H + 2
    assert offset == (P + 1) * ld and rows.shape[0] == 2 * (P + 1) + B * P * P
    return rows[P + 1:P + 1 + B * P * P].reshape(B, P, P, ld)[:, 1:-1, 1:-1, :Cn].copy()


def images(rows, B, P):
    """view of the padded images [B,P,P,ld] of a packed array"""
    return rows[P + 1:P + 1 + B * P * P].reshape(B, P, P, rows.shape[1])


def border_mask(P):
    """[P,P] bool: the 4P - 4 border pixels"""
    m = np.ones((P, P), bool)
    m[1:-1, 1:-1] = False
    return m


def ints(rng, shape):
    """operands of the exact tests: integers in [-3, 3] -- exact in bf16, and every partial sum of K products stays below 9 K"""
    return rng.randint(-3, 4, size=shape).astype(np.float64)


def max_abs_sum(k_terms, bias=3):
    """largest magnitude a sum of k_terms products of two integers in [-3, 3] (plus a bias) can reach"""
    return 9 * k_terms + bias


def pool_input(rng, n_img, H, Cn):
    """uniform over {0, 1, 2, 3}: windows tie at a positive maximum often, and some windows are all zero"""
    return rng.randint(0, 4, size=(n_img, H, H, Cn)).astype(np.float64)


def window_stats(x):
    """(share of 2x2 SAME windows whose maximum is positive and attained more than once, share of all-zero windows) of [B,H,H,C]"""
    B, H, _, Cn = x.shape
    Ho = (H + 1) // 2
    xp = np.full((B, 2 * Ho, 2 * Ho, Cn), -1.0)
    xp[:, :H, :H] = x
    win = np.stack([xp[:, dy::2, dx::2] for dy in range(2) for dx in range(2)], axis=0)
    mx = win.max(axis=0)
    tied = ((win == mx).sum(axis=0) > 1) & (mx > 0)
    return float(tied.mean()), float((mx == 0).mean())


def wflip_reference(W, cin, cin_ld, cout, Kt):
    """the kernel of the input-gradient convolution: W [9*cin, cout] (HWIO flattened) -> Wt [cin_ld, Kt],
    Wt[ci, tap*cout + co] = W[(8 - tap)*cin + ci, co]; zero pad rows and pad columns"""
    Wt = np.zeros((cin_ld, Kt), np.float64)
    W4 = W.reshape(9, cin, cout)
    for tap in range(9):
        Wt[:cin, tap * cout:(tap + 1) * cout] = W4[8 - tap]
    return Wt


# ---- grid geometry of the first layer's kernels, as the launchers in csrc/conv.hip compute it
def first_units(H, n_img):
    return n_img * H * (H // 4)


def first_fwd_grid(H, n_img):
    """(blocks, passes of the grid-stride loop)"""
    u = first_units(H, n_img)
    nb = min((u + 63) // 64, 4096)
    return nb, -(-u // (nb * 64))


def first_dw_grid(H, n_img):
    """(blocks, units per block, first block that starts past the last unit or None)"""
    u = first_units(H, n_img)
    nb = min(512, (u + 63) // 64)
    upb = -(-u // nb)
    empty = [b for b in range(nb) if b * upb >= u]
    return nb, upb, (empty[0] if empty else None)


FIRST_FWD_CASES = [(4, 3), (8, 5), (28, 1400)]                                  # (H, images)
FIRST_DW_CASES = [(4, 3), (4, 528), (4, 1040), (4, 8208), (28, 200)]           # (H, images): 1, 33, 65, 512 (empty tail), 512 (long loop) blocks
POOL_SIDES = [28, 14, 7, 1]
