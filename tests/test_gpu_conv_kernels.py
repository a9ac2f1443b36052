"""GPU tests of the CNN trunk, kernel by kernel (csrc/conv.hip and the conv-mode GEMMs of csrc/gemm_bf16.hip / gemm_f32.hip), through
the dmvae_debug_* entries on buffers this file owns.

Every operand is a small integer (exact in bf16), so every sum is an integer far below 2^24 and exact in fp32 whatever the order:
each comparison is for EQUALITY against the float64 oracle (oracle/dmvae_oracle.py), rounded once to the output type.  Every buffer
a kernel writes stands between two margins of a sentinel and is compared whole -- borders, pad channels, guard rows, margins."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dmvae_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import conv_layout as CL      # noqa: E402

F32, BF16 = 0, 1
TD = {F32: torch.float32, BF16: torch.bfloat16}
ES = {F32: 4, BF16: 2}
SENT = -384.0            # exact in bf16; never the margin's neighbour by accident: margins are compared, not searched for
MG = 256                 # margin elements in front of and behind every buffer (a multiple of 16 bytes in either type)
KNOB5_DEFAULT = 2        # g_conv_short as csrc/gemm_bf16.hip initialises it: the library has no getter, so the restore writes the default back
GEOM = [(6, 16, 32), (9, 64, 128), (16, 3, 3), (30, 16, 32)]        # P, images for the 64-row tiles, images for the 128-row tiles


@pytest.fixture(scope="module")
def hip():
    import dmvae_hip
    from dmvae_hip import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """a device buffer between two sentinel margins"""

    def __init__(self, host, dtype, tdt=None):
        self.tdt = tdt or TD[dtype]
        self.n = int(host.size)
        self.flat = torch.full((self.n + 2 * MG,), SENT, dtype=self.tdt, device="cuda")
        self.flat[MG:MG + self.n] = torch.as_tensor(np.array(host, dtype=np.float32).reshape(-1)).cuda().to(self.tdt)

    def ptr(self, off=0):
        return C.c_void_p(self.flat.data_ptr() + (MG + off) * self.flat.element_size())

    def body(self):
        return self.flat[MG:MG + self.n]

    def check(self, expected, what):
        """the whole buffer, margins included, equals `expected` (float64, rounded float32 -> the buffer's type once)"""
        exp = torch.full_like(self.flat, SENT)
        exp[MG:MG + self.n] = torch.as_tensor(np.array(expected, dtype=np.float32).reshape(-1)).cuda().to(self.tdt)
        if not torch.equal(self.flat, exp):
            got, want = self.flat.float().cpu().numpy(), exp.float().cpu().numpy()
            assert (got[:MG] == SENT).all() and (got[-MG:] == SENT).all(), "%s: wrote outside its buffer" % (what,)
            np.testing.assert_array_equal(got[MG:-MG], want[MG:-MG], err_msg=str(what))
            raise AssertionError("%s: torch.equal found a difference that the NumPy comparison did not" % (what,))


def sent(shape):
    return np.full(shape, SENT, np.float64)


def epilogue(L, kind, out, ldo, n_valid, bias=None, aux0=None, ld0=0):
    e = L.Epilogue()
    e.kind, e.out, e.ldo, e.n_valid = kind, out.value, ldo, n_valid
    if bias is not None:
        e.bias = bias.value
    if aux0 is not None:
        e.aux0, e.ld0 = aux0.value, ld0
    return e


class overrides:
    """tile / knob-5 override, restored on exit"""

    def __init__(self, L, tile=None, knob5=None):
        self.L, self.tile, self.knob5 = L, tile, knob5

    def __enter__(self):
        try:
            if self.tile:
                self.L.check(self.L.lib.dmvae_debug_set_tile(*self.tile), "set_tile")
            if self.knob5 is not None:
                self.L.check(self.L.lib.dmvae_debug_set_knob(5, self.knob5), "set_knob")
        except Exception:
            self.__exit__()
            raise

    def __exit__(self, *a):
        self.L.lib.dmvae_debug_set_tile(0, 0)
        self.L.lib.dmvae_debug_set_knob(5, KNOB5_DEFAULT)


def tile_variants(N):
    """(dtype, tile, knob 5, 128-row tile?) -- every conv tile N divides, the 128x64 tile under both settings of knob 5, and fp32"""
    v = [(BF16, (64, 64), None, False), (BF16, (128, 64), 2, True), (BF16, (128, 64), 0, True)]
    if N % 128 == 0:
        v += [(BF16, (64, 128), None, False), (BF16, (128, 128), None, True)]
    return v + [(F32, None, None, False)]


def tile_divides(tile, M, N):
    """gemm_bf16_tile_m takes a forced tile only where it divides M and N, and falls back to its own choice otherwise, without a word"""
    return tile is None or (M % tile[0] == 0 and N % tile[1] == 0)


# ------------------------------------------------------------------------------------------------ conv-mode forward
FWD_CFG = [(32, 64, 32, 32), (32, 64, 64, 64), (64, 64, 64, 64), (64, 128, 128, 128), (128, 128, 128, 128)]     # conv_c, N, n_valid, ldo


@functools.lru_cache(maxsize=4)
def fwd_case(P, n_img, conv_c, N, n_valid):
    rng = np.random.RandomState(P * 1000 + conv_c + N + n_valid)
    H, K = P - 2, CL.pad64(9 * conv_c)
    x = CL.ints(rng, (n_img, H, H, conv_c))
    W = np.zeros((K, N))
    W[:9 * conv_c] = CL.ints(rng, (9 * conv_c, N))          # pad COLUMNS (>= n_valid) are non-zero on purpose: the store must drop them
    b = CL.ints(rng, (N,))
    ref = np.maximum(O.im2col3x3(x) @ W[:9 * conv_c, :n_valid] + b[:n_valid], 0)
    for a in (x, W, b, ref):
        a.setflags(write=False)
    return x, W, b, ref


def run_fwd(L, dtype, P, n_img, conv_c, N, n_valid, ldo, lda, guard=0.0, tile=None):
    x, W, b, ref = fwd_case(P, GEOM_MAX[P], conv_c, N, n_valid)
    x, ref = x[:n_img], ref[:n_img]
    M, K = n_img * P * P, CL.pad64(9 * conv_c)
    assert tile_divides(tile, M, N), (tile, M, N)
    xr, xoff = CL.pack(x, lda, guard)
    A, Wd, bd = Buf(xr, dtype), Buf(W, dtype), Buf(b, F32)
    out = Buf(sent((2 * (P + 1) + M, ldo)), dtype)
    ooff = (P + 1) * ldo
    e = epilogue(L, L.EPI_BIAS_RELU, out.ptr(ooff), ldo, n_valid, bias=bd.ptr())
    L.check(L.lib.dmvae_debug_conv_gemm(stream(), dtype, L.GEMM_FWD, M, N, K, A.ptr(xoff), lda, Wd.ptr(), N, C.byref(e), 1, P, conv_c), "conv fwd")
    L.check(L.lib.dmvae_debug_zero_border(stream(), dtype, out.ptr(ooff), P, ldo, n_img), "zero_border")
    torch.cuda.synchronize()
    return out, CL.pack(ref, ldo, SENT)[0]


GEOM_MAX = {P: big for P, small, big in GEOM}


@pytest.mark.parametrize("geom", GEOM, ids=lambda g: "P%d" % g[0])
@pytest.mark.parametrize("cfg", FWD_CFG, ids=lambda c: "c%d_N%d_v%d" % c[:3])
def test_conv_forward_every_tile(hip, geom, cfg):
    """relu(im2col3x3(x) @ W + b) on the interior pixels, zero on the border, nothing outside the n_valid columns"""
    L = hip
    (P, small, big), (conv_c, N, n_valid, ldo) = geom, cfg
    for dtype, tile, knob5, rows128 in tile_variants(N):
        for lda in ([conv_c, 64] if cfg == FWD_CFG[0] else [conv_c]):       # 32 real channels stored 32 wide, and stored 64 wide
            with overrides(L, tile, knob5):
                out, want = run_fwd(L, dtype, P, big if rows128 else small, conv_c, N, n_valid, ldo, lda, tile=tile)
            out.check(want, ("fwd", P, cfg, dtype, tile, knob5, lda))


# ------------------------------------------------------------------------------------------------ conv-mode input gradient
@functools.lru_cache(maxsize=4)
def dx_case(P, n_img, cout, cin):
    rng = np.random.RandomState(P * 1000 + 7 * cout + cin)
    H = P - 2
    dy = CL.ints(rng, (n_img, H, H, cout))
    W = CL.ints(rng, (9 * cin, CL.pad64(cout)))              # pad columns (>= cout) non-zero: conv_wflip must not pick them up
    act = CL.pool_input(rng, n_img, H, cin)                  # the gate: zeros inside the image as well
    ref = O.col2im3x3(dy @ W[:, :cout].T, cin) * (act > 0)
    for a in (dy, W, act, ref):
        a.setflags(write=False)
    return dy, W, act, ref


def run_dx(L, dtype, P, n_img, cout, cin, guard=0.0, tile=None):
    dy, W, act, ref = dx_case(P, GEOM_MAX[P], cout, cin)
    dy, act, ref = dy[:n_img], act[:n_img], ref[:n_img]
    M, Kt, cin_np = n_img * P * P, CL.pad64(9 * cout), CL.pad64(cin)
    assert tile_divides(tile, M, cin_np), (tile, M, cin_np)
    dyr, doff = CL.pack(dy, cout, guard)
    actr, aoff = CL.pack(act, cin)
    A, Wd, G = Buf(dyr, dtype), Buf(W, dtype), Buf(actr, dtype)
    Wt = Buf(sent((cin_np, Kt)), dtype)
    out = Buf(sent(actr.shape), dtype)
    L.check(L.lib.dmvae_debug_conv_wflip(stream(), dtype, Wd.ptr(), cin, cin_np, cout, W.shape[1], Wt.ptr(), Kt), "conv_wflip")
    e = epilogue(L, L.EPI_RELU_MASK, out.ptr(aoff), cin, cin, aux0=G.ptr(aoff), ld0=cin)
    L.check(L.lib.dmvae_debug_conv_gemm(stream(), dtype, L.GEMM_DX, M, cin_np, Kt, A.ptr(doff), cout, Wt.ptr(), Kt, C.byref(e), 1, P, cout), "conv dx")
    torch.cuda.synchronize()
    Wt.check(CL.wflip_reference(W[:, :cout], cin, cin_np, cout, Kt), ("wflip", cout, cin, dtype))
    return out, CL.pack(ref, cin, SENT)[0]


@pytest.mark.parametrize("geom", GEOM, ids=lambda g: "P%d" % g[0])
@pytest.mark.parametrize("cin", [32, 64, 128])
@pytest.mark.parametrize("cout", [32, 64, 128])
def test_conv_input_gradient_every_tile(hip, geom, cout, cin):
    """col2im3x3(dy @ W.T) * (act > 0), the border exactly zero; the weights go through conv_wflip as in the plan"""
    L = hip
    P, small, big = geom
    for dtype, tile, knob5, rows128 in tile_variants(CL.pad64(cin)):
        with overrides(L, tile, knob5):
            out, want = run_dx(L, dtype, P, big if rows128 else small, cout, cin, tile=tile)
        out.check(want, ("dx", P, cout, cin, dtype, tile, knob5))


# ------------------------------------------------------------------------------------------------ conv-mode weight / bias gradient
DW_GEOM = [(16, 4, (1, 2, 8, 16)), (9, 512, (1, 3, 8))]       # P, images, splits (split 1 is the baseline the others must equal)
DW_CFG = [(64, 32), (64, 64), (128, 128)]                       # N, n_valid


@functools.lru_cache(maxsize=2)
def dw_input(P, n_img, conv_c):
    x = CL.ints(np.random.RandomState(P + conv_c), (n_img, P - 2, P - 2, conv_c))
    col = O.im2col3x3(x).reshape(-1, 9 * conv_c).T.copy()
    x.setflags(write=False)
    col.setflags(write=False)
    return x, col


@functools.lru_cache(maxsize=4)
def dw_case(P, n_img, conv_c, N, n_valid):
    x, col = dw_input(P, n_img, conv_c)
    dy = CL.ints(np.random.RandomState(P + conv_c + N + n_valid), (n_img, P - 2, P - 2, n_valid))
    dW = np.zeros((CL.pad64(9 * conv_c), N))                  # rows past 9 * conv_c and columns past n_valid: zero
    dW[:9 * conv_c, :n_valid] = col @ dy.reshape(-1, n_valid)
    db = np.zeros(N)
    db[:n_valid] = dy.reshape(-1, n_valid).sum(0)
    return x, dy, dW, db


def run_dw(L, dtype, P, n_img, conv_c, N, n_valid, split, A, dY, offs):
    kdim = CL.pad64(9 * conv_c)
    dW, db = Buf(sent((kdim, N)), F32), Buf(sent((N,)), F32)
    slab = Buf(sent((split * (kdim + 1) * N,)), F32) if split > 1 else None
    L.check(L.lib.dmvae_debug_conv_dw(stream(), dtype, n_img * P * P, P, conv_c, A.ptr(offs[0]), conv_c, dY.ptr(offs[1]), n_valid, N, n_valid, split,
                                      slab.ptr() if slab else None, dW.ptr(), db.ptr()), "conv dw")
    torch.cuda.synchronize()
    if slab is not None:
        assert (slab.flat[:MG] == SENT).all() and (slab.flat[-MG:] == SENT).all(), "slabs: wrote outside the buffer"
    return dW, db


@pytest.mark.parametrize("cfg", DW_CFG, ids=lambda c: "N%d_v%d" % c)          # (varies fastest: the patch matrix of a (geometry, conv_c) is built once)
@pytest.mark.parametrize("geom", DW_GEOM, ids=lambda g: "P%d" % g[0])
@pytest.mark.parametrize("conv_c", [32, 64, 128])
def test_conv_weight_gradient_splits_and_rings(hip, geom, cfg, conv_c):
    """col.T @ dy and dy.sum(0); zero pad rows (conv_c = 32: rows 288..319) and pad columns; every split gives the bits of split 1, twice"""
    L = hip
    (P, n_img, splits), (N, n_valid) = geom, cfg
    x, dy, dW_ref, db_ref = dw_case(P, n_img, conv_c, N, n_valid)
    (xr, xoff), (dyr, doff) = CL.pack(x, conv_c), CL.pack(dy, n_valid)
    for dtype in (BF16, F32):
        A, dY = Buf(xr, dtype), Buf(dyr, dtype)
        for knob5 in ((2, 0) if dtype == BF16 else (None,)):         # 3-slot and 4-slot rings of the 64x64 tile
            base = None
            for split in splits:
                for rep in range(1 if split == 1 else 2):
                    with overrides(L, None, knob5):
                        dW, db = run_dw(L, dtype, P, n_img, conv_c, N, n_valid, split, A, dY, (xoff, doff))
                    what = ("dw", P, conv_c, cfg, dtype, knob5, split, rep)
                    dW.check(dW_ref, what)
                    db.check(db_ref, what)
                    if base is None:
                        base = (dW.flat.clone(), db.flat.clone())
                    assert torch.equal(dW.flat, base[0]) and torch.equal(db.flat, base[1]), what


# ------------------------------------------------------------------------------------------------ guard rows
def test_guard_rows_never_reach_a_result(hip):
    """csrc/conv.hip: guard rows feed border-pixel outputs only (re-zeroed, or gated to zero) and meet only zero rows of dY"""
    L = hip
    P, n_img = 9, 64
    for dtype in (BF16, F32):
        a, want = run_fwd(L, dtype, P, n_img, 32, 64, 32, 32, 32, guard=0.0)
        b, _ = run_fwd(L, dtype, P, n_img, 32, 64, 32, 32, 32, guard=7.0)
        b.check(want, ("fwd, guard 7", dtype))
        assert torch.equal(a.flat, b.flat)
        a, want = run_dx(L, dtype, P, n_img, 64, 32, guard=0.0)
        b, _ = run_dx(L, dtype, P, n_img, 64, 32, guard=7.0)
        b.check(want, ("dx, guard 7", dtype))
        assert torch.equal(a.flat, b.flat)
        x, dy, dW_ref, db_ref = dw_case(16, 4, 32, 64, 32)
        dyr, doff = CL.pack(dy, 32)
        res = []
        for guard in (0.0, 7.0):
            xr, xoff = CL.pack(x, 32, guard)
            for split in (1, 8):
                dW, db = run_dw(L, dtype, 16, 4, 32, 64, 32, split, Buf(xr, dtype), Buf(dyr, dtype), (xoff, doff))
                dW.check(dW_ref, ("dw, guard", guard, dtype, split))
                db.check(db_ref, ("db, guard", guard, dtype, split))
                res.append(dW.flat)
        assert all(torch.equal(res[0], r) for r in res[1:])


# ------------------------------------------------------------------------------------------------ which kernel a tile override selects
def kernels_launched(L, fn):
    rows = (L.ProfRow * 32)()
    L.lib.dmvae_prof_collect(rows, 32)          # drop whatever was recorded before
    L.lib.dmvae_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.lib.dmvae_prof_enable(0)
        n = L.lib.dmvae_prof_collect(rows, 32)
    return [rows[i].name.decode() for i in range(n)]


def test_overrides_reach_every_conv_tile_variant(hip):
    """the tile / knob overrides of the tests above select the kernels launch_tiled has, for the forward and the weight gradient (the input
    gradient takes the same branch of launch_tiled; its names are not checked):
    gemm_bf16_conv_kernel<BM, BN, layout, epilogue, ring slots, waves>, the two enums as the binding numbers them"""
    L = hip
    P, n_img = 6, 32

    def kname(bm, bn, layout, epi, slots, waves):
        return "gemm_bf16_conv_kernel<%d, %d, %d, %d, %d, %d>" % (bm, bn, layout, epi, slots, waves)

    ring = {((64, 64), None): (4, 4), ((64, 128), None): (3, 4), ((128, 128), None): (2, 8), ((128, 64), 2): (2, 4), ((128, 64), 0): (3, 8)}
    for conv_c in (32, 64, 128):                      # K = 320 / 576 (short) / 1152
        for (tile, knob5), sw in ring.items():
            if conv_c == 128 and tile == (128, 64):
                sw = (3, 8)                           # K = 1152 always takes the 3-slot / 8-wave kernel
            with overrides(L, tile, knob5):
                got = kernels_launched(L, lambda: run_fwd(L, BF16, P, n_img, conv_c, 128, 128, 128, conv_c, tile=tile))
            assert kname(*tile, L.GEMM_FWD, L.EPI_BIAS_RELU, *sw) in got, (conv_c, tile, knob5, got)
    x, dy, _, _ = dw_case(16, 4, 32, 64, 32)
    (xr, xoff), (dyr, doff) = CL.pack(x, 32), CL.pack(dy, 32)
    A, dY = Buf(xr, BF16), Buf(dyr, BF16)
    for knob5, split, epi, slots in [(2, 1, L.EPI_ATOMIC_F32, 3), (0, 1, L.EPI_ATOMIC_F32, 4), (2, 8, L.EPI_STORE_F32, 3), (0, 8, L.EPI_STORE_F32, 4)]:
        with overrides(L, None, knob5):
            got = kernels_launched(L, lambda: run_dw(L, BF16, 16, 4, 32, 64, 32, split, A, dY, (xoff, doff)))
        assert kname(64, 64, L.GEMM_DW, epi, slots, 4) in got, (knob5, split, got)
        assert ("slab_reduce" in got) == (split > 1), got
    x, dy, _, _ = dw_case(16, 4, 32, 128, 128)
    (xr, xoff), (dyr, doff) = CL.pack(x, 32), CL.pack(dy, 128)
    A, dY = Buf(xr, BF16), Buf(dyr, BF16)
    got = kernels_launched(L, lambda: run_dw(L, BF16, 16, 4, 32, 128, 128, 1, A, dY, (xoff, doff)))
    assert kname(64, 128, L.GEMM_DW, L.EPI_ATOMIC_F32, 3, 4) in got, got


# ------------------------------------------------------------------------------------------------ first layer
def first_operands(rng, H, n_img, bstride):
    x = sent((n_img, bstride))                                   # the gap between images is never read: a sentinel would show
    img = CL.ints(rng, (n_img, H, H, 1))
    x[:, :H * H] = img.reshape(n_img, -1)
    return x, img


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("H,n_img,ld,bstride", [(4, 3, 32, 16), (4, 3, 64, 16), (8, 5, 32, 64), (8, 5, 64, 80), (28, 1400, 32, 784)])
def test_conv_first_forward(hip, dtype, H, n_img, ld, bstride):
    """relu(b + sum_t x[pix + tap t] W[t]) into the interior's 32 channels; border, pad channels and margins keep the sentinel"""
    L = hip
    rng = np.random.RandomState(H * n_img + ld)
    P, ldw = H + 2, 64
    x, img = first_operands(rng, H, n_img, bstride)
    W, b = CL.ints(rng, (9, ldw)), CL.ints(rng, (32,))           # columns 32..63 of W are not part of the layer
    want = sent((n_img, P, P, ld))
    want[:, 1:-1, 1:-1, :32] = np.maximum(O.im2col3x3(img) @ W[:, :32] + b, 0)
    out, X, Wd, bd = Buf(sent((n_img, P, P, ld)), dtype), Buf(x, dtype), Buf(W, dtype), Buf(b, F32)
    L.check(L.lib.dmvae_debug_conv_first_fwd(stream(), dtype, X.ptr(), bstride, H, n_img, Wd.ptr(), ldw, bd.ptr(), out.ptr(), ld), "conv_first_fwd")
    torch.cuda.synchronize()
    out.check(want, ("conv_first_fwd", dtype, H, n_img, ld, bstride))


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("case", list(zip(CL.FIRST_DW_CASES, [1, 33, 65, 512, 512], [32, 64, 32, 64, 32])), ids=lambda c: "H%d_n%d" % c[0])
def test_conv_first_weight_gradient(hip, dtype, case):
    """dW[t] = sum x[pix + tap t] dY[pix], db = sum dY, over every block count of the two-stage sum -- 1, 33, 65, 512 with blocks that
    start past the last unit, 512 with more than one pass per block -- twice, same bits"""
    L = hip
    (H, n_img), blocks, ld = case
    rng = np.random.RandomState(H + n_img)
    P, ldw, bstride = H + 2, 64, H * H
    x, img = first_operands(rng, H, n_img, bstride)
    dyi = CL.ints(rng, (n_img, H, H, 32))
    dy = np.full((n_img, P, P, ld), 5.0)                          # border pixels and pad channels of dY are never read
    dy[:, 1:-1, 1:-1, :32] = dyi
    dW_ref = sent((9, ldw))
    dW_ref[:, :32] = O.im2col3x3(img).reshape(-1, 9).T @ dyi.reshape(-1, 32)
    db_ref = dyi.reshape(-1, 32).sum(0)
    nb = C.c_int(0)
    L.check(L.lib.dmvae_debug_conv_first_dw(stream(), dtype, None, bstride, H, n_img, None, ld, None, ldw, None, None, 0, C.byref(nb)), "blocks")
    assert nb.value == blocks == CL.first_dw_grid(H, n_img)[0]
    X, dY = Buf(x, dtype), Buf(dy, dtype)
    runs = []
    for rep in range(2):
        dW, db, part = Buf(sent((9, ldw)), F32), Buf(sent((32,)), F32), Buf(sent((blocks * 320,)), F32)
        L.check(L.lib.dmvae_debug_conv_first_dw(stream(), dtype, X.ptr(), bstride, H, n_img, dY.ptr(), ld, dW.ptr(), ldw, db.ptr(), part.ptr(),
                                                blocks * 320, C.byref(nb)), "conv_first_dw")
        torch.cuda.synchronize()
        dW.check(dW_ref, ("conv_first_dw", dtype, case, rep))
        db.check(db_ref, ("conv_first_db", dtype, case, rep))
        assert (part.flat[:MG] == SENT).all() and (part.flat[-MG:] == SENT).all() and not (part.body() == SENT).any()
        runs.append((dW.flat, db.flat, part.flat))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("ld", [32, 128])
@pytest.mark.parametrize("H", CL.POOL_SIDES)
def test_maxpool_forward_and_first_maximum_gradient(hip, dtype, ld, H):
    """maxpool2_same, and maxpool2_same_backward(dout, first maximum) * (x > 0), on inputs that tie at a positive maximum in ~43 % of the
    windows and have all-zero windows (tests/test_conv_layout_host.py); both output forms; border pixels keep their sentinel"""
    L = hip
    P, Ho = H + 2, (H + 1) // 2
    for n_img in (1, 5):
        rng = np.random.RandomState(H * 10 + n_img + ld)
        x = CL.pool_input(rng, n_img, H, ld)
        pooled, route = O.maxpool2_same(x)
        dout = CL.ints(rng, (n_img, Ho, Ho, ld))
        din_ref = sent((n_img, P, P, ld))
        din_ref[:, 1:-1, 1:-1] = O.maxpool2_same_backward(dout, route) * (x > 0)
        xr, xoff = CL.pack(x, ld)
        X = Buf(xr, dtype)
        for border in (0, 1):
            Po = Ho + 2 * border
            want, dpool = sent((n_img, Po, Po, ld)), sent((n_img, Po, Po, ld))
            inner = (slice(None), slice(border, Po - border), slice(border, Po - border))
            want[inner], dpool[inner] = pooled, dout
            out = Buf(sent(want.shape), dtype)
            L.check(L.lib.dmvae_debug_maxpool2_fwd(stream(), dtype, X.ptr(xoff), H, ld, n_img, out.ptr(), border), "maxpool2_fwd")
            din, dP = Buf(sent(din_ref.shape), dtype), Buf(dpool, dtype)
            L.check(L.lib.dmvae_debug_maxpool2_bwd_relu(stream(), dtype, X.ptr(xoff), dP.ptr(), H, ld, n_img, din.ptr(), border), "maxpool2_bwd")
            torch.cuda.synchronize()
            out.check(want, ("maxpool2_fwd", dtype, ld, H, n_img, border))
            din.check(din_ref, ("maxpool2_bwd_relu", dtype, ld, H, n_img, border))


# ------------------------------------------------------------------------------------------------ zero_border, conv_wflip
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("P", [6, 9, 16, 30])
def test_zero_border_touches_exactly_the_border(hip, dtype, P):
    L = hip
    for ld in (32, 64, 128):
        for n_img in (1, 7):
            rows = 2 * (P + 1) + n_img * P * P
            a = Buf(sent((rows, ld)), dtype)
            L.check(L.lib.dmvae_debug_zero_border(stream(), dtype, a.ptr((P + 1) * ld), P, ld, n_img), "zero_border")
            torch.cuda.synchronize()
            want = sent((rows, ld))
            CL.images(want, n_img, P)[:, CL.border_mask(P)] = 0.0
            assert (want == 0).sum() == n_img * (4 * P - 4) * ld
            a.check(want, ("zero_border", dtype, P, ld, n_img))


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("cin,cin_ld,cout", [(32, 64, 32), (32, 64, 64), (64, 64, 128), (128, 128, 128)])
def test_conv_wflip_is_the_flipped_transposed_kernel(hip, dtype, cin, cin_ld, cout):
    L = hip
    rng = np.random.RandomState(cin + cout)
    Kt, ldw = CL.pad64(9 * cout), CL.pad64(cout)
    W = CL.ints(rng, (9 * cin, ldw))
    Wt, Wd = Buf(sent((cin_ld, Kt)), dtype), Buf(W, dtype)
    L.check(L.lib.dmvae_debug_conv_wflip(stream(), dtype, Wd.ptr(), cin, cin_ld, cout, ldw, Wt.ptr(), Kt), "conv_wflip")
    torch.cuda.synchronize()
    Wt.check(CL.wflip_reference(W[:, :cout], cin, cin_ld, cout, Kt), ("conv_wflip", dtype, cin, cin_ld, cout))
