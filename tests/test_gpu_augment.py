"""dmvae_augment_rows (csrc/augment.hip) on the GPU against the float64 oracle of tests/helpers/augment_oracle.py: lattice maps in bits, general
maps and the draw within DERIVED bounds, chunking, pad columns, refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import augment_oracle as AO                  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
U = 2.0 ** -24
SPEC = (30.0, 3.0, (0.8, 1.25), 10.0)        # rotate [deg], translate [px], scale (lo, hi), shear [deg]

# (n, H, W, ldx, ldo, row_base): 1 x 1 | ragged, several images per wave round | unequal strides that break the 16-byte alignment of most rows |
# the product size | padded strides and a row index past 2^31 | the largest image (the block owns it) | more images than a block holds, odd sides
SHAPES = [(1, 1, 1, 1, 1, 0), (5, 5, 3, 15, 15, 0), (33, 5, 3, 17, 20, 7), (7, 28, 28, 784, 784, 0), (9, 28, 28, 800, 788, (1 << 31) + 3),
          (3, 64, 64, 4096, 4096, 0), (130, 7, 9, 63, 64, 1)]
# more images than one sweep of the grid: 2048 blocks x 4 waves (wave form), 2048 blocks (block form: 33 x 33 > 1024 pixels)
SWEEPS = [(8200, 5, 3, 15, 15, 0), (2050, 33, 33, 1089, 1092, 5)]


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def grey(n, d, seed):
    """values in [0, 1) with exact zeros, as the pixels of an image set: the image range R is 1"""
    rng = np.random.RandomState(seed)
    return (rng.rand(n, d) * (rng.rand(n, d) < 0.6)).astype(np.float32)


def strided(X, ld, offset=0):
    """X as a view of columns offset .. offset + d of a [n][ld + offset] device buffer filled with NaN between the rows"""
    n, d = X.shape
    buf = torch.full((n, ld + offset), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, offset:offset + d] = dev(X)
    return buf[:, offset:offset + d], buf


def out_buffer(n, d, ld, offset=0):
    buf = torch.full((n, ld + offset), SENTINEL, dtype=torch.float32, device="cuda")
    return buf[:, offset:offset + d], buf


def spec_of(H, W, spec=SPEC):
    from dmvae_hip.augment import AugmentSpec
    return AugmentSpec(rotate=spec[0], translate=spec[1], scale=spec[2], shear=spec[3], image_shape=(H, W))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def coordinate_eps(theta, H, W):
    """eps_x, eps_y [n]: the float32 error of sx = fmaf(m00, j, fmaf(m01, i, m02)) over the image, two roundings of magnitudes at most
    |m00| W + |m01| H + |m02|, from the case's own theta"""
    t = np.abs(np.asarray(theta, dtype=np.float64))
    return 2 * U * (t[:, 0] * W + t[:, 1] * H + t[:, 2] + 1), 2 * U * (t[:, 3] * W + t[:, 4] * H + t[:, 5] + 1)


def warp_bound(theta, H, W, R=1.0, extra=0.0):
    """|out - warp64| per row: the blend is piecewise linear in the coordinates with slope at most R per pixel, and the blend itself
    (three fused lerps, three differences) errs by at most 8 * 2^-24 R"""
    ex, ey = coordinate_eps(theta, H, W)
    return R * (ex + ey + 2 * extra) + 8 * U * R


def random_thetas(n, H, W, seed):
    """float32 [n][6]: rotations up to 45 degrees, scales 0.5 .. 2, shears up to 20 degrees, translations up to W (H)"""
    rng = np.random.RandomState(seed)
    ang, sc = np.deg2rad(rng.uniform(-45, 45, n)), rng.uniform(0.5, 2.0, n)
    k = np.tan(np.deg2rad(rng.uniform(-20, 20, n)))
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    m00, m01, m10, m11 = (np.cos(ang) + k * np.sin(ang)) / sc, (np.sin(ang) - k * np.cos(ang)) / sc, -np.sin(ang) / sc, np.cos(ang) / sc
    qx, qy = cx + rng.uniform(-W, W, n), cy + rng.uniform(-H, H, n)
    return np.stack([m00, m01, cx - m00 * qx - m01 * qy, m10, m11, cy - m10 * qx - m11 * qy], -1).astype(np.float32)


def lattice_maps(H, W):
    """(name, theta) of the integer maps; the quarter turns need a square image"""
    maps = [("identity", [1, 0, 0, 0, 1, 0]), ("left 1", [1, 0, 1, 0, 1, 0]), ("right 2 down 1", [1, 0, -2, 0, 1, -1]), ("up 1", [1, 0, 0, 0, 1, 1]),
            ("out to the left", [1, 0, W, 0, 1, 0]), ("out to the bottom", [1, 0, 0, 0, 1, -H]), ("far out", [1, 0, -3 * W, 0, 1, 5 * H]),
            ("flip x", [-1, 0, W - 1, 0, 1, 0]), ("flip y", [1, 0, 0, 0, -1, H - 1])]
    if H == W:
        maps += [("quarter turn", [0, 1, 0, -1, 0, H - 1]), ("half turn", [-1, 0, W - 1, 0, -1, H - 1]), ("three quarter turn", [0, -1, W - 1, 1, 0, 0])]
    return maps


def lattice_expect(img, name, th):
    """what the map does to the image, by NumPy slicing where the map has a name for it, by the integer gather otherwise"""
    H, W = img.shape
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sx, sy = th[0] * j + th[1] * i + th[2], th[3] * j + th[4] * i + th[5]
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    want = np.where(ok, img[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], np.float32(0))
    named = {"identity": lambda: img, "flip x": lambda: img[:, ::-1], "flip y": lambda: img[::-1], "quarter turn": lambda: np.rot90(img, -1),
             "half turn": lambda: img[::-1, ::-1], "three quarter turn": lambda: np.rot90(img, 1)}
    if name in named:
        assert np.array_equal(want, named[name]()), name
    if name.startswith(("out", "far")):
        assert not want.any(), name
    return want


@pytest.mark.parametrize("n,H,W,ldx,ldo,row_base", SHAPES)
def test_lattice_maps_copy_bits(n, H, W, ldx, ldo, row_base):
    from dmvae_hip.augment import augment
    maps = lattice_maps(H, W)
    rows = max(n, len(maps))                                     # every map at least once, whatever n
    X = grey(rows, H * W, 3 + n)
    theta = np.array([maps[r % len(maps)][1] for r in range(rows)], np.float32)
    Xv, _ = strided(X, ldx)
    ov, obuf = out_buffer(rows, H * W, ldo)
    got, used = augment(Xv, spec_of(H, W), row_base=row_base, theta=dev(theta), out=ov, return_theta=True)
    assert got is ov and np.array_equal(bits(used.cpu().numpy()), bits(theta))
    host = obuf.cpu().numpy()
    for r in range(rows):
        name, th = maps[r % len(maps)]
        want = lattice_expect(X[r].reshape(H, W), name, th)
        assert np.array_equal(bits(host[r, :H * W]), bits(want.reshape(-1))), (r, name)
    assert (host[:, H * W:] == SENTINEL).all()                   # pad columns of out keep the sentinel


@pytest.mark.parametrize("n,H,W,ldx,ldo,row_base", SHAPES)
def test_general_maps_hold_the_derived_bound(n, H, W, ldx, ldo, row_base):
    from dmvae_hip.augment import augment
    rows = max(n, 8)
    X = grey(rows, H * W, 5 + n)
    theta = random_thetas(rows, H, W, 7 + n)
    Xv, _ = strided(X, ldx)
    ov, obuf = out_buffer(rows, H * W, ldo)
    augment(Xv, spec_of(H, W), theta=dev(theta), out=ov)
    host = obuf.cpu().numpy()
    err = np.abs(host[:, :H * W].astype(np.float64) - AO.warp64(X, theta, H, W)).max(axis=1)
    bound = warp_bound(theta, H, W)
    print("max err / bound = %.3f (err %.3e)" % ((err / bound).max(), err.max()))
    assert (err <= bound).all()
    assert (host[:, H * W:] == SENTINEL).all()
    if H * W > 1:
        assert host[:, :H * W].any()                             # (the maps keep part of most images in view)
    fresh = augment(Xv, spec_of(H, W), theta=dev(theta))         # allocated by the call
    assert fresh.shape == (rows, H * W) and fresh.is_contiguous() and np.array_equal(bits(fresh.cpu().numpy()), bits(host[:, :H * W]))


@pytest.mark.parametrize("xoff,ooff", [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (2, 1)])
def test_misaligned_bases_take_the_scalar_paths(xoff, ooff):
    """a 16-byte-aligned buffer entered at a column offset: every row of X (of out) is misaligned although ld and H W are multiples of 4"""
    from dmvae_hip.augment import augment
    n, H, W = 9, 28, 28
    X = grey(n, H * W, 21)
    theta = dev(random_thetas(n, H, W, 22))
    want = augment(dev(X), spec_of(H, W), theta=theta).cpu().numpy()            # the aligned call (held to the oracle above)
    Xv, _ = strided(X, 800, xoff)
    ov, obuf = out_buffer(n, H * W, 800, ooff)
    assert (Xv.data_ptr() % 16 != 0) == (xoff != 0) and (ov.data_ptr() % 16 != 0) == (ooff != 0)
    augment(Xv, spec_of(H, W), theta=theta, out=ov)
    host = obuf.cpu().numpy()
    assert np.array_equal(bits(host[:, ooff:ooff + H * W]), bits(want))
    assert (host[:, :ooff] == SENTINEL).all() and (host[:, ooff + H * W:] == SENTINEL).all()
    err = np.abs(want.astype(np.float64) - AO.warp64(X, theta.cpu().numpy(), H, W)).max(axis=1)
    assert (err <= warp_bound(theta.cpu().numpy(), H, W)).all()


def test_non_finite_and_huge_coordinates_give_zero():
    from dmvae_hip.augment import augment
    H, W = 6, 5
    X = grey(6, H * W, 2) + np.float32(0.25)
    theta = np.array([[np.nan, 0, 0, 0, 1, 0], [1, 0, np.inf, 0, 1, 0], [1, 0, 0, 0, 1, -np.inf], [3e38, 3e38, 3e38, 0, 1, 0], [1, 0, 0, 0, np.nan, 0],
                      [1, 0, 0, 0, 1, 0]], np.float32)
    got = augment(dev(X), spec_of(H, W), theta=dev(theta)).cpu().numpy()
    assert (got[:5] == 0).all() and np.array_equal(got[5], X[5])
    assert np.array_equal(got, AO.warp64(X, theta, H, W).astype(np.float32))


def test_the_draw_equals_the_oracles_to_64_ulp():
    """under ten float32 operations with sincosf, expf and tanf within a few ulp each; a swapped word moves a coefficient by its range"""
    from dmvae_hip.augment import augment
    n, H, W, row_base = 2048, 28, 28, 5
    X = dev(grey(n, H * W, 1))
    _, th = augment(X, spec_of(H, W), seed=11, counter=5, row_base=row_base, return_theta=True)
    th = th.cpu().numpy().astype(np.float64)
    p = AO.params(11, 5, row_base, n, SPEC)
    want = AO.theta64(p, H, W)
    lin, off = [0, 1, 3, 4], [2, 5]
    d = np.abs(th - want)
    b_lin = 64 * U * np.maximum(1.0, np.abs(want[:, lin]))
    b_off = 64 * U * np.maximum(np.maximum(1.0, np.abs(want[:, off])), max(W, H))
    print("draw: max err / bound  linear %.3f, offsets %.3f" % ((d[:, lin] / b_lin).max(), (d[:, off] / b_off).max()))
    assert (d[:, lin] <= b_lin).all() and (d[:, off] <= b_off).all()
    # the extreme draws lie inside the ranges -- the oracle's exactly, the device's as recovered from its matrices
    assert np.abs(p["angle"]).max() <= 30 and np.abs(p["tx"]).max() <= 3 and np.abs(p["ty"]).max() <= 3 and np.abs(p["shear"]).max() <= 10
    assert np.float32(0.8) * (1 - 1e-6) <= p["scale"].min() and p["scale"].max() <= np.float32(1.25) * (1 + 1e-6)
    scale = 1.0 / np.sqrt(th[:, 0] * th[:, 4] - th[:, 1] * th[:, 3])
    angle = np.rad2deg(np.arctan2(-th[:, 3], th[:, 4]))
    assert 0.8 - 1e-4 <= scale.min() < 0.81 and 1.24 < scale.max() <= 1.25 + 1e-4
    assert 29 < np.abs(angle).max() <= 30 + 1e-3 and angle.min() < -29 and angle.max() > 29
    assert np.abs(scale - p["scale"]).max() < 1e-4 and np.abs(angle - p["angle"]).max() < 1e-3


@pytest.mark.parametrize("n,H,W,ldx,ldo,row_base", SHAPES + SWEEPS[:1])
def test_end_to_end_draw_and_warp(n, H, W, ldx, ldo, row_base):
    from dmvae_hip.augment import augment
    X = grey(n, H * W, 9 + n)
    Xv, _ = strided(X, ldx)
    ov, obuf = out_buffer(n, H * W, ldo)
    _, th = augment(Xv, spec_of(H, W), seed=3, counter=8, row_base=row_base, out=ov, return_theta=True)
    host = obuf.cpu().numpy()
    assert (host[:, H * W:] == SENTINEL).all()
    again = augment(Xv, spec_of(H, W), theta=th)                 # the same maps, handed in: the same bits
    assert np.array_equal(bits(again.cpu().numpy()), bits(host[:, :H * W]))
    want_th = AO.theta64(AO.params(3, 8, row_base, n, SPEC), H, W)
    # the device's maps lie within the draw's bound B of the oracle's: a coordinate moves by at most B (W + H + 1)
    B = 64 * U * np.maximum(np.maximum(1.0, np.abs(want_th).max(axis=1)), max(W, H))
    assert (np.abs(th.cpu().numpy() - want_th) <= B[:, None]).all()
    err = np.abs(host[:, :H * W].astype(np.float64) - AO.warp64(X, want_th, H, W)).max(axis=1)
    bound = warp_bound(want_th, H, W, extra=B * (W + H + 1))
    print("max err / bound = %.3f" % (err / bound).max())
    assert (err <= bound).all()


@pytest.mark.parametrize("n,H,W,ldx,ldo,row_base", SHAPES + SWEEPS)
def test_identity_spec_returns_the_rows_in_bits(n, H, W, ldx, ldo, row_base):
    from dmvae_hip.augment import augment
    X = grey(n, H * W, 13 + n)
    Xv, _ = strided(X, ldx)
    ov, obuf = out_buffer(n, H * W, ldo)
    _, th = augment(Xv, spec_of(H, W, (0.0, 0.0, (1.0, 1.0), 0.0)), seed=6, counter=2, row_base=row_base, out=ov, return_theta=True)
    host = obuf.cpu().numpy()
    assert np.array_equal(bits(host[:, :H * W]), bits(X)) and (host[:, H * W:] == SENTINEL).all()
    assert np.array_equal(th.cpu().numpy(), np.tile(np.float32([1, 0, 0, 0, 1, 0]), (n, 1)))


@pytest.mark.parametrize("n,H,W,cut", [(33, 5, 3, 10), (33, 5, 3, 1), (12, 28, 28, 4), (11, 33, 33, 1), (11, 33, 33, 10)])
def test_row_chunks_with_their_row_base_equal_the_whole_call(n, H, W, cut):
    from dmvae_hip.augment import augment
    X = dev(grey(n, H * W, 6))
    s = spec_of(H, W)
    whole, th = augment(X, s, seed=9, counter=2, row_base=100, return_theta=True)
    parts, tparts = torch.full_like(whole, SENTINEL), torch.full_like(th, SENTINEL)
    _, tparts[:cut] = augment(X[:cut], s, seed=9, counter=2, row_base=100, out=parts[:cut], return_theta=True)
    _, tparts[cut:] = augment(X[cut:], s, seed=9, counter=2, row_base=100 + cut, out=parts[cut:], return_theta=True)
    assert torch.equal(whole, parts) and torch.equal(th, tparts)


def test_same_key_same_bits_other_key_other_maps():
    from dmvae_hip.augment import augment
    X = dev(grey(40, 81, 5))
    s = spec_of(9, 9)
    a, ta = augment(X, s, seed=3, counter=7, return_theta=True)
    b, tb = augment(X, s, seed=3, counter=7, return_theta=True)
    assert torch.equal(a, b) and torch.equal(ta, tb)
    for kw in (dict(seed=3, counter=8), dict(seed=4, counter=7), dict(seed=3, counter=7, row_base=1), dict(seed=3 + (1 << 32), counter=7),
               dict(seed=3, counter=7 + (1 << 32))):
        o, t = augment(X, s, return_theta=True, **kw)
        assert not (t == ta).all(dim=1).any() and not torch.equal(o, a), kw
    o, t = augment(X, s, seed=3, counter=7, row_base=1, return_theta=True)
    assert torch.equal(t[:-1], ta[1:])                           # row_base shifts the key: row r of the one is row r + 1 of the other
    assert torch.equal(ta, augment(X, s, seed=3 + (1 << 64), counter=7, return_theta=True)[1])      # the key is 64 bits wide


def test_bad_arguments_are_refused_and_nothing_is_enqueued():
    from dmvae_hip import _lib as L
    from dmvae_hip.augment import AugmentSpec, augment
    n, H, W, ld = 6, 3, 4, 14
    d = H * W
    xb = torch.full((2 * n, ld), 0.75, dtype=torch.float32, device="cuda")
    ob = torch.full((n, ld), SENTINEL, dtype=torch.float32, device="cuda")
    tin = torch.tensor([[1, 0, 0, 0, 1, 0]] * n, dtype=torch.float32, device="cuda")
    tout = torch.full((n, 6), SENTINEL, dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    F = 4                                                        # bytes per element
    good = dict(rotate_deg=10.0, translate_px=2.0, scale_lo=0.9, scale_hi=1.1, shear_deg=5.0)

    def call(X=xb.data_ptr(), ldx=ld, n_rows=n, H=H, W=W, row_base=0, p=good, theta_in=None, out=ob.data_ptr(), ldo=ld):
        ps = None if p is None else C.byref(L.AugmentParams(**p))
        return L.lib.dmvae_augment_rows(stream, X, ldx, n_rows, H, W, row_base, 1, 2, ps, theta_in, tout.data_ptr(), out, ldo)

    inf, nan = float("inf"), float("nan")
    bad = [(dict(X=None), "null X / out"), (dict(out=None), "null X / out"), (dict(p=None), "null params without theta_in"),
           (dict(n_rows=0), "n_rows=0"), (dict(n_rows=-3), "n_rows=-3"),
           (dict(H=0), "H=0"), (dict(W=0), "W=0"), (dict(H=65, ldx=65 * W, ldo=65 * W), "H=65"), (dict(W=65, ldx=65 * H, ldo=65 * H), "W=65"), (dict(H=-1), "H=-1"),
           (dict(ldx=d - 1), "ldx=11"), (dict(ldo=d - 1), "ldo=11"), (dict(row_base=-1), "row_base=-1"),
           (dict(row_base=(1 << 55) - n), "reaches 2\\^56"), (dict(row_base=(1 << 63) - 1), "reaches 2\\^56"),
           (dict(out=xb.data_ptr()), "out overlaps X"),                                        # the same rows
           (dict(out=xb.data_ptr() + F * d), "out overlaps X"),                                # the pad columns of row 0 onwards: inside X's span
           (dict(out=xb.data_ptr() + F * ((n - 1) * ld + d - 1)), "out overlaps X"),           # X's last element
           (dict(X=ob.data_ptr() + F * ((n - 1) * ld + d - 1)), "out overlaps X"),             # out's last element
           (dict(out=xb.data_ptr(), theta_in=tin.data_ptr(), p=None), "out overlaps X")]
    for key in ("rotate_deg", "translate_px", "shear_deg"):
        bad += [(dict(p=dict(good, **{key: v})), "ranges are finite and >= 0") for v in (-1.0, inf, nan)]
    bad += [(dict(p=dict(good, scale_lo=lo, scale_hi=hi)), "0 < scale_lo <= scale_hi")
            for lo, hi in ((0.0, 1.0), (-0.5, 1.0), (1.2, 1.1), (nan, 1.0), (0.5, inf), (0.5, nan))]
    for kw, text in bad:
        rc = call(**kw)
        assert rc == -1, kw                                      # DMVAE_EINVAL
        with pytest.raises(L.DmvaeError, match="dmvae_augment_rows: .*" + text):
            L.check(rc, "dmvae_augment_rows")
    torch.cuda.synchronize()
    assert (ob == SENTINEL).all() and (xb == 0.75).all() and (tout == SENTINEL).all()        # a checked return code: nothing ran
    # just clear of X's span is legal, the largest row index is, and with theta_in the ranges are not read
    assert call(out=xb.data_ptr() + F * ((n - 1) * ld + d)) == 0
    assert call(X=xb.data_ptr() + F * n * ld, out=xb.data_ptr(), ldo=ld) == 0
    assert call(row_base=(1 << 55) - n - 1) == 0
    assert call(p=None, theta_in=tin.data_ptr()) == 0 and call(p=dict(good, rotate_deg=nan), theta_in=tin.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ob[:, :d], xb[:n, :d]) and (ob[:, d:] == SENTINEL).all() and torch.equal(tout, tin)     # (the last call: the identity maps)
    # the Python surface refuses what is no [rows][columns] f32 device tensor, no image, no [n][6] theta before the library is called
    for X in (torch.zeros(3, 4), torch.zeros(3, 4, device="cuda", dtype=torch.float64), torch.zeros(16, device="cuda"), torch.zeros(4, 3, device="cuda").t()):
        with pytest.raises(ValueError, match="X must be"):
            augment(X, AugmentSpec())
    x = torch.zeros(3, 16, device="cuda")
    with pytest.raises(ValueError, match="out is"):
        augment(x, AugmentSpec(), out=torch.zeros(3, 25, device="cuda"))
    with pytest.raises(ValueError, match="no square image"):
        augment(torch.zeros(3, 15, device="cuda"), AugmentSpec())
    with pytest.raises(ValueError, match="theta must be"):
        augment(x, AugmentSpec(), theta=torch.zeros(3, 5, device="cuda"))
    with pytest.raises(ValueError, match="neither a spec nor theta"):
        augment(x)
    with pytest.raises(L.DmvaeError, match="H=1, W=4225"):
        augment(torch.zeros(2, 4225, device="cuda"), AugmentSpec(image_shape=(1, 4225)))
    with pytest.raises(L.DmvaeError, match="out overlaps X"):
        augment(x, AugmentSpec(), out=x)
