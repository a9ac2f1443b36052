"""GPU tests of dmvae_ssim_rows (csrc/ssim.hip) and dmvae_hip.ssim against the float64 oracle of tests/helpers/ssim_oracle.py.

Inputs are MNIST-like (19 % dense, blurred, scaled to [0, 1]); the other side of a comparison is, in turn, the same row, the row plus
clipped noise at five strengths, an unrelated row, 1 - X.  The oracle's own values must spread: over the cases at least one comparison
lies below 0, one in (0.3, 0.7) and one above 0.9, so that a constant cannot pass.

Tolerance of ssim: the worst-case rounding bound of the centred direct form, 8 (win^2 + 3) 2^-24 (5.9e-5 at win 11): each of the four
factors carries at most 2 (win^2 + 1) roundings relative to a denominator it cannot fall below.  It is a bound, not a measurement; the
largest device error per shape is printed.  Tolerance of sse: relative, (planes H W + 2) 2^-24; on rows of multiples of 1/16 sse is exact.
In bits: ssim(X, X) == 1.0, swapped sides give the same bits, and so does a second call into the same buffers."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import ssim_oracle as SO      # noqa: E402

pytestmark = pytest.mark.gpu

C1, C2 = SO.constants()
# (pairs, planes, H, W, win): one window; two windows; the MNIST shape; three planes; more than one workgroup with a ragged last one and
# a ragged last strip; the LDS limit (one comparison per workgroup)
SHAPES = [(1, 1, 11, 11, 11), (3, 1, 12, 11, 11), (5, 1, 28, 28, 11), (2, 3, 32, 32, 11), (257, 1, 16, 13, 7), (4, 1, 64, 64, 3)]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def padded(a, pad):
    """a [n][D] on the device at row stride D + pad, NaN between the rows: reading there would poison a comparison"""
    a = np.asarray(a, dtype=np.float32)
    t = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device="cuda")
    t[:, :a.shape[1]] = torch.as_tensor(a).cuda()
    return t


def raw(Xd, Yd, shape, w, n_pairs, ix=None, iy=None, out=None, want_sse=True, flag=None, expect=0):
    """dmvae_ssim_rows through the C entry on row-padded device buffers; out: the (ssim, sse) buffers of an earlier call, written again.
    Returns (ssim, sse or None, flag value, out)"""
    from dmvae_hip import _lib
    planes, H, W = shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    dev = lambda v: None if v is None else torch.as_tensor(np.asarray(v, dtype=np.int32)).cuda()
    ixd, iyd = dev(ix), dev(iy)
    if out is None:                                              # garbage to start with, guard words behind both vectors
        out = (torch.full((n_pairs + 2,), -5.0, dtype=torch.float32, device="cuda"), torch.full((n_pairs + 2,), -6.0, dtype=torch.float32, device="cuda"))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda") if flag is None else flag
    guards = [o[-2:].clone() for o in out]
    rc = _lib.lib.dmvae_ssim_rows(stream(), Xd.data_ptr(), Xd.stride(0), Xd.shape[0], None if ixd is None else ixd.data_ptr(),
                                  Yd.data_ptr(), Yd.stride(0), Yd.shape[0], None if iyd is None else iyd.data_ptr(), n_pairs, H, W, planes,
                                  w.ctypes.data, len(w), C1, C2, out[0].data_ptr(), out[1].data_ptr() if want_sse else None, flag.data_ptr())
    assert rc == expect, (rc, _lib.lib.dmvae_last_error())
    torch.cuda.synchronize()
    for o, g in zip(out, guards):
        assert torch.equal(o[-2:], g)                            # nothing behind the vectors is written
    return out[0][:n_pairs].cpu().numpy(), out[1][:n_pairs].cpu().numpy() if want_sse else None, int(flag.item()), out


@functools.lru_cache(maxsize=None)
def case(pairs, planes, H, W, win):
    """the rows of a shape and the oracle's values, computed once: X and Y hold `pairs` + 3 rows each (the indexed runs reach all of them)"""
    n = pairs + 3
    X = SO.mnist_like(n, planes, H, W, seed=H * 100 + W)
    Y = SO.other_side(X, seed=win, start=3 if pairs == 1 else 0)
    w = SO.gaussian_window(win, 1.5)
    rng = np.random.RandomState(pairs)
    ix = rng.randint(0, n, pairs)                                # repeats
    iy = rng.permutation(n)[:pairs]                              # a permutation
    shape = (planes, H, W)
    direct = SO.ssim_rows(X, Y, shape, w, C1, C2, ix=np.arange(pairs), iy=np.arange(pairs))
    indexed = SO.ssim_rows(X, Y, shape, w, C1, C2, ix=ix, iy=iy)
    within = SO.ssim_rows(X, X, shape, w, C1, C2, ix=ix, iy=iy)
    for v in direct + indexed + within:
        v.setflags(write=False)
    return dict(X=X, Y=Y, w=w, ix=ix, iy=iy, shape=shape, direct=direct, indexed=indexed, within=within)


def check(got, want, win, pixels, what):
    s, e = got
    ws, we = want
    assert np.isfinite(s).all() and np.isfinite(e).all(), what
    err = float(np.abs(s.astype(np.float64) - ws).max())
    rel = float((np.abs(e.astype(np.float64) - we) / np.maximum(we, 1e-30)).max())
    print("%s: largest |ssim - oracle| %.3g (bound %.3g), largest relative sse error %.3g (bound %.3g)"
          % (what, err, SO.u_bound(win), rel, (pixels + 2) * 2.0 ** -24))
    assert err <= SO.u_bound(win), (what, err)
    assert rel <= (pixels + 2) * 2.0 ** -24, (what, rel)
    return err


@pytest.mark.parametrize("pairs,planes,H,W,win", SHAPES)
def test_entry_against_the_oracle(pairs, planes, H, W, win):
    c = case(pairs, planes, H, W, win)
    shape, w, pixels = c["shape"], c["w"], planes * H * W
    Xd, Yd = padded(c["X"], 5), padded(c["Y"], 2)
    s, e, flag, out = raw(Xd, Yd, shape, w, pairs)
    assert flag == 0
    check((s, e), c["direct"], win, pixels, "%r direct" % (SHAPES[SHAPES.index((pairs, planes, H, W, win))],))
    # a second call into the same buffers: the same bits
    s2, e2, _, _ = raw(Xd, Yd, shape, w, pairs, out=out)
    assert s2.tobytes() == s.tobytes() and e2.tobytes() == e.tobytes()
    # without sse: ssim's bits stay, the sse buffer is not written
    s3, _, _, out3 = raw(Xd, Yd, shape, w, pairs, want_sse=False)
    assert s3.tobytes() == s.tobytes() and bool((out3[1] == -6.0).all())
    # swapped sides: the same bits, of ssim and of sse
    s4, e4, _, _ = raw(Yd, Xd, shape, w, pairs)
    assert s4.tobytes() == s.tobytes() and e4.tobytes() == e.tobytes()
    # through ix (repeats) and iy (a permutation)
    si, ei, flag, _ = raw(Xd, Yd, shape, w, pairs, ix=c["ix"], iy=c["iy"])
    assert flag == 0
    check((si, ei), c["indexed"], win, pixels, "  indexed")
    sj, ej, _, _ = raw(Yd, Xd, shape, w, pairs, ix=c["iy"], iy=c["ix"])
    assert sj.tobytes() == si.tobytes() and ej.tobytes() == ei.tobytes()
    # X and Y the same buffer
    sw, ew, flag, _ = raw(Xd, Xd, shape, w, pairs, ix=c["ix"], iy=c["iy"])
    assert flag == 0
    check((sw, ew), c["within"], win, pixels, "  one buffer")
    # every row against itself: exactly 1 and exactly 0
    n = len(c["X"])
    s1, e1, _, _ = raw(Xd, Xd, shape, w, n)
    assert s1.tobytes() == np.ones(n, dtype=np.float32).tobytes() and not e1.any()
    s1, e1, _, _ = raw(Xd, padded(c["X"], 0), shape, w, n)       # another buffer with the same values
    assert s1.tobytes() == np.ones(n, dtype=np.float32).tobytes() and not e1.any()


def test_the_cases_spread_over_the_range_of_ssim():
    vals = np.concatenate([np.concatenate([case(*s)[k][0] for k in ("direct", "indexed", "within")]) for s in SHAPES])
    assert (vals < 0.0).any() and ((vals > 0.3) & (vals < 0.7)).any() and (vals > 0.9).any(), (vals.min(), vals.max())
    big = case(*SHAPES[4])["direct"][0]                          # and within the one shape with hundreds of comparisons
    assert (big < 0.0).any() and ((big > 0.3) & (big < 0.7)).any() and ((big > 0.9) & (big < 1.0)).any()


def test_an_index_out_of_range_gives_nan_and_bit_1_and_leaves_the_other_rows():
    pairs, planes, H, W, win = SHAPES[4]
    c = case(pairs, planes, H, W, win)
    Xd, Yd = padded(c["X"], 5), padded(c["Y"], 2)
    good_s, good_e, _, _ = raw(Xd, Yd, c["shape"], c["w"], pairs, ix=c["ix"], iy=c["iy"])
    for side, r, value in (("ix", 130, len(c["X"])), ("iy", 0, -1), ("ix", pairs - 1, 2 ** 31 - 1)):
        idx = dict(ix=c["ix"].copy(), iy=c["iy"].copy())
        idx[side][r] = value
        s, e, flag, _ = raw(Xd, Yd, c["shape"], c["w"], pairs, **idx)
        assert flag == 2                                         # bit 1
        assert np.isnan(s[r]) and np.isnan(e[r])
        keep = np.arange(pairs) != r
        assert s[keep].tobytes() == good_s[keep].tobytes() and e[keep].tobytes() == good_e[keep].tobytes()
    # the flag is OR-ed into: other bits stay
    flag = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    idx = dict(ix=c["ix"].copy(), iy=c["iy"])
    idx["ix"][7] = -2
    assert raw(Xd, Yd, c["shape"], c["w"], pairs, flag=flag, **idx)[2] == 7
    # without a flag the NaN alone reports it
    from dmvae_hip import _lib
    out = torch.zeros(pairs, dtype=torch.float32, device="cuda")
    w, ixd, iyd = c["w"], torch.as_tensor(idx["ix"].astype(np.int32)).cuda(), torch.as_tensor(idx["iy"].astype(np.int32)).cuda()
    rc = _lib.lib.dmvae_ssim_rows(stream(), Xd.data_ptr(), Xd.stride(0), Xd.shape[0], ixd.data_ptr(), Yd.data_ptr(), Yd.stride(0), Yd.shape[0],
                                  iyd.data_ptr(), pairs, H, W, planes, w.ctypes.data, len(w), C1, C2, out.data_ptr(), None, None)
    assert rc == 0
    assert np.isnan(out.cpu().numpy()).tolist() == (np.arange(pairs) == 7).tolist()


def test_sse_is_exact_on_multiples_of_a_sixteenth():
    for pairs, planes, H, W, win in (SHAPES[2], SHAPES[3], SHAPES[5]):
        c = case(pairs, planes, H, W, win)
        X16, Y16 = np.round(c["X"] * 16) / 16, np.round(c["Y"] * 16) / 16
        n = len(X16)
        _, e, _, _ = raw(padded(X16, 1), padded(Y16, 7), c["shape"], c["w"], n)
        want = ((X16.astype(np.float64) - Y16.astype(np.float64)) ** 2).sum(axis=1)
        assert want.max() > 1.0 and np.array_equal(e.astype(np.float64), want)


def test_images_of_65_by_64_are_unsupported():
    from dmvae_hip import _lib
    Xd = torch.zeros((2, 65 * 64), dtype=torch.float32, device="cuda")
    _, _, flag, out = raw(Xd, Xd, (1, 65, 64), SO.gaussian_window(3, 1.5), 2, expect=-2)
    assert b"dmvae_ssim_rows" in _lib.lib.dmvae_last_error() and flag == 0
    assert bool((out[0] == -5.0).all()) and bool((out[1] == -6.0).all())       # nothing was enqueued


def test_module_functions_against_the_oracle():
    from dmvae_hip import ssim as S
    pairs, planes, H, W, win = SHAPES[2]
    c = case(pairs, planes, H, W, win)
    Xd, Yd = padded(c["X"], 3)[:, :H * W], torch.as_tensor(c["Y"]).cuda()     # a row-strided view is used where it lies
    s, e = S.ssim_enqueue(Xd[:pairs], Yd[:pairs], (H, W))
    want_s, want_e = c["direct"]
    assert s.dtype == e.dtype == torch.float32 and s.shape == e.shape == (pairs,)
    assert np.abs(s.cpu().numpy() - want_s).max() <= SO.u_bound(win)
    got = S.ssim(c["X"][:pairs], c["Y"][:pairs], (1, H, W), window=S.gaussian_window(11, 1.5))      # arrays are uploaded
    assert all(g.dtype == np.float64 and g.shape == (pairs,) for g in got)
    assert got[0].astype(np.float32).tobytes() == s.cpu().numpy().tobytes()
    assert np.allclose(got[1], want_e / (H * W), rtol=(H * W + 2) * 2.0 ** -24, atol=0.0)
    assert got[2][0] == np.inf and got[1][0] == 0.0              # the first comparison is a row against itself
    assert np.allclose(got[2][1:], 10.0 * np.log10(1.0 / (want_e[1:] / (H * W))), rtol=1e-6)
    gi = S.ssim(Xd, Yd, (H, W), ix=c["ix"], iy=c["iy"])
    assert np.abs(gi[0] - c["indexed"][0]).max() <= SO.u_bound(win)
    with pytest.raises(IndexError):
        S.ssim(Xd, Yd, (H, W), ix=[0, len(c["X"])], iy=[0, 1])
    # a uniform 7-tap window and another data range run through the same entry
    uni = np.full(7, 1.0 / 7, dtype=np.float32)
    c1, c2 = SO.constants(2.0)
    gu = S.ssim(Xd, Yd, (H, W), window=uni, data_range=2.0)
    wu, eu = SO.ssim_rows(c["X"], c["Y"], (1, H, W), uni, c1, c2)
    assert np.abs(gu[0] - wu).max() <= SO.u_bound(7)
    assert np.allclose(gu[2][1:], 10.0 * np.log10(4.0 / (eu[1:] / (H * W))), rtol=1e-5)


def test_pairwise_equals_the_oracles_loop_over_pairs():
    from dmvae_hip import ssim as S
    pairs, planes, H, W, win = SHAPES[1]
    X = SO.mnist_like(11, planes, H, W, seed=9)
    X[6] = X[2]                                                  # one pair of identical draws
    groups = np.array([1, 0, 1, 1, 0, 3, 1, 0, 3, 3, 4])         # sizes 3, 4, 0, 3, 1: an empty group and one without a pair
    ix, iy, pg = SO.group_pairs(groups, 5)
    want, _ = SO.ssim_rows(X, X, (planes, H, W), SO.gaussian_window(win, 1.5), C1, C2, ix=ix, iy=iy)
    Xd = torch.as_tensor(X).cuda()
    for g in (groups, torch.as_tensor(groups).cuda()):           # groups from the host, or a device vector
        s, e, gx, gy, gp = S.pairwise_enqueue(Xd, g, 5, (H, W))
        assert gx.cpu().tolist() == ix.tolist() and gy.cpu().tolist() == iy.tolist() and gp.cpu().tolist() == pg.tolist()
        s = s.cpu().numpy()
        assert np.abs(s - want).max() <= SO.u_bound(win)
        assert s[(ix == 2) & (iy == 6)].tolist() == [1.0] and (s < 1.0).sum() == len(s) - 1
    with pytest.raises(ValueError):
        S.pairwise_enqueue(Xd, np.arange(11), 11, (H, W))        # no group holds a pair
