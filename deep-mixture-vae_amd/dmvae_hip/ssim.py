"""Structural similarity on the device (dmvae_ssim_rows of include/dmvae_hip.h, csrc/ssim.hip): the SSIM of Wang et al. 2004 between
rows of images, valid windows only, a separable window, the second moments CENTRED on each window's own means (no E[x^2] - mu^2, which in
f32 cancels against c2 in flat regions).  With gaussian_window(11, 1.5) it is skimage's structural_similarity(gaussian_weights=True,
use_sample_covariance=False).  ssim(X, X) is 1.0 in bits, ssim(X, Y) and ssim(Y, X) are the same bits, and two calls agree bit for bit.
Nothing here imports skimage or sklearn."""
import ctypes as C
import math

import numpy as np
import torch

from ._lib import lib, check
from .gmm import _device_of, _rows_f32
from .knn import _int32_vector, _ld, _stream

MAX_WIN = 11
MAX_PIXELS = 4096            # H * W of one plane: the two planes of a pair are held in 32 KiB of LDS
ERR_INDEX = 2                # bit 1 of the error flag: an ix / iy entry out of range


def gaussian_window(win=11, sigma=1.5):
    """the win weights exp(-(t - (win - 1) / 2)^2 / (2 sigma^2)), computed in float64, normalised to sum 1, rounded to f32"""
    win = int(win)
    t = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    w = np.exp(-(t * t) / (2.0 * float(sigma) ** 2))
    return (w / w.sum()).astype(np.float32)


def constants(data_range=1.0, k1=0.01, k2=0.03):
    """(c1, c2) = ((k1 L)^2, (k2 L)^2) as the f32 values the kernel receives"""
    L = float(data_range)
    return float(np.float32((k1 * L) ** 2)), float(np.float32((k2 * L) ** 2))


def _plane_shape(shape, width):
    """(planes, H, W) of shape = (H, W) or (planes, H, W); ValueError unless it matches the rows' width"""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("shape = %r: (H, W) or (planes, H, W), all >= 1" % (shape,))
    if shape[0] * shape[1] * shape[2] != int(width):
        raise ValueError("shape = %r holds %d values, the rows hold %d" % (shape, shape[0] * shape[1] * shape[2], width))
    return shape


def _window(window, H, W):
    w = gaussian_window() if window is None else np.ascontiguousarray(np.asarray(window, dtype=np.float32).reshape(-1))
    win = len(w)
    if win % 2 == 0 or not 3 <= win <= MAX_WIN:
        raise ValueError("the window holds %d weights: odd, 3 .. %d" % (win, MAX_WIN))
    if win > min(H, W):
        raise ValueError("a window of %d does not fit into images of %d x %d" % (win, H, W))
    return w


def ssim_enqueue(X, Y, shape, ix=None, iy=None, window=None, data_range=1.0, k1=0.01, k2=0.03, flag=None):
    """dmvae_ssim_rows on the current stream: (ssim f32 [n_pairs], sse f32 [n_pairs]) device tensors without a synchronisation.  X, Y:
    device f32 [rows][planes H W] with unit column stride (row-strided views are used where they lie; X and Y may be the same tensor).
    Comparison r reads X[ix[r]] (X[r] without ix) and Y[iy[r]] (Y[r] without iy); ix, iy: int vectors, device or host.  shape: (H, W) or
    (planes, H, W); window: the 1-D weights of the separable window (default gaussian_window(11, 1.5)); c1 = (k1 data_range)^2,
    c2 = (k2 data_range)^2.  sse is the SUM of squared differences of the row.  flag: a device int32 [1] that gains bit 1 when an index is
    out of range (that comparison's outputs are NaN); None: no flag is kept.  ValueError, before the device is touched, when shape does not
    match the rows' width, the window does not fit, or the sides' comparison counts differ."""
    planes, H, W = _plane_shape(shape, X.shape[1])
    if Y.shape[1] != X.shape[1]:
        raise ValueError("the two sides' rows differ in width: %d != %d" % (X.shape[1], Y.shape[1]))
    w = _window(window, H, W)
    if H * W > MAX_PIXELS:
        raise ValueError("images of %d x %d: at most %d pixels per plane" % (H, W, MAX_PIXELS))
    n_x = len(ix) if ix is not None else X.shape[0]
    n_y = len(iy) if iy is not None else Y.shape[0]
    if n_x != n_y or n_x < 1:
        raise ValueError("the two sides hold %d and %d comparisons" % (n_x, n_y))
    dev = _device_of(X if isinstance(X, torch.Tensor) and X.is_cuda else Y)
    Xd = _rows_f32(X, dev)
    Yd = Xd if Y is X else _rows_f32(Y, dev)
    ixd = None if ix is None else _int32_vector(ix, dev)
    iyd = None if iy is None else _int32_vector(iy, dev)
    c1, c2 = constants(data_range, k1, k2)
    out = torch.empty((2, n_x), dtype=torch.float32, device=dev)
    assert flag is None or (flag.is_cuda and flag.dtype == torch.int32 and flag.numel() == 1)
    with torch.cuda.device(dev):
        check(lib.dmvae_ssim_rows(_stream(dev), Xd.data_ptr(), _ld(Xd), Xd.shape[0], None if ixd is None else ixd.data_ptr(),
                                  Yd.data_ptr(), _ld(Yd), Yd.shape[0], None if iyd is None else iyd.data_ptr(), n_x, H, W, planes,
                                  w.ctypes.data_as(C.c_void_p), len(w), c1, c2, out[0].data_ptr(), out[1].data_ptr(),
                                  None if flag is None else flag.data_ptr()), "dmvae_ssim_rows")
    return out[0], out[1]


def quality_from(ssim_vals, sse, pixels, data_range=1.0):
    """(ssim, mse, psnr) as float64 NumPy arrays from the kernel's two vectors: mse = sse / pixels, psnr = 10 log10(L^2 / mse), inf at mse 0"""
    s = np.asarray(ssim_vals, dtype=np.float64)
    mse = np.asarray(sse, dtype=np.float64) / float(pixels)
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(float(data_range) ** 2 / mse)
    return s, mse, psnr


def ssim(X, Y, shape, ix=None, iy=None, window=None, data_range=1.0, k1=0.01, k2=0.03):
    """(ssim, mse, psnr): float64 NumPy arrays, one entry per comparison (ssim_enqueue's arguments; arrays are uploaded).  mse is the mean
    squared difference over the row's planes H W values, psnr = 10 log10(data_range^2 / mse), inf where mse is 0.  IndexError when an ix /
    iy entry is out of range.  One synchronising copy."""
    dev = _device_of(X if isinstance(X, torch.Tensor) and X.is_cuda else Y)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    s, e = ssim_enqueue(X, Y, shape, ix, iy, window, data_range, k1, k2, flag=flag)
    host = torch.cat([s, e, flag.view(torch.float32)]).cpu().numpy()
    n = s.numel()
    if int(host[2 * n:].view(np.int32)[0]):
        raise IndexError("ssim: an ix / iy entry out of range")
    return quality_from(host[:n], host[n:2 * n], X.shape[1], data_range)


def group_pairs(groups, n_groups, n, dev):
    """(ix, iy, pair_group, counts): device int32 vectors of all pairs i < j of rows of one group -- groups ascending, inside a group i
    ascending and j ascending inside it -- the group of every pair, and the host list of the groups' row counts.  Built on the device: a
    stable sort of the groups and one triangle of indices per distinct group size.  Groups given on the host cost no read; a device
    vector costs one small read of the counts."""
    G = int(n_groups)
    if isinstance(groups, torch.Tensor):
        g = _int32_vector(groups, dev).long()
        counts = torch.bincount(g, minlength=G).cpu().tolist()
    else:
        gh = np.asarray(groups).reshape(-1).astype(np.int64)
        counts = np.bincount(gh, minlength=G).tolist()
        g = torch.as_tensor(gh).to(dev)
    if g.numel() != n or len(counts) != G:
        raise ValueError("groups must hold one entry in [0, %d) per row: %d entries for %d rows" % (G, g.numel(), n))
    order = torch.sort(g, stable=True).indices
    tri, ix, iy, pg, start = {}, [], [], [], 0
    for c, m in enumerate(counts):
        if m >= 2:
            if m not in tri:
                tri[m] = torch.triu_indices(m, m, 1, device=dev)
            ix.append(order[start + tri[m][0]])
            iy.append(order[start + tri[m][1]])
            pg.append(torch.full((tri[m].shape[1],), c, dtype=torch.int32, device=dev))
        start += m
    if not ix:
        raise ValueError("no group holds two rows: there is no pair")
    return torch.cat(ix).to(torch.int32), torch.cat(iy).to(torch.int32), torch.cat(pg), counts


def pairwise_enqueue(X, groups, n_groups, shape, window=None, data_range=1.0, k1=0.01, k2=0.03, flag=None):
    """the SSIM of all pairs i < j of rows of X inside each group: (ssim f32 [P], sse f32 [P], ix int32 [P], iy int32 [P], pair_group int32
    [P]) on the device, pairs in group_pairs' order.  The index vectors go to dmvae_ssim_rows as ix / iy with X on both sides: no row is
    gathered or copied.  The mean over a component's pairs is the mode-collapse measure of Odena et al. 2017."""
    planes, H, W = _plane_shape(shape, X.shape[1])
    _window(window, H, W)
    dev = _device_of(X)
    Xd = _rows_f32(X, dev)
    ix, iy, pg, _ = group_pairs(groups, n_groups, Xd.shape[0], dev)
    s, e = ssim_enqueue(Xd, Xd, (planes, H, W), ix, iy, window, data_range, k1, k2, flag=flag)
    return s, e, ix, iy, pg


def default_image_shape(input_dim):
    """(sqrt(input_dim), sqrt(input_dim)) when input_dim is a perfect square; ValueError asking for the shape otherwise"""
    side = math.isqrt(int(input_dim))
    if side * side != int(input_dim):
        raise ValueError("input_dim = %d is no perfect square: pass image_shape=(H, W) or (planes, H, W)" % input_dim)
    return (side, side)
