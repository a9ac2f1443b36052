"""float64 oracle of the structural similarity (csrc/ssim.hip, dmvae_hip/ssim.py), three ways:
  ssim_map / ssim_image / ssim_rows   the definition restated in float64: direct VALID windows, the 2-D weight g[a][b] = fl32(w1[a] w1[b]),
                                      means mx = sum g x, second moments CENTRED on them, S = (2 mx my + c1)(2 sxy + c2) /
                                      ((mx^2 + my^2 + c1)(sxx + syy + c2)), the mean of S over all windows of all planes;
  ssim_scipy                          skimage's structural_similarity(gaussian_weights=True, use_sample_covariance=False) restated with
                                      scipy.ndimage.gaussian_filter(truncate=3.5): filtered maps of x, y, xx, yy, xy on the reflect-padded
                                      image, E[x^2] - mu^2 moments, the crop of (win - 1) / 2 pixels, the mean (float64 throughout);
  ssim_f32_pinned                     an f32 emulation of the kernel's pinned operation sequence, for the two properties that hold in bits.
No skimage, no sklearn."""
import numpy as np


def gaussian_window(win=11, sigma=1.5):
    t = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    w = np.exp(-(t * t) / (2.0 * sigma ** 2))
    return (w / w.sum()).astype(np.float32)


def constants(data_range=1.0, k1=0.01, k2=0.03):
    """(c1, c2) rounded to f32, as the entry receives them"""
    return float(np.float32((k1 * data_range) ** 2)), float(np.float32((k2 * data_range) ** 2))


def weights2d(w1):
    """g[a][b] = fl32(w1[a] w1[b]) as float64"""
    w = np.asarray(w1, dtype=np.float32)
    return (w[:, None] * w[None, :]).astype(np.float32).astype(np.float64)


def u_bound(win):
    """the worst-case rounding bound of the centred direct form in f32: 8 (win^2 + 3) 2^-24"""
    return 8.0 * (win * win + 3) * 2.0 ** -24


def ssim_map(x, y, w1, c1, c2):
    """S of every valid window of one plane: float64 [H - win + 1][W - win + 1]"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    g = weights2d(w1)
    win = g.shape[0]
    wx = np.lib.stride_tricks.sliding_window_view(x, (win, win))
    wy = np.lib.stride_tricks.sliding_window_view(y, (win, win))
    mx, my = (wx * g).sum(axis=(2, 3)), (wy * g).sum(axis=(2, 3))
    dx, dy = wx - mx[:, :, None, None], wy - my[:, :, None, None]
    sxx, syy, sxy = (g * dx * dx).sum(axis=(2, 3)), (g * dy * dy).sum(axis=(2, 3)), (g * dx * dy).sum(axis=(2, 3))
    return (2.0 * mx * my + c1) * (2.0 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))


def ssim_image(x, y, w1, c1, c2):
    """the mean of S over all windows of all planes of x, y [planes][H][W]"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.mean([ssim_map(xp, yp, w1, c1, c2) for xp, yp in zip(x, y)]))


def ssim_rows(X, Y, shape, w1, c1, c2, ix=None, iy=None):
    """(ssim float64 [n], sse float64 [n]) of the comparisons X[ix[r]] against Y[iy[r]]; shape = (planes, H, W); only the first planes H W
    values of a row are read"""
    planes, H, W = shape
    n = len(ix) if ix is not None else (len(iy) if iy is not None else len(X))
    ix = np.arange(n) if ix is None else np.asarray(ix)
    iy = np.arange(n) if iy is None else np.asarray(iy)
    s, e = np.empty(n), np.empty(n)
    for r in range(n):
        x = np.asarray(X[ix[r]], dtype=np.float64)[:planes * H * W].reshape(planes, H, W)
        y = np.asarray(Y[iy[r]], dtype=np.float64)[:planes * H * W].reshape(planes, H, W)
        s[r] = ssim_image(x, y, w1, c1, c2)
        e[r] = ((x - y) ** 2).sum()
    return s, e


def group_pairs(groups, n_groups):
    """(ix, iy, pair_group): all pairs i < j of rows of one group, groups ascending, i ascending, j ascending inside it -- a plain loop"""
    groups = np.asarray(groups)
    ix, iy, pg = [], [], []
    for c in range(n_groups):
        rows = [i for i in range(len(groups)) if groups[i] == c]
        for a in range(len(rows)):
            for b in range(a + 1, len(rows)):
                ix.append(rows[a])
                iy.append(rows[b])
                pg.append(c)
    return np.array(ix, dtype=np.int64), np.array(iy, dtype=np.int64), np.array(pg, dtype=np.int64)


def ssim_scipy(x, y, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03):
    """skimage's definition on one plane, by scipy.ndimage (win = 2 int(3.5 sigma + 0.5) + 1 = 11 at sigma 1.5)"""
    from scipy.ndimage import gaussian_filter
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    f = lambda v: gaussian_filter(v, sigma, truncate=3.5, mode="reflect")
    ux, uy = f(x), f(y)
    vx, vy, vxy = f(x * x) - ux * ux, f(y * y) - uy * uy, f(x * y) - ux * uy
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    S = (2.0 * ux * uy + c1) * (2.0 * vxy + c2) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    pad = int(3.5 * sigma + 0.5)
    return float(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean())


def _fma32(g, p, acc):
    """fmaf on f32 arrays: the product of two f32 is exact in float64; the sum is rounded to float64, then to f32 (a double rounding
    that can differ from fmaf's in the last bit on rare inputs, and is applied alike to every accumulator: the bit properties stand)"""
    return (g.astype(np.float64) * p.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def ssim_f32_pinned(x, y, w1, c1, c2):
    """the kernel's sequence on x, y [planes][H][W] in f32: mx = fmaf(g, x, mx) over a, then b ascending; dx = fl(x - mx);
    sxx = fmaf(g, fl(dx dx), sxx), syy, sxy alike; S = fl(fl(2 fl(mx my) + c1) fl(2 sxy + c2)) / fl(fl(fl(mx mx) + fl(my my) + c1) fl(fl(sxx
    + syy) + c2)); the mean in float64, rounded to f32"""
    f32 = np.float32
    x, y, w = np.asarray(x, dtype=f32), np.asarray(y, dtype=f32), np.asarray(w1, dtype=f32)
    c1, c2, two, win = f32(c1), f32(c2), f32(2.0), len(w)
    total, count = 0.0, 0
    for xp, yp in zip(x, y):
        wx = np.lib.stride_tricks.sliding_window_view(xp, (win, win))
        wy = np.lib.stride_tricks.sliding_window_view(yp, (win, win))
        g = (w[:, None] * w[None, :]).astype(f32)
        mx, my = np.zeros(wx.shape[:2], dtype=f32), np.zeros(wx.shape[:2], dtype=f32)
        for a in range(win):
            for b in range(win):
                mx, my = _fma32(g[a, b], wx[:, :, a, b], mx), _fma32(g[a, b], wy[:, :, a, b], my)
        sxx, syy, sxy = np.zeros_like(mx), np.zeros_like(mx), np.zeros_like(mx)
        for a in range(win):
            for b in range(win):
                dx, dy = wx[:, :, a, b] - mx, wy[:, :, a, b] - my                 # (f32 - f32: rounded once)
                sxx, syy, sxy = _fma32(g[a, b], dx * dx, sxx), _fma32(g[a, b], dy * dy, syy), _fma32(g[a, b], dx * dy, sxy)
        a1, a2 = two * (mx * my) + c1, two * sxy + c2
        b1, b2 = (mx * mx + my * my) + c1, (sxx + syy) + c2
        S = (a1 * a2) / (b1 * b2)
        assert S.dtype == f32
        total += float(S.astype(np.float64).sum())
        count += S.size
    return f32(total / count)


# ---------------------------------------------------------------------------------------------------------------- test images
NOISE_STRENGTHS = (0.02, 0.05, 0.1, 0.2, 0.4)


def mnist_like(n, planes, H, W, seed):
    """n rows of `planes` H x W images in [0, 1], float32 [n][planes H W]: 19 % of the pixels set, blurred by the separable (1 2 1) / 4
    kernel (edge-padded), every image scaled to a maximum of 1 -- flat black regions, soft strokes, as MNIST has them"""
    rng = np.random.RandomState(seed)
    img = (rng.rand(n, planes, H, W) < 0.19).astype(np.float64)
    p = np.pad(img, ((0, 0), (0, 0), (1, 1), (0, 0)), mode="edge")
    img = 0.25 * p[:, :, :-2] + 0.5 * p[:, :, 1:-1] + 0.25 * p[:, :, 2:]
    p = np.pad(img, ((0, 0), (0, 0), (0, 0), (1, 1)), mode="edge")
    img = 0.25 * p[..., :-2] + 0.5 * p[..., 1:-1] + 0.25 * p[..., 2:]
    top = img.max(axis=(2, 3), keepdims=True)
    img = img / np.where(top > 0, top, 1.0)
    return img.reshape(n, planes * H * W).astype(np.float32)


def other_side(X, seed, start=0):
    """a partner for every row of X, the kinds in turn from kind `start` on: the same row, the row plus clipped Gaussian noise at the five
    NOISE_STRENGTHS, an unrelated row (the next one), 1 - X.  float32, in [0, 1]"""
    rng = np.random.RandomState(seed)
    Y = np.empty_like(X)
    for r in range(len(X)):
        kind = (r + start) % 8
        if kind == 0:
            Y[r] = X[r]
        elif kind <= 5:
            Y[r] = np.clip(X[r] + NOISE_STRENGTHS[kind - 1] * rng.randn(X.shape[1]), 0.0, 1.0)
        elif kind == 6:
            Y[r] = X[(r + 1) % len(X)]
        else:
            Y[r] = 1.0 - X[r]
    return Y.astype(np.float32)
