"""NumPy restatement of the random affine warp of csrc/augment.hip (the stream-9 row of the noise table of section 4), on
top of philox_oracle.py: exact integer words and uniforms, then float64.  Imports nothing of the package.

    draw of data-set row g = row_base + r at (seed, step = counter): blocks 2 g and 2 g + 1 of stream 9; u = (w >> 8) 2^-24, s = 2 u - 1;
      block 2 g:     angle = rotate s0 [deg], tx = translate s1, ty = translate s2, scale = exp(log lo + u3 (log hi - log lo))
      block 2 g + 1: shear = shear s0 [deg]                       (words 1 .. 3 reserved)
    forward, about c = ((W - 1) / 2, (H - 1) / 2):   p_out = c + t + F (p_in - c),   F = scale R(angle) Shear_x(tan shear)
    theta = the inverse, the SAMPLING map in pixel-index units:  (sx, sy) = M (j, i) + (m02, m12),  M = F^-1,  offset = c - M (c + t)
    warp: bilinear interpolation of the image extended by zeros at (sx, sy); a non-finite coordinate gives 0.

A spec is (rotate, translate, (lo, hi), shear); its numbers are rounded to float32 first, as the C struct holds them."""
import numpy as np

import philox_oracle as P

STREAM = 9
BLOCK_LIMIT = P.BLK_LIMIT                # 2 (row_base + n_rows) stays below it


def _spec32(spec):
    rotate, translate, (lo, hi), shear = spec
    return tuple(float(np.float32(v)) for v in (rotate, translate, lo, hi, shear))


def words(seed, counter, row_base, n_rows):
    """[n_rows][2][4]: the two blocks of every row, exact 32-bit words in uint64"""
    assert row_base >= 0 and 2 * (int(row_base) + int(n_rows)) < BLOCK_LIMIT
    blk = 2 * np.arange(int(row_base), int(row_base) + int(n_rows), dtype=np.uint64)[:, None] + np.arange(2, dtype=np.uint64)[None, :]
    return P.block(seed, counter, STREAM, blk)


def params(seed, counter, row_base, n_rows, spec):
    """dict of float64 [n_rows]: angle and shear in degrees, tx, ty in pixels, scale; uniforms exact on the 2^-24 grid"""
    rotate, translate, lo, hi, shear = _spec32(spec)
    w = words(seed, counter, row_base, n_rows)
    u = (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    s = 2.0 * u - 1.0
    # log lo and log hi - log lo as the launcher rounds them to float32
    llo = np.float64(np.float32(np.log(lo)))
    span = np.float64(np.float32(np.float32(np.log(hi)) - np.float32(np.log(lo))))
    return dict(angle=rotate * s[:, 0, 0], tx=translate * s[:, 0, 1], ty=translate * s[:, 0, 2], scale=np.exp(llo + u[:, 0, 3] * span),
                shear=shear * s[:, 1, 0])


def forward64(p, H, W):
    """the forward transform of every row as (F [n][2][2], centre c [2], t [n][2]) in (x, y) coordinates"""
    a, k = np.deg2rad(p["angle"]), np.tan(np.deg2rad(p["shear"]))
    cs, sn = np.cos(a), np.sin(a)
    R = np.stack([np.stack([cs, -sn], -1), np.stack([sn, cs], -1)], -2)
    S = np.stack([np.stack([np.ones_like(k), k], -1), np.stack([np.zeros_like(k), np.ones_like(k)], -1)], -2)
    F = p["scale"][:, None, None] * (R @ S)
    return F, np.array([(W - 1) / 2.0, (H - 1) / 2.0]), np.stack([p["tx"], p["ty"]], -1)


def theta64(p, H, W):
    """[n][6] float64 (m00 m01 m02 m10 m11 m12): the closed-form inverse of forward64"""
    a, k = np.deg2rad(p["angle"]), np.tan(np.deg2rad(p["shear"]))
    cs, sn, inv = np.cos(a), np.sin(a), 1.0 / p["scale"]
    m00, m01, m10, m11 = (cs + k * sn) * inv, (sn - k * cs) * inv, -sn * inv, cs * inv
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    qx, qy = cx + p["tx"], cy + p["ty"]
    return np.stack([m00, m01, cx - m00 * qx - m01 * qy, m10, m11, cy - m10 * qx - m11 * qy], -1)


def warp64(X, theta, H, W):
    """X [n][H W], theta [n][6] -> float64 [n][H W]: the zero-extended bilinear warp, every product and sum in float64"""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), H, W)
    th = np.asarray(theta, dtype=np.float64).reshape(len(X), 6)
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((len(X), H, W))
    for n in range(len(X)):
        m = th[n]
        with np.errstate(invalid="ignore", over="ignore"):
            sx = m[0] * j + m[1] * i + m[2]
            sy = m[3] * j + m[4] * i + m[5]
        ok = np.isfinite(sx) & np.isfinite(sy) & (sx > -1) & (sx < W) & (sy > -1) & (sy < H)
        sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0, sy - y0
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        pad = np.zeros((H + 2, W + 2))
        pad[1:-1, 1:-1] = X[n]                                   # index (y + 1, x + 1): taps at -1 and at H / W read the zero border
        v00, v01 = pad[y0 + 1, x0 + 1], pad[y0 + 1, x0 + 2]
        v10, v11 = pad[y0 + 2, x0 + 1], pad[y0 + 2, x0 + 2]
        val = (1 - fy) * ((1 - fx) * v00 + fx * v01) + fy * ((1 - fx) * v10 + fx * v11)
        out[n] = np.where(ok, val, 0.0)
    return out.reshape(len(X), H * W)
