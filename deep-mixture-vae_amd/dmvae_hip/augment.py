"""Random affine augmentation of rows on the device (dmvae_augment_rows of include/dmvae_hip.h, csrc/augment.hip): every row is a single-plane
H x W image and is warped by its own affine map -- zero-extended bilinear sampling, torch's grid_sample(bilinear, zeros, align_corners=True) in
pixel units.  The maps are given (theta [n][6], the sampling map from output pixel to source coordinate) or drawn from Philox stream 9 keyed by
(seed, counter, data-set row): batch size, row order, rank count and chunked calls do not enter.  DESIGN.md section 30."""
import ctypes as C
import math
from collections import namedtuple

import torch

from ._lib import lib, check, AugmentParams
from .binarize import _rows
from .knn import _ld, _stream

PHILOX_STREAM = 9
MAX_SIDE = 64
_U64 = (1 << 64) - 1
_KEYS = ("rotate", "translate", "scale", "shear")


class AugmentSpec(namedtuple("AugmentSpec", "rotate translate scale shear image_shape")):
    """rotate: the angle is uniform in +-rotate degrees; translate: tx and ty uniform in +-translate pixels; scale = (lo, hi): log-uniform;
    shear: the x-shear angle uniform in +-shear degrees; image_shape = (H, W), None: the square whose area is the column count."""
    __slots__ = ()

    def __new__(cls, rotate=0.0, translate=0.0, scale=(1.0, 1.0), shear=0.0, image_shape=None):
        try:
            lo, hi = scale
        except TypeError:
            raise ValueError("scale = %r: a pair (lo, hi)" % (scale,))
        vals = dict(rotate=float(rotate), translate=float(translate), shear=float(shear))
        for k, v in vals.items():
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError("%s = %r: a finite range >= 0" % (k, v))
        lo, hi = float(lo), float(hi)
        if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
            raise ValueError("scale = %r:%r: finite, 0 < lo <= hi" % (lo, hi))
        if image_shape is not None:
            image_shape = (int(image_shape[0]), int(image_shape[1]))
        return super().__new__(cls, vals["rotate"], vals["translate"], (lo, hi), vals["shear"], image_shape)

    def shape_for(self, n_cols):
        """(H, W) of rows of n_cols columns"""
        if self.image_shape is not None:
            H, W = self.image_shape
            if H < 1 or W < 1 or H * W != n_cols:
                raise ValueError("image_shape = %r does not make rows of %d columns" % (self.image_shape, n_cols))
            return H, W
        side = math.isqrt(int(n_cols))
        if side * side != n_cols:
            raise ValueError("rows of %d columns are no square image: give image_shape = (H, W)" % n_cols)
        return side, side

    def is_identity(self):
        return self.rotate == 0.0 and self.translate == 0.0 and self.shear == 0.0 and self.scale == (1.0, 1.0)

    def params(self):
        return AugmentParams(self.rotate, self.translate, self.scale[0], self.scale[1], self.shear)

    def __str__(self):
        """the string parse_augment reads back (image_shape is not part of it)"""
        return "rotate=%r,translate=%r,scale=%r:%r,shear=%r" % (self.rotate, self.translate, self.scale[0], self.scale[1], self.shear)


def parse_augment(text, image_shape=None):
    """ "rotate=10,translate=2,scale=0.9:1.1,shear=5" -> AugmentSpec; keys may be left out (their range is then zero, scale 1:1)"""
    if isinstance(text, AugmentSpec):
        return text
    kw = {}
    for item in str(text).split(","):
        item = item.strip()
        if not item:
            continue
        key, sep, val = item.partition("=")
        key = key.strip()
        if key not in _KEYS:
            raise ValueError("augment spec: unknown key %r in %r (one of %s)" % (key, item, ", ".join(_KEYS)))
        if key in kw:
            raise ValueError("augment spec: key %r given twice" % key)
        try:
            if not sep:
                raise ValueError
            if key == "scale":
                lo, colon, hi = val.partition(":")
                if not colon:
                    raise ValueError
                kw[key] = (float(lo), float(hi))
            else:
                kw[key] = float(val)
        except ValueError:
            raise ValueError("augment spec: malformed value for %r: %r (%s)" % (key, item, "scale=LO:HI" if key == "scale" else "%s=NUMBER" % key))
        try:
            AugmentSpec(**{key: kw[key]})
        except ValueError as e:
            raise ValueError("augment spec: %s" % e)
    return AugmentSpec(image_shape=image_shape, **kw)


def augment(X, spec=None, seed=0, counter=0, row_base=0, theta=None, out=None, return_theta=False):
    """The warped rows of the device tensor X [n][H W] as a device f32 tensor (allocated when `out` is None; otherwise written into `out`, which
    must not overlap X; its pad columns are left alone).  theta: device f32 [n][6] sampling maps to use in place of the draw (spec then only
    gives the image shape; None: the square).  row_base: the index of X[0] in the unpermuted data set, so that calls on chunks of a data set
    equal one call on all of it.  return_theta: (out, the [n][6] maps used).  Enqueues on the current stream and does not synchronise."""
    X = _rows(X, "X")
    n, d = X.shape
    if spec is None:
        if theta is None:
            raise ValueError("augment: neither a spec nor theta")
        spec = AugmentSpec()
    spec = parse_augment(spec)
    H, W = spec.shape_for(d)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=X.device)
    out = _rows(out, "out")
    if tuple(out.shape) != (n, d) or out.device != X.device:
        raise ValueError("out is %s on %s, X is %s on %s" % (tuple(out.shape), out.device, (n, d), X.device))
    if theta is not None:
        if not (isinstance(theta, torch.Tensor) and theta.device == X.device and theta.dtype == torch.float32 and tuple(theta.shape) == (n, 6)
                and theta.is_contiguous()):
            raise ValueError("theta must be a contiguous device f32 [%d][6] tensor beside X" % n)
    used = torch.empty((n, 6), dtype=torch.float32, device=X.device) if return_theta else None
    p = spec.params()
    with torch.cuda.device(X.device):
        check(lib.dmvae_augment_rows(_stream(X.device), X.data_ptr(), _ld(X), n, H, W, int(row_base), int(seed) & _U64, int(counter) & _U64, C.byref(p),
                                     None if theta is None else theta.data_ptr(), None if used is None else used.data_ptr(), out.data_ptr(), _ld(out)),
              "dmvae_augment_rows")
    return (out, used) if return_theta else out
