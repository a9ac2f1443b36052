"""Binarised rows on the device (dmvae_binarize_rows of include/dmvae_hip.h, csrc/binarize.hip): the binarised-MNIST protocol on the resident
rows.  mode "bernoulli" is the stochastic binarisation out = (u < x) with u from Philox stream 8 keyed by (seed, counter, data-set row, column)
-- batch size, row order, rank count and chunked calls do not enter; mode "threshold" is the fixed out = (x > 0.5).  DESIGN.md section 26."""
import torch

from ._lib import lib, check
from .knn import _ld, _stream

MODES = {"bernoulli": 0, "threshold": 1}
PHILOX_STREAM = 8
_U64 = (1 << 64) - 1


def _rows(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] >= 1 and t.shape[1] >= 1
            and (t.shape[1] == 1 or t.stride(1) == 1) and (t.shape[0] == 1 or t.stride(0) >= t.shape[1])):
        raise ValueError("%s must be a device f32 [rows][columns] tensor with unit column stride (a row-strided view is taken where it lies)" % what)
    return t


def binarize(X, seed=0, counter=0, row_base=0, mode="bernoulli", out=None):
    """The binarised rows of the device tensor X [n][d] as a device f32 tensor of 0 / 1 (allocated when `out` is None; otherwise written into
    `out`, which must not overlap X; its pad columns are left alone).  row_base: the index of X[0] in the unpermuted data set, so that calls
    on chunks of a data set equal one call on all of it.  Enqueues on the current stream and does not synchronise."""
    if mode not in MODES:
        raise ValueError("mode = %r: one of %s" % (mode, ", ".join(sorted(MODES))))
    X = _rows(X, "X")
    n, d = X.shape
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=X.device)
    out = _rows(out, "out")
    if tuple(out.shape) != (n, d) or out.device != X.device:
        raise ValueError("out is %s on %s, X is %s on %s" % (tuple(out.shape), out.device, (n, d), X.device))
    with torch.cuda.device(X.device):
        check(lib.dmvae_binarize_rows(_stream(X.device), X.data_ptr(), _ld(X), n, d, int(row_base), int(seed) & _U64, int(counter) & _U64, MODES[mode],
                                      out.data_ptr(), _ld(out)), "dmvae_binarize_rows")
    return out
