"""Linear probe on the device (dmvae_softmax_xent / dmvae_linear_scores of include/dmvae_hip.h, csrc/probe.hip): are the classes linearly
separable in the rows of Z?  One kernel pass over all rows gives the mean multinomial cross-entropy of a softmax regression and its
gradient; scipy's L-BFGS-B drives it from the host, two small copies per evaluation.  On top of it sklearn's
LogisticRegression(solver="lbfgs") objective for the multinomial case.  Nothing here imports sklearn."""
import ctypes as C

import numpy as np
import torch

from ._lib import lib, check
from .gmm import _device_of, _rows_f32
from .knn import _int32_vector, _ld, _stream
from .metrics import argmax_labels

MAX_N, MAX_D, MAX_C, MAX_DC = 1 << 22, 512, 256, 16384


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _vec_f32(v, dev, n, what):
    if v is None:
        return None
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(v, dtype=np.float32)))
    t = t.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    if t.numel() != n:
        raise ValueError("%s must hold %d entries, not %d" % (what, n, t.numel()))
    return t


def xent_workspace(n, D, n_classes, dev):
    """(ws uint8, out float64 [1 + D C + C], flag int32 [1]) on the device for dmvae_softmax_xent at this shape; flag starts at zero"""
    nbytes = lib.dmvae_softmax_xent_ws_bytes(int(n), int(D), int(n_classes))
    if nbytes < 0:
        check(int(nbytes), "dmvae_softmax_xent_ws_bytes")
    return (torch.empty(int(nbytes), dtype=torch.uint8, device=dev), torch.empty(1 + (D + 1) * n_classes, dtype=torch.float64, device=dev),
            torch.zeros(1, dtype=torch.int32, device=dev))


def xent_enqueue(Z, classes, W, b, shift, scale, ws, out, flag):
    """dmvae_softmax_xent on the current stream: device tensors Z [n][D] f32 (unit column stride), classes int32 [n], W [D][C] f32 (unit
    column stride), b [C], shift / scale [D] or both None; ws, out, flag from xent_workspace.  Only enqueues."""
    assert Z.is_cuda and Z.dtype == torch.float32 and Z.dim() == 2 and W.is_cuda and W.dtype == torch.float32 and W.dim() == 2
    assert classes.is_cuda and classes.dtype == torch.int32 and classes.is_contiguous() and classes.numel() == Z.shape[0]
    (n, D), Cn, dev = Z.shape, W.shape[1], Z.device
    assert W.shape[0] == D and b.numel() == Cn and out.numel() == 1 + (D + 1) * Cn and out.dtype == torch.float64
    with torch.cuda.device(dev):
        check(lib.dmvae_softmax_xent(_stream(dev), Z.data_ptr(), _ld(Z), n, D, _ptr(shift), _ptr(scale), classes.data_ptr(), Cn, W.data_ptr(), _ld(W),
                                     b.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), flag.data_ptr()), "dmvae_softmax_xent")
    return out


def softmax_xent(Z, y, W, b, shift=None, scale=None):
    """(loss, gW [D][C], gb [C]) in float64: the mean over the rows of Z [n][D] of the cross-entropy of softmax(x W + b) against the
    classes y (integers in [0, C)), x = (Z - shift) * scale, and its gradient -- no penalty term.  Device tensors are used where they lie
    (row-strided f32 views included); arrays are uploaded.  IndexError: a class outside [0, C)."""
    dev = _device_of(Z)
    Zd, Wd = _rows_f32(Z, dev), _rows_f32(W, dev)
    (n, D), Cn = Zd.shape, Wd.shape[1]
    bd, sh, sc = _vec_f32(b, dev, Cn, "b"), _vec_f32(shift, dev, D, "shift"), _vec_f32(scale, dev, D, "scale")
    ws, out, flag = xent_workspace(n, D, Cn, dev)
    xent_enqueue(Zd, _int32_vector(y, dev), Wd, bd, sh, sc, ws, out, flag)
    host = out.cpu().numpy()
    if int(flag.item()):
        raise IndexError("softmax_xent: a class outside [0, %d)" % Cn)
    return float(host[0]), host[1:1 + D * Cn].reshape(D, Cn).copy(), host[1 + D * Cn:].copy()


def scores_enqueue(Z, W, b, shift=None, scale=None, out=None):
    """dmvae_linear_scores: the logits b + x W of the rows of Z as a device f32 [M][C] (or into `out`, unit column stride); only enqueues"""
    assert Z.is_cuda and Z.dtype == torch.float32 and Z.dim() == 2 and W.is_cuda and W.dtype == torch.float32 and W.dim() == 2
    (M, D), Cn, dev = Z.shape, W.shape[1], Z.device
    if out is None:
        out = torch.empty((M, Cn), dtype=torch.float32, device=dev)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == M and out.shape[1] >= Cn and out.stride(1) == 1
    with torch.cuda.device(dev):
        check(lib.dmvae_linear_scores(_stream(dev), Z.data_ptr(), _ld(Z), M, D, _ptr(shift), _ptr(scale), W.data_ptr(), _ld(W), b.data_ptr(), Cn,
                                      out.data_ptr(), _ld(out)), "dmvae_linear_scores")
    return out


class LogisticRegression:
    """sklearn.linear_model.LogisticRegression(C, tol, max_iter, solver="lbfgs") on the device for the multinomial objective

        mean_i loss_i + ||W||_F^2 / (2 C n),   the bias unpenalised,

    minimised by scipy's L-BFGS-B (gtol = tol, ftol = 64 eps, maxiter = max_iter) from zeros.  With TWO classes this is still the
    two-column softmax, where sklearn fits a single logit: the predictions agree, the coefficients are sklearn's halved and mirrored
    (and the penalty acts on both columns).  Per evaluation the float64 parameters go to the device as f32, one kernel pass over all rows
    leaves loss and gradient in one buffer, which comes back in one pinned copy; the penalty is added in float64 on the host.
    standardize: the fit rows' column mean and 1 / std (float64 on the device; a zero variance gives scale 1) reach the kernels as
    shift and scale -- no standardised copy of the rows is stored.  n_classes: y then holds integers in [0, n_classes) (NumPy or a
    device tensor) and classes_ = arange(n_classes); otherwise classes_ are the sorted distinct values of y.
    After fit: coef_ [C][D] and intercept_ [C] (float64, in raw feature space, the scaling folded back), coef_std_ / intercept_std_ (in
    the fitted space) with shift_ / scale_ (f32, NumPy; None without standardize), n_iter_, n_fev_, converged_."""

    def __init__(self, C=1.0, tol=1e-4, max_iter=100, fit_intercept=True, standardize=False, n_classes=None):
        if not float(C) > 0:
            raise ValueError("C must be positive")
        if n_classes is not None and not 2 <= int(n_classes) <= MAX_C:
            raise ValueError("n_classes must be in 2 .. %d" % MAX_C)
        self.C, self.tol, self.max_iter = float(C), float(tol), int(max_iter)
        self.fit_intercept, self.standardize = bool(fit_intercept), bool(standardize)
        self.n_classes = None if n_classes is None else int(n_classes)

    def fit(self, X, y):
        from scipy.optimize import minimize
        dev = _device_of(X)
        Z = _rows_f32(X, dev)
        n, D = Z.shape
        device_y = isinstance(y, torch.Tensor) and y.is_cuda
        if self.n_classes is None:
            yh = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
            self.classes_, inv = np.unique(yh, return_inverse=True)
            cls = _int32_vector(inv, dev)
        else:
            self.classes_ = np.arange(self.n_classes)
            cls = _int32_vector(y, dev)
        Cn = len(self.classes_)
        if cls.numel() != n:
            raise ValueError("y must hold one entry per row of X: %d != %d" % (cls.numel(), n))
        if Cn < 2:
            raise ValueError("the probe needs at least two classes")
        if self.standardize:
            Zd = Z.double()
            mean, var = Zd.mean(0), Zd.var(0, unbiased=False)
            self._shift = mean.float().contiguous()
            self._scale = torch.where(var > 0, var.rsqrt(), torch.ones_like(var)).float().contiguous()
            del Zd
        else:
            self._shift = self._scale = None
        ws, out, flag = xent_workspace(n, D, Cn, dev)
        nW, nP = D * Cn, (D + 1) * Cn
        params = torch.zeros(nP, dtype=torch.float32, device=dev)                # W [D][C], then b [C]
        Wd, bd = params[:nW].view(D, Cn), params[nW:]
        p_host = torch.zeros(nP, dtype=torch.float32).pin_memory()
        o_host = torch.empty(1 + nP, dtype=torch.float64).pin_memory()
        p_np, o_np = p_host.numpy(), o_host.numpy()
        nvar = nP if self.fit_intercept else nW
        pen = 1.0 / (self.C * n)
        stream = torch.cuda.current_stream(dev)

        def fun(theta):
            p_np[:nvar] = theta                                                  # float64 -> f32
            params.copy_(p_host, non_blocking=True)
            xent_enqueue(Z, cls, Wd, bd, self._shift, self._scale, ws, out, flag)
            o_host.copy_(out, non_blocking=True)
            stream.synchronize()
            w = theta[:nW]
            g = o_np[1:1 + nvar].copy()
            g[:nW] += pen * w
            return float(o_np[0]) + 0.5 * pen * float(w @ w), g

        res = minimize(fun, np.zeros(nvar), jac=True, method="L-BFGS-B",
                       options=dict(gtol=self.tol, ftol=64 * np.finfo(np.float64).eps, maxiter=self.max_iter))
        if (device_y or self.n_classes is not None) and int(flag.item()):
            raise IndexError("LogisticRegression.fit: a class outside [0, %d)" % Cn)
        theta = np.zeros(nP)
        theta[:nvar] = res.x
        p_np[:] = theta                                                          # the scores use the f32 parameters the last evaluations saw
        params.copy_(p_host)
        self._W, self._b = Wd, bd
        self.coef_std_ = theta[:nW].reshape(D, Cn).T.copy()
        self.intercept_std_ = theta[nW:].copy()
        if self.standardize:
            self.shift_, self.scale_ = self._shift.cpu().numpy(), self._scale.cpu().numpy()
            sc, sh = self.scale_.astype(np.float64), self.shift_.astype(np.float64)
            self.coef_ = self.coef_std_ * sc[None, :]
            self.intercept_ = self.intercept_std_ - self.coef_ @ sh
        else:
            self.shift_ = self.scale_ = None
            self.coef_, self.intercept_ = self.coef_std_.copy(), self.intercept_std_.copy()
        self.n_iter_, self.n_fev_, self.converged_ = int(res.nit), int(res.nfev), bool(res.success)
        self.objective_ = float(res.fun)
        return self

    def decision_function(self, X):
        """the logits of the rows of X as a device f32 [M][C] tensor (dmvae_linear_scores; only enqueues)"""
        dev = self._W.device
        return scores_enqueue(_rows_f32(X, dev), self._W, self._b, self._shift, self._scale)

    def predict(self, X):
        return self.classes_[argmax_labels(self.decision_function(X)).cpu().numpy()]

    def predict_proba(self, X):
        return torch.softmax(self.decision_function(X).double(), dim=1).cpu().numpy()

    def score(self, X, y):
        y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
        return float(np.mean(self.predict(X) == y))
