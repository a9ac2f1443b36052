"""What the suites of the fused weight-gradient + Adam epilogue share (tests/test_gpu_dw_adam_forms.py, tests/test_gpu_gemm256_forms.py):
the five arenas of tests/helpers/adam_exact.py on the device, padded bf16 operands, the state blob, the problems and the context of a
launch, the knob context and the profiler rows of a call.  Needs the GPU."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import adam_exact as AX
import gemm_exact as GX

F = np.float32
ARENAS = ("param", "grad", "m", "v", "shadow")
NOT_HOST_T = C.c_uint64(2 ** 64 - 1)                    # dmvae_adam_tf: t = state->adam_t as it stands


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launched(L, rc, what):
    """the launch was accepted and ran to its end.  A launch that faults leaves the device in no state to go on with: the session ends here
    instead of sending the remaining cases after it"""
    try:
        L.check(rc, what)
        torch.cuda.synchronize()
    except (L.DmvaeError, RuntimeError) as err:
        pytest.exit("%s: %s -- nothing more is launched" % (what, err), returncode=1)


@contextlib.contextmanager
def forced(L, knobs):
    try:
        for k, v in knobs.items():
            L.check(L.lib.dmvae_debug_set_knob(k, v))
        yield
    finally:
        for k, v in GX.KNOB_DEFAULTS.items():
            L.lib.dmvae_debug_set_knob(k, v)


def profiled(L, fn):
    """({profiler row: scopes recorded} of the launches fn makes, fn's result)"""
    rows = (L.ProfRow * 32)()
    L.lib.dmvae_prof_collect(rows, 32)          # drop whatever was recorded before
    L.lib.dmvae_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.lib.dmvae_prof_enable(0)
        n = L.lib.dmvae_prof_collect(rows, 32)
    return {rows[i].name.decode(): int(rows[i].launches) for i in range(n)}, out


class Operand:
    """a bf16 operand [rows][width] inside a leading dimension of width + 64, between guard bands; pads and guards hold NaN"""

    def __init__(self, data):
        rows, width = data.shape
        self.ld = width + GX.PAD["bf16"]
        host = torch.full((2 * GX.GUARD + rows * self.ld,), GX.NAN_BF16_BITS, dtype=torch.int16)
        host[GX.GUARD:GX.GUARD + rows * self.ld].view(rows, self.ld)[:, :width] = torch.as_tensor(np.ascontiguousarray(data)).to(torch.bfloat16).view(torch.int16)
        self.dev = host.cuda()
        self.ptr = self.dev.data_ptr() + 2 * GX.GUARD


def state_blob(L):
    """the device step state as step_finalize leaves it for the update t = adam_t: the fused forms read lr_t, the stand-alone kernel
    recomputes it from lr and adam_t (to the same float32: test_lr_t_rounds_the_same_on_host_and_device)"""
    st = L.State()
    st.adam_t, st.lr, st.lr_t = AX.T_STEP, float(AX.LR), float(AX.lr_t(AX.T_STEP))
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).cuda()


def upload(init):
    return {k: torch.as_tensor(init[k].view(np.int16) if k == "shadow" else init[k]).cuda() for k in ARENAS}


def download(dev):
    return {k: (dev[k].cpu().numpy().view(np.uint16) if k == "shadow" else dev[k].cpu().numpy()) for k in ARENAS}


def problems(L, lay, dev, kind=AX.EPI_ADAM):
    probs = (L.GemmProblem * len(lay.probs))()
    keep = []
    for i, q in enumerate(lay.probs):
        p, _, _ = AX.gradients(q)
        A, B = Operand(p.A_mem), Operand(p.B_mem)       # X [K][M], dY [K][N]
        keep += [A, B]
        r = probs[i]
        r.M, r.N, r.K = q.M, q.N, q.K
        r.A, r.lda, r.B, r.ldb = A.ptr, A.ld, B.ptr, B.ld
        r.epi.kind = kind
        r.epi.out, r.epi.ldo = dev["grad"].data_ptr() + 4 * lay.w_off[i], lay.ldo[i]
        r.epi.out2 = dev["grad"].data_ptr() + 4 * lay.b_off[i] if q.bias else None
    return probs, keep


def context(L, lay, dev, state, mode, store_grad, gscale):
    ctx = L.AdamCtx()
    ctx.param, ctx.grad, ctx.m, ctx.v = (dev[k].data_ptr() for k in ("param", "grad", "m", "v"))
    ctx.param_bf16 = dev["shadow"].data_ptr() if mode["shadow"] else None
    ctx.state = state.data_ptr()
    ctx.beta1, ctx.beta2, ctx.epsilon, ctx.grad_scale = float(AX.B1), float(AX.B2), float(AX.EPS), gscale
    ctx.store_grad, ctx.ieee = store_grad, mode["ieee"]
    ctx.seg_off, ctx.seg_n = lay.seg_off, lay.seg_n
    return ctx


def bits(a):
    b = np.ascontiguousarray(a).view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)
    return b
