"""What the exact GEMM suites share (tests/test_gpu_gemm_forms.py, tests/test_gpu_gemm256_forms.py): padded, guarded, sentinel-filled device
buffers, the epilogue of a gemm_exact problem, the launch through dmvae_gemm / dmvae_gemm_grouped, the comparisons, the knob context and
the profiler rows of a call.  Needs the GPU; the inputs and expected values are tests/helpers/gemm_exact.py's."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_exact as GX

T_INT = {"bf16": torch.int16, "f32": torch.int32}
T_FLT = {"bf16": torch.bfloat16, "f32": torch.float32}
IN_SENT = {"bf16": GX.NAN_BF16_BITS, "f32": GX.NAN_F32_BITS}
OUT_SENT = {"bf16": GX.SENT_BF16_BITS, "f32": GX.NAN_F32_BITS}
ACT_EPIS = (GX.EPI_BIAS_RELU, GX.EPI_RELU_MASK, GX.EPI_LATENT, GX.EPI_BIAS_RECON)       # epilogues whose `out` has the activation type


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """[rows][width] inside a leading dimension of width + PAD, between two guard bands of GUARD elements; whatever is not data holds a
    sentinel.  fill = "in": data + NaN pads; "out": all sentinel (7.0 for bf16, a NaN pattern for f32); "zero": zeros inside sentinel pads."""

    def __init__(self, rows, width, kind, data=None, fill="in"):
        self.rows, self.width, self.kind = rows, width, kind
        self.ld = width + GX.PAD[kind]
        self.sent = (IN_SENT if fill == "in" else OUT_SENT)[kind]
        host = torch.full((2 * GX.GUARD + rows * self.ld,), self.sent, dtype=T_INT[kind])
        body = host[GX.GUARD:GX.GUARD + rows * self.ld].view(rows, self.ld)
        if data is not None:
            assert data.shape == (rows, width)
            body[:, :width] = torch.as_tensor(np.ascontiguousarray(data, dtype=np.float64)).to(T_FLT[kind]).view(T_INT[kind])
        elif fill == "zero":
            body[:, :width] = 0
        self.dev = host.cuda()
        self.ptr = self.dev.data_ptr() + GX.GUARD * host.element_size()

    def read(self):
        """(bit patterns of [rows][width], guards and pad columns untouched?)"""
        host = self.dev.cpu()
        body = host[GX.GUARD:-GX.GUARD].view(self.rows, self.ld)
        clean = bool((host[:GX.GUARD] == self.sent).all() and (host[-GX.GUARD:] == self.sent).all() and (body[:, self.width:] == self.sent).all())
        return body[:, :self.width].contiguous(), clean


def values(res, name):
    bits, kind = res[name]
    return bits.view(T_FLT[kind]).double().numpy()


def setup(L, kind, p):
    """device buffers and the epilogue of problem p for a launch of type kind ("bf16" | "f32")"""
    pair, M, N = p.pair, p.M, p.N
    b = {"A": Buf(p.A_mem.shape[0], p.A_mem.shape[1], kind, p.A_mem), "B": Buf(p.B_mem.shape[0], p.B_mem.shape[1], kind, p.B_mem)}
    e = L.Epilogue()
    e.kind = pair.epi
    if p.bias is not None:
        b["bias"] = Buf(1, N, "f32", p.bias.reshape(1, N))
        e.bias = b["bias"].ptr
    for name, (arr, k) in p.aux.items():
        b[name] = Buf(M, arr.shape[1], kind if k == "act" else "f32", arr)
        setattr(e, name, b[name].ptr)
        setattr(e, "ld" + name[-1], b[name].ld)
    fill = "zero" if pair.epi == GX.EPI_ATOMIC_F32 else "out"
    b["out"] = Buf(M, 2 * N if pair.epi == GX.EPI_LATENT else N, kind if pair.epi in ACT_EPIS else "f32", fill=fill)
    e.out, e.ldo = b["out"].ptr, b["out"].ld
    if pair.epi == GX.EPI_LATENT:
        e.d_off = N
    if pair.layout == GX.DW:
        b["out2"] = Buf(1, N, "f32", fill=fill)                      # the fused bias gradient
        e.out2 = b["out2"].ptr
    if pair.epi == GX.EPI_BIAS_RECON:
        b["out2"] = Buf(M, N, "f32", fill="out")                     # the logits copy
        e.out2, e.ldo2 = b["out2"].ptr, b["out2"].ld
        cells = L.lib.dmvae_gemm_partials(L.BF16 if kind == "bf16" else L.F32, M, N)
        assert cells == (M // 64) * (N // 64)
        b["partials"] = Buf(1, cells, "f32", fill="out")             # NaN: a cell that is not written shows
        e.partials = b["partials"].ptr
        e.m_valid, e.n_valid, e.recon_kind, e.scale = p.m_valid, p.n_valid, pair.recon_kind, GX.RECON_SCALE
    return b, e


def collect(b, what):
    res = {}
    for name in ("out", "out2", "partials"):
        if name in b:
            bits, clean = b[name].read()
            assert clean, "%s: `%s` was written outside [rows][width] (pad columns / guard bands)" % (what, name)
            res[name] = (bits, b[name].kind)
    return res


def launched(L, rc, what):
    """the launch was accepted and ran to its end.  A launch that faults leaves the device in no state to go on with: the session ends here
    instead of sending the remaining cases after it"""
    try:
        L.check(rc, what)
        torch.cuda.synchronize()
    except (L.DmvaeError, RuntimeError) as err:
        pytest.exit("%s: %s -- nothing more is launched" % (what, err), returncode=1)


def run(L, kind, p):
    b, e = setup(L, kind, p)
    what = "%s %dx%dx%d %s" % (p.pair.name, p.M, p.N, p.K, kind)
    launched(L, L.lib.dmvae_gemm(stream(), L.BF16 if kind == "bf16" else L.F32, p.pair.layout, p.M, p.N, p.K, C.c_void_p(b["A"].ptr), b["A"].ld,
                                 C.c_void_p(b["B"].ptr), b["B"].ld, C.byref(e), p.pair.split), what)
    return collect(b, what)


def run_grouped(L, pair, shapes):
    n = len(shapes)
    probs = (L.GemmProblem * n)()
    keep = []
    for i, (M, N, K) in enumerate(shapes):
        p = GX.make(pair.name, M, N, K)
        b, e = setup(L, "bf16", p)
        q = probs[i]
        q.M, q.N, q.K = M, N, K
        q.A, q.lda, q.B, q.ldb = b["A"].ptr, b["A"].ld, b["B"].ptr, b["B"].ld
        q.epi = e
        keep.append((p, b))
    launched(L, L.lib.dmvae_gemm_grouped(stream(), L.BF16, pair.layout, probs, n), "dmvae_gemm_grouped %s" % pair.name)
    return [(p, collect(b, "grouped %s %dx%dx%d" % (pair.name, p.M, p.N, p.K))) for p, b in keep]


def verify(p, kind, res, bm, bn):
    """the exact part: outputs, the logits copy, and -- real reconstruction kind -- the loss partials of every (bm x bn) tile"""
    what = "%s %dx%dx%d %s" % (p.pair.name, p.M, p.N, p.K, kind)
    for name in ("out", "out2"):
        if name in p.expected:
            arr, k = p.expected[name]
            want = GX.bf16_round(arr) if (k == "act" and kind == "bf16") else arr
            np.testing.assert_array_equal(values(res, name), want, err_msg="%s: %s" % (what, name))
    if "partials" in res:
        cells = values(res, "partials").reshape(p.M // 64, p.N // 64)
        assert not np.isnan(cells).any(), "%s: a loss-partial cell was not written" % what
        if "terms" in p.expected:
            terms = p.expected["terms"][0]
            np.testing.assert_array_equal(GX.tile_sums(cells, bm // 64, bn // 64), GX.tile_sums(terms, bm, bn), err_msg="%s: loss partial per tile" % what)
            assert cells.sum() == terms.sum(), what


def verify_inexact(p, kind, res, yard):
    """binary reconstruction kind / sigmoid: `res` must have the bits of `yard` (the 64 x 64 / 4-wave form on the same inputs; None: the f32
    kernel has one form), and the yardstick is within the tolerances of test_epilogues of float64"""
    what = "%s %dx%dx%d %s" % (p.pair.name, p.M, p.N, p.K, kind)
    if yard is not None:
        assert torch.equal(res["out"][0], yard["out"][0]), "%s: not the bits of the 64 x 64 form (%d elements differ)" % (
            what, int((res["out"][0] != yard["out"][0]).sum()))
    else:
        yard = res
    if p.pair.epi == GX.EPI_BIAS_SIGMOID:
        logits = p.expected["logits"][0]
        np.testing.assert_allclose(values(yard, "out"), 1.0 / (1.0 + np.exp(-logits)), atol=1e-3 if kind == "bf16" else 2e-6, err_msg=what)
        return
    per, dref = GX.binary_reference(p, p.expected["out2"][0])
    np.testing.assert_allclose(values(yard, "out"), dref, atol=3e-5 if kind == "bf16" else 1e-7, rtol=1e-2 if kind == "bf16" else 1e-5, err_msg=what)
    for r in (res, yard):
        assert values(r, "partials").sum() == pytest.approx(per.sum(), rel=2e-5), what


@contextlib.contextmanager
def forced(L, tile=(0, 0), knobs=None):
    """knob 6 = 0 (the 256 x 256 macro tile never takes a case), the tile override and the knobs of a form; every default restored"""
    try:
        L.check(L.lib.dmvae_debug_set_knob(6, 0))
        L.check(L.lib.dmvae_debug_set_tile(*tile))
        for k, v in (knobs or {}).items():
            L.check(L.lib.dmvae_debug_set_knob(k, v))
        yield
    finally:
        L.lib.dmvae_debug_set_tile(0, 0)
        for k, v in GX.KNOB_DEFAULTS.items():
            L.lib.dmvae_debug_set_knob(k, v)


def kernels_launched(L, fn):
    """(names of the profiler rows of the launches fn makes, fn's result)"""
    rows = (L.ProfRow * 32)()
    L.lib.dmvae_prof_collect(rows, 32)          # drop whatever was recorded before
    L.lib.dmvae_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.lib.dmvae_prof_enable(0)
        n = L.lib.dmvae_prof_collect(rows, 32)
    return [rows[i].name.decode() for i in range(n)], out


def bf16_name(bm, bn, pair, nstage, nw):
    return "gemm_bf16_kernel<%d, %d, %d, %d, %d, %d>" % (bm, bn, pair.layout, pair.epi, nstage, nw)
