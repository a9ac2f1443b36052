"""Every fused epilogue of the dense GEMMs on every tile form, each forced alone and held to an EXACT reference.

launch_tiled / grouped_launch (csrc/gemm_bf16.hip) send a (layout, epilogue) pair to one of about ten instantiations, and the epilogue
code depends on the tile: quads per thread, the prefetched bias quad / ReLU gates / reconstruction targets, the LAT_PRE register path,
the swizzled LDS round trip, the cell a tile writes its loss partial to, the supertile order.  Here dmvae_debug_set_tile and knobs
0 / 1 / 7 / 9 / 18 force each form, the profiler rows say which instantiation really ran, and the inputs come from
tests/helpers/gemm_exact.py: small integers for which every intermediate is representable, so all comparisons are equalities
(tests/test_gemm_exact_host.py checks those conditions on the CPU).  Every buffer has a leading dimension wider than its matrix and a
guard band on either side; outputs are prefilled with a sentinel, input pads hold NaN: an element not written, written twice from the
wrong tile, a store outside [M][N] or a read of a pad column all show.  The binary reconstruction kind and the sigmoid use the hardware
exponential: their logits are exact, their outputs must have the bits of the 64 x 64 / 4-wave form (element-wise arithmetic), and that
form is held to float64 at the tolerances of test_gpu_kernels.py::test_epilogues."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import gemm_exact as GX      # noqa: E402

T_INT = {"bf16": torch.int16, "f32": torch.int32}
T_FLT = {"bf16": torch.bfloat16, "f32": torch.float32}
IN_SENT = {"bf16": GX.NAN_BF16_BITS, "f32": GX.NAN_F32_BITS}
OUT_SENT = {"bf16": GX.SENT_BF16_BITS, "f32": GX.NAN_F32_BITS}
ACT_EPIS = (GX.EPI_BIAS_RELU, GX.EPI_RELU_MASK, GX.EPI_LATENT, GX.EPI_BIAS_RECON)       # epilogues whose `out` has the activation type


@pytest.fixture(scope="module")
def hip():
    import dmvae_hip      # noqa: F401
    from dmvae_hip import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    assert (_lib.GEMM_FWD, _lib.GEMM_DX, _lib.GEMM_DW) == (GX.FWD, GX.DX, GX.DW)
    assert (_lib.EPI_BIAS_RELU, _lib.EPI_BIAS_F32, _lib.EPI_BIAS_RECON, _lib.EPI_RELU_MASK, _lib.EPI_LATENT, _lib.EPI_STORE_F32, _lib.EPI_ATOMIC_F32,
            _lib.EPI_BIAS_SIGMOID) == tuple(range(8))
    return _lib


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


# ------------------------------------------------------------------------------------------------ every pair on every form
@pytest.mark.parametrize("case", GX.dense_cases(), ids=lambda c: c.id)
def test_form_pair_exact(hip, case):
    """one (form, pair) over the K set (1, 2, 3, 5, 9 K tiles per slice) on a 5 x 3 tile grid; the first launch runs under the profiler and
    must be the instantiation the form names -- a form that fell back to the heuristic would pass vacuously otherwise"""
    L, f, pair = hip, case.form, case.pair
    for i, K in enumerate(case.Ks):
        p = GX.make(pair.name, case.M, case.N, K)
        with forced(L, (f.bm, f.bn), f.knobs):
            if i == 0:
                names, res = kernels_launched(L, lambda: run(L, "bf16", p))
                assert names == [bf16_name(f.bm, f.bn, pair, f.nstage, f.nw)], (case.id, names)
                print("KERNEL %s -> %s" % (case.id, names[0]))
            else:
                res = run(L, "bf16", p)
        verify(p, "bf16", res, f.bm, f.bn)
        if pair.name in GX.INEXACT:
            with forced(L, (64, 64)):
                yard = run(L, "bf16", p)
            verify(p, "bf16", yard, 64, 64)
            verify_inexact(p, "bf16", res, yard)


@pytest.mark.parametrize("case", GX.supertile_cases(), ids=lambda c: c.id)
def test_supertile_order_covers_every_tile_once(hip, case):
    """knob 0 = 2, 3, 4 on five tile rows: the last supertile is shorter than the others.  The order is a bijection onto the tiles or some
    tile is dropped (sentinel left) while another is computed twice"""
    L, f = hip, case.form
    for K in case.Ks:
        p = GX.make(case.pair.name, case.M, case.N, K)
        with forced(L, (f.bm, f.bn), {**f.knobs, 0: case.group_m}):
            res = run(L, "bf16", p)
        verify(p, "bf16", res, f.bm, f.bn)


@pytest.mark.parametrize("case", GX.THIN_CASES, ids=lambda c: c.id)
def test_thin_dz_tiles_exact(hip, case):
    """the dZ GEMM on 16-row (two waves) and 32-row tiles, 16 and 17 K tiles: exact, and the bits of the general 64 x 64 tile (knob 18 = 0)"""
    L, pair = hip, GX.PAIRS["dx_latent"]
    for K in case.Ks:
        p = GX.make("dx_latent", case.M, case.N, K)
        with forced(L, (0, 0), {18: case.knob}):
            names, res = kernels_launched(L, lambda: run(L, "bf16", p))
        assert names == [bf16_name(case.rows, 64, pair, 4, case.nw)], names
        print("KERNEL %s K=%d -> %s" % (case.id, K, names[0]))
        verify(p, "bf16", res, 64, 64)
        with forced(L, (0, 0), {18: 0}):
            names0, res0 = kernels_launched(L, lambda: run(L, "bf16", p))
        assert names0 == [bf16_name(64, 64, pair, 4, 4)], names0
        verify(p, "bf16", res0, 64, 64)
        assert torch.equal(res["out"][0], res0["out"][0])


# ------------------------------------------------------------------------------------------------ grouped launches
@pytest.mark.parametrize("case", GX.grouped_cases(), ids=lambda c: c.id)
def test_grouped_launch_exact(hip, case):
    """four problems of mixed shapes in ONE dmvae_gemm_grouped call, each on padded buffers of its own, each held to its exact product:
    all 64 x 64 tiles, the planned per-problem tiles, the largest tiles (knob 2), four and eight waves (knob 9)"""
    L = hip
    with forced(L, (0, 0), case.knobs):
        names, out = kernels_launched(L, lambda: run_grouped(L, case.pair, case.shapes))
    assert names == ["gemm_bf16_grouped_mixed_tiles<L%d, E%d>" % (case.pair.layout, case.pair.epi)], names
    print("KERNEL grouped %s -> %s" % (case.id, names[0]))
    for p, res in out:
        verify(p, "bf16", res, 64, 64)


def test_grouped_dx_streaming_kernel_and_tiles_exact(hip):
    """K = 128: the group the streaming kernel (csrc/heads_dx.hip) takes with knob 13 = 1 and the grouped tiles with 0 -- both exact, the same bits"""
    L, pair = hip, GX.PAIRS["dx_relu_mask"]
    outs = []
    for knob, want in ((0, "gemm_bf16_grouped_mixed_tiles<L1, E3>"), (1, "heads_dx_stream_kernel")):
        with forced(L, (0, 0), {13: knob}):
            names, out = kernels_launched(L, lambda: run_grouped(L, pair, GX.GROUP_DX_STREAM))
        assert names == [want], names
        print("KERNEL grouped dx K=128 knob13=%d -> %s" % (knob, names[0]))
        for p, res in out:
            verify(p, "bf16", res, 64, 64)
        outs.append(out)
    for (_, a), (_, b) in zip(*outs):
        assert torch.equal(a["out"][0], b["out"][0])


# ------------------------------------------------------------------------------------------------ the f32 kernel
@pytest.mark.parametrize("case", GX.f32_cases(), ids=lambda c: c.id)
def test_f32_kernel_exact(hip, case):
    """csrc/gemm_f32.hip (one instantiation per pair) on the same pairs, padded leading dimensions and guards"""
    L, pair = hip, case.pair
    for i, K in enumerate(case.Ks):
        p = GX.make(pair.name, case.M, case.N, K)
        with forced(L):
            names, res = kernels_launched(L, lambda: run(L, "f32", p))
        assert names == [("gemm_f32_fwd", "gemm_f32_dx", "gemm_f32_dw")[pair.layout]], names
        verify(p, "f32", res, 64, 64)
        if pair.name in GX.INEXACT:
            verify_inexact(p, "f32", res, None)
