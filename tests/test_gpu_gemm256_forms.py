"""The 256 x 256 macro tile (csrc/gemm_bf16_256.hip) held to EXACT references: every epilogue it is instantiated for, the column sums it
leaves for the next weight-gradient launch, the bias gradient it makes of such sums, and its K slices into slabs.

The kernel has its own copy of what tests/test_gpu_gemm_forms.py checks on the small tiles -- the swizzled LDS round trip, the prefetched
bias quad / ReLU gates / reconstruction targets, the supertile and XCD-run tile order, the loss cells (16 per tile, the sum in cell 0) --
and that file turns the macro tile off.  Here knob 6 = 2 sends every shape that divides by 256 to it; inputs, padded buffers, guard
bands, sentinels and the comparisons are that file's (tests/helpers/gemm_exact.py; the conditions are checked on the CPU by
tests/test_gemm_exact_host.py), and every case asserts from the profiler rows that the macro-tile kernel really ran.

Two mechanisms only the step reaches (csrc/step.hip) come through dmvae_debug_gemm256:
  * csum_out: RELU_MASK / BIAS_RECON leave the column sums of the bf16-rounded output per 256-row tile; csum_in: a weight-gradient
    problem takes such partials and its extra workgroups add them in ascending order into the bias gradient (and its Adam update);
  * K slices of a weight-gradient problem into slabs, alone and merged with other problems in one grid (Multi256's start / nsl / extra).
One step-level identity closes the loop: the output layer's bias gradient of a macro-tile plan is the column sum of its dxlogits."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "helpers") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "helpers"))

import gemm_exact as GX                  # noqa: E402
import adam_exact as AX                  # noqa: E402
import step_launch_dump as D             # noqa: E402
import gemm_harness as GF                # noqa: E402      Buf, setup, collect, verify, verify_inexact, launched, kernels_launched, forced
import adam_harness as DA                # noqa: E402      the arenas of the fused Adam epilogue on the device

Buf, values, stream = GF.Buf, GF.values, GF.stream
EINVAL, EUNSUPPORTED = -1, -2            # include/dmvae_hip.h
F = np.float32


@pytest.fixture(scope="module")
def hip():
    import dmvae_hip      # noqa: F401
    from dmvae_hip import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    assert (_lib.GEMM_FWD, _lib.GEMM_DX, _lib.GEMM_DW) == (GX.FWD, GX.DX, GX.DW) and _lib.EPI_ADAM == AX.EPI_ADAM
    return _lib


@contextlib.contextmanager
def macro(L, knobs=None):
    """knob 6 = 2: the macro tile takes whatever divides by 256 and it is instantiated for; every default restored"""
    try:
        L.check(L.lib.dmvae_debug_set_tile(0, 0))
        L.check(L.lib.dmvae_debug_set_knob(6, 2))
        for k, v in (knobs or {}).items():
            L.check(L.lib.dmvae_debug_set_knob(k, v))
        yield
    finally:
        L.lib.dmvae_debug_set_tile(0, 0)
        for k, v in {**GX.KNOB_DEFAULTS, **D.KNOB_DEFAULTS}.items():
            L.lib.dmvae_debug_set_knob(k, v)


def what_of(p):
    return "%s %dx%dx%d" % (p.pair.name, p.M, p.N, p.K)


def loss_cells(p, res):
    """16 cells per 256 x 256 tile, all written, the tile's sum in cell 0 and exact zeros in the other 15"""
    cells = values(res, "partials").reshape(p.M // 256, 4, p.N // 256, 4)
    assert not np.isnan(cells).any(), "%s: a loss-partial cell was not written" % what_of(p)
    rest = cells.copy()
    rest[:, 0, :, 0] = 0.0
    assert not rest.any(), "%s: a loss partial outside cell 0 of its tile" % what_of(p)
    assert (cells[:, 0, :, 0] > 0).all(), "%s: a tile without a loss partial in its cell 0" % what_of(p)      # (every tile holds valid elements)
    return cells[:, 0, :, 0]


# ------------------------------------------------------------------------------------------------ every pair, through dmvae_gemm
@pytest.mark.parametrize("case", GX.macro_cases(), ids=lambda c: c.id)
def test_macro_pair_exact(hip, case):
    """one pair over the K set on 5 x 3 macro tiles (or one tile, one K tile); each launch three times on fresh sentinel-filled buffers and
    compared each time (a racy hand-off of the staggered wave groups rarely fails twice the same way); the first runs under the profiler"""
    L, pair = hip, case.pair
    for K in case.Ks:
        p = GX.make(pair.name, case.M, case.N, K)
        for rep in range(3):
            with macro(L):
                if rep == 0:
                    names, res = GF.kernels_launched(L, lambda: GF.run(L, "bf16", p))
                    assert names == case.rows, (case.id, K, names)
                    print("KERNEL %s K=%d -> %s" % (case.id, K, names))
                else:
                    res = GF.run(L, "bf16", p)
            GF.verify(p, "bf16", res, 256, 256)
            if "partials" in res:
                loss_cells(p, res)
            if pair.name in GX.INEXACT:
                if rep == 0:
                    with GF.forced(L, (64, 64)):
                        yard = GF.run(L, "bf16", p)
                    GF.verify(p, "bf16", yard, 64, 64)
                GF.verify_inexact(p, "bf16", res, yard)


@pytest.mark.parametrize("case", GX.macro_fallback_cases(), ids=lambda c: c.id)
def test_pairs_without_a_macro_instantiation_stay_on_the_small_tiles(hip, case):
    L, pair = hip, case.pair
    for K in case.Ks:
        p = GX.make(pair.name, case.M, case.N, K)
        with macro(L):
            names, res = GF.kernels_launched(L, lambda: GF.run(L, "bf16", p))
        assert names and not [n for n in names if "gemm_bf16_256" in n or n == "colsum_slabs"], (case.id, names)
        print("KERNEL %s K=%d -> %s" % (case.id, K, names))
        GF.verify(p, "bf16", res, 64, 64)
        if pair.name in GX.INEXACT:
            with GF.forced(L, (64, 64)):
                yard = GF.run(L, "bf16", p)
            GF.verify_inexact(p, "bf16", res, yard)


# ------------------------------------------------------------------------------------------------ dmvae_debug_gemm256
def item(p, b, e, **kw):
    return dict(p=p, b=b, e=e, **kw)


def call256(L, layout, items, ctx=None):
    """dmvae_debug_gemm256's return code for problems given as item(...) dicts"""
    n = len(items)
    probs = (L.DebugGemm256Problem * n)()
    for q, it in zip(probs, items):
        p, b = it["p"], it["b"]
        q.p.M, q.p.N, q.p.K = it.get("shape", (p.M, p.N, p.K))
        q.p.A, q.p.lda, q.p.B, q.p.ldb = b["A"].ptr, b["A"].ld, b["B"].ptr, b["B"].ld
        q.p.epi = it["e"]
        q.csum_out, q.csum_in = it.get("csum_out"), it.get("csum_in")
        q.csum_ld, q.csum_rows = it.get("csum_ld", 0), it.get("csum_rows", 0)
        q.k_split, q.slab_stride = it.get("k_split", 0), it.get("slab_stride", 0)
    return L.lib.dmvae_debug_gemm256(stream(), layout, probs, n, C.byref(ctx) if ctx is not None else None)


def run256(L, layout, items, what, ctx=None):
    """the call under the profiler: the names of its rows"""
    names, _ = GF.kernels_launched(L, lambda: GF.launched(L, call256(L, layout, items, ctx), "dmvae_debug_gemm256 %s" % what))
    print("KERNEL %s -> %s" % (what, names))
    return names


def refused(L, rc, code, text=None):
    torch.cuda.synchronize()
    msg = L.lib.dmvae_last_error().decode()
    assert rc == code, (rc, code, msg)
    assert text is None or text in msg, msg


def untouched(buf):
    bits, clean = buf.read()
    return clean and bool((bits == buf.sent).all())


@pytest.mark.parametrize("key", GX.CSUM_OUT_CASES, ids=lambda k: "%s-%dx%dx%d" % k)
def test_csum_out(hip, key):
    """the column sums per 256-row tile of what the launch stores (rounded to bf16; rows / columns beyond the valid counts are zeros), pads of
    the [M / 256][N + 32] table and its guards untouched; without csum_out the same output bits and nothing else"""
    L = hip
    p = GX.make(*key)
    row = "gemm_bf16_256_kernel<%d, %d>" % (p.pair.layout, p.pair.epi)
    b, e = GF.setup(L, "bf16", p)
    cs = Buf(p.M // 256, p.N, "f32", fill="out")
    with macro(L, {6: 0}):      # (the entry reaches the macro tile whatever knob 6 says)
        names = run256(L, p.pair.layout, [item(p, b, e, csum_out=cs.ptr, csum_ld=cs.ld)], "csum_out " + what_of(p))
    assert names == [row], names
    res = GF.collect(b, what_of(p))
    GF.verify(p, "bf16", res, 256, 256)
    if "partials" in res:
        loss_cells(p, res)
    bits, clean = cs.read()
    assert clean, "%s: csum_out was written outside [M / 256][N]" % what_of(p)
    got = bits.view(torch.float32).double().numpy()
    if p.pair.name in GX.INEXACT:
        GF.verify_inexact(p, "bf16", res, None)         # (the float64 tolerances of the existing suite; the bits of the 64 x 64 form: test_macro_pair_exact)
        # the binary kind's gradient comes from the hardware exponential: the reference is the column sum of the bf16 values the kernel itself
        # stored.  They are exact in f32; a tile's column is 256 addends = 255 f32 additions in some order, each rounded to nearest
        # (relative error <= 2^-24 of a partial sum, itself <= the sum of |addends|): |error| <= 255 x 2^-24 x sum |addends|
        out = values(res, "out")
        want, bound = GX.tile_colsums(out), 255 * 2.0 ** -24 * GX.tile_colsums(np.abs(out))
        err = np.abs(got - want)
        print("CSUM %s: max |error| / bound = %.3g" % (what_of(p), float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), "%s: csum_out off by more than 255 x 2^-24 x sum |addends| in %d columns" % (what_of(p), int((err > bound).sum()))
        assert np.abs(want).max() > 0
    else:
        np.testing.assert_array_equal(got, GX.csum_out_expected(p), err_msg="%s: csum_out" % what_of(p))
    # csum_out = NULL: the same launch, nothing else written
    b0, e0 = GF.setup(L, "bf16", p)
    with macro(L):
        names = run256(L, p.pair.layout, [item(p, b0, e0)], "no csum_out " + what_of(p))
    assert names == [row], names
    res0 = GF.collect(b0, what_of(p))
    for k in res:
        assert torch.equal(res[k][0], res0[k][0]), "%s: `%s` differs with and without csum_out" % (what_of(p), k)


def dw_setup(L, p, with_bias=True):
    b, e = GF.setup(L, "bf16", p)
    if not with_bias:
        del b["out2"]
        e.out2 = None
    return b, e


def csum_in_store_item(L, shape):
    M, N, K, rows = shape
    p = GX.make("dw_store_db", M, N, K)
    part = GX.csum_in_partials(M, N, K, rows)
    pb = Buf(1, rows * N, "f32", part.reshape(1, rows * N))
    b, e = dw_setup(L, p)
    return item(p, b, e, csum_in=pb.ptr, csum_ld=N, csum_rows=rows, part=part, keep=pb)


def csum_in_store_verify(it):
    p, part = it["p"], it["part"]
    res = GF.collect(it["b"], what_of(p))
    np.testing.assert_array_equal(values(res, "out"), p.expected["out"][0], err_msg="%s: dW" % what_of(p))
    want = np.zeros(p.N, dtype=F)
    for r in range(part.shape[0]):
        want = want + part[r].astype(F)
    np.testing.assert_array_equal(values(res, "out2").reshape(p.N), want.astype(np.float64), err_msg="%s: db, the ascending sum of the partials" % what_of(p))
    assert not np.array_equal(want.astype(np.float64), p.expected["out2"][0].reshape(p.N))      # (a db recomputed from dY would differ)
    assert it["keep"].read()[1]


@pytest.mark.parametrize("shape", GX.CSUM_IN_CASES, ids=lambda s: "%dx%dx%d-rows%d" % s)
def test_csum_in_store(hip, shape):
    """DW + STORE_F32 with partials that are NOT the column sums of B: db is their ascending sum (integers: exact), the slab column sums of B
    are not computed; partials with a leading dimension other than N are refused"""
    L = hip
    M, N, K, rows = shape
    it = csum_in_store_item(L, shape)
    p, part = it["p"], it["part"]
    with macro(L):
        names = run256(L, GX.DW, [it], "csum_in " + what_of(p))
    assert names == ["gemm_bf16_256_kernel<2, 5>"], names
    csum_in_store_verify(it)
    # csum_ld != N
    b2, e2 = dw_setup(L, p)
    pw = Buf(rows, N, "f32", part)
    with macro(L):
        names, rc = GF.kernels_launched(L, lambda: call256(L, GX.DW, [item(p, b2, e2, csum_in=pw.ptr, csum_ld=pw.ld, csum_rows=rows)]))
    refused(L, rc, EINVAL, "column-sum partials must be [rows][N]")
    assert names == [] and untouched(b2["out"]) and untouched(b2["out2"])


def test_csum_in_store_merged(hip):
    """two such problems in ONE call: a merged grid of the STORE_F32 instantiation, the bias-gradient workgroups of both behind all
    tiles (Multi256's extra[] with more than one entry, bias_seg_block<STORE_F32>)"""
    L = hip
    items = [csum_in_store_item(L, GX.CSUM_IN_CASES[i]) for i in GX.CSUM_IN_MERGED]
    with macro(L):
        names = run256(L, GX.DW, items, "csum_in merged %s" % (GX.CSUM_IN_MERGED,))
    assert names == ["gemm_bf16_256_dw_multi_kernel<5>"], names
    for it in items:
        csum_in_store_verify(it)


def adam_items(L, lay, dev, parts):
    items, keep = [], []
    for i, q in enumerate(lay.probs):
        p, _, _ = AX.gradients(q)
        A, B = DA.Operand(p.A_mem), DA.Operand(p.B_mem)
        e = L.Epilogue()
        e.kind = AX.EPI_ADAM
        e.out, e.ldo = dev["grad"].data_ptr() + 4 * lay.w_off[i], lay.ldo[i]
        e.out2 = dev["grad"].data_ptr() + 4 * lay.b_off[i]
        pb = Buf(1, parts[i].size, "f32", parts[i].reshape(1, -1))
        keep.append(pb)
        items.append(item(p, {"A": A, "B": B}, e, csum_in=pb.ptr, csum_ld=q.N, csum_rows=parts[i].shape[0]))
    return items, keep


@pytest.mark.parametrize("which", [(1,), (0, 1, 2)], ids=["one", "merged"])
def test_csum_in_adam(hip, which):
    """DW + ADAM: the bias gradient the extra workgroups make of the partials goes through adam_quad; all five arenas, whole, against
    adam_exact's float32 oracle on (dW, the ascending sum of the partials) -- one problem, and three merged into one grid with their
    bias-gradient workgroups behind all tiles"""
    L = hip
    shapes = [GX.CSUM_IN_CASES[i] for i in which]
    lay = AX.Layout([AX.Prob(M, N, K, True) for (M, N, K, _) in shapes])
    init = AX.initial_state(lay, 17)
    dev, state = DA.upload(init), DA.state_blob(L)
    parts = [GX.csum_in_partials(*s) for s in shapes]
    items, keep = adam_items(L, lay, dev, parts)
    gscale = 0.5
    ctx = DA.context(L, lay, dev, state, AX.MODES["ieee"], 1, gscale)
    with macro(L):
        names = run256(L, GX.DW, items, "csum_in adam %s" % (which,), ctx)
    assert names == [AX.MULTI_ROW], names
    got = DA.download(dev)
    idx, g = [], []
    for i, q in enumerate(lay.probs):
        _, dW, _ = AX.gradients(q)
        db = np.zeros(q.N, dtype=F)
        for r in range(parts[i].shape[0]):
            db = db + parts[i][r].astype(F)
        idx += [lay.w_index(i).reshape(-1), lay.b_index(i)]
        g += [dW.reshape(-1), db]
    idx, g = np.concatenate(idx), np.concatenate(g)
    exp = {k: a.copy() for k, a in init.items()}
    pn, mn, vn = AX.adam_f32(init["param"][idx], init["m"][idx], init["v"][idx], g, gscale, AX.lr_t(AX.T_STEP))
    exp["param"][idx], exp["m"][idx], exp["v"][idx], exp["grad"][idx] = pn, mn, vn, g
    exp["shadow"][idx] = AX.bf16_bits(pn)
    for k in DA.ARENAS:
        e_, g_ = DA.bits(exp[k]), DA.bits(got[k])
        if k == "grad":                                 # an exact zero may carry either sign
            e_, g_ = np.where(e_ == 0x80000000, 0, e_), np.where(g_ == 0x80000000, 0, g_)
        bad = np.flatnonzero(e_ != g_)
        assert bad.size == 0, "csum_in adam %s: `%s` differs from the oracle in %d elements, first at arena offset %d" % (which, k, bad.size, bad[0])


def test_csum_chain_dx_to_dw(hip):
    """the column sums a dx_relu_mask launch leaves are the csum_in of the weight-gradient problem whose B operand is that launch's output:
    db is the float64 column sum of the bf16 output, exactly"""
    L = hip
    p, X, dY, dW, db = GX.chain_problem()
    tiles = p.M // 256
    b, e = GF.setup(L, "bf16", p)
    cs = Buf(1, tiles * p.N, "f32", fill="out")                     # [tiles][N], csum_ld = N: what the weight-gradient launch takes
    with macro(L):
        names = run256(L, GX.DX, [item(p, b, e, csum_out=cs.ptr, csum_ld=p.N)], "chain dx " + what_of(p))
    assert names == ["gemm_bf16_256_kernel<1, 3>"], names
    res = GF.collect(b, what_of(p))
    GF.verify(p, "bf16", res, 256, 256)
    out = values(res, "out")
    # the weight-gradient problem GX.CHAIN_DW = (256, 768, 1280) is no make() problem (tests/test_gemm_exact_host.py checks its sizes and
    # exactness apart, test_csum_in_partials_and_the_chain).  Its B operand IS the dx launch's output buffer: that is the chain, so its pad
    # columns hold the output sentinel 7.0, not NaN -- a read past column N would not poison this result; the NaN-padded B operands of
    # test_macro_pair_exact[*dw_store_db] and test_csum_in_store cover that
    w = {"A": Buf(p.M, GX.CHAIN_X, "bf16", X), "B": b["out"], "out": Buf(GX.CHAIN_X, p.N, "f32", fill="out"), "out2": Buf(1, p.N, "f32", fill="out")}
    ew = L.Epilogue()
    ew.kind = GX.EPI_STORE_F32
    ew.out, ew.ldo, ew.out2 = w["out"].ptr, w["out"].ld, w["out2"].ptr
    with macro(L):
        names = run256(L, GX.DW, [item(p, w, ew, shape=GX.CHAIN_DW, csum_in=cs.ptr, csum_ld=p.N, csum_rows=tiles)], "chain dw")
    assert names == ["gemm_bf16_256_kernel<2, 5>"], names
    rw = GF.collect(w, "chain dw")
    assert cs.read()[1]
    np.testing.assert_array_equal(values(rw, "out"), dW, err_msg="dW = X^T dY")
    np.testing.assert_array_equal(values(rw, "out2").reshape(p.N), out.sum(0), err_msg="db = column sum of the bf16 dY")
    np.testing.assert_array_equal(out.sum(0), db)


# ------------------------------------------------------------------------------------------------ K slices into slabs
GAP = 64                                                # elements between two slabs


class Sliced:
    """a DW + STORE_F32 problem whose K slices go to slabs slab_stride apart, inside one sentinel-filled buffer with room for one slab more"""

    def __init__(self, L, M, N, ks, nsl):
        self.p = p = GX.make("dw_store_db", M, N, ks * nsl)
        self.ks, self.nsl = ks, nsl
        self.b = {"A": Buf(p.A_mem.shape[0], p.A_mem.shape[1], "bf16", p.A_mem), "B": Buf(p.B_mem.shape[0], p.B_mem.shape[1], "bf16", p.B_mem)}
        self.ldo = N + GX.PAD["f32"]
        self.stride = M * self.ldo + GAP
        self.slab = Buf(1, (nsl + 1) * self.stride, "f32", fill="out")
        self.e = L.Epilogue()
        self.e.kind = GX.EPI_STORE_F32
        self.e.out, self.e.ldo = self.slab.ptr, self.ldo

    def item(self, **kw):
        if self.nsl == 1:
            return item(self.p, self.b, self.e, **kw)
        return item(self.p, self.b, self.e, **dict(dict(k_split=self.ks, slab_stride=self.stride), **kw))

    def verify(self):
        p = self.p
        bits, clean = self.slab.read()
        assert clean, "%s: written outside the slab buffer" % what_of(p)
        flat = bits.reshape(-1)
        vals = flat.view(torch.float32).double().numpy()
        free = np.ones(flat.numel(), dtype=bool)
        want = GX.slice_partials(p, self.ks, self.nsl)
        for y in range(self.nsl):
            idx = (y * self.stride + np.arange(p.M)[:, None] * self.ldo + np.arange(p.N)[None, :])
            np.testing.assert_array_equal(vals[idx], want[y], err_msg="%s: slab %d of %d (k_split %d)" % (what_of(p), y, self.nsl, self.ks))
            free[idx.reshape(-1)] = False
        assert bool((flat.numpy()[free] == self.slab.sent).all()), "%s: pad columns, a gap between slabs or the slab behind the last slice was written" % what_of(p)


@pytest.mark.parametrize("which", [(0,), (1,), (2,), (3,), GX.SLICE_MERGED], ids=lambda w: "-".join("%dx%dx%dx%d" % GX.SLICE_CASES[i] for i in w))
def test_k_slices_into_slabs(hip, which):
    """slices one, two and three K tiles deep, two or three of them: every slab is the exact partial product of its K range and nothing else
    is written; two sliced problems of different slice counts and an unsliced one merged into one grid"""
    L = hip
    probs = [Sliced(L, *GX.SLICE_CASES[i]) for i in which]
    for rep in range(3):
        if rep:
            probs = [Sliced(L, *GX.SLICE_CASES[i]) for i in which]
        with macro(L):
            names = run256(L, GX.DW, [s.item() for s in probs], "k slices %s" % (which,))
        assert names == ["gemm_bf16_256_dw_multi_kernel<5>"], names
        for s in probs:
            s.verify()


def test_k_slice_refusals_launch_nothing(hip):
    L = hip
    M, N, ks, nsl = GX.SLICE_CASES[0]
    # with the fused bias gradient
    s = Sliced(L, M, N, ks, nsl)
    o2 = Buf(1, N, "f32", fill="out")
    s.e.out2 = o2.ptr
    # without slab_stride
    t = Sliced(L, M, N, ks, nsl)
    # with the Adam epilogue
    lay = AX.Layout([AX.Prob(M, N, ks * nsl, False)])
    init = AX.initial_state(lay, 5)
    dev, state = DA.upload(init), DA.state_blob(L)
    ctx = DA.context(L, lay, dev, state, AX.MODES["ieee"], 1, 0.5)
    u = Sliced(L, M, N, ks, nsl)
    u.e.kind = AX.EPI_ADAM
    u.e.out, u.e.ldo = dev["grad"].data_ptr() + 4 * lay.w_off[0], lay.ldo[0]
    with macro(L):
        names, rcs = GF.kernels_launched(L, lambda: (call256(L, GX.DW, [s.item()]), call256(L, GX.DW, [t.item(slab_stride=0)]),
                                                     call256(L, GX.DW, [u.item()], ctx)))
    torch.cuda.synchronize()
    assert rcs == (EINVAL, EINVAL, EINVAL) and names == [], (rcs, names)
    assert untouched(s.slab) and untouched(o2) and untouched(t.slab) and untouched(u.slab)
    got = DA.download(dev)
    for k in DA.ARENAS:
        assert np.array_equal(DA.bits(got[k]), DA.bits(init[k])), "a refused call wrote to `%s`" % k


def test_entry_refuses_what_the_macro_tile_does_not_take(hip):
    L = hip
    with macro(L):
        p = GX.make("fwd_bias_f32", 256, 256, 64)
        b, e = GF.setup(L, "bf16", p)
        names, rc = GF.kernels_launched(L, lambda: call256(L, GX.FWD, [item(p, b, e)]))
        refused(L, rc, EUNSUPPORTED, "not instantiated")
        assert names == [] and untouched(b["out"])
        p = GX.make("fwd_store", 320, 192, 64)
        b, e = GF.setup(L, "bf16", p)
        refused(L, call256(L, GX.FWD, [item(p, b, e)]), EINVAL, "multiples of 256")
        assert untouched(b["out"])
        p = GX.make("fwd_store", 256, 256, 64)
        b, e = GF.setup(L, "bf16", p)
        refused(L, call256(L, GX.FWD, [item(p, b, e), item(p, b, e)]), EINVAL, "one problem")
        cs = Buf(1, 256, "f32", fill="out")
        refused(L, call256(L, GX.FWD, [item(p, b, e, csum_out=cs.ptr, csum_ld=cs.ld)]), EINVAL, "csum_out")
        refused(L, call256(L, GX.FWD, [item(p, b, e, k_split=128, slab_stride=1 << 20)]), EINVAL, "k_split")
        assert untouched(b["out"]) and untouched(cs)


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("knob6", [2, 0], ids=["macro", "small-tiles"])
@pytest.mark.parametrize("B", [256, 512])
def test_step_output_bias_gradient_is_the_column_sum_of_dxlogits(hip, B, knob6):
    """one forward_backward of the macro geometry: the reconstruction launch leaves dxlogits' column sums per 256-row tile (csrc/step.hip),
    the output layer's weight-gradient problem takes them as [B_pad / 256][padded input width] partials.  b_out's gradient is then an f32 sum of the B
    bf16 values of a column: B - 1 additions rounded to nearest, |error| <= (B - 1) x 2^-24 x sum |dxlogits| of the column.  The control
    (knob 6 = 0) gets the same sum from the ones-operand MFMA of the small tiles"""
    L = hip
    case = dict(B=B, dtype="bf16", kw=D.MACRO)
    what = "step B=%d knob6=%d" % (B, knob6)
    with macro(L, {6: knob6}):
        try:                                            # as launched(): after a launch that faults nothing more is sent to the device
            eng, X, perm = D.make_engine(case)
            eng.load_batch(X, perm, 0, B)
            torch.cuda.synchronize()
            names, _ = GF.kernels_launched(L, lambda: eng.forward_backward(B))
        except (L.DmvaeError, RuntimeError) as err:
            pytest.exit("%s: %s -- nothing more is launched" % (what, err), returncode=1)
    print("KERNEL step B=%d knob6=%d -> %s" % (B, knob6, names))
    if knob6 == 2:
        assert "gemm_bf16_256_kernel<0, 2>" in names and "colsum_slabs" not in names, names
        assert [n for n in names if n.startswith("gemm_bf16_256_dw_multi_kernel") or n == "gemm_bf16_256_kernel<2, 5>"], names
    else:
        assert not [n for n in names if "gemm_bf16_256" in n], names
    dl = eng.view("dxlogits")
    assert dl.dtype == torch.bfloat16 and tuple(dl.shape) == (B, D.MACRO["input_dim"])
    dl = dl.double().cpu().numpy()
    db = eng.grad_view("b_out").double().cpu().numpy()
    want, bound = dl.sum(0), (B - 1) * 2.0 ** -24 * np.abs(dl).sum(0)
    err = np.abs(db - want)
    print("STEP B=%d knob6=%d: max |db - colsum| = %.3g, max bound %.3g, max |error| / bound = %.3g" % (
        B, knob6, float(err.max()), float(bound.max()), float((err / np.maximum(bound, 1e-300)).max())))
    assert np.abs(want).max() > 0 and (bound > 0).all()
    assert (err <= bound).all(), "b_out's gradient is not the column sum of dxlogits in %d of %d columns" % (int((err > bound).sum()), err.size)
