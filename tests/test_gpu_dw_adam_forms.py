"""The fused weight-gradient + Adam epilogue (DMVAE_EPI_ADAM, dmvae_gemm_grouped_dw_adam) on every form, each forced alone and held to a
BIT-EXACT oracle.

Every bf16 training step ends in this call: it writes the model.  Its epilogue exists once per tile -- the 64 x 64, 128 x 64 and
128 x 128 bodies of gemm_bf16_grouped_kernel<DW, ADAM> (each with its own adam_pipelined unrolling and 32-bit offset arithmetic over the
un-swizzled parked tile, and an adam_quad for the bias gradient), the 256 x 256 macro tile (csrc/gemm_bf16_256.hip: adam_pipelined per
wave, the bias gradient from slab column sums in extra workgroups, one problem or several merged into one grid) -- plus the extra arena
segment (the lead workgroups of the grouped grid, or the stand-alone kernel when nothing stays grouped).  Here knobs 2 and 6 force each,
the profiler rows say which kernel families ran and how often, and tests/helpers/adam_exact.py supplies inputs for which the expected
result is exact: integer gradients and a float32 restatement of adam_elem (tests/test_adam_exact_host.py checks the conditions on the
CPU, and that the nonzero, all-different m / v / param make a load from a neighbouring quad, row or column block change the result).

All five arenas (param, grad, m, v, bf16 shadow) share one layout with guard bands, pad columns (ldo = N + 32) and gaps, and are compared
WHOLE, as bit patterns: the tensors with the oracle, everything else with what was there before the launch.  Comparisons are equalities
of bits in every mode; the production mode (hardware square root and reciprocal) is held to the bits of the stand-alone kernel
dmvae_adam_tf on the exact gradient and the same state, and that to float64 within the tolerances of
tests/test_gpu_kernels.py::test_adam_tf_matches_oracle_over_steps.

(Knob 1 -- eight waves for the 128-row tiles -- is set to 0 and to 1 for the 128-row groups; it selects among the dense launches'
instantiations only: the grouped kernel has one form, four waves, whatever it says.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dmvae_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import gemm_exact as GX      # noqa: E402
import adam_exact as AX      # noqa: E402
from adam_harness import (ARENAS, F, NOT_HOST_T, bits, context, download, forced, launched, problems, profiled, state_blob, stream,      # noqa: E402,F401
                          upload)


@pytest.fixture(scope="module")
def hip():
    import dmvae_hip      # noqa: F401
    from dmvae_hip import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    assert _lib.EPI_ADAM == AX.EPI_ADAM and _lib.GEMM_DW == GX.DW
    return _lib


def run_case(L, case, with_segment=True):
    """the launch of one case on fresh arenas: (layout, initial arenas, arenas after the launch, profiler rows).  with_segment = False:
    the same arenas, the segment's elements in their place, but the launch is told of no segment (ctx.seg_n = 0)"""
    mode = AX.MODES[case.mode]
    lay = AX.Layout(case.probs, pad=case.pad, seg_n=case.seg_n)
    init = AX.initial_state(lay, 11)
    dev, state = upload(init), state_blob(L)
    probs, keep = problems(L, lay, dev)
    ctx = context(L, lay, dev, state, mode, case.store_grad, case.gscale)
    if not with_segment:
        ctx.seg_n = 0
    call = lambda: launched(L, L.lib.dmvae_gemm_grouped_dw_adam(stream(), probs, len(lay.probs), C.byref(ctx)), "dmvae_gemm_grouped_dw_adam %s" % case.id)
    with forced(L, case.knobs):
        rows, _ = profiled(L, call)
    return lay, init, download(dev), rows


def standalone_update(L, gscale):
    """the yardstick of the production mode: dmvae_adam_tf (bf16 mode: the same hardware square root and reciprocal) on the compacted
    elements with their exact gradient and the same state blob; itself held to float64 at the project's tolerances"""
    def update(p, m, v, g):
        n = len(p)
        assert n % 4 == 0
        d = [torch.as_tensor(np.ascontiguousarray(a, dtype=F)).cuda() for a in (p, g, m, v)]
        sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        launched(L, L.lib.dmvae_adam_tf(stream(), n, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(sh), 0.0, float(AX.B1), float(AX.B2),
                                        float(AX.EPS), gscale, 0, NOT_HOST_T, L.ptr(state_blob(L))), "dmvae_adam_tf")
        pn, mn, vn = (d[i].cpu().numpy() for i in (0, 2, 3))
        ref = ({"a": p.astype(np.float64)}, {"a": m.astype(np.float64)}, {"a": v.astype(np.float64)})
        O.adam_tf(ref[0], {"a": g.astype(np.float64) * gscale}, ref[1], ref[2], AX.T_STEP, lr=0.002)
        np.testing.assert_allclose(pn, ref[0]["a"], rtol=3e-6, atol=3e-7)
        np.testing.assert_allclose(mn, ref[1]["a"], rtol=1e-5, atol=2e-7)
        np.testing.assert_allclose(vn, ref[2]["a"], rtol=3e-5, atol=1e-12)
        np.testing.assert_array_equal(sh.cpu().view(torch.int16).numpy().view(np.uint16), AX.bf16_bits(pn))
        return pn, mn, vn
    return update


def verify(L, case, lay, init, got):
    """all five arenas, whole, as bit patterns"""
    mode = AX.MODES[case.mode]
    update = standalone_update(L, case.gscale) if case.mode == "fast" else None
    exp, idx, _ = AX.expected_arenas(lay, init, case.gscale, AX.lr_t(AX.T_STEP), mode["shadow"], case.store_grad, update)
    touched = np.zeros(lay.n, dtype=bool)
    touched[idx] = True
    for k in ARENAS:
        e, g = bits(exp[k]), bits(got[k])
        if k == "grad":                                 # an exact zero may carry either sign
            e, g = np.where(e == 0x80000000, 0, e), np.where(g == 0x80000000, 0, g)
        bad = e != g
        print("CHECK %s %s: %d of %d updated elements differ, %d of %d others were written" % (
            case.id, k, int(bad[touched].sum()), int(touched.sum()), int(bad[~touched].sum()), int((~touched).sum())))
        assert not bad[~touched].any(), "%s: `%s` was written outside the tensors (pad columns / gaps / guards / an arena this mode does not write): %d elements, first at %d" % (
            case.id, k, int(bad[~touched].sum()), int(np.flatnonzero(bad & ~touched)[0]))
        assert not bad[touched].any(), "%s: `%s` differs from the oracle in %d of %d elements, first at arena offset %d" % (
            case.id, k, int(bad[touched].sum()), int(touched.sum()), int(np.flatnonzero(bad & touched)[0]))
    return exp


# ------------------------------------------------------------------------------------------------ every form alone
@pytest.mark.parametrize("case", AX.form_cases(), ids=lambda c: c.id)
def test_form_exact(hip, case):
    """one group on one forced form in one mode: the kernel families the form names ran, that often, and every arena has the expected bits"""
    L = hip
    lay, init, got, rows = run_case(L, case)
    print("KERNEL %s -> %s" % (case.id, sorted(rows.items())))
    assert rows == case.rows, (case.id, rows)
    verify(L, case, lay, init, got)


# ------------------------------------------------------------------------------------------------ the extra arena segment
@pytest.mark.parametrize("case", AX.segment_cases(), ids=lambda c: c.id)
def test_segment_exact_and_tiles_unmoved(hip, case):
    """seg_n = 4 / 1024 / 4100 behind the tensors, riding a grouped launch (lead workgroups in the first ids, the tiles' ids shifted by
    g.lead) or with every problem peeled to the macro tile (the stand-alone kernel takes it): the segment has the oracle's bits, and the
    tensors the bits they get without a segment"""
    L = hip
    lay, init, got, rows = run_case(L, case)
    print("KERNEL %s -> %s" % (case.id, sorted(rows.items())))
    assert rows == case.rows, (case.id, rows)
    verify(L, case, lay, init, got)
    _, init0, got0, rows0 = run_case(L, case, with_segment=False)
    assert AX.ADAM_ROW not in rows0 and {k: v for k, v in rows.items() if k != AX.ADAM_ROW} == rows0
    seg = lay.seg_index()
    for k in ARENAS:
        assert np.array_equal(bits(init[k]), bits(init0[k]))
        same = bits(got[k]) == bits(got0[k])
        same[seg] = True
        assert same.all(), "%s: `%s` differs outside the segment with and without it: %d elements" % (case.id, k, int((~same).sum()))
        assert np.array_equal(bits(got0[k][seg]), bits(init[k][seg])), "%s: the launch without a segment wrote `%s` there" % (case.id, k)
    for k in ("param", "m", "v"):
        assert (bits(got[k][seg]) != bits(init[k][seg])).mean() > 0.99      # (with it, it was updated at all)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(hip):
    """every bad argument is DMVAE_EINVAL before anything is launched: the arenas keep their bits"""
    L = hip
    lay = AX.Layout(AX.G64, seg_n=8)
    init = AX.initial_state(lay, 3)
    dev, state = upload(init), state_blob(L)
    mode = AX.MODES["ieee"]

    def call(probs, n, ctx):
        return L.lib.dmvae_gemm_grouped_dw_adam(stream(), probs, n, C.byref(ctx))

    good, keep = problems(L, lay, dev)
    ctx = context(L, lay, dev, state, mode, 1, 0.5)
    many = (L.GemmProblem * 17)(*([good[i] for i in range(4)] * 4 + [good[0]]))
    refused = {}
    with forced(L, {6: 0, 2: 0}):
        store, keep2 = problems(L, lay, dev, kind=GX.EPI_STORE_F32)
        refused["a problem of kind STORE_F32"] = call(store, 4, ctx)
        one, keep3 = problems(L, lay, dev)
        one[2].epi.kind = GX.EPI_ATOMIC_F32
        refused["one problem of kind ATOMIC_F32 among ADAM"] = call(one, 4, ctx)
        noout, keep4 = problems(L, lay, dev)
        noout[1].epi.out = None
        refused["out = NULL"] = call(noout, 4, ctx)
        c = context(L, lay, dev, state, mode, 1, 0.5)
        c.state = None
        refused["state = NULL"] = call(good, 4, c)
        c = context(L, lay, dev, state, mode, 1, 0.5)
        c.seg_off = lay.seg_off + 2
        refused["seg_off % 4 != 0"] = call(good, 4, c)
        c = context(L, lay, dev, state, mode, 1, 0.5)
        c.seg_n = 6
        refused["seg_n % 4 != 0"] = call(good, 4, c)
        refused["n = 0"] = call(good, 0, ctx)
        refused["n = 17"] = call(many, 17, ctx)
    torch.cuda.synchronize()
    assert refused == {k: AX.EINVAL for k in refused}, refused
    got = download(dev)
    for k in ARENAS:
        assert np.array_equal(bits(got[k]), bits(init[k])), "a refused call wrote to `%s`" % k
