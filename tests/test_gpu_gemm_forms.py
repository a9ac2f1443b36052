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
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import gemm_exact as GX      # noqa: E402
from gemm_harness import bf16_name, forced, kernels_launched, run, run_grouped, verify, verify_inexact      # noqa: E402


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
