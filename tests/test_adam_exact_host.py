"""CPU checks of tests/helpers/adam_exact.py, the oracle of tests/test_gpu_dw_adam_forms.py: the float32 restatement of adam_elem agrees
with the float64 oracle, the gradients of every (shape, K) of the case table are exact, the initial state discriminates -- an m, v or
param quad loaded from a neighbouring quad, row or 16-column block changes almost every result --, and the case table is the one the
GPU file runs."""
import os
import re
import sys

import numpy as np
import pytest

import dmvae_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import gemm_exact as GX      # noqa: E402
import adam_exact as AX      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_float32_oracle_agrees_with_the_float64_oracle_over_steps():
    """the data of tests/test_gpu_kernels.py::test_adam_tf_matches_oracle_over_steps, its tolerances"""
    rng = np.random.RandomState(4)
    n = 4096 + 64
    p = {"a": rng.randn(n).astype(F).astype(np.float64)}
    m, v = O.adam_tf_init(p)
    p32, m32, v32 = p["a"].astype(F), np.zeros(n, F), np.zeros(n, F)
    for t in range(1, 6):
        g = (rng.randn(n) * 10 ** rng.uniform(-4, 1)).astype(F).astype(np.float64)
        O.adam_tf(p, {"a": g}, m, v, t, lr=0.002)
        p32, m32, v32 = AX.adam_f32(p32, m32, v32, (g * 2.0).astype(F), 0.5, AX.lr_t(t))
        np.testing.assert_allclose(p32, p["a"], rtol=3e-6, atol=3e-7)
        np.testing.assert_allclose(m32, m["a"], rtol=1e-5, atol=2e-7)
        np.testing.assert_allclose(v32, v["a"], rtol=3e-5, atol=1e-12)


def test_float32_oracle_agrees_with_the_float64_oracle_on_the_test_state():
    """one step from the initial state of the GPU cases (nonzero m and v, integer gradients, t = 3)"""
    lay = AX.Layout(AX.G128x64)
    init = AX.initial_state(lay, 1)
    for gscale in (0.5, 1.0):
        exp, idx, g = AX.expected_arenas(lay, init, gscale, AX.lr_t(AX.T_STEP), True, 1)
        p = {"a": init["param"][idx].astype(np.float64)}
        m, v = {"a": init["m"][idx].astype(np.float64)}, {"a": init["v"][idx].astype(np.float64)}
        O.adam_tf(p, {"a": g.astype(np.float64) * gscale}, m, v, AX.T_STEP, lr=0.002)
        np.testing.assert_allclose(exp["param"][idx], p["a"], rtol=3e-6, atol=3e-7)
        np.testing.assert_allclose(exp["m"][idx], m["a"], rtol=1e-5, atol=2e-7)
        np.testing.assert_allclose(exp["v"][idx], v["a"], rtol=3e-5, atol=1e-12)
        np.testing.assert_array_equal(exp["shadow"][idx], AX.bf16_bits(exp["param"][idx]))
        np.testing.assert_array_equal(exp["grad"][idx], g)


def test_oracle_lines_are_single_float32_operations():
    """no float64 sneaks in (a product kept in double and rounded once would be a fused multiply-add), and the constants are the kernel's:
    1 - beta formed in float32"""
    rng = np.random.RandomState(0)
    p, m, v, g = (rng.randn(4096).astype(F) for _ in range(4))
    v = np.abs(v)
    pn, mn, vn = AX.adam_f32(p, m, v, g, 0.5, AX.lr_t(3))
    gj = g * F(0.5)
    assert np.array_equal(mn, AX.B1 * m + (F(1) - AX.B1) * gj)
    assert np.array_equal(vn, AX.B2 * v + ((F(1) - AX.B2) * gj) * gj)
    assert np.array_equal(pn, p - (AX.lr_t(3) * mn) / (np.sqrt(vn) + AX.EPS))
    fused = (AX.B1.astype(np.float64) * m + (1.0 - AX.B1.astype(np.float64)) * gj).astype(F)      # what one rounding would give
    assert (fused != mn).any()
    assert float(F(1) - AX.B1) != 1.0 - 0.9 and F(1) - AX.B2 == F(1.0 - float(AX.B2))


@pytest.mark.parametrize("t", [1, 2, 3, 4, 5])
def test_lr_t_rounds_the_same_on_host_and_device(t):
    """adam_lr_t evaluates one double expression and rounds it to float32; host and device pow / sqrt differ by a few double ulps at
    most (~1e-16 relative = 2e-9 float32 ulps), which changes the float32 only when the double sits that close to a rounding boundary"""
    assert AX.lr_t_margin(t) > 1e-6, (t, AX.lr_t_margin(t))
    assert AX.T_STEP >= 3


@pytest.mark.parametrize("q", AX.all_probs(), ids=lambda q: "%dx%dx%d" % (q.M, q.N, q.K))
def test_gradients_are_exact(q):
    p, dW, db = AX.gradients(q)
    bad = [what for what, ok in GX.exactness_report(p).items() if not ok]
    assert not bad, (q, bad)
    assert p.pair.layout == GX.DW and p.A_mem.shape == (q.K, q.M) and p.B_mem.shape == (q.K, q.N)
    for g in (dW, db):                                  # integers below 2^24, and halves of them: g * grad_scale is exact
        assert np.array_equal(g, np.rint(g)) and np.abs(g).max() < 2 ** 24 and np.array_equal((g * F(0.5)).astype(np.float64), g.astype(np.float64) / 2)
    assert np.array_equal(dW.astype(np.float64), p.A @ p.B) and np.array_equal(db.astype(np.float64), p.B.sum(0))
    assert (dW != 0).mean() > 0.9                       # (a gradient of zeros would leave m and v nearly as they were)


def _changed(a, b, idx):
    return (a["param"][idx] != b["param"][idx]) | (a["m"][idx] != b["m"][idx]) | (a["v"][idx] != b["v"][idx])


@pytest.mark.parametrize("group", ["G64", "G128x64", "G128x128", "M_MIXED"])
def test_initial_state_discriminates(group):
    """m, then v, then param taken from one quad, one row (ldo) and one 16-column block further: more than 99 % of the updated elements
    of every tensor get another result -- a misplaced load in some form cannot produce the expected bits by accident"""
    lay = AX.Layout(getattr(AX, group), seg_n=1024)
    init = AX.initial_state(lay, 7)
    lrt = AX.lr_t(AX.T_STEP)
    ref, idx, _ = AX.expected_arenas(lay, init, 0.5, lrt, True, 0)
    for which in ("m", "v", "param"):
        for i in range(len(lay.probs)):
            for shift in (4, lay.ldo[i], 16):
                moved = dict(init)
                moved[which] = np.roll(init[which], -shift)
                got, _, _ = AX.expected_arenas(lay, moved, 0.5, lrt, True, 0)
                for tidx in (lay.w_index(i), lay.b_index(i)):
                    if tidx is not None:
                        frac = _changed(ref, got, tidx).mean()
                        assert frac > 0.99, (group, which, i, shift, frac)
    moved = dict(init)
    moved["m"] = np.roll(init["m"], -4)
    got, _, _ = AX.expected_arenas(lay, moved, 0.5, lrt, True, 0)
    assert _changed(ref, got, lay.seg_index()).mean() > 0.99


def test_layout_has_pads_gaps_and_guards():
    lay = AX.Layout(AX.G64, seg_n=4100)
    owned = np.zeros(lay.n, dtype=int)
    for idx in lay.tensors() + [lay.seg_index()]:
        owned[idx.reshape(-1)] += 1
    assert owned.max() == 1 and not owned[:GX.GUARD].any() and not owned[-GX.GUARD:].any()
    for i, q in enumerate(lay.probs):
        assert lay.ldo[i] == q.N + AX.LDO_PAD and not owned[lay.w_off[i] + q.N:lay.w_off[i] + lay.ldo[i]].any()       # pad columns
        end = lay.w_off[i] + q.M * lay.ldo[i]
        assert not owned[end:end + AX.GAP].any()                                                                     # the gap behind
    assert lay.seg_off > max(lay.w_off) and lay.seg_off % 4 == 0
    assert AX.Layout(AX.G64, pad=0).ldo == [q.N for q in AX.G64]
    assert lay.n < 2 ** 30                              # the fused update's 32-bit element offsets (ADAM_QUADS_MAX_ELEMS)


def test_case_table_covers_the_forms():
    cases = AX.all_cases()
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids))
    small = [c for c in cases if c.knobs[6] == 0]
    forced = [c for c in small if c.knobs[2] in (0, 2) and not c.seg_n]
    tiles = {}
    for c in forced:
        kinds = {AX.tile_kind(q, c.knobs[2]) for q in c.probs}
        assert len(kinds) == 1, (c.id, kinds)           # each tile form alone in its launch
        tiles.setdefault(kinds.pop(), set()).add((c.mode, c.knobs.get(1)))
    assert set(tiles) == {(64, 64), (128, 64), (128, 128)}
    for bm in ((128, 64), (128, 128)):
        assert {(m, k) for m in AX.MODES for k in (0, 1)} <= tiles[bm]
    assert {m for m, _ in tiles[(64, 64)]} == set(AX.MODES)
    for c in small:
        assert all(q.M in (64, 128, 192, 256) and q.N in (64, 128, 192, 256) for q in c.probs)
        assert {q.K for q in c.probs} <= {64, 192, 320} and any(not q.bias for q in c.probs) and any(q.bias for q in c.probs)
    assert {q.K for c in small for q in c.probs} == {64, 192, 320}
    macro = [c for c in cases if c.knobs[6] == 2]
    assert {q.K for c in macro for q in c.probs if q.M % 256 == 0 and q.N % 256 == 0} == {128, 576}
    assert any(len(c.probs) == 1 and c.probs[0][:2] == (256, 256) for c in macro) and any(len(c.probs) == 1 and c.probs[0][:2] == (256, 512) and c.probs[0].bias for c in macro)
    assert any(c.rows == {AX.MULTI_ROW: 1} and len(c.probs) == 3 for c in macro)                          # three problems, one grid
    assert any(AX.GROUPED_ROW in c.rows and any(q[:2] == (192, 64) for q in c.probs) for c in macro)      # one problem stays grouped
    segs = [c for c in cases if c.seg_n]
    assert {c.seg_n for c in segs if c.rows == {AX.GROUPED_ROW: 1}} == set(AX.SEG_NS) == {4, 1024, 4100}
    assert {c.seg_n for c in segs if AX.ADAM_ROW in c.rows} == set(AX.SEG_NS)
    assert {c.store_grad for c in cases} == {0, 1} and {c.gscale for c in cases} == {0.5, 1.0} and {c.pad for c in cases} == {0, AX.LDO_PAD}
    assert sum(c.gscale == 0.5 for c in cases) > sum(c.gscale == 1.0 for c in cases) and sum(c.pad != 0 for c in cases) > sum(c.pad == 0 for c in cases)
    for mode in AX.MODES:
        assert {c.store_grad for c in cases if c.mode == mode} == {0, 1}


def test_gpu_file_runs_this_table_and_header_agrees():
    src = open(os.path.join(ROOT, "tests", "test_gpu_dw_adam_forms.py")).read()
    for table in ("AX.form_cases()", "AX.segment_cases()"):
        assert table in src, table
    assert not re.search(r"pytest\.mark\.(skip|xfail)|pytest\.(skip|xfail)\(", src)
    hdr = open(os.path.join(ROOT, "include", "dmvae_hip.h")).read()
    assert int(re.search(r"DMVAE_EPI_ADAM\s*=\s*(\d+)", hdr).group(1)) == AX.EPI_ADAM
    assert int(re.search(r"DMVAE_EINVAL\s*=\s*(-?\d+)", hdr).group(1)) == AX.EINVAL
    assert "test_gpu_dw_adam_forms.py" in open(os.path.join(ROOT, "include", "dmvae_hip_debug.h")).read()
    flags = open(os.path.join(ROOT, "deep-mixture-vae_amd", "build.py")).read()
    # nothing in the library's compile flags lets sqrtf or / be less than correctly rounded (the bit equalities rest on it)
    assert not re.search(r"fast-math|unsafe-fp|approx-func|no-hip-fp32-correctly-rounded|ffp-contract=fast|-Ofast|denormals", flags)
