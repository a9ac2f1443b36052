"""CPU checks of tests/helpers/finalize_oracle.py, the float32 model of step_finalize_block that tests/test_gpu_step_finalize.py holds
the five kernels to: it sums what float64 sums, its exact roundings are exact, and the test inputs tell its order of additions from a
descending one, from a pairwise np.sum and from a swapped pairing of the wave sums -- were they unable to, the bit-exact GPU tests would
accept those orders too."""
import fractions
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import adam_exact as AX            # noqa: E402
import finalize_oracle as FO       # noqa: E402
import gemm_exact as GX            # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _expected(case, order="model", adam_t=7, wrap=True, bump=1):
    inp = FO.inputs(case)
    return inp, FO.finalize(inp.rp, inp.lp, inp.inv_B, FO.initial_state(adam_t, wrap), bump, inp.part, order)


@pytest.mark.parametrize("case", FO.CASES, ids=FO.case_id)
def test_oracle_matches_float64_within_the_float32_bound(case):
    """a sum of n float32 terms in any order is within (n - 1) u sum|x| of the exact sum (u = 2^-24), the multiply by inv_B adds one more u"""
    nr, nl, nblk, ncol = case
    inp, exp = _expected(case)
    u = 2.0 ** -24
    for got, x, n in ((exp.exact["last_recon"], inp.rp, nr), (exp.exact["last_klz"], inp.lp[0::2], nl), (exp.exact["last_klc"], inp.lp[1::2], nl)):
        x = x.astype(np.float64)
        want = x.sum() * float(inp.inv_B)
        assert abs(float(got) - want) <= (n + 1) * u * np.abs(x).sum() * float(inp.inv_B) + 2.0 ** -149, (case, got, want)
        assert got > 0
    p = inp.part.astype(np.float64)
    bound = nblk * u * np.abs(p).sum(axis=0) + 2.0 ** -149
    assert (np.abs(exp.gout.astype(np.float64) - p.sum(axis=0)) <= bound).all(), case
    assert exp.gout.dtype == F and exp.gout.shape == (ncol,)


@pytest.mark.parametrize("case", FO.CASES, ids=FO.case_id)
def test_inputs_tell_the_modelled_order_from_a_wrong_one(case):
    """wherever an order CAN differ from the model's (FO.distinguishable: three values in a chain, three waves with values), at least one
    output differs in its bits on the test inputs -- where it cannot, none does -- and so do the two roundings of a multiply-add"""
    bad = [what for what, ok in FO.discriminates(case).items() if not ok]
    assert not bad, (case, bad)
    assert tuple(case) in FO.SEEDS


def test_every_wrong_order_is_told_apart_in_several_cases():
    for order in FO.ORDERS[1:]:
        assert sum(FO.distinguishable(c, order) for c in FO.CASES) >= 3, order
    # ... and the prior-table sums alone, which most of the workgroups compute, tell the two orders that reach them
    for order in ("descending", "pairwise"):
        n = 0
        for c in FO.CASES:
            inp = FO.inputs(c)
            n += int(not np.array_equal(FO.column_sums(inp.part).view(np.uint32), FO.column_sums(inp.part, order).view(np.uint32)))
        assert n >= 3, order


def test_round_f32_rounds_once_to_nearest_even():
    Fr = fractions.Fraction
    one, ulp = Fr(1), Fr(2) ** -23
    assert FO.round_f32(one + ulp / 2) == F(1.0)                                  # tie: to the even neighbour
    assert FO.round_f32(one + 3 * ulp / 2) == F(1.0) + F(2.0 ** -22)
    assert FO.round_f32(one + ulp / 2 + Fr(2) ** -80) == F(1.0) + F(2.0 ** -23)   # just above the tie: float64 would round it to the tie first
    assert np.float32(float(one + ulp / 2 + Fr(2) ** -80)) == F(1.0)              # (the double rounding this function avoids)
    assert FO.round_f32(-(one + ulp / 2 + Fr(2) ** -80)) == -(F(1.0) + F(2.0 ** -23))
    assert FO.round_f32(Fr(2) ** -149 * 3 / 2) == F(2.0 ** -148) and FO.round_f32(Fr(2) ** -150) == F(0.0) and FO.round_f32(0) == F(0.0)
    rng = np.random.RandomState(3)
    for x in rng.randn(2000) * 10 ** rng.uniform(-30, 30, size=2000):
        assert FO.round_f32(Fr(float(x))) == F(x)                                 # one rounding of a double: what NumPy does
    a, b, c = F(0.37), F(3.1415927), F(-1.1624893)
    ma = FO.mul_add(a, b, c)
    assert ma[FO.OFF] == F(F(a * b) + c) and ma[FO.ON] == F(np.float64(a) * np.float64(b) + np.float64(c))      # (a * b is exact in double, the sum here too)


@pytest.mark.parametrize("case", FO.CASES, ids=FO.case_id)
def test_one_rounding_per_operator_and_the_contracted_forms(case):
    """the accepted values restate block 0 one float32 operation per operator (the kernel compiles it under contract(off)); the contracted
    forms are single roundings of the exact expression, neighbours of the accepted value, and the form hipcc compiled before the pragma
    differs from it on these inputs"""
    assert FO.ACCEPT == (FO.OFF,)
    inp, exp = _expected(case)
    st = FO.initial_state(7, True)
    rs, zs, cs = FO.block_sums(inp.rp, inp.lp)
    recon, klz, klc = F(rs * inp.inv_B), F(zs * inp.inv_B), F(cs * inp.inv_B)
    e = exp.exact
    assert (FO.bits(e["last_recon"]), FO.bits(e["last_klz"]), FO.bits(e["last_klc"])) == (FO.bits(recon), FO.bits(klz), FO.bits(klc))
    assert FO.bits(e["last_loss"]) == FO.bits(F(recon + F(st.kl_ratio * F(klc + klz))))
    for name, x in (("epoch_loss", e["last_loss"]), ("epoch_recon", recon), ("epoch_klz", klz), ("epoch_klc", klc)):
        assert FO.bits(e[name]) == FO.bits(F(getattr(st, name) + F(x * st.epoch_weight))), name
        assert abs(FO.bits(exp.contracted[name]) - FO.bits(e[name])) <= 1, name
    pats = exp.contracted["last_loss"]
    assert len(pats) == 9 and FO.bits(pats[("off", "off")]) == FO.bits(e["last_loss"])
    d = np.float64
    t = F(d(cs) * d(inp.inv_B) + d(klz))                 # (a product of two float32 is exact in double; these sums round once more: checked against Fraction below)
    shipped = pats[FO.SHIPPED_BEFORE]
    Fr = fractions.Fraction
    t_exact = FO.round_f32(Fr(float(cs)) * Fr(float(inp.inv_B)) + Fr(float(klz)))
    assert FO.bits(shipped) == FO.bits(FO.round_f32(Fr(float(rs)) * Fr(float(inp.inv_B)) + Fr(float(F(st.kl_ratio * t_exact)))))
    assert abs(FO.bits(t) - FO.bits(t_exact)) <= 1
    assert FO.bits(shipped) != FO.bits(e["last_loss"]) and all(abs(FO.bits(v) - FO.bits(e["last_loss"])) <= 2 for v in pats.values())
    assert "klc" in FO.diagnose(exp, "last_loss", shipped) and "no contraction" in FO.diagnose(exp, "last_loss", F(0.0))
    fused = [k for k in FO.EPOCH_FIELDS if FO.bits(exp.contracted[k]) != FO.bits(e[k])]
    assert fused and FO.diagnose(exp, fused[0], exp.contracted[fused[0]]) == "the fused multiply-add"


@pytest.mark.parametrize("t", FO.ADAM_TS)
def test_lr_t_rounds_the_same_on_host_and_device(t):
    """the rule of test_adam_exact_host.py: only t whose lr_t sits away from a float32 rounding boundary are used (the update's t = adam_t + 1)"""
    assert AX.lr_t_margin(t + 1) > 1e-6, (t, AX.lr_t_margin(t + 1))


def test_state_transitions():
    inp = FO.inputs(FO.CASES[2])
    for adam_t in FO.ADAM_TS:
        for wrap in (True, False):
            for bump in (0, 1):
                st = FO.initial_state(adam_t, wrap)
                e = FO.finalize(inp.rp, inp.lp, inp.inv_B, st, bump, inp.part).exact
                assert e["noise_step"] == 42 and e["batch_cursor"] == 0 and e["batches_per_epoch"] == (13 if wrap else 0)
                assert e["adam_t"] == adam_t + bump
                assert FO.bits(e["lr_t"]) == FO.bits(AX.lr_t(adam_t + 1) if bump else FO.LR_T_SENT)
    st = FO.initial_state(0, True)._replace(batch_cursor=3)
    assert FO.finalize(inp.rp, inp.lp, inp.inv_B, st, 1, inp.part).exact["batch_cursor"] == 4


def test_model_follows_the_kernel_source():
    """the lines of csrc/common.h the model restates are still there, block 0's under contract(off)"""
    src = open(os.path.join(ROOT, "deep-mixture-vae_amd", "csrc", "common.h")).read()
    body = src[src.index("void step_finalize_block("):src.index("template <int NW>\n__device__ __forceinline__ float block_sum_waves")]
    for line in ("for (int i = threadIdx.x; i < f.nr; i += 256) a += f.rp[i];", "r = (red[0] + red[1]) + (red[2] + red[3]);",
                 "for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);", "for (int r = rg; r < f.nblk; r += 16) s += f.part[(int64_t)r * f.ncol + col];",
                 "for (int g = 0; g < 16; ++g) t += red[g][threadIdx.x];"):
        assert line in src, line
    for line in ("const float loss = recon + st->kl_ratio * (klc + klz);", "st->epoch_loss += loss * st->epoch_weight;", "* f.inv_B;"):
        assert line in body, line
    head = body[body.index("if (blk == 0) {"):body.index("float a = 0.f, z = 0.f, c = 0.f;")]
    assert "#pragma clang fp contract(off)" in head, "block 0 of step_finalize_block is compiled without FMA contraction"
    assert FO.CASES == ((1, 1, 1, 1), (3, 5, 1, 20), (255, 256, 16, 16), (256, 257, 17, 17), (300, 700, 37, 200), (1024, 512, 256, 1280), (1024, 512, 512, 1280))


@pytest.mark.parametrize("key", FO.gemm_problem_keys(), ids=lambda k: "%s-%dx%dx%d" % k)
def test_carrier_products_are_exact(key):
    """the GEMMs the riders ride in are held to the exact integer product of gemm_exact.py: its conditions hold at these shapes"""
    bad = [what for what, ok in GX.exactness_report(GX.make(*key)).items() if not ok]
    assert not bad, (key, bad)


def test_rider_tables():
    cs = FO.carriers()
    assert [c.id for c in cs][:3] == ["dz-64rows", "dz-32rows", "dz-16rows"] and len(cs) == 3 + len(GX.FORMS)
    assert [c.carries_fin for c in cs] == [True, True, False] + [True] * len(GX.FORMS)
    for c in cs:
        assert c.M % 64 == 0 and c.N % 64 == 0 and c.K % 64 == 0 and c.K > 64          # what dmvae_gemm takes; more than one K tile
        assert (c.M // c.bm) >= 3 and (c.pair == "dx_latent" or (c.M // c.bm, c.N // c.bn) == (3, 2))
        assert (c.M // c.bm) * (c.N // c.bn) + 16 + 24 <= 512                            # room for the largest rider set as second workgroups
    assert 1 + -(-FO.FIN_14[3] // 16) == 14 and 1 + -(-FO.FIN_2[3] // 16) == 2 and FO.FIN_14 in FO.CASES and FO.FIN_2 in FO.CASES
    assert all(g is None or g[0] % 8 == 0 for _, _, g in FO.RIDER_SETS)
    assert not any(f and g and g[2] for _, f, g in FO.RIDER_SETS)                        # finalize never with a gather addressed through the cursor
    st = FO.initial_state(7, True)
    assert st.batch_cursor * FO.GATHER_CURSOR_BATCH + FO.GATHER_NVALID > FO.GATHER_N > st.batch_cursor * FO.GATHER_CURSOR_BATCH
    assert FO.GATHER_FIRST + FO.GATHER_NVALID > FO.GATHER_N > FO.GATHER_FIRST and FO.GATHER_DIMS[0] % 4 == 0 and FO.GATHER_DIMS[1] % 4 != 0
    rng = np.random.RandomState(0)
    data, perm = rng.rand(5, 3).astype(F), np.array([4, 0, 9, -1, 2], dtype=np.int32)
    e = FO.gather_expected(data, perm, 1, 6, 8, 4)
    assert np.array_equal(e[0, :3], data[0]) and not e[1].any() and not e[2].any() and np.array_equal(e[3, :3], data[2]) and not e[4:].any() and not e[:, 3].any()
    ids = [g[0] for g in FO.grouped_cases()]
    assert len(ids) == len(set(ids)) == 10 and {tuple(s[2] for s in g[2]) for g in FO.grouped_cases()} == {(64,), (128, 128), (256,), (512, 64)}
