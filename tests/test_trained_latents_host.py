"""CPU tests of what tests/test_gpu_trained_latents.py stands on (tests/helpers/trained_latents.py): for every (form, shape, kind) the GPU
tests run, that the two restatements of the latent stage are restatements of the oracle (in float64), that the inputs are in the regime
they claim (one-hot q and gamma, a few rows decided by a few nats, gradient through gamma, vanished probabilities), that the float32
yardsticks are finite, that the tolerance rule is not vacuous (2 max |yard - oracle| < 1 % of max |oracle| for every output), that rows
with a clear arg-max are at least 95 % of each VaDE case, and that the rule sees four corruptions of the kernels' algebra.

The large-table form of VaDE (csrc/latent_vade_mfma.hip) meets these conditions on kind "floor" only because it takes mean, z and the prior
means from a common origin before it expands the squares (vade_origin_kernel; expanded() restates it).  Expanded from zero, a row on
the collapsed cluster has z^2 ip, -2 z pm ip and pm^2 ip of about 1e6 each per dimension, their sum over D = 256 is 2.5e8 where one float32
ulp is 16, and the float32 scores were off by 18, 56 and 65 nats at the three shapes (gamma by 0.06, 0.16, 0.04; 75 % clear rows)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import trained_latents as TL    # noqa: E402
import vade_large as V          # noqa: E402

IDS = [TL.case_id(*c) for c in TL.CASES]
EXPANDED = [c for c in TL.CASES if TL.FORMS[c[0]][1] == "expanded"]
VADE = [c for c in TL.CASES if TL.FORMS[c[0]][0] == "vade"]


def parts(case):
    form, shape, kind, tau = case
    mode, which = TL.FORMS[form][:2]
    return form, shape, kind, tau, mode, which, TL.get_case(shape, kind), TL.get_oracle(shape, kind, mode, tau), TL.get_yard(shape, kind, mode, which, tau)


def test_every_form_gets_its_kinds_and_the_exclusions_stay_within_their_cap():
    for form, (mode, _, shapes, kinds, _) in TL.FORMS.items():
        assert set(kinds) >= {"separated", "competing", "floor"}
        assert ("vanishing" in kinds) == (mode != "vade")
    assert len(TL.EXCLUDED) <= 3
    assert all(e[3] not in ("w", "klz") and e[3] in TL.OUTPUTS for e in TL.EXCLUDED)
    assert all((e[0], e[1], e[2]) in {c[:3] for c in TL.CASES} for e in TL.EXCLUDED)


@pytest.mark.parametrize("case", TL.CASES, ids=IDS)
def test_restatements_are_the_oracle_in_float64(case):
    """expanded_f64 == direct_f64 == O.latent_backward / O.vade_latent_backward to 1e-9 of each output's maximum"""
    form, shape, kind, tau, mode, which, c, o, _ = parts(case)
    got = [("direct", TL.direct_f64(c, mode, tau))]
    if which == "expanded":
        got.append(("expanded", TL.expanded_f64(c, mode)))
    for name, g in got:
        for n in TL.OUTPUTS:
            if n in o:
                err, top = TL.yard_error(o[n], g[n]), float(np.max(np.abs(o[n])))
                assert err <= 1e-9 * top, (name, n, err, top)


@pytest.mark.parametrize("case", TL.CASES, ids=IDS)
def test_inputs_are_in_the_trained_regime(case):
    form, shape, kind, tau, mode, which, c, o, y = parts(case)
    for k in ("mean", "lv", "eps", "logits", "gumbel", "pm", "plv"):
        assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k
    if mode == "vade":
        assert np.median(o["w"].max(1)) >= 0.99
        gap = TL.top_two_gap(o["u"])
    else:
        assert np.median(o["q"].max(1)) >= 0.99
        gap = TL.top_two_gap(c["logits"])
    if kind in ("competing", "floor"):
        assert (gap < 8.0).mean() >= 0.20, (gap < 8.0).mean()
        if mode == "vade":
            # the quantities of vade_large.gamma_is_soft; max |G| over the entries whose gamma is not 0.0 in float64: G against a collapsed
            # cluster (kind floor) is r / B T / 2 with T ~ 1e7 on entries that carry nothing in any arithmetic
            x = V.expanded(c["mean"], c["lv"], c["eps"], c["pm"], c["plv"], TL.KL_RATIO)
            du, G = float(np.abs(x["du"]).max()), float(np.abs(x["G"])[o["w"] > 0].max())
            assert du >= 1e-3 * G, (du, G)                # the path through gamma carries gradient
        else:
            assert np.abs(o["dlogits"][c["comp"]]).max() >= 1e-3 * np.abs(o["dlogits"]).max()
    if kind == "floor":
        dead = np.all(c["plv"] == c["plv"][0, :], axis=0) & np.all(c["pm"] == np.float32(0.5), axis=0)
        assert dead.sum() == TL.N_DEAD
        assert (np.bincount(c["c"], minlength=shape[2])[np.argmin(c["plv"].sum(1))]) == TL.N_COLLAPSED_ROWS
    if kind == "vanishing":
        q32 = y["q"]
        assert (q32 == 0.0).any() and ((q32 > 1e-30) & (q32 < 1e-15)).any()
        assert c["vrows"].sum() == TL.N_VANISHING_ROWS and (c["gumbel"][c["vrows"]] == np.float32(TL.GUMBEL_ATOM)).sum() == TL.N_VANISHING_ROWS


@pytest.mark.parametrize("case", TL.CASES, ids=IDS)
def test_yardsticks_are_finite(case):
    y = parts(case)[-1]
    for n, v in y.items():
        assert np.all(np.isfinite(v)), n


@pytest.mark.parametrize("case", TL.CASES, ids=IDS)
def test_tolerance_is_not_vacuous(case):
    form, shape, kind, tau, mode, which, c, o, y = parts(case)
    bad = []
    for n in TL.outputs_of(form, shape, kind):
        err, top = TL.yard_error(o[n], y[n]), float(np.max(np.abs(o[n])))
        if not 2.0 * err < 0.01 * top:
            bad.append((n, err, top))
    assert not bad, bad


@pytest.mark.parametrize("case", VADE, ids=[TL.case_id(*c) for c in VADE])
def test_clear_rows_are_most_rows(case):
    form, shape, kind, tau, mode, which, c, o, y = parts(case)
    clear = TL.clear_rows(o["u"], y["u"])
    assert clear.mean() >= 0.95, (clear.mean(), TL.u_error(o["u"], y["u"]))
    assert np.array_equal(np.argmax(y["w"], 1)[clear], np.argmax(o["w"], 1)[clear])


@pytest.mark.parametrize("corrupt", TL.CORRUPTIONS)
@pytest.mark.parametrize("case", EXPANDED, ids=[TL.case_id(*c) for c in EXPANDED])
def test_a_corrupted_algebra_leaves_the_tolerance(case, corrupt):
    """dropping c2, pm of cluster k + 1, the last 64 columns of the 2D contraction dropped, log(g) for log(g + 1e-20): at least one output
    of every case misses tolerance(...).  The last one exists only where some probability is below 1e-20 * 2^24: every VaDE case (gamma is
    one-hot to the last bit on most rows) and the vanishing rows; in the other DMVAE cases the smallest q is above 1e-9 and the two
    logarithms are the same float32 number -- asserted, so that the claim is not taken on trust."""
    form, shape, kind, tau, mode, which, c, o, y = parts(case)
    with np.errstate(all="ignore"):                 # (log 0 is the point of the last corruption)
        bad = TL.expanded(c, mode, corrupt=corrupt)
    if corrupt == "log_no_floor" and mode == "exact" and kind != "vanishing":
        assert y["q"].min() > 1e-9
        for n in TL.outputs_of(form, shape, kind):
            assert np.array_equal(bad[n], y[n]), n
        return
    missed = [n for n in TL.outputs_of(form, shape, kind) if not TL.within(n, bad[n], o[n], y[n])[0]]
    assert missed, "no output sees the corruption"
