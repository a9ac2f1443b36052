"""Host-side tests of the Sinkhorn-divergence family (csrc/sinkhorn.hip, dmvae_hip/sinkhorn.py): dmvae_sinkhorn_softmin is declared,
exported and bound and refuses bad arguments by name before anything is enqueued, the model and CLI surface exists, sinkhorn.hip compiles for
gfx950 without a spill or scratch, sinkhorn_divergence refuses bad arguments before any device use, and the float64 oracle the GPU tests lean
on (tests/helpers/sinkhorn_oracle.py) holds the properties of the divergence itself."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import sinkhorn_oracle as SO      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-mixture-vae_amd")


def test_entry_is_declared_exported_and_bound():
    from dmvae_hip import _lib
    hdr_full = open(os.path.join(ROOT, "include", "dmvae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    declared = set(re.findall(r"\b(dmvae_[a-z0-9_]+)\s*\(", hdr))
    name = "dmvae_sinkhorn_softmin"
    assert name in declared and name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert len(_lib.lib.dmvae_sinkhorn_softmin.argtypes) == 13
    assert _lib.ABI_VERSION == 5 and _lib.lib.dmvae_abi_version() == 5 and "#define DMVAE_ABI_VERSION 5" in hdr_full      # entries are only added
    assert "logsumexp_j" in hdr_full and "No 1/2 factor" in hdr_full                 # the header restates the contract
    assert '"sinkhorn.hip"' in open(os.path.join(PKG, "build.py")).read()
    import dmvae_hip.sinkhorn as S
    src = open(S.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+(sklearn|geomloss|ot)\b", src, flags=re.M)
    for fn in ("softmin_enqueue", "sinkhorn_divergence"):
        assert callable(getattr(S, fn))
    assert "knn_tile_d2(" in open(os.path.join(PKG, "csrc", "sinkhorn.hip")).read()  # the tile body is reused, not restated


def test_bad_arguments_are_refused_by_name_before_anything_is_enqueued():
    from dmvae_hip import _lib
    f = _lib.lib.dmvae_sinkhorn_softmin
    buf = [np.zeros(64, dtype=np.float32) for _ in range(6)]     # host memory: a refused call touches none of it
    X, Y, g, lb, prev, out = [b.ctypes.data for b in buf]
    good = dict(X=X, ldx=4, N=4, Y=Y, ldy=4, M=4, D=4, g=g, lb=lb, eps=1.0, prev=prev, out=out)
    big = (1 << 20) + 1
    for change in (dict(X=None), dict(Y=None), dict(out=None), dict(N=0), dict(M=0), dict(D=0), dict(N=-1), dict(N=big), dict(M=big), dict(ldx=3),
                   dict(ldy=3), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(eps=1e-45)):
        a = dict(good, **change)
        rc = f(None, a["X"], a["ldx"], a["N"], a["Y"], a["ldy"], a["M"], a["D"], a["g"], a["lb"], a["eps"], a["prev"], a["out"])
        assert rc == -1, change                                  # DMVAE_EINVAL
        assert b"dmvae_sinkhorn_softmin" in _lib.lib.dmvae_last_error(), change
    assert all(not b.any() for b in buf)


def test_model_and_cli_surface_exists():
    import base_models
    import models
    for cls in (base_models.DeepMixtureVAE, base_models.VaDE, models.DeepMoE, models.DeepVariationalMoE):
        assert callable(cls.get_sample_distance)
    import train
    assert train.parser.parse_args([]).sample_distance is False
    assert train.parser.parse_args(["--sample_distance"]).sample_distance is True


def test_sinkhorn_hip_compiles_without_spill_or_scratch(tmp_path):
    out = tmp_path / "sinkhorn.s"
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-mllvm",
                        "-amdgpu-mfma-vgpr-form=1", "-S", "--cuda-device-only", os.path.join(PKG, "csrc", "sinkhorn.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    txt = out.read_text()
    assert "sinkhorn_softmin_kernel" in txt
    assert set(re.findall(r"\.vgpr_spill_count: +\d+", txt)) == {".vgpr_spill_count: 0"}
    assert set(re.findall(r"\.private_segment_fixed_size: +\d+", txt)) == {".private_segment_fixed_size: 0"}
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count: +(\d+)", txt)]
    assert vgprs and max(vgprs) <= 128                           # four workgroups per CU: what DESIGN.md section 25 reports


def test_sinkhorn_divergence_refuses_bad_arguments_before_any_device_use():
    from dmvae_hip.sinkhorn import sinkhorn_divergence
    X, Y = np.zeros((6, 3), dtype=np.float32), np.ones((5, 3), dtype=np.float32)      # CPU inputs: a refusal comes before the upload
    for kw in (dict(fake=np.ones((5, 4), dtype=np.float32)), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps_rel=0.0), dict(tol=-1e-3),
               dict(max_iter=0), dict(check_every=0), dict(real_groups=np.zeros(5, dtype=np.int64)), dict(fake_groups=np.zeros(6, dtype=np.int64)),
               dict(log_a=np.zeros(5, dtype=np.float32)), dict(log_b=np.zeros(6, dtype=np.float32))):
        with pytest.raises(ValueError):
            sinkhorn_divergence(X, **dict(dict(fake=Y), **kw))


def clouds(n, m, d, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(n, d).astype(np.float32), (0.5 + 0.8 * rng.randn(m, d)).astype(np.float32)


def test_oracle_softmin_against_a_double_loop_and_closed_forms():
    import math
    X, Y = clouds(5, 7, 3, 0)
    rng = np.random.RandomState(1)
    g, lb, prev, eps = rng.randn(7), np.log(rng.dirichlet(np.ones(7))), rng.randn(5), 0.37
    lb[2] = -np.inf                                              # a column without mass
    out, bar = SO.softmin(X, Y, eps, g, lb, prev)
    for i in range(5):
        t = [lb[j] + g[j] / eps - sum((float(X[i][c]) - float(Y[j][c])) ** 2 for c in range(3)) / eps for j in range(7) if j != 2]
        mx = max(t)
        want = 0.5 * (prev[i] - eps * (mx + math.log(sum(math.exp(v - mx) for v in t))))
        assert abs(out[i] - want) <= 1e-13 * (abs(want) + 1) and 0 < bar[i] <= 1e-4 * (abs(out[i]) + eps)
    # one column: out_i = d2_i0 - eps h_0;   identical rows, uniform weights, g = 0: out = 0;   no live column: +inf
    one, _ = SO.softmin(X, Y[:1], eps, g[:1], lb[:1])
    assert np.allclose(one, SO.pair_d2(X, Y[:1])[:, 0] - eps * (lb[0] + g[0] / eps), rtol=0, atol=1e-13)
    same, sbar = SO.softmin(np.tile(X[:1], (4, 1)), np.tile(X[:1], (9, 1)), eps)
    assert np.all(np.abs(same) <= 1e-15) and np.all(sbar > 0)
    empty, ebar = SO.softmin(X, Y, eps, None, np.full(7, -np.inf))
    assert np.all(np.isposinf(empty)) and not ebar.any()


def test_oracle_divergence_properties():
    X, Y = clouds(40, 55, 4, 2)
    scale, mean_cost = SO.scale_and_mean_cost(X, Y)
    assert abs(mean_cost - np.mean([[np.sum((x.astype(np.float64) - y) ** 2) for y in Y] for x in X])) <= 1e-12 * mean_cost
    eps = float(np.float32(0.05 * mean_cost))
    sched = SO.schedule(scale, eps)
    assert sched[0] == float(np.float32(scale)) and all(a > b for a, b in zip(sched, sched[1:])) and sched[-1] > eps >= 0.7 * sched[-1] * (1 - 1e-6)
    # S(X, X) = 0 within its own bar once converged; S > 0 for a shifted copy
    zero = SO.divergence(X, X, eps, scale, iters=(300, 60, 60))
    assert abs(zero["divergence"]) <= zero["bar"] and zero["bar"] <= 1e-2 * eps
    shifted = SO.divergence(X, X + np.float32(0.5), eps, scale, iters=(300, 60, 60))
    assert shifted["divergence"] > 10 * shifted["bar"] and 0.05 < shifted["divergence"] / shifted["ot"] < 0.95
    # the per-group sums add up to S; a group without rows: 0 and nan
    g_r, g_f = np.arange(40) % 3, np.where(np.arange(55) % 4 == 2, 4, np.arange(55) % 4)      # group 2 of the generated rows is empty
    res = SO.divergence(X, Y, eps, scale, tol=1e-6, real_groups=g_r, fake_groups=g_f)
    assert abs(res["per_real_group"].sum() + res["per_fake_group"].sum() - res["divergence"]) <= 1e-12 * abs(res["divergence"])
    assert res["per_fake_group"][2] == 0.0 and np.isnan(res["mean_per_fake_group"][2]) and not np.isnan(res["mean_per_real_group"]).any()
    assert abs(res["divergence"] - (res["ot"] - 0.5 * res["ot_real"] - 0.5 * res["ot_fake"])) <= 1e-12 * abs(res["ot"])
    assert res["divergence"] > 0 and max(res["err"]) <= 1e-6
    # a dense plan from the converged potentials has the marginals a and b within tol
    f, g, p, q = res["potentials"]
    P = SO.plan(X, Y, f, g, eps)
    assert np.abs(P.sum(axis=0) - 1.0 / 55).sum() <= 1e-6 and np.abs(P.sum(axis=1) - 1.0 / 40).sum() <= 1e-6
    assert abs((P * SO.pair_d2(X, Y)).sum() + eps * np.sum(P * np.log(P * 40 * 55)) - res["ot"]) <= 1e-5 * res["ot"]       # the primal value
    Pa = SO.plan(X, X, p, p, eps)
    assert np.abs(Pa.sum(axis=1) - 1.0 / 40).sum() <= 1e-6 and np.abs(Pa - Pa.T).max() <= 1e-15
    # weights: moving the mass of a row to its duplicate changes nothing
    la = np.log(np.full(41, 1.0 / 40))
    la[0] = la[40] = np.log(0.5 / 40)
    dup = SO.divergence(np.concatenate([X, X[:1]]), Y, eps, scale, tol=1e-6, log_a=la)
    assert abs(dup["divergence"] - res["divergence"]) <= 1e-4 * eps
