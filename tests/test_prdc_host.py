"""Host-side tests of the sample-quality family (csrc/prdc.hip, dmvae_hip/prdc.py): dmvae_prdc_counts is declared, exported and bound and
refuses bad arguments by name before anything is enqueued, the model and CLI surface exists, prdc.hip compiles for gfx950 without a spill
or scratch, and the float64 oracle the GPU tests lean on (tests/helpers/prdc_oracle.py) agrees with a brute-force double loop, with closed
forms and with a hand-worked case."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import prdc_oracle as PO      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-mixture-vae_amd")


def test_entry_is_declared_exported_and_bound():
    from dmvae_hip import _lib
    hdr_full = open(os.path.join(ROOT, "include", "dmvae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    declared = set(re.findall(r"\b(dmvae_[a-z0-9_]+)\s*\(", hdr))
    assert "dmvae_prdc_counts" in declared and "dmvae_prdc_counts" in _lib.EXPORTS and hasattr(_lib.lib, "dmvae_prdc_counts")
    assert len(_lib.lib.dmvae_prdc_counts.argtypes) == 14
    assert _lib.ABI_VERSION == 5 and _lib.lib.dmvae_abi_version() == 5 and "#define DMVAE_ABI_VERSION 5" in hdr_full      # entries are only added
    assert "CLOSED" in hdr_full and "d2 <= r2" in hdr_full       # the header says which ball rule holds
    assert '"prdc.hip"' in open(os.path.join(PKG, "build.py")).read()
    import dmvae_hip.prdc as P
    src = open(P.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+(sklearn|prdc)\b", src, flags=re.M)
    for name in ("counts_enqueue", "radii_enqueue", "prdc"):
        assert callable(getattr(P, name))


def test_bad_arguments_are_refused_by_name_before_anything_is_enqueued():
    from dmvae_hip import _lib
    f = _lib.lib.dmvae_prdc_counts
    buf = [np.zeros(64, dtype=np.float32) for _ in range(8)]     # host memory: a refused call touches none of it
    R, F, rR2, rF2, fir, rif, rmin, rj = [b.ctypes.data for b in buf]
    good = dict(R=R, ldr=4, N=4, F=F, ldf=4, M=4, D=4, rR2=rR2, rF2=rF2, fir=fir, rif=rif, rmin=rmin, rj=rj)
    big = (1 << 20) + 1
    for change in (dict(N=0), dict(M=0), dict(D=0), dict(M=big), dict(N=big), dict(N=-1), dict(R=None), dict(F=None), dict(rR2=None), dict(rF2=None),
                   dict(fir=None), dict(rif=None), dict(rmin=None), dict(ldr=3), dict(ldf=3)):
        a = dict(good, **change)
        rc = f(None, a["R"], a["ldr"], a["N"], a["F"], a["ldf"], a["M"], a["D"], a["rR2"], a["rF2"], a["fir"], a["rif"], a["rmin"], a["rj"])
        assert rc == -1, change                                  # DMVAE_EINVAL
        assert b"dmvae_prdc_counts" in _lib.lib.dmvae_last_error(), change
    from dmvae_hip.prdc import radii_enqueue

    class Rows:                                                  # radii_enqueue checks k against the rows before it touches the device
        shape = (6, 3)
    for k in (0, 6, 257):
        with pytest.raises(ValueError):
            radii_enqueue(Rows(), k)


def test_model_and_cli_surface_exists():
    import base_models
    import models
    for cls in (base_models.DeepMixtureVAE, base_models.VaDE, models.DeepMoE, models.DeepVariationalMoE):
        assert callable(cls.get_sample_quality)
    import train
    assert train.parser.parse_args([]).sample_quality == 0
    assert train.parser.parse_args(["--sample_quality", "5"]).sample_quality == 5


def test_prdc_hip_compiles_without_spill_or_scratch(tmp_path):
    out = tmp_path / "prdc.s"
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-mllvm",
                        "-amdgpu-mfma-vgpr-form=1", "-S", "--cuda-device-only", os.path.join(PKG, "csrc", "prdc.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    txt = out.read_text()
    assert "prdc_pairs_kernel" in txt
    assert set(re.findall(r"\.vgpr_spill_count: +\d+", txt)) == {".vgpr_spill_count: 0"}
    assert set(re.findall(r"\.private_segment_fixed_size: +\d+", txt)) == {".private_segment_fixed_size: 0"}


def brute(R, F, rR2, rF2, k):
    N, M, D = len(R), len(F), len(R[0])
    d = [[sum((float(R[i][c]) - float(F[j][c])) ** 2 for c in range(D)) for j in range(M)] for i in range(N)]
    fir = [sum(1 for i in range(N) if d[i][j] <= rR2[i]) for j in range(M)]
    rif = [sum(1 for j in range(M) if d[i][j] <= rF2[j]) for i in range(N)]
    mn = [min(d[i]) for i in range(N)]
    mj = [d[i].index(mn[i]) for i in range(N)]
    return fir, rif, mn, mj, dict(precision=sum(1 for c in fir if c) / M, recall=sum(1 for c in rif if c) / N, density=sum(fir) / (k * M),
                                  coverage=sum(1 for i in range(N) if mn[i] <= rR2[i]) / N)


def test_oracle_against_a_brute_force_double_loop():
    rng = np.random.RandomState(0)
    R, F = rng.randint(-3, 4, (23, 2)).astype(np.float64), rng.randint(-3, 4, (31, 2)).astype(np.float64)       # many exact ties
    for k in (1, 3):
        rR2, rF2 = PO.radii(R, k), PO.radii(F, k)
        for X, r2 in ((R, rR2), (F, rF2)):
            for i in range(len(X)):
                assert r2[i] == sorted(sum((X[i][c] - X[l][c]) ** 2 for c in range(2)) for l in range(len(X)) if l != i)[k - 1]
        fir, rif, mn, mj, want = brute(R, F, rR2, rF2, k)
        c = PO.counts(R, F, rR2, rF2)
        assert c["fake_in_real"].tolist() == fir and c["real_in_fake"].tolist() == rif
        assert c["real_min_d2"].tolist() == mn and c["real_min_j"].tolist() == mj
        got = PO.prdc(R, F, k)
        assert {m: got[m] for m in want} == want and got["k"] == k
    g_r, g_f = rng.randint(0, 3, len(R)), rng.randint(0, 4, len(F))
    got = PO.prdc(R, F, 3, real_groups=g_r, fake_groups=g_f)
    c = PO.counts(R, F, PO.radii(R, 3), PO.radii(F, 3))
    for g in range(3):
        rows = [i for i in range(len(R)) if g_r[i] == g]
        assert got["recall_per_group"][g] == sum(1 for i in rows if c["real_in_fake"][i] > 0) / len(rows)
        assert got["coverage_per_group"][g] == sum(1 for i in rows if c["real_min_d2"][i] <= PO.radii(R, 3)[i]) / len(rows)
    for g in range(4):
        rows = [j for j in range(len(F)) if g_f[j] == g]
        assert got["precision_per_group"][g] == sum(1 for j in rows if c["fake_in_real"][j] > 0) / len(rows)
        assert got["density_per_group"][g] == sum(int(c["fake_in_real"][j]) for j in rows) / (3 * len(rows))


def test_oracle_closed_forms():
    rng = np.random.RandomState(1)
    R = rng.randn(40, 3)                                         # distinct rows
    for k in (1, 4):
        got = PO.prdc(R, R, k)
        # F = R: a row lies in its own ball (d2 = 0) and in the balls of the rows it is among the k nearest of -- summed over the rows,
        # k per ball -- so the counts add up to (k + 1) N
        assert got["precision"] == got["recall"] == got["coverage"] == 1.0 and got["density"] == (k + 1) / k
        far = PO.prdc(R, R + 1000.0, k)                          # further apart than any radius
        assert far["precision"] == far["recall"] == far["density"] == far["coverage"] == 0.0


def test_oracle_on_five_collinear_points():
    # real rows at 0, 1, 3 and generated rows at 2, 6 on a line, k = 1: rR2 = (1, 1, 4), rF2 = (16, 16)
    # d2 = [[4, 36], [1, 25], [1, 9]]: the generated row at 2 lies ON the ball of the real row at 1 (1 <= 1: closed) and inside that of 3
    R, F = np.array([[0.0], [1.0], [3.0]]), np.array([[2.0], [6.0]])
    assert PO.radii(R, 1).tolist() == [1.0, 1.0, 4.0] and PO.radii(F, 1).tolist() == [16.0, 16.0]
    c = PO.counts(R, F, PO.radii(R, 1), PO.radii(F, 1))
    assert c["d2"].tolist() == [[4.0, 36.0], [1.0, 25.0], [1.0, 9.0]]
    assert c["fake_in_real"].tolist() == [2, 0] and c["real_in_fake"].tolist() == [1, 1, 2]
    assert c["real_min_d2"].tolist() == [4.0, 1.0, 1.0] and c["real_min_j"].tolist() == [0, 0, 0]
    got = PO.prdc(R, F, 1)
    assert (got["precision"], got["recall"], got["density"], got["coverage"]) == (0.5, 1.0, 1.0, 2.0 / 3.0)      # with < coverage would be 1/3
    und = PO.undecided(c["d2"], np.array([1.0, 1.0, 4.0])[:, None], PO.u_bar(1))
    assert und.tolist() == [[False, False], [True, False], [False, False]]
    assert not PO.undecided(c["d2"], np.inf, PO.u_bar(1)).any()
