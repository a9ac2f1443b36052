"""Host-side tests of the structural-similarity family (csrc/ssim.hip, dmvae_hip/ssim.py): dmvae_ssim_rows is declared, exported and bound
and refuses bad arguments by name before anything is enqueued, the Python and CLI surface exists, ssim.hip compiles for gfx950 without a
spill or scratch, and the float64 oracle the GPU tests lean on (tests/helpers/ssim_oracle.py) agrees with a brute-force quadruple loop,
with the scipy.ndimage formulation of skimage's definition, with closed forms and with a hand-worked window; its f32 emulation of the
pinned sequence holds the two bit properties."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import ssim_oracle as SO      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-mixture-vae_amd")
C1, C2 = SO.constants()


def test_entry_is_declared_exported_and_bound():
    from dmvae_hip import _lib
    hdr_full = open(os.path.join(ROOT, "include", "dmvae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    declared = set(re.findall(r"\b(dmvae_[a-z0-9_]+)\s*\(", hdr))
    assert "dmvae_ssim_rows" in declared and "dmvae_ssim_rows" in _lib.EXPORTS and hasattr(_lib.lib, "dmvae_ssim_rows")
    assert len(_lib.lib.dmvae_ssim_rows.argtypes) == 20
    assert _lib.ABI_VERSION == 5 and _lib.lib.dmvae_abi_version() == 5 and "#define DMVAE_ABI_VERSION 5" in hdr_full      # entries are only added
    assert "CENTRED" in hdr_full and "ssim(X, X) == 1.0f" in hdr_full       # the header restates the contract
    assert '"ssim.hip"' in open(os.path.join(PKG, "build.py")).read()
    import dmvae_hip.ssim as S
    src = open(S.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+(sklearn|skimage)\b", src, flags=re.M)
    for name in ("gaussian_window", "ssim_enqueue", "ssim", "pairwise_enqueue"):
        assert callable(getattr(S, name))


def call(f, a):
    return f(None, a["X"], a["ldx"], a["nx"], a["ix"], a["Y"], a["ldy"], a["ny"], a["iy"], a["n"], a["H"], a["W"], a["planes"], a["w1"], a["win"],
             C.c_float(C1), C.c_float(C2), a["ssim"], a["sse"], a["flag"])


def test_bad_arguments_are_refused_by_name_before_anything_is_enqueued():
    from dmvae_hip import _lib
    f = _lib.lib.dmvae_ssim_rows
    buf = [np.zeros(4096, dtype=np.float32) for _ in range(5)]   # host memory: a refused call touches none of it
    X, Y, out, sse, flag = [b.ctypes.data for b in buf]
    w = SO.gaussian_window()
    good = dict(X=X, ldx=144, nx=4, ix=None, Y=Y, ldy=144, ny=4, iy=None, n=4, H=12, W=12, planes=1, w1=w.ctypes.data, win=11, ssim=out, sse=sse,
                flag=flag)
    einval = (dict(X=None), dict(Y=None), dict(ssim=None), dict(w1=None), dict(n=0), dict(n=-3), dict(nx=0), dict(ny=0), dict(H=0), dict(W=0),
              dict(planes=0), dict(win=1), dict(win=4), dict(win=10), dict(win=13), dict(H=9, ldx=200, ldy=200), dict(W=7, ldx=200, ldy=200),
              dict(ldx=143), dict(ldy=143), dict(planes=2))
    for change in einval:
        assert call(f, dict(good, **change)) == -1, change       # DMVAE_EINVAL
        assert b"dmvae_ssim_rows" in _lib.lib.dmvae_last_error(), change
    for change in (dict(H=65, W=64, ldx=4160, ldy=4160), dict(H=4097, W=11, ldx=1 << 20, ldy=1 << 20)):
        assert call(f, dict(good, **change)) == -2, change       # DMVAE_EUNSUPPORTED
        assert b"dmvae_ssim_rows" in _lib.lib.dmvae_last_error(), change
    assert all(not b.any() for b in buf)


def test_python_arguments_are_checked_before_the_device_is_touched():
    from dmvae_hip import ssim as S

    class Rows:                                                  # no tensor: anything past the checks would fail differently
        shape = (6, 144)
    for shape in ((12, 13), (2, 12, 12), (144,), (0, 12, 12)):
        with pytest.raises(ValueError):
            S.ssim_enqueue(Rows(), Rows(), shape)
    with pytest.raises(ValueError):
        S.ssim_enqueue(Rows(), Rows(), (16, 9))                  # the default 11-tap window does not fit 9 columns
    for window in (np.ones(4) / 4, np.ones(13) / 13, np.ones(1)):
        with pytest.raises(ValueError):
            S.ssim_enqueue(Rows(), Rows(), (12, 12), window=window)
    with pytest.raises(ValueError):
        S.default_image_shape(150)
    assert S.default_image_shape(784) == (28, 28)
    w = S.gaussian_window()
    assert w.dtype == np.float32 and len(w) == 11 and np.array_equal(w, SO.gaussian_window()) and abs(float(w.astype(np.float64).sum()) - 1.0) < 2e-7
    assert np.array_equal(w, w[::-1]) and w[5] == w.max()
    assert S.constants() == (C1, C2) and C1 == float(np.float32(1e-4)) and C2 == float(np.float32(9e-4))


def test_model_and_cli_surface_exists():
    import base_models
    import models
    for cls in (base_models.DeepMixtureVAE, base_models.VaDE, models.DeepMoE, models.DeepVariationalMoE):
        assert callable(cls.get_reconstruction_quality) and callable(cls.get_sample_diversity)
    import train
    a = train.parser.parse_args([])
    assert a.recon_quality is False and a.sample_diversity == 0
    a = train.parser.parse_args(["--recon_quality", "--sample_diversity", "4"])
    assert a.recon_quality is True and a.sample_diversity == 4


def test_ssim_hip_compiles_without_spill_or_scratch(tmp_path):
    out = tmp_path / "ssim.s"
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-mllvm",
                        "-amdgpu-mfma-vgpr-form=1", "-S", "--cuda-device-only", os.path.join(PKG, "csrc", "ssim.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    txt = out.read_text()
    assert len(re.findall(r"\.name: +_ZN5dmvae16ssim_rows_kernelILi\d+EE", txt)) == 5          # windows 3, 5, 7, 9, 11
    assert set(re.findall(r"\.vgpr_spill_count: +\d+", txt)) == {".vgpr_spill_count: 0"}
    assert set(re.findall(r"\.private_segment_fixed_size: +\d+", txt)) == {".private_segment_fixed_size: 0"}
    assert max(int(v) for v in re.findall(r"\.vgpr_count: +(\d+)", txt)) <= 128                # 4 waves per SIMD


def brute(x, y, w1, c1, c2):
    """the definition as a quadruple loop in Python floats, one plane"""
    H, W, win = len(x), len(x[0]), len(w1)
    g = [[float(np.float32(np.float32(w1[a]) * np.float32(w1[b]))) for b in range(win)] for a in range(win)]
    total, count = 0.0, 0
    for i in range(H - win + 1):
        for j in range(W - win + 1):
            mx = sum(g[a][b] * x[i + a][j + b] for a in range(win) for b in range(win))
            my = sum(g[a][b] * y[i + a][j + b] for a in range(win) for b in range(win))
            sxx = sum(g[a][b] * (x[i + a][j + b] - mx) ** 2 for a in range(win) for b in range(win))
            syy = sum(g[a][b] * (y[i + a][j + b] - my) ** 2 for a in range(win) for b in range(win))
            sxy = sum(g[a][b] * (x[i + a][j + b] - mx) * (y[i + a][j + b] - my) for a in range(win) for b in range(win))
            total += (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
            count += 1
    return total / count, count


@pytest.mark.parametrize("H,W,win", [(11, 11, 11), (5, 4, 3), (12, 13, 7)])
def test_oracle_against_a_brute_force_quadruple_loop(H, W, win):
    X = SO.mnist_like(8, 1, H, W, seed=H)
    Y = SO.other_side(X, seed=W)
    w = SO.gaussian_window(win, 1.5)
    got, sse = SO.ssim_rows(X, Y, (1, H, W), w, C1, C2)
    for r in range(len(X)):
        x, y = X[r].astype(np.float64).reshape(H, W).tolist(), Y[r].astype(np.float64).reshape(H, W).tolist()
        want, count = brute(x, y, w, C1, C2)
        assert count == (H - win + 1) * (W - win + 1)
        assert abs(got[r] - want) <= 1e-13, (r, got[r], want)
        assert abs(sse[r] - sum((a - b) ** 2 for ra, rb in zip(x, y) for a, b in zip(ra, rb))) <= 1e-12


def test_oracle_against_the_scipy_formulation_of_skimage():
    X = SO.mnist_like(12, 1, 28, 28, seed=3)
    Y = SO.other_side(X, seed=4)
    got, _ = SO.ssim_rows(X, Y, (1, 28, 28), SO.gaussian_window(), C1, C2)
    want = [SO.ssim_scipy(X[r].reshape(28, 28), Y[r].reshape(28, 28)) for r in range(len(X))]
    assert np.abs(got - np.array(want)).max() <= 1e-8
    assert got.min() < 0.0 and got.max() == 1.0 and ((got > 0.3) & (got < 0.7)).any()


def test_oracle_closed_forms():
    w = SO.gaussian_window()
    X = SO.mnist_like(4, 2, 14, 12, seed=5)
    got, sse = SO.ssim_rows(X, X, (2, 14, 12), w, C1, C2)
    assert np.array_equal(got, np.ones(4)) and not sse.any()     # identical images: numerator and denominator are the same expression
    gsum = SO.weights2d(w).sum()                                 # (the f32-rounded weights add up to 1 within 1e-7: the means carry it)
    for a, b in ((0.25, 0.75), (0.0, 1.0), (0.5, 0.5)):
        x, y = np.full((1, 13, 12), a), np.full((1, 13, 12), b)
        ma, mb = gsum * a, gsum * b
        want = (2 * ma * mb + C1) / (ma * ma + mb * mb + C1)     # both variances vanish: the second factor is c2 / c2
        assert abs(SO.ssim_image(x, y, w, C1, C2) - want) <= 1e-12
        assert abs(want - (2 * a * b + C1) / (a * a + b * b + C1)) <= 1e-6


def test_oracle_on_a_hand_worked_window():
    # one 3 x 3 window, weights (1 2 1) / 4 (exact in f32): x is 1 at the centre and 0 elsewhere, y is 0.  g[1][1] = 1/4, so mx = 1/4, my = 0,
    # sxx = 1/4 (3/4)^2 + 3/4 (1/4)^2 = 3/16, syy = sxy = 0:  S = c1 c2 / ((1/16 + c1)(3/16 + c2))
    w = np.array([0.25, 0.5, 0.25], dtype=np.float32)
    x = np.zeros((1, 3, 3))
    x[0, 1, 1] = 1.0
    y = np.zeros((1, 3, 3))
    want = C1 * C2 / ((1.0 / 16 + C1) * (3.0 / 16 + C2))
    assert abs(SO.ssim_image(x, y, w, C1, C2) - want) <= 1e-15
    s, e = SO.ssim_rows(x.reshape(1, 9), y.reshape(1, 9), (1, 3, 3), w, C1, C2)
    assert abs(s[0] - want) <= 1e-15 and e[0] == 1.0
    # y = x / 2: my = 1/8, syy = sxx / 4, sxy = sxx / 2
    want = (2 * 0.25 * 0.125 + C1) * (2 * 3.0 / 32 + C2) / ((1.0 / 16 + 1.0 / 64 + C1) * (3.0 / 16 + 3.0 / 64 + C2))
    assert abs(SO.ssim_image(x, x / 2, w, C1, C2) - want) <= 1e-15


def test_f32_emulation_holds_the_two_bit_properties_and_stays_near_the_oracle():
    w = SO.gaussian_window()
    X = SO.mnist_like(16, 1, 28, 28, seed=7)
    Y = SO.other_side(X, seed=8)
    want, _ = SO.ssim_rows(X, Y, (1, 28, 28), w, C1, C2)
    worst = 0.0
    for r in range(len(X)):
        x, y = X[r].reshape(1, 28, 28), Y[r].reshape(1, 28, 28)
        assert SO.ssim_f32_pinned(x, x, w, C1, C2) == np.float32(1.0)          # exactly
        a, b = SO.ssim_f32_pinned(x, y, w, C1, C2), SO.ssim_f32_pinned(y, x, w, C1, C2)
        assert a.tobytes() == b.tobytes()                                      # the same bits with the sides swapped
        worst = max(worst, abs(float(a) - want[r]))
    assert worst <= SO.u_bound(11), worst                        # (measured: about 1e-7 with the final rounding to f32)


def test_group_pairs_and_image_generator():
    ix, iy, pg = SO.group_pairs([1, 0, 1, 1, 0, 2], 3)
    assert ix.tolist() == [1, 0, 0, 2] and iy.tolist() == [4, 2, 3, 3] and pg.tolist() == [0, 1, 1, 1]
    X = SO.mnist_like(5, 3, 9, 8, seed=0)
    assert X.shape == (5, 216) and X.dtype == np.float32 and X.min() == 0.0 and X.max() == 1.0
    assert 0.1 < float((X > 0).mean()) and float((X == 0).mean()) > 0.1      # strokes and flat black regions
