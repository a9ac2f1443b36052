"""CPU tests of the augmentation feature: the float64 oracle against itself (forward x inverse) and against torch's
grid_sample, stream 9 against the other rows of the noise table, parse_augment, Dataset(augment=...) without a device, the CLI flags and the new
entry's declaration / export / binding.  tests/test_gpu_augment.py holds the kernel to the oracle."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import augment_oracle as AO       # noqa: E402
import philox_oracle as P         # noqa: E402

SPEC = (30.0, 3.0, (0.8, 1.25), 10.0)


def test_forward_times_theta_is_the_identity():
    for H, W, row_base in ((28, 28, 0), (5, 3, 7), (64, 64, (1 << 31) + 3), (1, 1, 0)):
        p = AO.params(4, 2, row_base, 64, SPEC)
        F, c, t = AO.forward64(p, H, W)
        th = AO.theta64(p, H, W).reshape(-1, 2, 3)
        M, off = th[:, :, :2], th[:, :, 2]
        assert np.abs(F @ M - np.eye(2)).max() <= 1e-12 and np.abs(M @ F - np.eye(2)).max() <= 1e-12
        # a source point p_in goes to p_out = c + t + F (p_in - c); the sampling map brings it back
        rng = np.random.RandomState(H)
        pin = rng.rand(64, 2) * [W, H]
        pout = c + t + np.einsum("nab,nb->na", F, pin - c)
        back = np.einsum("nab,nb->na", M, pout) + off
        assert np.abs(back - pin).max() <= 1e-12 * max(H, W)
    ident = AO.theta64(AO.params(1, 1, 0, 5, (0.0, 0.0, (1.0, 1.0), 0.0)), 9, 7)
    assert np.array_equal(ident, np.tile([1.0, 0, 0, 0, 1.0, 0], (5, 1)))


def test_the_draws_lie_in_their_ranges_and_read_the_words_the_table_names():
    n, row_base = 4096, 11
    p = AO.params(3, 5, row_base, n, SPEC)
    assert np.abs(p["angle"]).max() <= 30 and np.abs(p["angle"]).max() > 29 and np.abs(p["tx"]).max() <= 3 and np.abs(p["ty"]).max() <= 3
    assert np.abs(p["shear"]).max() <= 10 and np.abs(p["shear"]).max() > 9.5
    lo, hi = np.float32(0.8), np.float32(1.25)
    assert p["scale"].min() >= lo * (1 - 1e-6) and p["scale"].max() <= hi * (1 + 1e-6) and p["scale"].min() < 0.81 and p["scale"].max() > 1.24
    assert abs(np.log(p["scale"]).mean()) < 0.02                 # log-uniform about 1
    for r in (0, 1, 77):
        g = row_base + r
        w0, w1 = P.block(3, 5, AO.STREAM, np.uint64(2 * g)), P.block(3, 5, AO.STREAM, np.uint64(2 * g + 1))
        s = lambda w: 2.0 * ((int(w) >> 8) * 2.0 ** -24) - 1.0
        assert p["angle"][r] == 30.0 * s(w0[0]) and p["tx"][r] == 3.0 * s(w0[1]) and p["ty"][r] == 3.0 * s(w0[2]) and p["shear"][r] == 10.0 * s(w1[0])
    # chunks with their row_base are the whole call; another key is another draw
    q = AO.params(3, 5, row_base + 100, 50, SPEC)
    assert all(np.array_equal(q[k], p[k][100:150]) for k in p)
    for other in (AO.params(4, 5, row_base, n, SPEC), AO.params(3, 6, row_base, n, SPEC), AO.params(3, 5, row_base + 1, n, SPEC)):
        assert not np.array_equal(other["angle"], p["angle"])
    assert AO.STREAM == 9 and AO.STREAM not in (P.STREAM_EPS, P.STREAM_GUMBEL, P.STREAM_EVAL, P.STREAM_GMM_SEED, 4, 5, 6, 7, 8)
    blk = np.arange(0, 2048, dtype=np.uint64)
    mine = {tuple(int(x) for x in r) for r in P.block(0, 3, AO.STREAM, blk)}
    for sid in range(9):
        assert not mine & {tuple(int(x) for x in r) for r in P.block(0, 3, sid, blk)}, sid


@pytest.mark.parametrize("H,W", [(5, 3), (28, 28)])
def test_warp64_equals_grid_sample_after_the_unit_conversion(H, W):
    """theta maps pixel indices; grid_sample(align_corners=True) maps [-1, 1] onto pixel centres 0 .. W - 1: x = (xn + 1) (W - 1) / 2"""
    import torch
    import torch.nn.functional as F
    rng = np.random.RandomState(10 * H + W)
    n = 8
    X = rng.rand(n, H * W)
    ang, sc = np.deg2rad(rng.uniform(-45, 45, n)), rng.uniform(0.5, 2.0, n)
    k = np.tan(np.deg2rad(rng.uniform(-20, 20, n)))
    theta = np.stack([(np.cos(ang) + k * np.sin(ang)) / sc, (np.sin(ang) - k * np.cos(ang)) / sc, rng.uniform(-W, W, n),
                      -np.sin(ang) / sc, np.cos(ang) / sc, rng.uniform(-H, H, n)], -1)
    theta[0] = [1, 0, 0, 0, 1, 0]
    theta[1] = [1, 0, 0.5, 0, 1, -0.5]                          # half a pixel: the border taps reach outside
    want = AO.warp64(X, theta, H, W)
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sx = theta[:, 0, None, None] * j + theta[:, 1, None, None] * i + theta[:, 2, None, None]
    sy = theta[:, 3, None, None] * j + theta[:, 4, None, None] * i + theta[:, 5, None, None]
    grid = np.stack([2 * sx / (W - 1) - 1, 2 * sy / (H - 1) - 1], -1)
    got = F.grid_sample(torch.as_tensor(X.reshape(n, 1, H, W)), torch.as_tensor(grid), mode="bilinear", padding_mode="zeros", align_corners=True)
    got = got.numpy().reshape(n, H * W)
    print("max |warp64 - grid_sample| = %.3e" % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(want[0], X[0]) and 0.05 < (want != 0).mean() < 1.0


def test_warp64_special_maps():
    X = np.arange(1.0, 13.0).reshape(1, 12)                     # 3 x 4
    H, W = 3, 4
    img = X.reshape(H, W)
    shift = AO.warp64(X, [[1, 0, 1, 0, 1, 0]], H, W).reshape(H, W)           # samples x + 1: the image moves one pixel left
    assert np.array_equal(shift[:, :3], img[:, 1:]) and (shift[:, 3] == 0).all()
    assert (AO.warp64(X, [[1, 0, W, 0, 1, 0]], H, W) == 0).all() and (AO.warp64(X, [[1, 0, 0, 0, 1, -H]], H, W) == 0).all()
    assert np.array_equal(AO.warp64(X, [[-1, 0, W - 1, 0, 1, 0]], H, W).reshape(H, W), img[:, ::-1])
    assert (AO.warp64(X, [[np.nan, 0, 0, 0, 1, 0]], H, W) == 0).all() and (AO.warp64(X, [[1, 0, np.inf, 0, 1, 0]], H, W) == 0).all()


def test_parse_augment_round_trips_and_refuses():
    from dmvae_hip.augment import AugmentSpec, parse_augment
    s = parse_augment("rotate=10,translate=2,scale=0.9:1.1,shear=5")
    assert s == AugmentSpec(rotate=10.0, translate=2.0, scale=(0.9, 1.1), shear=5.0) and s.image_shape is None and not s.is_identity()
    assert parse_augment(str(s)) == s and parse_augment(s) is s
    assert parse_augment("") == AugmentSpec() and AugmentSpec().is_identity() and parse_augment(" translate = 3 ") == AugmentSpec(translate=3.0)
    assert parse_augment("shear=1", image_shape=(4, 6)).image_shape == (4, 6)
    for text, key in (("rotate=10,flip=1", "flip"), ("rotate=ten", "rotate"), ("scale=0.9", "scale"), ("scale=0.9:x", "scale"), ("translate", "translate"),
                      ("shear=", "shear"), ("rotate=-1", "rotate"), ("scale=1.2:0.9", "scale"), ("scale=0:1", "scale"), ("translate=inf", "translate"),
                      ("rotate=1,rotate=2", "rotate"), ("shear=nan", "shear")):
        with pytest.raises(ValueError, match=key):
            parse_augment(text)
    assert s.shape_for(784) == (28, 28) and AugmentSpec(image_shape=(5, 3)).shape_for(15) == (5, 3)
    with pytest.raises(ValueError, match="no square image"):
        s.shape_for(15)
    with pytest.raises(ValueError, match="image_shape"):
        AugmentSpec(image_shape=(5, 3)).shape_for(16)
    p = s.params()
    assert (p.rotate_deg, p.translate_px, p.shear_deg) == (10.0, 2.0, 5.0) and p.scale_lo == np.float32(0.9) and p.scale_hi == np.float32(1.1)


def _numpy_state_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_dataset_without_augment_takes_no_new_code_path_and_with_it_draws_nothing_from_numpy(monkeypatch):
    from includes import utils
    rng = np.random.RandomState(2)
    X, cls = rng.rand(30, 16).astype(np.float32), rng.randint(0, 3, 30)

    def never(*a, **k):
        raise AssertionError("augment=None asked for the training buffer")
    monkeypatch.setattr(utils.Dataset, "_augmented_rows", never)
    np.random.seed(3)
    ds = utils.Dataset((X, cls), batch_size=10)
    assert ds.augment is None and ds.train_rows("cpu") is ds.device_rows("cpu") and list(ds._device) == ["cpu"]
    ds.reshuffle()
    assert ds.train_rows("cpu") is ds.device_rows("cpu") and ds.draw_counter_augment() == 1
    plain_state = np.random.get_state()
    np.random.seed(3)
    aug = utils.Dataset((X, cls), batch_size=10, augment="rotate=5", augment_seed=9)
    aug.reshuffle()
    assert _numpy_state_equal(plain_state, np.random.get_state()) and np.array_equal(aug.order, ds.order)
    assert aug.augment.rotate == 5.0 and aug.augment_seed == 9 and aug.draw_counter_augment() == 1 and aug.draw_counter() == 0
    assert np.array_equal(aug.data, X[aug.order]) and aug.device_rows("cpu") is aug._device["cpu"]       # the clean rows, as ever
    with pytest.raises(ValueError, match="no square image"):
        utils.Dataset((X[:, :15], cls), augment="rotate=5")
    with pytest.raises(ValueError, match="flip"):
        utils.Dataset((X, cls), augment="flip=1")


def test_cli_parses_the_flags_and_rejects_them_for_the_moe_models():
    import train
    args = train.parser.parse_args([])
    assert args.augment is None and args.augment_seed == 0 and args.aug_consistency is None and args.aug_draws == 4
    args = train.parser.parse_args(["--augment", "rotate=10,translate=2", "--augment_seed", "5", "--aug_consistency", "translate=2", "--aug_draws", "3"])
    assert (args.augment, args.augment_seed, args.aug_consistency, args.aug_draws) == ("rotate=10,translate=2", 5, "translate=2", 3)
    for flag in ("--augment", "--augment_seed", "--aug_consistency", "--aug_draws"):
        assert flag in train.__doc__
    for model in ("dmoe", "dvmoe"):
        for flag in ("--augment", "--aug_consistency"):
            args = train.parser.parse_args(["--model", model, "--dataset", "synthetic", "--n_epochs", "0", flag, "rotate=3"])
            with pytest.raises(ValueError, match="--augment / --aug_consistency with --model %s" % model):
                train.main(args)


def test_entry_is_declared_exported_and_bound():
    import ctypes as C
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    decl = re.search(r"int dmvae_augment_rows\((.*?)\);", hdr, flags=re.S).group(1)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["stream", "X", "ldx", "n_rows", "H", "W", "row_base", "seed", "counter", "p", "theta_in", "theta_out",
                                                           "out", "ldo"]
    assert "dmvae_augment_rows" in _lib.EXPORTS and len(_lib.lib.dmvae_augment_rows.argtypes) == len(params)
    struct = re.search(r"typedef struct dmvae_augment_params \{(.*?)\} dmvae_augment_params;", hdr, flags=re.S).group(1)
    fields = [f.split()[-1] for f in struct.replace("\n", " ").split(";") if f.strip()]
    assert fields == [n for n, _ in _lib.AugmentParams._fields_] and all(t is C.c_float for _, t in _lib.AugmentParams._fields_)
    assert C.sizeof(_lib.AugmentParams) == 20
    assert _lib.ABI_VERSION == 5 and _lib.lib.dmvae_abi_version() == 5          # an added entry and a NEW struct: no existing struct grew
    assert re.search(r"#define DMVAE_ABI_VERSION 5\b", hdr)
    from dmvae_hip import augment as A
    assert A.PHILOX_STREAM == AO.STREAM and A.MAX_SIDE == 64
