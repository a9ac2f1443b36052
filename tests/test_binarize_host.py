"""CPU tests of the binarisation feature: the oracle's block / word mapping (tests/helpers/binarize_oracle.py), its
independence of chunking, stream 8 against the other rows of the noise table, Dataset(binarize=...) without a device, the CLI flags and the
new entry's declaration / export / binding.  tests/test_gpu_binarize.py holds the kernel and the plumbing to the oracle."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import binarize_oracle as BO      # noqa: E402
import philox_oracle as P         # noqa: E402

# (row_base, n_rows, n_cols) of every call the GPU tests make, and the product sizes (70 000 x 784: train + test rows of MNIST)
SIZES = [(0, 1, 1), (0, 3, 5), (0, 7, 784), (0, 33, 130), (62_000_000, 5, 70), (0, 200, 70), (0, 4, 64), (0, 2731, 787), (0, 70_000, 784)]


@pytest.mark.parametrize("row_base,n_rows,n_cols", [(0, 3, 5), (7, 33, 130), (62_000_000, 5, 70), (3, 1, 1), (2, 4, 7)])
def test_word_and_block_of_every_element(row_base, n_rows, n_cols):
    """element (r, c) reads word idx & 3 of block idx >> 2, idx = (row_base + r) n_cols + c, computed here element by element in Python
    integers; with n_cols no multiple of 4 a block's four words straddle two rows"""
    blk, word = BO.layout(row_base, n_rows, n_cols)
    w = BO.words(9, 4, row_base, n_rows, n_cols)
    u = BO.uniforms(9, 4, row_base, n_rows, n_cols)
    assert u.dtype == np.float32
    for r in range(n_rows):
        for c in range(0, n_cols, max(1, n_cols // 7)):
            idx = (row_base + r) * n_cols + c
            assert (int(blk[r, c]), int(word[r, c])) == (idx >> 2, idx & 3)
            one = int(P.block(9, 4, BO.STREAM, np.uint64(idx >> 2))[idx & 3])
            assert int(w[r, c]) == one
            assert float(u[r, c]) == (one >> 8) * 2.0 ** -24 == float(P.uniform_at(9, 4, BO.STREAM, np.uint64(idx)))
    if n_cols % 4 and n_rows > 1:
        assert any(int(blk[r, n_cols - 1]) == int(blk[r + 1, 0]) for r in range(n_rows - 1))      # a block shared by two rows
    if row_base == 62_000_000:
        assert int(BO.flat_index(row_base, n_rows, n_cols).min()) > 1 << 32


def test_rule_at_the_ends_of_the_grid_and_outside_the_unit_interval():
    X = np.array([[0.0, 1.0, -0.25, 1.5, np.nan, 2.0 ** -24, 0.5, np.float32(0.5) + np.float32(2.0 ** -24)]], np.float32)
    for counter in range(64):
        b = BO.binarize(X, seed=2, counter=counter)
        assert b.dtype == np.float32 and b[0, :5].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0]
        u = BO.uniforms(2, counter, 0, 1, 8)
        assert b[0, 5] == float(u[0, 5] == 0.0)                  # 2^-24 fires on the grid's zero alone
    assert BO.binarize(X, mode="threshold")[0].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def test_chunked_calls_equal_the_whole_call():
    rng = np.random.RandomState(0)
    X = rng.rand(37, 13).astype(np.float32)
    whole = BO.binarize(X, seed=5, counter=3, row_base=11)
    for cut in (1, 10, 36):
        parts = np.concatenate([BO.binarize(X[:cut], seed=5, counter=3, row_base=11), BO.binarize(X[cut:], seed=5, counter=3, row_base=11 + cut)])
        assert np.array_equal(whole, parts)
    assert not np.array_equal(whole, BO.binarize(X, seed=5, counter=3, row_base=12))
    assert not np.array_equal(whole, BO.binarize(X, seed=5, counter=4, row_base=11))
    assert not np.array_equal(whole, BO.binarize(X, seed=6, counter=3, row_base=11))
    assert 0.3 < whole.mean() < 0.7


def test_stream_eight_is_apart_from_every_other_stream_at_the_sizes_used():
    """no (block, word) is drawn twice by a call; every block index stays below 2^56, so the stream id in bits 56 .. 63 of the counter is
    8 and no other; and at one (seed, step) the blocks stream 8 reads share no output with the same block indices of streams 0 .. 7"""
    for row_base, n_rows, n_cols in SIZES:
        last_blk = ((row_base + n_rows) * n_cols - 1) >> 2
        assert last_blk < P.BLK_LIMIT and (row_base + n_rows) * n_cols < BO.FLAT_LIMIT
        if n_rows * n_cols <= 1 << 16:
            blk, word = BO.layout(row_base, n_rows, n_cols)
            key = (blk * np.uint64(4) + word.astype(np.uint64)).reshape(-1)
            assert np.unique(key).size == key.size
            assert int(blk.max()) == last_blk
    assert BO.FLAT_LIMIT >> 2 == P.BLK_LIMIT
    assert BO.STREAM not in (P.STREAM_EPS, P.STREAM_GUMBEL, P.STREAM_EVAL, P.STREAM_GMM_SEED, 4, 5, 6, 7)
    seed, step = 0, 3
    for first in (0, (62_000_000 * 70) >> 2, (70_000 * 784 >> 2) - 2048):
        blk = np.arange(first, first + 2048, dtype=np.uint64)
        mine = {tuple(int(x) for x in r) for r in P.block(seed, step, BO.STREAM, blk)}
        assert len(mine) == 2048
        for sid in range(8):
            other = P.block(seed, step, sid, blk)
            assert not mine & {tuple(int(x) for x in r) for r in other}, sid
            assert (other != P.block(seed, step, BO.STREAM, blk)).any(axis=1).all()


def _numpy_state_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mode", ["off", "static", "dynamic", "threshold"])
def test_dataset_consumes_the_numpy_draws_it_always_did(mode):
    from includes.utils import Dataset
    rng = np.random.RandomState(1)
    X, cls = rng.rand(50, 12).astype(np.float32), rng.randint(0, 3, 50)
    np.random.seed(3)
    ds = Dataset((X, cls), batch_size=20, binarize=mode, binarize_seed=4)
    after_init = np.random.get_state()
    order0 = ds.order.copy()
    ds.reshuffle()
    after_reshuffle = np.random.get_state()
    np.random.seed(3)
    p0 = np.random.permutation(50)
    assert _numpy_state_equal(after_init, np.random.get_state()) and np.array_equal(order0, p0)
    p1 = np.random.permutation(50)
    assert _numpy_state_equal(after_reshuffle, np.random.get_state()) and np.array_equal(ds.order, p0[p1])
    assert ds.binarize == mode and ds.binarize_seed == 4
    assert ds.draw_counter() == (1 if mode == "dynamic" else 0)
    before = np.random.get_state()
    still = Dataset((X, cls), batch_size=20, shuffle=False, binarize=mode)
    still.reshuffle()
    assert _numpy_state_equal(before, np.random.get_state())    # an unshuffled set draws nothing, whatever the mode
    assert np.array_equal(still.order, np.arange(50)) and still.draw_counter() == (1 if mode == "dynamic" else 0)


def test_dataset_off_takes_no_new_code_path(monkeypatch):
    from includes import utils
    rng = np.random.RandomState(2)
    X, cls = rng.rand(30, 8).astype(np.float32), rng.randint(0, 3, 30)

    def never(*a, **k):
        raise AssertionError("binarize='off' asked for the second buffer / the host draw")
    monkeypatch.setattr(utils.Dataset, "_binarized_rows", never)
    ds = utils.Dataset((X, cls), batch_size=10)
    assert ds.binarize == "off"
    rows = ds.device_rows("cpu")
    assert rows is ds.device_rows("cpu") and list(ds._device) == ["cpu"] and np.array_equal(rows.numpy(), X)
    ds.reshuffle()
    assert ds.device_rows("cpu") is rows and list(ds._device) == ["cpu"]
    assert np.array_equal(ds.data, X[ds.order])
    got = np.concatenate(list(ds.get_batches()))
    assert np.array_equal(got, X[ds.order]) and ds.device_rows("cpu") is rows


@pytest.mark.parametrize("mode", ["static", "dynamic", "threshold"])
def test_host_views_refuse_before_a_device_draw_exists(mode):
    from includes.utils import Dataset
    rng = np.random.RandomState(2)
    ds = Dataset((rng.rand(30, 8).astype(np.float32), rng.randint(0, 3, 30)), batch_size=10, binarize=mode)
    with pytest.raises(RuntimeError, match="no device draw exists yet.*no CPU fallback"):
        ds.data
    with pytest.raises(RuntimeError, match="no device draw exists yet"):
        next(ds.get_batches())
    assert len(ds.classes) == 30                                 # the classes are no draw
    with pytest.raises(ValueError, match="binarize = 'bernoulli'"):
        Dataset((rng.rand(3, 2), np.zeros(3)), binarize="bernoulli")


def test_cli_parses_the_flags_and_rejects_them_for_the_moe_models():
    import train
    args = train.parser.parse_args([])
    assert args.binarize == "off" and args.binarize_seed == 0
    for mode in ("off", "static", "dynamic", "threshold"):
        args = train.parser.parse_args(["--binarize", mode, "--binarize_seed", "17"])
        assert args.binarize == mode and args.binarize_seed == 17
    with pytest.raises(SystemExit):
        train.parser.parse_args(["--binarize", "bernoulli"])
    assert "--binarize" in train.__doc__ and "--binarize_seed" in train.__doc__
    for model in ("dmoe", "dvmoe"):
        args = train.parser.parse_args(["--model", model, "--dataset", "synthetic", "--n_epochs", "0", "--binarize", "static"])
        with pytest.raises(ValueError, match="--binarize static with --model %s" % model):
            train.main(args)


def test_entry_is_declared_exported_and_bound():
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    decl = re.search(r"int dmvae_binarize_rows\((.*?)\);", hdr, flags=re.S).group(1)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["stream", "X", "ldx", "n_rows", "n_cols", "row_base", "seed", "counter", "mode", "out", "ldo"]
    assert "dmvae_binarize_rows" in _lib.EXPORTS and len(_lib.lib.dmvae_binarize_rows.argtypes) == len(params)
    assert _lib.lib.dmvae_abi_version() == _lib.ABI_VERSION      # an added entry point, no struct grew: the version stays
    from dmvae_hip import binarize as B
    assert B.PHILOX_STREAM == BO.STREAM and B.MODES == {"bernoulli": 0, "threshold": 1}
