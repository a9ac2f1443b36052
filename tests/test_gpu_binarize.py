"""dmvae_binarize_rows (csrc/binarize.hip) and its plumbing through Dataset(binarize=...) on the GPU, held bit for bit to the NumPy oracle of
tests/helpers/binarize_oracle.py (exact Philox words, one float32 compare): DESIGN.md section 26."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import binarize_oracle as BO                 # noqa: E402
import binarize_frequency_bound as FB        # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def grey(n, d, seed):
    """values in [0, 1) with exact zeros, as the pixels of an image set"""
    rng = np.random.RandomState(seed)
    return (rng.rand(n, d) * (rng.rand(n, d) < 0.6)).astype(np.float32)


def strided(X, ld, offset=0):
    """X as a view of columns offset .. offset + d of a [n][ld] device buffer filled with NaN between the rows"""
    n, d = X.shape
    buf = torch.full((n, ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, offset:offset + d] = dev(X)
    return buf[:, offset:offset + d], buf


def out_buffer(n, d, ld, offset=0):
    buf = torch.full((n, ld), SENTINEL, dtype=torch.float32, device="cuda")
    return buf[:, offset:offset + d], buf


# 1 x 1 | ragged columns | the product width | unequal strides, groups straddling rows, rows whose offset breaks the 16-byte alignment |
# a flat index past 2^32 | more groups than one sweep of the grid holds (2048 blocks x 256 lanes x 4 elements) with ragged columns
SHAPES = [(1, 1, 1, 1, 0), (3, 5, 5, 5, 0), (7, 784, 784, 784, 0), (33, 130, 192, 136, 0), (5, 70, 70, 70, 62_000_000), (2731, 787, 787, 787, 3)]


@pytest.mark.parametrize("n,d,ldx,ldo,row_base", SHAPES)
def test_bits_equal_the_oracle(n, d, ldx, ldo, row_base):
    from dmvae_hip.binarize import binarize
    X = grey(n, d, 3 + n)
    Xv, _ = strided(X, ldx)
    ov, obuf = out_buffer(n, d, ldo)
    got = binarize(Xv, seed=11, counter=5, row_base=row_base, out=ov)
    assert got is ov
    want = BO.binarize(X, seed=11, counter=5, row_base=row_base)
    host = obuf.cpu().numpy()
    assert np.array_equal(host[:, :d], want)
    assert (host[:, d:] == SENTINEL).all()                       # pad columns of out keep the sentinel
    if n * d > 1000:
        assert 0.1 < want.mean() < 0.5
    fresh = binarize(Xv, seed=11, counter=5, row_base=row_base)  # allocated by the call
    assert fresh.shape == (n, d) and fresh.is_contiguous() and np.array_equal(fresh.cpu().numpy(), want)


@pytest.mark.parametrize("xoff,ooff", [(1, 0), (0, 3), (2, 1)])
def test_misaligned_bases_take_the_scalar_paths(xoff, ooff):
    """a 16-byte-aligned buffer entered at a column offset: every group of X (of out) is misaligned although ld and n_cols are multiples of 4"""
    from dmvae_hip.binarize import binarize
    n, d = 9, 64
    X = grey(n, d, 21)
    Xv, _ = strided(X, 72, xoff)
    ov, obuf = out_buffer(n, d, 72, ooff)
    binarize(Xv, seed=4, counter=1, out=ov)
    host = obuf.cpu().numpy()
    assert np.array_equal(host[:, ooff:ooff + d], BO.binarize(X, seed=4, counter=1))
    assert (host[:, :ooff] == SENTINEL).all() and (host[:, ooff + d:] == SENTINEL).all()


def test_special_inputs():
    from dmvae_hip.binarize import binarize
    row = np.array([0.0, 1.0, -0.25, 1.5, np.nan, 2.0 ** -24, -0.0, np.inf, -np.inf, 0.5], np.float32)
    X = np.tile(row, (64, 1))
    hit_zero = 0
    for counter in range(4):
        got = binarize(dev(X), seed=2, counter=counter).cpu().numpy()
        assert np.array_equal(got, BO.binarize(X, seed=2, counter=counter))
        assert (got[:, 0] == 0).all() and (got[:, 1] == 1).all() and (got[:, 2] == 0).all() and (got[:, 3] == 1).all()      # 0, 1, -0.25, 1.5
        assert (got[:, 4] == 0).all() and (got[:, 6] == 0).all() and (got[:, 7] == 1).all() and (got[:, 8] == 0).all()      # NaN, -0, inf, -inf
        assert np.array_equal(got[:, 5], (BO.uniforms(2, counter, 0, 64, 10)[:, 5] == 0).astype(np.float32))              # 2^-24: on u = 0 alone
        hit_zero += int(got[:, 5].sum())
    assert hit_zero == 0                                          # (no word of these 256 lies below 2^8)
    thr = binarize(dev(X), mode="threshold").cpu().numpy()
    assert np.array_equal(thr, np.tile(np.array([0, 1, 0, 1, 0, 0, 0, 1, 0, 0], np.float32), (64, 1)))


@pytest.mark.parametrize("n,d,ldx,ldo", [(3, 5, 5, 5), (33, 130, 192, 136), (7, 784, 784, 784)])
def test_threshold_mode_is_x_above_one_half(n, d, ldx, ldo):
    from dmvae_hip.binarize import binarize
    X = grey(n, d, 8)
    X[0, :min(d, 3)] = [0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(0.5), np.float32(0))][:min(d, 3)]
    Xv, _ = strided(X, ldx)
    ov, obuf = out_buffer(n, d, ldo)
    binarize(Xv, seed=1, counter=2, row_base=9, mode="threshold", out=ov)     # seed, counter and row_base do not enter
    host = obuf.cpu().numpy()
    assert np.array_equal(host[:, :d], (X > np.float32(0.5)).astype(np.float32)) and (host[:, d:] == SENTINEL).all()
    assert np.array_equal(host[:, :d], BO.binarize(X, mode="threshold"))


def test_same_key_same_bits_other_key_other_bits():
    from dmvae_hip.binarize import binarize
    X = dev(grey(40, 70, 5))
    a, b = binarize(X, seed=3, counter=7), binarize(X, seed=3, counter=7)
    assert torch.equal(a, b)
    assert not torch.equal(a, binarize(X, seed=3, counter=8))
    assert not torch.equal(a, binarize(X, seed=4, counter=7))
    assert not torch.equal(a, binarize(X, seed=3, counter=7, row_base=1))
    assert torch.equal(a, binarize(X, seed=3 + (1 << 64), counter=7))       # the key is 64 bits wide
    assert not torch.equal(a, binarize(X, seed=3 + (1 << 32), counter=7)) and not torch.equal(a, binarize(X, seed=3, counter=7 + (1 << 32)))


@pytest.mark.parametrize("n,d,cut", [(33, 130, 10), (33, 130, 1), (7, 784, 4), (11, 5, 3)])
def test_row_chunks_with_their_row_base_equal_the_whole_call(n, d, cut):
    from dmvae_hip.binarize import binarize
    X = dev(grey(n, d, 6))
    whole = binarize(X, seed=9, counter=2, row_base=100)
    parts = torch.full_like(whole, SENTINEL)
    binarize(X[:cut], seed=9, counter=2, row_base=100, out=parts[:cut])
    binarize(X[cut:], seed=9, counter=2, row_base=100 + cut, out=parts[cut:])
    assert torch.equal(whole, parts)
    assert np.array_equal(whole.cpu().numpy(), BO.binarize(X.cpu().numpy(), seed=9, counter=2, row_base=100))


def test_bad_arguments_are_refused_and_nothing_is_enqueued():
    from dmvae_hip import _lib as L
    from dmvae_hip.binarize import binarize
    n, d, ld = 6, 10, 12
    xb = torch.full((2 * n, ld), 0.75, dtype=torch.float32, device="cuda")
    ob = torch.full((n, ld), SENTINEL, dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    F = 4                                                        # bytes per element

    def call(X=xb.data_ptr(), ldx=ld, n_rows=n, n_cols=d, row_base=0, mode=0, out=ob.data_ptr(), ldo=ld):
        return L.lib.dmvae_binarize_rows(stream, X, ldx, n_rows, n_cols, row_base, 1, 2, mode, out, ldo)

    bad = [(dict(X=None), "null X / out"), (dict(out=None), "null X / out"),
           (dict(n_rows=0), "n_rows=0"), (dict(n_rows=-3), "n_rows=-3"), (dict(n_cols=0), "n_cols=0"), (dict(n_cols=-1), "n_cols=-1"),
           (dict(ldx=d - 1), "ldx=9"), (dict(ldo=d - 1), "ldo=9"), (dict(row_base=-1), "row_base=-1"), (dict(mode=2), "mode=2"), (dict(mode=-1), "mode=-1"),
           (dict(row_base=(1 << 58) // d), "reaches 2\\^58"), (dict(row_base=(1 << 63) - 1), "reaches 2\\^58"),
           (dict(out=xb.data_ptr()), "out overlaps X"),                                        # the same rows
           (dict(out=xb.data_ptr() + F * d), "out overlaps X"),                                # the pad columns of row 0 onwards: inside X's span
           (dict(out=xb.data_ptr() + F * ((n - 1) * ld + d - 1)), "out overlaps X"),           # X's last element
           (dict(X=ob.data_ptr() + F * ((n - 1) * ld + d - 1)), "out overlaps X")]             # out's last element
    for kw, text in bad:
        rc = call(**kw)
        assert rc != 0, kw
        with pytest.raises(L.DmvaeError, match="dmvae_binarize_rows: .*" + text):
            L.check(rc, "dmvae_binarize_rows")
    torch.cuda.synchronize()
    assert (ob == SENTINEL).all() and (xb == 0.75).all()         # a checked return code: nothing ran
    # just clear of X's span is legal: the first byte after X's last element, and rows that END where X begins
    assert call(out=xb.data_ptr() + F * ((n - 1) * ld + d)) == 0
    assert call(X=xb.data_ptr() + F * n * ld, out=xb.data_ptr(), ldo=ld) == 0
    assert call(row_base=(1 << 58) // d - n - 1) == 0            # the largest flat index the entry takes
    torch.cuda.synchronize()
    # the Python surface refuses what is no [rows][columns] f32 device tensor before the library is called
    for X in (torch.zeros(3, 4), torch.zeros(3, 4, device="cuda", dtype=torch.float64), torch.zeros(12, device="cuda"), torch.zeros(4, 3, device="cuda").t()):
        with pytest.raises(ValueError, match="X must be"):
            binarize(X)
    with pytest.raises(ValueError, match="out is"):
        binarize(torch.zeros(3, 4, device="cuda"), out=torch.zeros(3, 5, device="cuda"))
    with pytest.raises(ValueError, match="mode = 'static'"):
        binarize(torch.zeros(3, 4, device="cuda"), mode="static")
    with pytest.raises(L.DmvaeError, match="out overlaps X"):
        x = torch.zeros(3, 4, device="cuda")
        binarize(x, out=x)


# 2 x the oracle's own figure for this input, 0.0839843750: printed by tests/helpers/binarize_frequency_bound.py (CPU, NumPy oracle alone)
FREQUENCY_BOUND = 0.1679687500


def test_frequency_of_the_draws_follows_x():
    """the mean of the draws at counters 0 .. 255 against x, per element of the fixed 4 x 64 input.  The draws are bit-equal to the oracle's
    (asserted here as well), so the deviation is the oracle's and the bound checks the rule, not luck."""
    from dmvae_hip.binarize import binarize
    X = FB.frequency_input()
    assert X.shape == (4, 64) and X.min() > 0 and X.max() < 1
    Xd = dev(X)
    draws = torch.stack([binarize(Xd, seed=0, counter=c) for c in range(FB.N_DRAWS)]).cpu().numpy()
    got = FB.max_deviation(lambda _, c: draws[c])
    print("max |mean - x| = %.10f (bound %.10f)" % (got, FREQUENCY_BOUND))
    assert got <= FREQUENCY_BOUND
    assert all(np.array_equal(draws[c], BO.binarize(X, seed=0, counter=c)) for c in range(FB.N_DRAWS))
    assert got == FREQUENCY_BOUND / 2


# ---------------------------------------------------------------------------------------------------------------- plumbing
I, D, K, B, N = 70, 5, 3, 40, 200


def small_model(seed=3):
    import base_models
    m = base_models.DeepMixtureVAE("dmvae", "binary", I, D, K, activation="relu", initializer="xavier", batch_size=B, dtype="bf16",
                                   enc_layers=(64, 48), head_dim=80, dec_layers=(80, 48, 64), seed=seed).build_graph()
    m.define_train_step(0.002, 1000, 0.9)
    return m


@pytest.fixture(scope="module")
def rows():
    rng = np.random.RandomState(17)
    return grey(N, I, 17), rng.randint(0, K, N)


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in a)


@pytest.mark.parametrize("mode", ["static", "threshold"])
def test_an_epoch_on_a_binarised_set_equals_an_epoch_on_the_oracles_rows(rows, mode):
    from includes.utils import Dataset
    X, cls = rows
    want_rows = BO.binarize(X, seed=7, counter=0, mode="threshold" if mode == "threshold" else "bernoulli")
    out = []
    for kw, data_rows in ((dict(binarize=mode, binarize_seed=7), X), (dict(), want_rows)):
        m = small_model()
        np.random.seed(5)
        data = Dataset((data_rows, cls), batch_size=B, **kw)
        losses = [m.train_op(None, data, 1.0) for _ in range(2)]     # (a static draw is kept: epoch 2 trains on the same rows)
        out.append((losses, m.state_dict(), data.device_rows(m.engine.device).cpu().numpy(), data.data, np.random.get_state()))
    (la, pa, ra, ha, sa), (lb, pb, rb, hb, sb) = out
    assert np.array_equal(ra, want_rows) and np.array_equal(rb, want_rows)
    assert np.array_equal(ha, hb)                                # the host view presents the draw, in the current order
    assert np.isfinite(la).all() and np.array_equal(np.float64(la).view(np.uint64), np.float64(lb).view(np.uint64))
    assert same_bits(pa, pb)
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb))     # and the same NumPy draws were consumed


def test_dynamic_redraws_in_place_and_keeps_the_captured_step(rows):
    from includes.utils import Dataset
    X, cls = rows
    m = small_model()
    dv = m.engine.device
    np.random.seed(5)
    data = Dataset((X, cls), batch_size=B, binarize="dynamic", binarize_seed=9)
    assert data.draw_counter() == 0
    l1 = m.train_op(None, data, 1.0)                             # draw 0, then the epoch's reshuffle: counter 1
    buf, ptr, replay = data.device_rows(dv), data.device_rows(dv).data_ptr(), m._replay
    assert replay is not None and data.draw_counter() == 1
    assert np.array_equal(buf.cpu().numpy(), BO.binarize(X, seed=9, counter=1))      # (device_rows just redrew: the counter was stale)
    l2 = m.train_op(None, data, 1.0)                             # trains on draw 1, reshuffles: counter 2
    assert data.draw_counter() == 2
    trained_on = buf.cpu().numpy().copy()                        # the buffer after epoch 2, before anybody asks for the rows again
    assert np.array_equal(trained_on, BO.binarize(X, seed=9, counter=1))
    assert not np.array_equal(trained_on, BO.binarize(X, seed=9, counter=0))
    assert m._replay is replay                                   # no recapture: the graph holds the buffer's address
    again = data.device_rows(dv)
    assert again is buf and again.data_ptr() == ptr
    assert np.array_equal(again.cpu().numpy(), BO.binarize(X, seed=9, counter=2))
    assert np.array_equal(data.data, BO.binarize(X, seed=9, counter=2)[data.order])
    assert np.isfinite([l1, l2]).all()
    # a set that is never reshuffled keeps one draw: the log-likelihood walks it in its current order
    held = Dataset((X, cls), batch_size=B, shuffle=False, binarize="dynamic", binarize_seed=9)
    first = held.device_rows(dv).cpu().numpy()
    m.get_log_likelihood(None, held, k=2, counter=0)
    assert np.array_equal(held.device_rows(dv).cpu().numpy(), first) and np.array_equal(first, BO.binarize(X, seed=9, counter=0))
    # the grey rows stay resident and untouched beside the draw
    assert np.array_equal(data._device[str(dv)].cpu().numpy(), X)


def test_dynamic_epochs_equal_epochs_on_the_oracles_draws(rows):
    """two epochs under "dynamic" against two one-epoch data sets of the oracle's draws 0 and 1 in the same orders: the redraw is enqueued before
    the steps that read it, and nothing else changes"""
    from includes.utils import Dataset
    X, cls = rows
    m = small_model()
    np.random.seed(5)
    data = Dataset((X, cls), batch_size=B, binarize="dynamic", binarize_seed=9)
    la = [m.train_op(None, data, 1.0) for _ in range(2)]
    pa = m.state_dict()

    m = small_model()
    np.random.seed(5)
    d0 = Dataset((BO.binarize(X, seed=9, counter=0), cls), batch_size=B)
    lb = [m.train_op(None, d0, 1.0)]
    d1 = Dataset((BO.binarize(X, seed=9, counter=1), cls), batch_size=B, shuffle=False)
    d1.order = d0.order.copy()
    d1.shuffle = True                                            # (continues d0's cumulative order with the next NumPy permutation)
    lb.append(m.train_op(None, d1, 1.0))
    assert np.array_equal(np.float64(la).view(np.uint64), np.float64(lb).view(np.uint64))
    assert same_bits(pa, m.state_dict())


def test_log_likelihood_of_a_static_test_set_equals_that_of_the_oracles_rows(rows):
    from includes.utils import Dataset
    X, cls = rows
    m = small_model()
    np.random.seed(6)
    a = Dataset((X, cls), batch_size=B, binarize="static", binarize_seed=2)
    np.random.seed(6)
    b = Dataset((BO.binarize(X, seed=2, counter=0), cls), batch_size=B)
    np.random.seed(6)
    g = Dataset((X, cls), batch_size=B)
    lla, llb, llg = (m.get_log_likelihood(None, ds, k=3, counter=1) for ds in (a, b, g))
    assert np.isfinite(lla) and lla == llb and lla != llg
    acc = []
    for ds in (a, b):                                            # the host evaluation reads the draw too (one reshuffle each, the same one)
        np.random.seed(8)
        acc.append(m.get_accuracy(None, ds))
    assert acc[0] == acc[1] and np.array_equal(a.order, b.order)


def test_off_returns_the_tensor_it_always_did(rows):
    from includes.utils import Dataset
    X, cls = rows
    data = Dataset((X, cls), batch_size=B)
    dv = torch.device("cuda", torch.cuda.current_device())
    t = data.device_rows(dv)
    data.reshuffle()
    assert data.device_rows(dv) is t and t is data._device[str(dv)] and list(data._device) == [str(dv)]
    assert np.array_equal(t.cpu().numpy(), X) and data.binarize == "off"
