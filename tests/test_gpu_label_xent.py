"""GPU tests of the semi-supervised label stage alone (csrc/label_xent.hip through dmvae_label_xent), on caller buffers whose dlogits is
pre-filled with known values:

  shapes     K in {2, 10, 63, 64, 65, 257} (the lane-stride boundaries of a 64-lane wave and more than one trip per lane) x n_valid in
             {1, 37, 64} (a lone row, a ragged last workgroup, sixteen full ones), a non-identity permutation and first = 7; and 300 rows
             = 75 workgroups, more than the 64 that share one ticket (the join then goes through the top ticket)
  labels     none, all, mixed, and the two edge classes 0 and K - 1
  logits     mild N(0, 1), spread over +-80 (a naive float32 softmax overflows), and in every case one row of equal logits, whose arg-max is
             index 0 (np.argmax's rule): counted correct under label 0, not under label K - 1
  bars       f32: tolerance() of tests/helpers/moe_cases.py, the bars of test_gpu_moe_head.py (the project's bar, its absolute part raised to
             twice the float32 yardstick's own error where that is larger); bf16: every stored element within one bf16 ulp of the float64
             result on top of that bar -- test_gpu_moe_head.py's own bar for dlogits.  Everything the stage must not touch is compared by
             bits; the counts are exact; two runs give identical bits; an out-of-range label sets the flag, skips its row and changes
             nothing else.

CPU side: tests/test_label_xent_host.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import label_xent_oracle as LO      # noqa: E402
import moe_cases as MC              # noqa: E402

pytestmark = pytest.mark.gpu

f64 = np.float64
KS = (2, 10, 63, 64, 65, 257)
NS = (1, 37, 64)
PATTERNS = ("none", "all", "mixed", "edges")
REGIMES = ("mild", "spread")
N_DATA, FIRST, EXTRA = 200, 7, 3          # label rows, the batch's offset into the permutation, rows / columns beyond the valid ones


def make_case(K, n, pattern, regime, seed, n_data=N_DATA):
    rng = np.random.RandomState(seed)
    ld_lg, ld_dl = K + 3, K + 5
    lg = (rng.randn(n + EXTRA, ld_lg) if regime == "mild" else rng.uniform(-80.0, 80.0, (n + EXTRA, ld_lg))).astype(np.float32)
    tie = n // 2
    lg[tie, :K] = np.float32(0.75)                       # the row of equal logits
    pre = rng.randn(n + EXTRA, ld_dl).astype(np.float32)
    if pattern == "none":
        y = np.full(n, -1)
    elif pattern == "all":
        y = rng.randint(0, K, n)
        y[tie] = 0                                       # the tie goes to index 0: correct
    elif pattern == "mixed":
        y = np.where(rng.rand(n) < 0.4, rng.randint(0, K, n), -1)
        y[tie] = K - 1                                   # ... and is not K - 1
    else:
        y = np.where(np.arange(n) % 2 == 0, 0, K - 1)
    perm = rng.permutation(n_data).astype(np.int32)
    labels = rng.randint(-1, K, n_data).astype(np.int32)          # what the rest of the data set holds is never read for this batch
    labels[perm[FIRST:FIRST + n]] = y
    return dict(K=K, n=n, n_data=n_data, lg=lg, pre=pre, y=np.asarray(y), perm=perm, labels=labels, ld_lg=ld_lg, ld_dl=ld_dl)


def launch(c, dtype, scale, runs=1, row_loss=True, labels=None):
    """-> (dlogits after [n + EXTRA][ld_dl] torch, acc float64 [6], row_loss f32 [n] or None, flag)"""
    from dmvae_hip import _lib
    n, K = c["n"], c["K"]
    lg = torch.as_tensor(c["lg"]).cuda()
    dl = torch.as_tensor(c["pre"]).cuda().to(dtype)
    lab = torch.as_tensor(c["labels"] if labels is None else labels).cuda()
    perm = torch.as_tensor(c["perm"]).cuda()
    acc = torch.zeros(int(_lib.lib.dmvae_label_xent_acc_elems(n)), dtype=torch.float64, device="cuda")
    rl = torch.full((n + EXTRA,), -7.0, dtype=torch.float32, device="cuda") if row_loss else None
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    for _ in range(runs):
        rc = _lib.lib.dmvae_label_xent(torch.cuda.current_stream().cuda_stream, lg.data_ptr(), c["ld_lg"], n, K, lab.data_ptr(), c["n_data"], perm.data_ptr(), FIRST,
                                       float(scale), _lib.BF16 if dtype == torch.bfloat16 else _lib.F32, dl.data_ptr(), c["ld_dl"],
                                       rl.data_ptr() if row_loss else None, acc.data_ptr(), err.data_ptr())
        assert rc == 0, _lib.lib.dmvae_last_error()
    torch.cuda.synchronize()
    a = acc.cpu().numpy()
    assert not np.any(a[6:])                             # tickets and partial slots are back at zero
    if row_loss:
        assert bool((rl[n:] == -7.0).all())              # rows beyond n_valid are not written
    return dl, a[:6].copy(), (rl[:n].cpu().numpy() if row_loss else None), int(err.item())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check(c, dtype, scale=0.8125):
    n, K = c["n"], c["K"]
    pre_t = torch.as_tensor(c["pre"]).cuda().to(dtype)
    pre = pre_t.float().cpu().numpy().astype(f64)        # (bf16: the rounded pre-fill is the known value)
    got_t, acc, rl, flag = launch(c, dtype, scale)
    got = got_t.float().cpu().numpy().astype(f64)
    o, y32 = LO.term(c["lg"][:n, :K], c["y"], scale), LO.term_f32(c["lg"][:n, :K], c["y"], scale)
    lab = o["labelled"]
    assert flag == 0
    # what must keep its bits: rows without a label, rows >= n_valid, columns >= K
    keep = torch.ones_like(pre_t, dtype=torch.bool)
    keep[:n, :K] = torch.as_tensor(~lab).cuda()[:, None]
    assert torch.equal(bits(got_t)[keep], bits(pre_t)[keep])
    # the labelled rows against the float64 result
    want = pre[:n, :K] + o["d"]
    yard = (pre[:n, :K].astype(np.float32) + y32["d"]).astype(f64)
    if lab.any():
        rtol, atol = MC.tolerance("dlogits", want[lab], yard[lab])
        e = np.abs(got[:n, :K] - want)[lab]
        lim = atol + rtol * np.abs(want[lab]) + (MC.bf16_ulp(want[lab]) if dtype == torch.bfloat16 else 0.0)
        print("label_xent K=%d n=%d %s dlogits error %.3e yardstick %.3e atol %.3e" % (K, n, str(dtype)[6:], e.max(), MC.yard_error(want[lab], yard[lab]), atol))
        assert np.all(np.isfinite(got)) and np.all(e <= lim), (float(e.max()), np.unravel_index(np.argmax(e - lim), e.shape))
    # loss per row and summed, counts exact
    rtol, atol = MC.tolerance("loss", o["loss_rows"], y32["loss_rows"])
    assert np.all(np.abs(rl - o["loss_rows"]) <= atol + rtol * np.abs(o["loss_rows"])) and not rl[~lab].any()
    rtol, atol = MC.tolerance("loss", o["loss"], float(y32["loss_rows"].astype(f64).sum()))
    assert abs(acc[3] - o["loss"]) <= atol + rtol * abs(o["loss"]), (acc[3], o["loss"])
    assert acc[3] == float(rl.astype(f64).sum()) or abs(acc[3] - rl.astype(f64).sum()) <= 1e-12 * max(1.0, abs(acc[3]))      # float64 sums of the same float32 terms
    assert (acc[4], acc[5]) == (o["n_labelled"], o["n_correct"]) and np.array_equal(acc[:3], acc[3:])
    return o


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", KS)
def test_stage_against_the_oracle(K, dtype):
    seed = 0
    for n in NS:
        for pattern in PATTERNS:
            for regime in REGIMES:
                seed += 1
                o = check(make_case(K, n, pattern, regime, 1000 * K + seed), dtype)
                tie = n // 2
                if pattern == "all":
                    assert o["correct"][tie]             # equal logits, label 0
                if pattern == "mixed":
                    assert o["labelled"][tie] and not o["correct"][tie]
                if pattern == "none":
                    assert o["n_labelled"] == 0 and o["loss"] == 0.0


@pytest.mark.parametrize("pattern", ["mixed", "all", "none"])
def test_more_workgroups_than_one_ticket_group(pattern):
    """300 rows = 75 workgroups: a full group of 64 and one of 11 behind it, joined by the top ticket"""
    c = make_case(10, 300, pattern, "mild", 8, n_data=400)
    check(c, torch.float32)
    a, b = launch(c, torch.float32, 0.3, runs=2), launch(c, torch.float32, 0.3, runs=2)
    assert torch.equal(bits(a[0]), bits(b[0])) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[1][:3], 2.0 * a[1][3:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_two_runs_give_the_same_bits_and_the_epoch_sums_add_up(dtype):
    c = make_case(65, 37, "mixed", "spread", 5)
    a = launch(c, dtype, 0.3)
    b = launch(c, dtype, 0.3)
    assert torch.equal(bits(a[0]), bits(b[0])) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    twice = launch(c, dtype, 0.3, runs=2)
    assert np.array_equal(twice[1][:3], 2.0 * a[1][3:]) and np.array_equal(twice[1][3:], a[1][3:])      # epoch slots add, batch slots are the last launch's
    no_rows = launch(c, dtype, 0.3, row_loss=False)
    assert torch.equal(bits(no_rows[0]), bits(a[0])) and no_rows[1].tobytes() == a[1].tobytes()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_zero_coefficient_writes_nothing(dtype):
    c = make_case(10, 37, "all", "mild", 6)
    c["pre"][:, :] = -0.0                                # a sum with +0 would flip these signs
    dl, acc, rl, flag = launch(c, dtype, 0.0)
    assert torch.equal(bits(dl), bits(torch.as_tensor(c["pre"]).cuda().to(dtype))) and flag == 0
    assert acc[4] == 37 and acc[3] > 0                   # the loss is still measured


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_an_out_of_range_label_is_flagged_and_skipped(dtype):
    c = make_case(10, 37, "all", "mild", 7)
    rows = c["perm"][FIRST:FIRST + 37]
    bad, clean = c["labels"].copy(), c["labels"].copy()
    bad[rows[3]], bad[rows[20]] = 10, -2                 # K and below -1
    clean[rows[3]] = clean[rows[20]] = -1
    a = launch(c, dtype, 0.5, labels=bad)
    b = launch(c, dtype, 0.5, labels=clean)
    assert a[3] == 1 and b[3] == 0
    assert torch.equal(bits(a[0]), bits(b[0])) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    pre = torch.as_tensor(c["pre"]).cuda().to(dtype)
    assert torch.equal(bits(a[0])[[3, 20]], bits(pre)[[3, 20]]) and a[1][4] == 35
    # a permutation entry outside the label array: bit 1, the row skipped
    c2 = make_case(10, 37, "all", "mild", 7)
    c2["perm"][FIRST + 5] = N_DATA
    d = launch(c2, dtype, 0.5)
    assert d[3] == 2 and d[1][4] == 36 and torch.equal(bits(d[0])[5], bits(pre)[5])
