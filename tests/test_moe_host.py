"""Host-side tests of the mixture-of-experts models (no GPU): the float64 restatement against torch autograd, the label
generators and MEDataset against the reference's semantics (code/includes/utils.py:37-74, 378-425), the CLI dispatch and the
C ABI of the new entries; and what tests/test_gpu_moe_head.py rests on (tests/helpers/moe_cases.py, moe_oracle.head_f32): the float64
backward of the head is the derivative of its forward at every shape of the GPU tests, the float32 yardstick meets on its own the bars
the kernel is held to, every "trained" classification case is in the regime it is named after, and the arg-max of nearly every row is
decided by more than the yardstick's error (pytest -s prints, per case, the clear-row share, the smallest true-label probability and
max |dq|)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import dmvae_oracle as O      # noqa: E402
import moe_cases as MC        # noqa: E402
import moe_oracle as MO       # noqa: E402


def _torch_head(P, q_logits, Y, classification, n):
    import torch
    P = torch.tensor(P, dtype=torch.float64, requires_grad=True)
    lg = torch.tensor(q_logits, dtype=torch.float64, requires_grad=True)
    Y = torch.tensor(Y, dtype=torch.float64)
    q = torch.softmax(lg, dim=1)
    if classification:
        s = torch.softmax(P, dim=2)
        u = (s * q[:, :, None]).sum(1)
        p = u / u.sum(1, keepdim=True)
        loss = -(Y * torch.log(p + 1e-20)).sum(1).sum() * 1000.0 / n
    else:
        y = (P * q[:, :, None]).sum(1)
        loss = 0.5 * ((y - Y) ** 2).sum() / n
    loss.backward()
    return loss.item(), P.grad.numpy(), lg.grad.numpy()


@pytest.mark.parametrize("classification", [1, 0])
@pytest.mark.parametrize("E,Od,n", [(5, 10, 37), (10, 1, 16), (3, 7, 5)])
def test_head_backward_matches_autograd(classification, E, Od, n):
    rng = np.random.RandomState(E * 100 + Od)
    P = rng.randn(n, E, Od)
    lg = rng.randn(n, E)
    Y = np.eye(Od)[rng.randint(0, Od, n)] if classification else rng.randn(n, Od)
    q = O.softmax(lg)
    r = MO.head_forward(P, q, Y, classification)
    dP, dq = MO.head_backward(r, classification, 1.0 / n)
    dlg = q * (dq - np.sum(q * dq, axis=1, keepdims=True))
    loss, tdP, tdlg = _torch_head(P, lg, Y, classification, n)
    assert abs(r["loss_rows"].sum() / n - loss) <= 1e-9 * max(1.0, abs(loss))
    np.testing.assert_allclose(dP, tdP, rtol=1e-9, atol=1e-12 * max(1.0, np.abs(tdP).max()))
    np.testing.assert_allclose(dlg, tdlg, rtol=1e-9, atol=1e-12 * max(1.0, np.abs(tdlg).max()))


@pytest.mark.parametrize("featLearn", [0, 1])
@pytest.mark.parametrize("lossVAE", [0, 1])
@pytest.mark.parametrize("classification", [1, 0])
@pytest.mark.parametrize("mode", ["exact", "relaxed"])
def test_whole_model_backward_matches_autograd(featLearn, lossVAE, classification, mode):
    """MO.backward (VAE terms + MoE terms through the heads and the trunk) against autograd of the whole MoE loss"""
    import torch
    E, Od, n, I, D = 4, 3, 11, 12, 3
    cfg = O.Config(I, D, E, (9,), 8, (7,), "binary")
    p = O.init_params(cfg, seed=2)
    rng = np.random.RandomState(7)
    p["W_moe"] = rng.randn(D if featLearn else I, E * Od) * 0.3
    p["b_moe"] = rng.randn(E * Od) * 0.1
    p["b_logits"] = rng.randn(E) * 0.5
    X = rng.rand(n, I)
    Y = np.eye(Od)[rng.randint(0, Od, n)] if classification else rng.randn(n, Od)
    eps = rng.randn(n, D)
    gum = O.sample_gumbel((n, E), rng) if mode == "relaxed" else None
    a = MO.forward(p, cfg, X, eps, Y, E, Od, featLearn, classification, lossVAE, kl_ratio=0.6, mode=mode, gumbel=gum)
    g = MO.backward(p, cfg, a, E, Od, featLearn, classification, lossVAE)

    T = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    x = torch.tensor(X)
    relu = torch.relu
    h = relu(x @ T["W_enc0"] + T["b_enc0"])
    zh, ch = relu(h @ T["W_zh"] + T["b_zh"]), relu(h @ T["W_ch"] + T["b_ch"])
    mean, lv, logits = zh @ T["W_mean"] + T["b_mean"], zh @ T["W_logvar"] + T["b_logvar"], ch @ T["W_logits"] + T["b_logits"]
    Z = mean + torch.exp(lv / 2) * torch.tensor(eps)
    xl = relu(Z @ T["W_dec0"] + T["b_dec0"]) @ T["W_out"] + T["b_out"]
    recon = (torch.clamp(xl, min=0) - xl * x + torch.log1p(torch.exp(-xl.abs()))).sum(1).mean()
    q = torch.softmax(logits, 1)
    pm, plv = T["prior_means"], T["prior_log_vars"]
    if mode == "exact":
        w = q
        t = plv[None] - lv[:, None] - 1 + (torch.exp(lv)[:, None] + (mean[:, None] - pm[None]) ** 2) * torch.exp(-plv)[None]
        klz = 0.5 * (w * t.sum(2)).sum(1).mean()
    else:
        w = torch.softmax(logits + torch.tensor(gum), 1)          # Gumbel-Softmax at temperature 1 (priors.py:170-181)
        bpm, bplv = w @ pm, w @ plv
        klz = 0.5 * (bplv - lv - 1 + (torch.exp(lv) + (mean - bpm) ** 2) * torch.exp(-bplv)).sum(1).mean()
    klc = (q * (torch.log(q + 1e-20) + np.log(E))).sum(1).mean()
    vae = recon + 0.6 * (klc + klz)
    inp = relu(mean) if featLearn else x
    P = (inp @ T["W_moe"] + T["b_moe"]).reshape(n, E, Od)
    if classification:
        s = torch.softmax(P, 2)
        u = (s * q[:, :, None]).sum(1)
        pr = u / u.sum(1, keepdim=True)
        lm = -(torch.tensor(Y) * torch.log(pr + 1e-20)).sum(1).mean() * 1000.0
    else:
        lm = 0.5 * (((P * q[:, :, None]).sum(1) - torch.tensor(Y)) ** 2).sum(1).mean()
    total = lm + (vae if lossVAE else 0.0)
    assert abs(float(total) - a["loss_total"]) <= 1e-9 * max(1.0, abs(a["loss_total"]))
    total.backward()
    for k, t in T.items():
        ref = t.grad.numpy() if t.grad is not None else np.zeros_like(p[k])
        np.testing.assert_allclose(g[k], ref, rtol=1e-9, atol=1e-9 * max(1e-12, np.abs(ref).max()), err_msg=k)


def _ds(n_tr=30, n_te=12, I=6, K=4, seed=0):
    import types
    r = np.random.RandomState(seed)
    return types.SimpleNamespace(train_data=r.rand(n_tr, I).astype(np.float32), test_data=r.rand(n_te, I).astype(np.float32),
                                 train_classes=r.randint(0, K, n_tr), test_classes=r.randint(0, K, n_te), n_classes=K)


def test_regression_labels_match_the_reference_formula():
    from includes.utils import generate_regression_variable
    ds = _ds()
    np.random.seed(11)
    tr, te = generate_regression_variable(ds, 3)
    np.random.seed(11)                                       # utils.py:37-59, restated with its [N, O, E_d] tensor
    biases = np.random.randn(3, 4)
    weights = np.random.randn(3, 6, 4)
    full = np.swapaxes(np.matmul(ds.train_data, weights), 0, 1) + biases
    ref_tr = full[range(len(ds.train_data)), :, ds.train_classes]
    full = np.swapaxes(np.matmul(ds.test_data, weights), 0, 1) + biases
    ref_te = full[range(len(ds.test_data)), :, ds.test_classes]
    np.testing.assert_allclose(tr, ref_tr, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(te, ref_te, rtol=1e-5, atol=1e-6)
    assert np.random.rand() == (np.random.seed(11), np.random.randn(3 * 4 + 3 * 6 * 4), np.random.rand())[2]   # same draws consumed


def test_classification_labels_are_one_hot():
    from includes.utils import generate_classification_variables
    ds = _ds()
    tr, te = generate_classification_variables(ds)
    assert tr.shape == (30, 4) and np.array_equal(tr.argmax(1), ds.train_classes) and np.all(tr.sum(1) == 1)
    assert np.array_equal(te.argmax(1), ds.test_classes)


def test_load_data_fills_labels_only_for_moe():
    from includes.utils import load_data
    d = load_data("synthetic", n_train=50, n_test=20)
    assert d.train_labels is None
    d = load_data("synthetic", n_train=50, n_test=20, classification=True, output_dim=1, moe=True)
    assert d.train_labels.shape == (50, 10) and d.test_labels.shape == (20, 10)
    d = load_data("synthetic", n_train=50, n_test=20, classification=False, output_dim=3, moe=True)
    assert d.train_labels.shape == (50, 3)


def test_medataset_draw_order():
    from includes.utils import MEDataset
    X = np.arange(23 * 2, dtype=np.float32).reshape(23, 2)
    cls = np.arange(23) % 5
    lbl = np.arange(23, dtype=np.float32)[:, None] * 10
    np.random.seed(4)
    s0 = np.random.get_state()[1].copy()
    d = MEDataset((X, cls, lbl), batch_size=10)
    assert np.array_equal(np.random.get_state()[1], s0)              # no draw at construction (unlike Dataset)
    np.random.seed(4)
    d = MEDataset((X, cls, lbl), batch_size=10)
    batches = list(d.get_batches())
    np.random.seed(4)
    perm = np.random.permutation(23)                                  # one draw per epoch
    assert [len(b[0]) for b in batches] == [10, 10, 3] and d.epoch_len == 3
    got = np.concatenate([b[0] for b in batches])
    assert np.array_equal(got, X[perm])
    assert np.array_equal(np.concatenate([b[1] for b in batches]), lbl[perm])        # yields (X, labels, classes)
    assert np.array_equal(np.concatenate([b[2] for b in batches]), cls[perm])
    perm2 = np.random.permutation(23)
    np.random.seed(4)
    np.random.permutation(23)
    list(d.get_batches())
    assert np.array_equal(d.data, X[perm][perm2])                     # the second epoch permutes the permuted rows


def test_moe_clustering_accuracy_with_fewer_experts_than_classes():
    from includes.utils import get_moe_clustering_accuracy
    logits = np.eye(5)[np.arange(20) % 5]
    classes = np.arange(20) % 10
    acc = get_moe_clustering_accuracy(logits, classes, 10)
    assert acc == 10 / 20


def test_cli_dispatches_the_moe_models():
    import train
    args = train.parser.parse_args(["--model", "vademoe", "--dataset", "synthetic"])
    with pytest.raises(NotImplementedError):
        train.main(args)
    args = train.parser.parse_args(["--model", "dvmoe", "--dataset", "synthetic", "--classification", "--n_epochs", "0"])
    try:
        train.main(args)
    except NotImplementedError as e:       # (without a GPU it may stop later, at the device session; never at the dispatch)
        pytest.fail("dvmoe raised NotImplementedError: %s" % e)
    except Exception:
        pass
    for flag in ("n_experts", "classification", "output_dim", "featLearn"):
        act = [a for a in train.parser._actions if a.dest == flag][0]
        assert "unused" not in act.help


def test_moe_config_layout_matches_gcc(tmp_path):
    import ctypes as C
    import subprocess
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct dmvae_moe_config \{(.*?)\} dmvae_moe_config;", hdr, flags=re.S).group(1)
    fields = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.MoeConfig._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmvae_hip.h"\nint main(void){printf("%zu", sizeof(dmvae_moe_config));'
                   + "".join('printf(" %%zu", offsetof(dmvae_moe_config, %s));' % f for f in fields) + "return 0;}")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "l")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.MoeConfig)] + [getattr(_lib.MoeConfig, f).offset for f in fields]
    for name in ("dmvae_plan_attach_moe", "dmvae_plan_moe_set_labels", "dmvae_plan_moe_predict"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)


def test_attach_limits_on_the_host():
    """attach is host-only: limits and the arena layout (W_moe last weight matrix, b_moe last bias, non-MoE offsets shifted)"""
    import ctypes as C
    from dmvae_hip import _lib
    cfg = _lib.Config()
    cfg.input_dim, cfg.latent_dim, cfg.n_classes = 784, 8, 10
    cfg.n_enc, cfg.head_dim, cfg.n_dec = 1, 128, 1
    cfg.enc[0] = 128
    cfg.dec[0] = 128
    cfg.dtype, cfg.max_batch = _lib.F32, 100

    def plan():
        h = C.c_void_p()
        _lib.check(_lib.lib.dmvae_plan_create(C.byref(cfg), C.byref(h)))
        return h

    def table(h):
        sz = _lib.Sizes()
        _lib.check(_lib.lib.dmvae_plan_sizes(h, C.byref(sz)))
        t = {}
        for i in range(sz.n_tensors):
            ti = _lib.TensorInfo()
            _lib.check(_lib.lib.dmvae_plan_tensor(h, i, C.byref(ti)))
            t[ti.name.decode()] = (ti.offset, ti.rows, ti.cols, ti.ld)
        return sz, t
    m = _lib.MoeConfig()
    m.n_experts, m.output_dim, m.labels, m.label_rows = 10, 65, 1, 1
    assert _lib.lib.dmvae_plan_attach_moe(plan(), C.byref(m)) == -1
    m.n_experts, m.output_dim = 5, 10
    assert _lib.lib.dmvae_plan_attach_moe(plan(), C.byref(m)) == -1          # E != n_classes
    base = plan()
    s0, t0 = table(base)
    h = plan()
    m.n_experts = 10
    _lib.check(_lib.lib.dmvae_plan_attach_moe(h, C.byref(m)))
    s1, t1 = table(h)
    assert t1["W_moe"][1:] == (784, 100, 128) and t1["b_moe"][1:] == (1, 100, 128)
    wend = max(o + r * ld for k, (o, r, c, ld) in t0.items() if k.startswith("W_"))
    assert t1["W_moe"][0] >= wend - 1 and t1["W_moe"][0] < min(o for k, (o, _, _, _) in t1.items() if k.startswith("b_"))
    assert t1["prior_means"][0] == t1["b_moe"][0] + 128
    assert all(t1[k][0] == t0[k][0] for k in t0 if k.startswith("W_"))      # weights keep their offsets
    assert s1.param_elems > s0.param_elems and s1.work_bytes > s0.work_bytes


# ---- the cases of tests/test_gpu_moe_head.py
CASES = [(s, k, c, f) for s in MC.SHAPES for k in MC.KINDS for c in (1, 0) for f in (0, 1)]
IDS = [MC.case_id(*c) for c in CASES]


def run(shape, kind, classification, featLearn):
    c = MC.get_case(shape, kind, classification, featLearn)
    h = MC.head_inputs(c)
    kw = dict(mean=h["mean"], W=c["params"]["W_moe"], bias=c["params"]["b_moe"]) if featLearn else {}
    o = MC.oracle(h["logits"], h["P"], h["Y"], classification, 1.0 / MC.N, **kw)
    y = MC.yardstick(h["logits"], h["P"], h["Y"], classification, 1.0 / MC.N, **kw)
    return c, h, o, y


@pytest.mark.parametrize("shape", MC.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("classification", [1, 0])
def test_float64_backward_is_the_derivative_of_the_forward(shape, classification):
    """central differences of inv_B sum_b loss_rows in P and in q (q as a free variable, as head_backward takes it), on the mild case: 24 entries
    of each, among them the last expert's last output of the last row.  h = 1e-5 on O(1) inputs: truncation ~1e-10, rounding ~1e-16 L / h ~ 1e-7 of
    a loss of ~1e4 / n -- the bar is 1e-6 of the largest gradient entry plus 1e-7."""
    c = MC.get_case(shape, "mild", classification, 0)
    hin = MC.head_inputs(c)
    P, Y = hin["P"], hin["Y"]
    q = MC.O.softmax(hin["logits"])
    inv_B = 1.0 / MC.N
    f = lambda P_, q_: MO.head_forward(P_, q_, Y, classification)["loss_rows"].sum() * inv_B
    dP, dq = MO.head_backward(MO.head_forward(P, q, Y, classification), classification, inv_B)
    rng = np.random.RandomState(7)
    h = 1e-5
    for arr, grad, which in ((P, dP, 0), (q, dq, 1)):
        idx = [tuple(s - 1 for s in arr.shape)] + [tuple(rng.randint(0, s) for s in arr.shape) for _ in range(23)]
        bar = 1e-6 * np.abs(grad).max() + 1e-7
        for i in idx:
            hi, lo = arr.copy(), arr.copy()
            hi[i] += h
            lo[i] -= h
            fd = ((f(hi, q) - f(lo, q)) if which == 0 else (f(P, hi) - f(P, lo))) / (2 * h)
            assert abs(fd - grad[i]) <= bar, (which, i, fd, grad[i], bar)


def test_dlogits_from_is_the_softmax_backward():
    rng = np.random.RandomState(0)
    lg, dq = rng.randn(6, 9), rng.randn(6, 9)
    q = MC.O.softmax(lg)
    h = 1e-6
    for i in [(0, 0), (3, 8), (5, 4)]:
        hi, lo = lg.copy(), lg.copy()
        hi[i] += h
        lo[i] -= h
        fd = (np.sum(MC.O.softmax(hi) * dq) - np.sum(MC.O.softmax(lo) * dq)) / (2 * h)
        assert abs(fd - MO.dlogits_from(q, dq)[i]) <= 1e-8


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_yardstick_meets_the_bars_on_its_own(case, capsys):
    """head_f32 against the float64 oracle under the project's bars alone (MC.project_bar: no help from itself), and what the case promises"""
    shape, kind, classification, featLearn = case
    c, h, o, y = run(*case)
    names = ("pred", "dP", "dlogits", "loss", "err") + (("P_fl", "gmu") if featLearn else ())
    for k in names:
        rtol, atol = MC.project_bar(k, o[k])
        atol = max(atol, 2.0 ** -126)       # what float32 cannot hold at all: (2, 1, 5) trained regression has max |dlogits| = 1e-77 in the oracle
        ok, err, _ = MC.within(k, y[k], o[k], y[k], tol=(rtol, atol))
        assert ok, (k, err, (rtol, atol))
    if featLearn:       # the collapsed latent dimension: mean = 0.0 exactly, where [mean > 0] and [mean >= 0] differ
        assert not np.any(h["mean"][:, -1]) and np.any(c["params"]["W_moe"][-1]) and not np.any(o["gmu"][:, -1])
    line = MC.case_id(*case)
    if classification:
        clear = MC.clear_rows(o["pred"], y["pred"])
        p_true = np.sum(o["pred"] * h["Y"], axis=1)
        line += ": clear rows %.3f, min true-label p %.2e, max |dq| %.2e, gate weights 0.0f %d" % (
            clear.mean(), p_true.min(), np.abs(o["dq"]).max(), int((y["q"] == 0).sum()))
        assert clear.mean() >= 0.95
        # the yardstick's error count is the oracle's on the clear rows
        assert np.array_equal(y["err_rows"][clear], o["err_rows"][clear])
        if kind == "trained" and shape[1] > 1:          # (O = 1: p = 1 in every row, the loss and every gradient are 0: no regime to be in)
            assert p_true.min() < 1e-30
            assert np.any(y["q"] == 0.0)
            assert np.abs(o["dq"]).max() > 1e15
            wrong = o["err_rows"].sum() / MC.N
            assert 0.05 <= wrong <= 0.2, wrong
        if shape[1] == 1:
            assert o["loss"] == 0.0 and not np.any(o["dP"]) and not np.any(o["dlogits"])
    else:
        line += ": max |pred| %.2e" % np.abs(o["pred"]).max()
    with capsys.disabled():
        print("\n  " + line, end="")


def test_trained_gate_is_one_hot_and_dead_experts_are_zero_in_float32():
    for shape in MC.SHAPES:
        c, h, o, y = run(shape, "trained", 1, 0)
        E = shape[0]
        dead = np.arange(E) >= E - MC.n_dead(E)
        assert not np.any(y["q"][:, dead]) and np.all(o["q"][:, dead] > 0)          # 0.0 in float32, not in the oracle
        if E - MC.n_dead(E) > 1:
            assert np.median(o["q"].max(1)) > 0.99


def test_the_yardstick_sees_a_wrong_kernel():
    """the bars are not vacuous: the algebra with one mistake in it (no `- qdq`; the last output slot dropped from dP) misses them by far"""
    c, h, o, y = run((16, 64, 24), "mild", 0, 0)          # regression: in classification sum_e q dq = sum_o p gp - gpp is analytically 0
    bad = y["q"] * y["dq"]
    assert not MC.within("dlogits", bad, o["dlogits"], y["dlogits"])[0]
    c, h, o, y = run((16, 64, 24), "mild", 1, 0)
    dP = y["dP"].copy()
    dP[:, :, 48:] = 0
    assert not MC.within("dP", dP, o["dP"], y["dP"])[0]
