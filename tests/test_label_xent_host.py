"""Host-side tests of the semi-supervised label term (csrc/label_xent.hip): the entries are declared, exported and bound
at ABI 5, dmvae_label_xent refuses every bad argument by name before anything is enqueued, label_xent.hip compiles for gfx950 without a
spill or scratch, the CLI flags parse, choose_labeled / Dataset(labeled=) keep their promises, VaDE and the MoE classes refuse, and the
float64 oracle the GPU tests lean on (tests/helpers/label_xent_oracle.py) agrees with a brute-force double loop and a hand-worked row."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import label_xent_oracle as LO      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-mixture-vae_amd")
ENTRIES = {"dmvae_label_xent": 16, "dmvae_label_xent_acc_elems": 1, "dmvae_plan_attach_labels": 2, "dmvae_plan_set_labels": 3}


def test_entries_are_declared_exported_and_bound():
    from dmvae_hip import _lib
    hdr_full = open(os.path.join(ROOT, "include", "dmvae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    declared = set(re.findall(r"\b(dmvae_[a-z0-9_]+)\s*\(", hdr))
    for name, nargs in ENTRIES.items():
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert len(getattr(_lib.lib, name).argtypes) == nargs, name
    assert _lib.ABI_VERSION == 5 and _lib.lib.dmvae_abi_version() == 5 and "#define DMVAE_ABI_VERSION 5" in hdr_full      # entries are only added
    assert "typedef struct dmvae_label_config" in hdr and '"label_xent.hip"' in open(os.path.join(PKG, "build.py")).read()
    assert "SERVED" in hdr_full and "np.argmax" in hdr_full      # the header says what staged / prefetched passes do and which tie rule holds
    import ctypes as C
    assert C.sizeof(_lib.LabelConfig) == 24
    # four rows per workgroup: eight leading doubles, sixteen per group of 64 workgroups (its ticket's line), then a triple per workgroup
    assert [_lib.lib.dmvae_label_xent_acc_elems(n) for n in (0, 1, 4, 5, 64, 256, 257)] == [8, 27, 27, 30, 72, 216, 235]
    from dmvae_hip import StepEngine
    for m in ("set_labels", "set_label_weight", "label_acc", "zero_label_acc"):
        assert callable(getattr(StepEngine, m))


def test_bad_arguments_are_refused_by_name_before_anything_is_enqueued():
    from dmvae_hip import _lib
    f = _lib.lib.dmvae_label_xent
    keep = [np.zeros(64, dtype=np.float32) for _ in range(6)]     # host memory: a refused call touches none of it
    lg, lab, perm, dl, acc, err = [b.ctypes.data for b in keep]
    good = dict(logits=lg, ld_lg=4, n_valid=4, K=4, labels=lab, label_rows=8, perm=perm, first=0, scale=1.0, act=0, dl=dl, ld_dl=4, row_loss=None,
                acc=acc, err=err)
    bad = (dict(logits=None), dict(labels=None), dict(dl=None), dict(acc=None), dict(err=None), dict(K=0), dict(n_valid=-1), dict(ld_lg=3),
           dict(ld_dl=3), dict(label_rows=0), dict(act=2), dict(act=-1), dict(scale=float("nan")), dict(scale=float("inf")), dict(first=-1),
           dict(perm=None, first=5), dict(perm=None, n_valid=9, label_rows=8))
    named = ("logits", "labels", "dlogits", "acc", "err_flag", "K", "n_valid", "ld_lg", "ld_dl", "label_rows", "act_dtype", "act_dtype", "scale", "scale",
             "first", "perm", "perm")
    for change, word in zip(bad, named):
        a = dict(good, **change)
        rc = f(None, a["logits"], a["ld_lg"], a["n_valid"], a["K"], a["labels"], a["label_rows"], a["perm"], a["first"], a["scale"], a["act"],
               a["dl"], a["ld_dl"], a["row_loss"], a["acc"], a["err"])
        msg = _lib.lib.dmvae_last_error()
        assert rc == -1, change                                  # DMVAE_EINVAL
        assert b"dmvae_label_xent" in msg and word.encode() in msg, (change, msg)
    assert all(not b.any() for b in keep)


def test_label_xent_hip_compiles_without_spill_or_scratch(tmp_path):
    out = tmp_path / "label_xent.s"
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-mllvm",
                        "-amdgpu-mfma-vgpr-form=1", "-S", "--cuda-device-only", os.path.join(PKG, "csrc", "label_xent.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    txt = out.read_text()
    assert "label_xent_kernel" in txt
    assert set(re.findall(r"\.vgpr_spill_count: +\d+", txt)) == {".vgpr_spill_count: 0"}
    assert set(re.findall(r"\.private_segment_fixed_size: +\d+", txt)) == {".private_segment_fixed_size: 0"}


def test_cli_flags_parse():
    import train
    d = train.parser.parse_args([])
    assert d.n_labeled == 0 and d.label_weight == 1.0 and d.label_seed == 0
    a = train.parser.parse_args(["--n_labeled", "100", "--label_weight", "0.5", "--label_seed", "3"])
    assert (a.n_labeled, a.label_weight, a.label_seed) == (100, 0.5, 3)
    assert "--n_labeled" in (train.__doc__ or "")


def test_choose_labeled_is_stratified_repeatable_and_leaves_the_global_stream():
    from includes.utils import choose_labeled
    rng = np.random.RandomState(5)
    classes = rng.randint(0, 10, 700)
    np.random.seed(11)
    before = np.random.get_state()
    a = choose_labeled(classes, 103, 10, seed=2)
    b = choose_labeled(classes, 103, 10, seed=2)
    c = choose_labeled(classes, 103, 10, seed=3)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert len(a) == 103 == len(np.unique(a)) and np.all(np.diff(a) > 0)
    # 103 // 10 = 10 each, the remainder 3 to the classes 0, 1, 2
    assert np.bincount(classes[a], minlength=10).tolist() == [11, 11, 11] + [10] * 7
    sub = np.arange(300)
    s = choose_labeled(classes, 20, 10, seed=2, rows=sub)
    assert s.max() < 300 and np.bincount(classes[s], minlength=10).tolist() == [2] * 10
    assert len(choose_labeled(classes, 0, 10, seed=0)) == 0
    short = np.array([0, 0, 0, 1, 2])
    with pytest.raises(ValueError, match="class 1"):
        choose_labeled(short, 6, 3, seed=0)


def test_dataset_labels_survive_reshuffles():
    from includes.utils import Dataset, choose_labeled
    rng = np.random.RandomState(6)
    X, cls = rng.rand(50, 7).astype(np.float32), rng.randint(0, 4, 50)
    lab = choose_labeled(cls, 8, 4, seed=1)
    np.random.seed(0)
    ds = Dataset((X, cls), batch_size=16, labeled=lab)
    want = np.full(50, -1, dtype=np.int32)
    want[lab] = cls[lab]
    assert ds.n_labeled == 8 and np.array_equal(ds.labeled, lab)
    for _ in range(3):
        y = ds.host_labels()
        assert y.dtype == np.int32 and np.array_equal(y, want)          # indexed by data-set row: the order does not enter
        assert np.array_equal(y[ds.order][ds.classes != y[ds.order]], np.full(42, -1))
        ds.reshuffle()
    plain = Dataset((X, cls), batch_size=16)
    assert plain.labeled is None and plain.n_labeled == 0 and np.array_equal(plain.host_labels(), np.full(50, -1))
    with pytest.raises(ValueError):
        Dataset((X, cls), batch_size=16, labeled=[50])


def test_vade_and_the_moe_classes_refuse():
    import base_models
    import models
    with pytest.raises(NotImplementedError, match="p\\(c\\|z\\)"):
        base_models.VaDE("v", "binary", 20, 3, 4, label_weight=1.0)
    for cls, args in ((models.DeepMoE, ("m", "binary", 20, 2, 4, True)), (models.DeepVariationalMoE, ("m", "binary", 20, 3, 2, 4, True))):
        with pytest.raises((TypeError, NotImplementedError)):
            cls(*args, label_weight=1.0)
    m = base_models.DeepMixtureVAE("d", "binary", 20, 3, 4, label_weight=0.5)          # nothing is built before build_graph
    assert m.label_weight == 0.5 and base_models.DeepMixtureVAE("d", "binary", 20, 3, 4).label_weight is None
    assert callable(base_models.DeepMixtureVAE.get_direct_accuracy)


def brute(logits, y, coef):
    n, K = len(logits), len(logits[0])
    loss, d, nl, nc = [0.0] * n, [[0.0] * K for _ in range(n)], 0, 0
    for r in range(n):
        if y[r] < 0 or y[r] >= K:
            continue
        mx = max(logits[r])
        se = sum(math.exp(v - mx) for v in logits[r])
        loss[r] = math.log(se) + mx - logits[r][y[r]]
        for k in range(K):
            d[r][k] = coef * (math.exp(logits[r][k] - mx) / se - (1.0 if k == y[r] else 0.0))
        nl += 1
        nc += logits[r].index(mx) == y[r]
    return loss, d, nl, nc


def test_oracle_against_a_brute_force_double_loop():
    rng = np.random.RandomState(0)
    for K in (2, 5, 65):
        lg = rng.randn(9, K) * 3.0
        lg[4] = 1.5                                              # a row of equal logits: arg-max 0
        y = rng.randint(-1, K, 9)
        y[4], y[5], y[6] = 0, -1, K                              # the tie counts as correct for label 0; no label; out of range
        loss, d, nl, nc = brute(lg.tolist(), y.tolist(), 0.37)
        t = LO.term(lg, y, 0.37)
        assert np.allclose(t["loss_rows"], loss, rtol=1e-13, atol=1e-13) and np.allclose(t["d"], d, rtol=1e-13, atol=1e-15)
        assert (t["n_labelled"], t["n_correct"]) == (nl, nc) and t["correct"][4] and not t["labelled"][5] and not t["labelled"][6]
        assert t["bad"].tolist() == [False] * 6 + [True] + [False] * 2
        assert not t["d"][5].any() and not t["d"][6].any() and abs(t["d"][t["labelled"]].sum(axis=1)).max() < 1e-15
        y32 = LO.term_f32(lg, y, 0.37)
        assert y32["d"].dtype == np.float32 and np.abs(y32["d"] - t["d"]).max() < 1e-6
    big = np.array([[80.0, -80.0, 0.0], [-80.0, 80.0, 79.0]])    # a naive softmax overflows in float32
    t, y32 = LO.term(big, [1, 1], 1.0), LO.term_f32(big, [1, 1], 1.0)
    assert np.all(np.isfinite(y32["d"])) and abs(t["loss_rows"][0] - 160.0) < 1e-12 and np.allclose(y32["loss_rows"], t["loss_rows"], rtol=1e-6)


def test_oracle_on_a_hand_worked_row():
    # logits (0, ln 3), label 0: q = (1/4, 3/4), l = ln 4, coefficient 2: d = 2 (1/4 - 1, 3/4) = (-3/2, 3/2); arg-max 1: not correct
    t = LO.term(np.array([[0.0, math.log(3.0)]]), [0], 2.0)
    assert abs(t["loss_rows"][0] - math.log(4.0)) < 1e-15 and np.allclose(t["d"][0], [-1.5, 1.5], rtol=0, atol=1e-15)
    assert t["n_labelled"] == 1 and t["n_correct"] == 0
    assert LO.batch_labels(np.array([5, 6, 7, 8]), np.array([3, 2, 1, 0]), 1, 2).tolist() == [7, 6]
    assert LO.coefficient(3.0, 1.0 / 6.0) == float(np.float32(3.0) * np.float32(1.0 / 6.0))
