"""Host tests of the device evaluation's Python side (eval="device" / `train.py --eval device`): the Hungarian step factored
out of get_clustering_accuracy / get_moe_clustering_accuracy, the option's parsing and validation, the new C entries."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def confusion(weights, classes, R):
    d = np.zeros((R, R), dtype=np.int64)
    np.add.at(d, (np.argmax(weights, axis=-1), np.asarray(classes, dtype=np.int64)), 1)
    return d


@pytest.mark.parametrize("N,K", [(1, 1), (50, 3), (1000, 10), (777, 50)])
def test_hungarian_helper_equals_get_clustering_accuracy(N, K):
    from includes.utils import accuracy_from_confusion, get_clustering_accuracy
    rng = np.random.RandomState(N + K)
    w, cls = rng.randn(N, K), rng.randint(0, K, N)
    assert accuracy_from_confusion(confusion(w, cls, K), N) == get_clustering_accuracy(w, cls)
    assert accuracy_from_confusion(confusion(w, cls, K).astype(np.int32), N) == get_clustering_accuracy(w, cls)      # as the device returns it


@pytest.mark.parametrize("N,E,C", [(400, 5, 10), (400, 10, 10), (300, 12, 4)])
def test_hungarian_helper_equals_get_moe_clustering_accuracy(N, E, C):
    from includes.utils import accuracy_from_confusion, get_moe_clustering_accuracy
    rng = np.random.RandomState(N + E + C)
    w, cls = rng.randn(N, E), rng.randint(0, C, N)
    cls[0] = C - 1
    assert accuracy_from_confusion(confusion(w, cls, max(E, C)), N) == get_moe_clustering_accuracy(w, cls, C)


def test_perfect_and_permuted_clusterings_score_one():
    from includes.utils import accuracy_from_confusion
    d = np.zeros((4, 4), dtype=np.int64)
    for k, c in enumerate((2, 0, 3, 1)):
        d[k, c] = 5 + k
    assert accuracy_from_confusion(d, d.sum()) == 1.0


def test_cli_eval_flag_defaults_to_host_and_rejects_other_values():
    sys.argv = ["train.py"]
    train = importlib.import_module("train")
    assert train.parser.parse_args([]).eval == "host"
    assert train.parser.parse_args(["--eval", "device"]).eval == "device"
    with pytest.raises(SystemExit):
        train.parser.parse_args(["--eval", "gpu"])


def test_models_take_the_eval_option():
    import base_models
    import models
    kw = dict(activation="relu", initializer="xavier")
    for cls in (base_models.DeepMixtureVAE, base_models.VaDE):
        assert cls("a", "binary", 40, 6, 5, **kw).eval == "host"
        assert cls("a", "binary", 40, 6, 5, eval="device", **kw).eval == "device"
        with pytest.raises(ValueError):
            cls("a", "binary", 40, 6, 5, eval="gpu", **kw)
    assert models.DeepMoE("m", "binary", 40, 3, 5, True).eval == "host"
    assert models.DeepVariationalMoE("m", "binary", 40, 6, 3, 5, True, eval="device").eval == "device"
    with pytest.raises(ValueError):
        models.DeepMoE("m", "binary", 40, 3, 5, True, eval="gpu")


def test_new_entries_are_declared_exported_and_bound():
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    for name, nargs in (("dmvae_confusion_add", 12), ("dmvae_plan_eval_clusters", 14)):
        m = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in _lib.EXPORTS
        fn = getattr(_lib.lib, name)
        assert len(fn.argtypes) == nargs
    assert _lib.ABI_VERSION == 5


def test_datasets_keep_int32_classes_for_the_device():
    from includes.utils import Dataset, MEDataset
    assert callable(Dataset.device_classes) and callable(MEDataset.device_classes)
