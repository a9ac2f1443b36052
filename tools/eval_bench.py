"""Times get_accuracy over one data set with eval="host" (arg-max and confusion matrix in NumPy from scores copied back per batch)
and eval="device" (both on the GPU from the resident rows), in the same process, for DeepMixtureVAE and for VaDE (k = 10 draws).

    python tools/eval_bench.py [--out profiles/eval_accuracy.txt] [--rows 60000] [--batch 100] [--repeats 5]

Data: the synthetic 784-column images (includes.utils.synthetic_images) with classes from a seed; the reference's layer widths,
bf16, device noise.  One warm call per mode first, then the median of the repeats; every call ends in a synchronising read-back,
and the device is synchronised before the clock starts."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))


def timed(model, data, repeats, **kw):
    import torch
    np.random.seed(0)
    acc = model.get_accuracy(None, data, **kw)            # warm call: code objects loaded, rows and classes uploaded
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.get_accuracy(None, data, **kw)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return acc, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import base_models
    from includes.utils import Dataset, synthetic_images
    X = synthetic_images(a.rows, 784, seed=0)
    cls = np.random.RandomState(0).randint(0, 10, a.rows)
    med = statistics.median
    lines = ["eval_bench: get_accuracy over %d x 784 f32 rows, batch %d, K = 10, z = 10, bf16; a warm call, then %d timed calls per mode; seconds" % (
        a.rows, a.batch, a.repeats)]
    for name, cls_, kw in (("DeepMixtureVAE", base_models.DeepMixtureVAE, {}), ("VaDE (k = 10)", base_models.VaDE, {"k": 10})):
        res = {}
        for mode in ("host", "device"):
            np.random.seed(0)
            m = cls_("m", "binary", 784, 10, 10, activation="relu", initializer="xavier", batch_size=a.batch, dtype="bf16", seed=1,
                     eval=mode).build_graph()
            data = Dataset((X, cls), batch_size=a.batch)
            res[mode] = timed(m, data, a.repeats, **kw)
            t = res[mode][1]
            lines.append("%-16s eval=%-6s median %.4f   (min %.4f max %.4f)   accuracy %.4f" % (name, mode, med(t), min(t), max(t), res[mode][0]))
        lines.append("%-16s ratio host / device   %.1f" % (name, med(res["host"][1]) / med(res["device"][1])))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
