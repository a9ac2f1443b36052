"""Times one dmvae_binarize_rows pass (csrc/binarize.hip) over the resident rows of MNIST-sized data -- 70 000 x 784 f32, the train + test rows
the dmvae / vade runs hold -- against the torch composition (torch.rand_like(X) < X).float() in the same process, and one training epoch of the
cfg2 model (784-500-500-2000-64, K = 10, batch 4096, bf16) on those rows with Dataset(binarize="dynamic") against binarize="off".

    python tools/binarize_bench.py [--out profiles/binarize.txt] [--rows 70000] [--cols 784] [--repeats 5] [--epochs 5]

The pass reads 4 and writes 4 bytes per element (algorithmic); the fraction of 8 TB/s (the HBM peak of the MI355X) it reaches is reported.
Per mode: one warm call, then --repeats calls between HIP events, each followed by a synchronisation; the median with min and max.  The epochs:
one untimed round (upload), then --epochs rounds over the two data sets in turn; in a round each set runs one untimed epoch (the graph is
recaptured when the rows' buffer changes) and one timed epoch: the epoch's own seconds (train_op's last_epoch: behind the upload, the redraw
and the permutation) and the wall clock around train_op, which holds the redraw; medians."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))

HBM_PEAK = 8.0e12


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def fmt(v, unit="us", scale=1e3):
    return "%.1f %s (min %.1f max %.1f)" % (statistics.median(v) * scale, unit, min(v) * scale, max(v) * scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=70000)
    ap.add_argument("--cols", type=int, default=784)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=5, help="timed epochs per data set; 0 leaves the epochs out")
    a = ap.parse_args()
    import torch
    from dmvae_hip.binarize import binarize
    from includes.utils import Dataset, synthetic_images
    assert torch.cuda.is_available(), "binarize_bench needs a GPU"
    n, d = a.rows, a.cols
    Xh = synthetic_images(n, d, seed=0)
    X = torch.as_tensor(Xh).cuda()
    out = torch.empty_like(X)
    nbytes = 8.0 * n * d
    lines = ["binarize_bench: one pass over %d x %d f32 rows (%.1f MB read + written); one warm call, then %d calls between HIP events, synchronised "
             "(median, min, max)" % (n, d, nbytes / 1e6, a.repeats)]
    runs = [("dmvae_binarize_rows, Bernoulli draw", lambda: binarize(X, seed=0, counter=1, out=out)),
            ("dmvae_binarize_rows, threshold     ", lambda: binarize(X, mode="threshold", out=out)),
            ("(torch.rand_like(X) < X).float()   ", lambda: (torch.rand_like(X) < X).float())]
    med = []
    for name, fn in runs:
        fn()
        torch.cuda.synchronize()
        t = [timed(fn, torch) for _ in range(a.repeats)]
        med.append(statistics.median(t))
        lines.append("  %s  %s   %.2f TB/s = %.2f of 8 TB/s" % (name, fmt(t), nbytes / (med[-1] * 1e-3) / 1e12, nbytes / (med[-1] * 1e-3) / HBM_PEAK))
        print(lines[-1], flush=True)
    lines.append("  torch / Bernoulli draw  %.2f x" % (med[2] / med[0]))
    print(lines[-1], flush=True)
    del out
    if a.epochs > 0:
        import base_models
        cls = np.random.RandomState(0).randint(0, 10, n)
        m = base_models.DeepMixtureVAE("bench", "binary", d, 64, 10, activation="relu", initializer="xavier", batch_size=4096, dtype="bf16",
                                       seed=0).build_graph()
        m.define_train_step(0.002, 1000, 0.9)
        np.random.seed(0)
        sets = {mode: Dataset((Xh, cls), batch_size=4096, binarize=mode) for mode in ("off", "dynamic")}
        own, wall = {k: [] for k in sets}, {k: [] for k in sets}
        for rnd in range(a.epochs + 1):                          # (round 0, untimed: the uploads)
            for mode, ds in sets.items():
                m.train_op(None, ds, 1.0)                        # (the rows' buffer changed: recapture outside the timed epoch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.train_op(None, ds, 1.0)
                w = time.perf_counter() - t0
                if rnd > 0:
                    own[mode].append(m.last_epoch["seconds"])
                    wall[mode].append(w)
        lines.append("one epoch of the cfg2 model (784-500-500-2000-64, K = 10, bf16) on %d rows, batch 4096, %d steps; %d epochs of each data set in turn:"
                     % (n, m.last_epoch["steps"], a.epochs))
        for mode in sets:
            lines.append("  binarize=%-8s steps alone %s   wall clock of train_op %s" % (repr(mode), fmt(own[mode], "ms"), fmt(wall[mode], "ms")))
        lines.append("  dynamic - off, wall clock medians: %+.3f ms (the redraw is one pass per epoch)"
                     % ((statistics.median(wall["dynamic"]) - statistics.median(wall["off"])) * 1e3))
        print("\n".join(lines[-4:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
