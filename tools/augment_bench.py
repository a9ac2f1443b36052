"""Times one dmvae_augment_rows pass (csrc/augment.hip) over the resident rows of MNIST-sized data -- 70 000 x 784 f32 as 28 x 28 images, the
train + test rows the dmvae / vade runs hold -- against dmvae_binarize_rows on the same rows in the same run (the yardstick: the same 8 bytes
per element), against the torch composition affine_grid + grid_sample on the same maps, and one training epoch of the cfg2 model
(784-500-500-2000-64, K = 10, batch 4096, bf16) on those rows with Dataset(augment=...) against a plain epoch.

    python tools/augment_bench.py [--out profiles/augment.txt] [--rows 70000] [--side 28] [--repeats 5] [--epochs 5] [--spec SPEC]

The pass reads 4 and writes 4 bytes per element (algorithmic); the fraction of 8 TB/s (the HBM peak of the MI355X) it reaches is reported.
Per row: one warm call, then --repeats calls between HIP events, each followed by a synchronisation; the median with min and max.  The torch
composition is handed the kernel's own maps, converted to normalised units outside the timed region.  The epochs: as tools/binarize_bench.py
-- one untimed round (upload), then --epochs rounds over the two data sets in turn; in a round each set runs one untimed epoch (the graph is
recaptured when the rows' buffer changes) and one timed epoch: the epoch's own seconds and the wall clock around train_op, which holds the
redraw; medians."""
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


def normalised(theta, H, W):
    """the [n][2][3] matrices affine_grid(align_corners=True) takes for the pixel-unit sampling maps theta [n][6]"""
    m = theta.double().view(-1, 2, 3)
    ax, ay = (W - 1) / 2.0, (H - 1) / 2.0
    out = m.clone()
    out[:, 0, 1] = m[:, 0, 1] * ay / ax
    out[:, 0, 2] = (m[:, 0, 0] * ax + m[:, 0, 1] * ay + m[:, 0, 2]) / ax - 1.0
    out[:, 1, 0] = m[:, 1, 0] * ax / ay
    out[:, 1, 2] = (m[:, 1, 0] * ax + m[:, 1, 1] * ay + m[:, 1, 2]) / ay - 1.0
    return out.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=70000)
    ap.add_argument("--side", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=5, help="timed epochs per data set; 0 leaves the epochs out")
    ap.add_argument("--spec", default="rotate=10,translate=2,scale=0.9:1.1,shear=5")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from dmvae_hip.augment import augment, parse_augment
    from dmvae_hip.binarize import binarize
    from includes.utils import Dataset, synthetic_images
    assert torch.cuda.is_available(), "augment_bench needs a GPU"
    n, H, W = a.rows, a.side, a.side
    d = H * W
    spec = parse_augment(a.spec)
    Xh = synthetic_images(n, d, seed=0)
    X = torch.as_tensor(Xh).cuda()
    out = torch.empty_like(X)
    _, theta = augment(X, spec, seed=0, counter=1, out=out, return_theta=True)
    tn = normalised(theta, H, W)
    ref = F.grid_sample(X.view(n, 1, H, W), F.affine_grid(tn, (n, 1, H, W), align_corners=True), mode="bilinear", padding_mode="zeros", align_corners=True)
    gap = float((ref.view(n, d) - out).abs().max())
    nbytes = 8.0 * n * d
    lines = ["augment_bench: one pass over %d x %d f32 rows as %d x %d images (%.1f MB read + written), spec %s; one warm call, then %d calls between HIP "
             "events, synchronised (median, min, max)" % (n, d, H, W, nbytes / 1e6, spec, a.repeats),
             "  max |kernel - grid_sample| on these rows: %.3e" % gap]
    runs = [("dmvae_augment_rows, drawn maps         ", lambda: augment(X, spec, seed=0, counter=1, out=out)),
            ("dmvae_augment_rows, given maps         ", lambda: augment(X, spec, theta=theta, out=out)),
            ("dmvae_binarize_rows, Bernoulli draw    ", lambda: binarize(X, seed=0, counter=1, out=out)),
            ("affine_grid + grid_sample (torch)      ", lambda: F.grid_sample(X.view(n, 1, H, W), F.affine_grid(tn, (n, 1, H, W), align_corners=True), mode="bilinear",
                                                                              padding_mode="zeros", align_corners=True))]
    med = []
    for name, fn in runs:
        fn()
        torch.cuda.synchronize()
        t = [timed(fn, torch) for _ in range(a.repeats)]
        med.append(statistics.median(t))
        lines.append("  %s  %s   %.2f TB/s = %.2f of 8 TB/s" % (name, fmt(t), nbytes / (med[-1] * 1e-3) / 1e12, nbytes / (med[-1] * 1e-3) / HBM_PEAK))
        print(lines[-1], flush=True)
    lines.append("  augment / binarize  %.2f x      torch / augment  %.2f x" % (med[0] / med[2], med[3] / med[0]))
    print(lines[-1], flush=True)
    del out, ref
    if a.epochs > 0:
        import base_models
        cls = np.random.RandomState(0).randint(0, 10, n)
        m = base_models.DeepMixtureVAE("bench", "binary", d, 64, 10, activation="relu", initializer="xavier", batch_size=4096, dtype="bf16",
                                       seed=0).build_graph()
        m.define_train_step(0.002, 1000, 0.9)
        np.random.seed(0)
        sets = {"plain": Dataset((Xh, cls), batch_size=4096), "augment": Dataset((Xh, cls), batch_size=4096, augment=spec)}
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
        lines.append("one epoch of the cfg2 model (%d-500-500-2000-64, K = 10, bf16) on %d rows, batch 4096, %d steps; %d epochs of each data set in turn:"
                     % (d, n, m.last_epoch["steps"], a.epochs))
        for mode in sets:
            lines.append("  %-8s steps alone %s   wall clock of train_op %s" % (mode, fmt(own[mode], "ms"), fmt(wall[mode], "ms")))
        lines.append("  augment - plain, wall clock medians: %+.3f ms (the redraw is one pass per epoch)"
                     % ((statistics.median(wall["augment"]) - statistics.median(wall["plain"])) * 1e3))
        print("\n".join(lines[-4:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
