"""What the semi-supervised label stage (csrc/label_xent.hip) costs a training step, at the shapes of cfg1 (784-500-500-
2000-10, K = 10, batch 100) and cfg2 (z = 64, batch 4096) of BASELINE.json, bf16, one GPU:

    a step of an un-attached plan | an attached plan at w = 0 | attached, 100 rows of the data set labelled | attached, every row labelled

as the product runs them -- captured steps replayed from the device cursor -- and the stand-alone kernel (dmvae_label_xent) at each batch size
with no row, 100 rows in 70 000 and every row labelled.

    python tools/label_bench.py [--out profiles/label_bench.txt] [--rows 70000] [--steps 200] [--rounds 7]

Method (steady state, spread first): every engine is built and captured once; one untimed round warms every shape; then --rounds rounds, each
visiting the variants in turn (alternating, so that drift of the shared host hits all of them alike), --steps replays per visit between two
HIP events closed by a synchronisation.  Per variant the median of the rounds with min and max: the min..max range of the UN-ATTACHED plan is
the run-to-run spread every difference has to be read against.  The un-attached figure is what bench.py measures for the same shape."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))

CFGS = {"cfg1": dict(batch=100, latent_dim=10, n_classes=10), "cfg2": dict(batch=4096, latent_dim=64, n_classes=10)}


def window(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def fmt(v):
    return "%9.2f us (min %.2f max %.2f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=70000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    from dmvae_hip import StepEngine, _lib
    from includes.utils import choose_labeled, synthetic_images
    assert torch.cuda.is_available(), "label_bench needs a GPU"
    N = a.rows
    X = torch.as_tensor(synthetic_images(N, 784, seed=0)).cuda()
    classes = np.arange(N) % 10
    few = np.full(N, -1, dtype=np.int32)
    idx = choose_labeled(classes, 100, 10, seed=0)
    few[idx] = classes[idx]
    label_sets = {"none": np.full(N, -1, dtype=np.int32), "100": few, "all": classes.astype(np.int32)}
    label_dev = {k: torch.as_tensor(v).cuda() for k, v in label_sets.items()}
    perm = torch.randperm(N, device="cuda").to(torch.int32)
    lines = ["label_bench: %d rows, %d replays per visit, %d rounds (median, min, max); bf16, one GPU" % (N, a.steps, a.rounds)]
    for name, cfg in CFGS.items():
        B = cfg["batch"]
        nb = N // B
        variants = []
        for label, labels, w in (("un-attached", None, None), ("attached, w = 0", "100", 0.0), ("attached, 100 labelled", "100", float(N) / 100.0),
                                 ("attached, all labelled", "all", 1.0)):
            eng = StepEngine(784, cfg["latent_dim"], cfg["n_classes"], dtype="bf16", max_batch=B, labels=None if labels is None else label_dev[labels])
            eng.init_parameters(0)
            eng.reset_epoch(nb)
            if w is not None:
                eng.set_label_weight(w)
            replay = eng.capture_step(X, perm)
            eng.reset_epoch(nb)
            variants.append((label, eng, replay, []))

        def visit(eng, replay, reps):
            left = reps
            t = 0.0
            while left > 0:                          # an epoch holds nb steps: the cursor goes back to 0 outside the timed window
                n = min(left, nb)
                eng.reset_epoch(nb)
                t += window(torch, replay, n) * n
                left -= n
            return t / reps
        for label, eng, replay, _ in variants:       # the untimed round
            visit(eng, replay, min(a.steps, 50))
        for _ in range(a.rounds):
            for label, eng, replay, out in variants:
                out.append(visit(eng, replay, a.steps))
        lines.append("%s (batch %d): one captured step" % (name, B))
        base = statistics.median(variants[0][3])
        for label, eng, replay, out in variants:
            lines.append("  %-24s %s  %+7.2f us against un-attached" % (label, fmt(out), statistics.median(out) - base))
            if eng.labels is not None:
                assert eng.label_err() == 0
        # the stand-alone kernel on a batch of this size
        K = cfg["n_classes"]
        lg = torch.randn(B, 64, device="cuda")
        dl = torch.randn(B, 64, device="cuda").to(torch.bfloat16)
        acc = torch.zeros(int(_lib.lib.dmvae_label_xent_acc_elems(B)), dtype=torch.float64, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        alone = []
        for lname in ("none", "100", "all"):
            lab = label_dev[lname]

            def call():
                _lib.check(_lib.lib.dmvae_label_xent(stream, lg.data_ptr(), 64, B, K, lab.data_ptr(), N, perm.data_ptr(), 0, 1.0 / B, _lib.BF16, dl.data_ptr(), 64,
                                                     None, acc.data_ptr(), err.data_ptr()), "dmvae_label_xent")
            window(torch, call, 50)
            alone.append((lname, [window(torch, call, 10 * a.steps) for _ in range(a.rounds)]))
        for lname, out in alone:
            lines.append("  dmvae_label_xent alone, %4s labelled: %s per launch, back to back" % (lname, fmt(out)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
