"""Times dmvae_ssim_rows (csrc/ssim.hip) against the usual torch composition of SSIM -- five conv2d moment maps (x, y, xx, yy, xy) under
the same 2-D weights, the second moments as E[x^2] - mu^2 -- at the same rows in the same process, and counts how often the two differ.

    python tools/ssim_bench.py [--out profiles/ssim.txt] [--repeats 7] [--model-rows 10000]

Shapes: 10 000 and 65 536 pairs of 28 x 28, 10 000 pairs of 3 x 32 x 32, the 11-tap Gaussian window.  Rows are MNIST-like (19 % of the
pixels set, blurred, scaled to [0, 1]); the other side is the row plus clipped noise of strength 0.1.  Per shape: two warm calls of each,
then --repeats calls of each IN TURN between HIP events, medians reported with min and max.  The kernel walks every window twice over
121 taps -- about 10 f32 operations per tap and window -- so 324 windows of a 28 x 28 pair cost about 4e5 operations: the expectation
held against the measurement is under 1 ms for 10 000 pairs and no slower than the torch composition, which streams five maps through HBM.
Then the differences: the share of rows whose torch SSIM is further than 1e-4 from the kernel's (the E[x^2] - mu^2 form cancels against
c2 = 9e-4 in flat regions away from 0; the kernel's centred moments do not), with the largest difference, on the rows as they are (flat
regions at exactly 0, where nothing cancels) and inverted (flat regions at 1).  Last, a whole
get_reconstruction_quality (gather, encode, decode, copy, SSIM per batch) of the MNIST-sized bf16 model on --model-rows synthetic rows,
wall clock around the call (it ends in its one copy back)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def fmt(v):
    return "%.3f ms (min %.3f max %.3f)" % (statistics.median(v), min(v), max(v))


def mnist_like(n, planes, H, W, torch, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    img = (torch.rand((n * planes, 1, H, W), device="cuda", generator=g) < 0.19).float()
    k = torch.tensor([0.25, 0.5, 0.25], device="cuda")
    k2 = (k[:, None] * k[None, :]).view(1, 1, 3, 3)
    img = torch.nn.functional.conv2d(torch.nn.functional.pad(img, (1, 1, 1, 1), mode="replicate"), k2)
    img = img / img.amax(dim=(2, 3), keepdim=True).clamp_min(1e-20)
    return img.view(n, planes * H * W).contiguous()


def torch_ssim(X, Y, shape, g2, c1, c2, torch, chunk=16384):
    """the five-conv2d composition, per-row mean over the valid windows of all planes"""
    planes, H, W = shape
    out = []
    for s in range(0, X.shape[0], chunk):
        x, y = X[s:s + chunk].view(-1, 1, H, W), Y[s:s + chunk].view(-1, 1, H, W)
        conv = lambda v: torch.nn.functional.conv2d(v, g2)
        mx, my = conv(x), conv(y)
        sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
        S = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
        out.append(S.view(-1, planes * S.shape[2] * S.shape[3]).mean(dim=1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--model-rows", type=int, default=10000, help="rows of the whole get_reconstruction_quality; 0 leaves it out")
    a = ap.parse_args()
    import torch
    from dmvae_hip import ssim as S
    assert torch.cuda.is_available(), "ssim_bench needs a GPU"
    w = S.gaussian_window()
    c1, c2 = S.constants()
    wt = torch.as_tensor(w).cuda()
    g2 = (wt[:, None] * wt[None, :]).view(1, 1, 11, 11)
    lines = ["ssim_bench: dmvae_ssim_rows against five torch conv2d moment maps (E[x^2] - mu^2), 11-tap Gaussian window; two warm calls, then "
             "%d calls of each in turn between HIP events (median, min, max)" % a.repeats]
    for n, shape in ((10000, (1, 28, 28)), (65536, (1, 28, 28)), (10000, (3, 32, 32))):
        X = mnist_like(n, *shape, torch, seed=n)
        Y = (X + 0.1 * torch.randn(X.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))).clamp_(0.0, 1.0)
        run_hip = lambda: S.ssim_enqueue(X, Y, shape)
        run_torch = lambda: torch_ssim(X, Y, shape, g2, c1, c2, torch)
        for _ in range(2):
            run_hip(), run_torch()
        torch.cuda.synchronize()
        th, tt = [], []
        for _ in range(a.repeats):
            th.append(timed(run_hip, torch))
            tt.append(timed(run_torch, torch))
        mh, mt = statistics.median(th), statistics.median(tt)
        got, ref = run_hip()[0].double(), run_torch().double()
        diff = (got - ref).abs()
        ones = S.ssim_enqueue(X, X, shape)[0]
        ones_t = torch_ssim(X, X, shape, g2, c1, c2, torch)
        inv = ((1.0 - X).contiguous(), (1.0 - Y).contiguous())      # white background: the flat regions sit at 1, where x^2 and mu^2 are near 1
        diff_inv = (S.ssim_enqueue(inv[0], inv[1], shape)[0].double() - torch_ssim(inv[0], inv[1], shape, g2, c1, c2, torch).double()).abs()
        windows = n * shape[0] * (shape[1] - 10) * (shape[2] - 10)
        lines += ["%d pairs of %s:" % (n, " x ".join(str(v) for v in shape)),
                  "  dmvae_ssim_rows   %s   %.2f G windows/s" % (fmt(th), windows / mh / 1e6),
                  "  torch, 5 conv2d   %s" % fmt(tt),
                  "  torch / HIP  %.2f x;  rows further than 1e-4 apart: %.4f of them, largest difference %.3g (mean SSIM %.4f)"
                  % (mt / mh, float((diff > 1e-4).double().mean()), float(diff.max()), float(got.mean())),
                  "  the same rows inverted (1 - x, flat regions at 1): %.4f of them further than 1e-4 apart, largest difference %.3g"
                  % (float((diff_inv > 1e-4).double().mean()), float(diff_inv.max())),
                  "  a row against itself: HIP %.4f of the rows are 1.0 in bits, torch %.4f (largest |1 - ssim| %.3g)"
                  % (float((ones == 1.0).double().mean()), float((ones_t == 1.0).double().mean()), float((ones_t.double() - 1.0).abs().max()))]
        print("\n".join(lines[-6:]), flush=True)
        del X, Y
    if a.model_rows > 0:
        import base_models
        from includes.utils import Dataset
        X = mnist_like(a.model_rows, 1, 28, 28, torch, seed=0).cpu().numpy()
        data = Dataset((X, np.random.RandomState(0).randint(0, 10, a.model_rows)), batch_size=1000, shuffle=False)
        m = base_models.DeepMixtureVAE("bench", "binary", 784, 10, 10, activation="relu", initializer="xavier", batch_size=1000, dtype="bf16", seed=0,
                                       eval="device").build_graph()
        m.get_reconstruction_quality(None, data)
        torch.cuda.synchronize()
        t = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            m.get_reconstruction_quality(None, data)
            t.append((time.perf_counter() - t0) * 1e3)
        lines.append("get_reconstruction_quality of %d rows, 784-500-500-2000-10 bf16 model, batch 1000, wall clock: %s" % (a.model_rows, fmt(t)))
        print(lines[-1], flush=True)
        m.get_sample_diversity(None, n_per_cluster=32)
        torch.cuda.synchronize()
        t = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            m.get_sample_diversity(None, n_per_cluster=32)
            t.append((time.perf_counter() - t0) * 1e3)
        lines.append("get_sample_diversity, 32 draws of each of 10 components (4960 + 1440 comparisons), same model, wall clock: %s" % fmt(t))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
