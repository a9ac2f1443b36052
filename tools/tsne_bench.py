"""Times the t-SNE of the prior samples' scatter: dmvae_hip.tsne.TSNE (exact, on the device) against the sklearn call cluster_scatter
makes with tsne="host" (Barnes-Hut on the CPU), in the same process.

    python tools/tsne_bench.py [--out profiles/tsne.txt] [--repeats 5] [--sklearn-repeats 1] [--dims 10,64] [--per-cluster 1000]

Data: 10 clusters x --per-cluster samples, z ~ N(mu_c, I) with mu_c = 4 * randn(D) from a seed -- the shape of what mnist_sample_plot
embeds (1000 per cluster: 10 000 points).  Device: one warm-up fit, then HIP events around the whole fit (joint P, 1000 iterations, KL:
everything dmvae_tsne_fit enqueues), the median of the repeats; the per-iteration time is that of a second set of fits with n_iter = 0
subtracted, over n_iter.  The floor quoted beside it is 4 N^2 bytes of P per iteration at 6.29 TB/s.  --sklearn-repeats 0 leaves the
sklearn fit out.  Both KL divergences are printed: the device's is exact, sklearn's is what Barnes-Hut reports."""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))


def device_ms(torch, tsne, Xd, cfg, ws, repeats):
    """median / min / max milliseconds of dmvae_tsne_fit between two HIP events, after one warm-up fit; and the last KL"""
    tsne.fit(Xd, cfg, ws)
    torch.cuda.synchronize()
    ms, kl = [], None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, kl = tsne.fit(Xd, cfg, ws)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms), float(kl.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn-repeats", type=int, default=1)
    ap.add_argument("--dims", default="10,64")
    ap.add_argument("--per-cluster", type=int, default=1000)
    ap.add_argument("--n_iter", type=int, default=1000)
    a = ap.parse_args()
    import torch
    from dmvae_hip import tsne
    assert torch.cuda.is_available(), "tsne_bench needs a GPU"
    K, n = 10, a.per_cluster
    N = K * n
    lines = ["tsne_bench: %d clusters x %d samples = %d points, n_iter = %d, perplexity 30; %d device repeats after a warm-up (HIP events around the "
             "whole fit), %d sklearn run(s); medians" % (K, n, N, a.n_iter, a.repeats, a.sklearn_repeats)]
    for D in [int(d) for d in a.dims.split(",")]:
        rs = np.random.RandomState(1)
        X = (np.repeat(4.0 * rs.randn(K, D), n, axis=0) + rs.randn(N, D)).astype(np.float32)
        Xd = torch.as_tensor(X).cuda()
        cfg = tsne.config(N, D, n_iter=a.n_iter)
        ws = tsne.workspace(cfg, Xd.device)
        med, lo, hi, kl = device_ms(torch, tsne, Xd, cfg, ws, a.repeats)
        cfg0 = tsne.config(N, D, n_iter=0)
        med0, _, _, _ = device_ms(torch, tsne, Xd, cfg0, ws, a.repeats)
        per_iter_us = (med - med0) * 1e3 / max(a.n_iter, 1)
        floor_us = 4.0 * N * N / 6.29e12 * 1e6
        lines += ["D = %d" % D,
                  "  device fit, whole            %.1f ms   (min %.1f max %.1f)   KL %.4f" % (med, lo, hi, kl),
                  "  joint P + start + KL alone   %.1f ms   (the same call with n_iter = 0)" % med0,
                  "  per iteration                %.1f us   (floor: 4 N^2 bytes at 6.29 TB/s = %.1f us)" % (per_iter_us, floor_us)]
        if a.sklearn_repeats > 0:
            from sklearn.manifold import TSNE
            sk_s, sk = [], None
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for _ in range(a.sklearn_repeats):
                    t0 = time.perf_counter()
                    sk = TSNE(n_components=2).fit(X)
                    sk_s.append(time.perf_counter() - t0)
            s = statistics.median(sk_s)
            lines += ["  sklearn TSNE(n_components=2)  %.1f s    (Barnes-Hut, OMP_NUM_THREADS=%s)   KL %.4f   n_iter %d" % (
                          s, os.environ.get("OMP_NUM_THREADS", "unset"), sk.kl_divergence_, sk.n_iter_),
                      "  ratio sklearn / device whole  %.0f" % (s * 1e3 / med)]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
