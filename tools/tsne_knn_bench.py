"""Times the kNN-sparse t-SNE (dmvae_hip.tsne, method="knn": P over the nearest rows, exact repulsion) -- beside the dense form where that
fits, on the whole-data-set shape where it does not, and beside sklearn's Barnes-Hut on the CPU.

    python tools/tsne_knn_bench.py [--out profiles/tsne_knn.txt] [--repeats 5] [--n_iter 1000] [--big 70000] [--dims 10,64] [--splits 0]
                                   [--sklearn-seconds 600]

Data: 10 clusters, z ~ N(mu_c, I) with mu_c = 4 * randn(D) from a seed, the rows dealt to the clusters in turn -- tsne_bench's data.
Method, as tsne_bench: one warm-up fit, then HIP events around the WHOLE fit -- for the knn form the neighbour search, the conditional p,
the symmetrisation (with its one host read of nnz), the start, the iterations and the KL -- and the median of the repeats; "setup" is the
same call with n_iter = 0, "per iteration" their difference over n_iter.
  1. 10 x 1000 points: the knn form and the dense form in this same run.
  2. --big rows (the model's 70 000: train + test) at every D of --dims: the knn form alone (the dense form stops at 32 768 rows).
  3. sklearn.manifold.TSNE(method="barnes_hut") on the --big rows at the first D, in a child process that is ended after
     --sklearn-seconds (0 leaves it out); the tool says so when it did not finish.
--gpu 0 runs step 3 alone (it needs no GPU)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))


def blobs(N, D, K=10):
    rs = np.random.RandomState(1)
    return (4.0 * rs.randn(K, D)[np.arange(N) % K] + rs.randn(N, D)).astype(np.float32)


def timed(torch, call, repeats):
    """median / min / max milliseconds between two HIP events around call(), after one warm-up; and what the last call returned"""
    call()
    torch.cuda.synchronize()
    ms, out = [], None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms), out


def knn_lines(torch, tsne, Xd, n_iter, repeats, splits):
    N = Xd.shape[0]
    cfg = tsne.knn_config(N, n_iter=n_iter, col_splits=splits)
    ws = tsne.knn_workspace(cfg, Xd.device)
    med, lo, hi, (_, kl) = timed(torch, lambda: tsne.knn_fit(Xd, cfg, ws), repeats)
    cfg0 = tsne.knn_config(N, n_iter=0, col_splits=splits)
    med0, _, _, _ = timed(torch, lambda: tsne.knn_fit(Xd, cfg0, ws), repeats)
    per_us = (med - med0) * 1e3 / max(n_iter, 1)
    pairs = float(N) * N
    return med, ["  knn form, whole fit          %.1f ms   (min %.1f max %.1f)   KL %.4f   k %d   nnz %d   col_splits %s" % (
                     med, lo, hi, float(kl.item()), cfg.k, cfg.nnz, splits or "auto"),
                 "  knn form, setup alone        %.1f ms   (neighbours, conditional p, CSR, start, KL: the same call with n_iter = 0)" % med0,
                 "  knn form, per iteration      %.1f us   (%.2f G pairs: %.2f T pairs/s)" % (per_us, pairs / 1e9, pairs / (per_us * 1e-6) / 1e12)]


def sklearn_child(N, D):
    import warnings
    from sklearn.manifold import TSNE
    X = blobs(N, D)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        sk = TSNE(n_components=2, method="barnes_hut", n_jobs=int(os.environ.get("OMP_NUM_THREADS", "1"))).fit(X)
        print("SKLEARN %.1f %.4f %d" % (time.perf_counter() - t0, sk.kl_divergence_, sk.n_iter_), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n_iter", type=int, default=1000)
    ap.add_argument("--big", type=int, default=70000)
    ap.add_argument("--dims", default="10,64")
    ap.add_argument("--splits", type=int, default=0)
    ap.add_argument("--sklearn-seconds", type=int, default=600)
    ap.add_argument("--gpu", type=int, default=1)
    ap.add_argument("--sklearn-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.sklearn_child:
        N, D = (int(v) for v in a.sklearn_child.split(","))
        return sklearn_child(N, D)
    dims = [int(d) for d in a.dims.split(",")]
    lines = ["tsne_knn_bench: n_iter = %d, perplexity 30; %d repeats after a warm-up (HIP events around the whole fit); medians" % (a.n_iter, a.repeats)]
    if a.gpu:
        import torch
        from dmvae_hip import tsne
        assert torch.cuda.is_available(), "tsne_knn_bench needs a GPU (--gpu 0: the sklearn run alone)"
        D = dims[0]
        Xd = torch.as_tensor(blobs(10000, D)).cuda()
        lines += ["1. 10 x 1000 = 10000 points, D = %d: both forms in this run" % D]
        med_knn, ls = knn_lines(torch, tsne, Xd, a.n_iter, a.repeats, a.splits)
        lines += ls
        cfg = tsne.config(10000, D, n_iter=a.n_iter)
        ws = tsne.workspace(cfg, Xd.device)
        med, lo, hi, (_, kl) = timed(torch, lambda: tsne.fit(Xd, cfg, ws), a.repeats)
        cfg0 = tsne.config(10000, D, n_iter=0)
        med0, _, _, _ = timed(torch, lambda: tsne.fit(Xd, cfg0, ws), a.repeats)
        lines += ["  dense form, whole fit        %.1f ms   (min %.1f max %.1f)   KL %.4f" % (med, lo, hi, float(kl.item())),
                  "  dense form, setup alone      %.1f ms" % med0,
                  "  dense form, per iteration    %.1f us" % ((med - med0) * 1e3 / max(a.n_iter, 1)),
                  "  ratio knn / dense, whole fit %.2f" % (med_knn / med)]
        del ws
        for D in dims:
            Xd = torch.as_tensor(blobs(a.big, D)).cuda()
            lines += ["2. %d rows, D = %d" % (a.big, D)]
            lines += knn_lines(torch, tsne, Xd, a.n_iter, a.repeats, a.splits)[1]
    if a.sklearn_seconds > 0:
        cmd = [sys.executable, os.path.abspath(__file__), "--sklearn-child", "%d,%d" % (a.big, dims[0])]
        threads = os.environ.get("OMP_NUM_THREADS", "unset")
        head = "3. sklearn TSNE(method=\"barnes_hut\") on %d rows, D = %d, OMP_NUM_THREADS=%s:" % (a.big, dims[0], threads)
        t0, out = time.perf_counter(), None
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        while out is None and time.perf_counter() - t0 < a.sklearn_seconds:
            try:
                out = child.communicate(timeout=min(60.0, max(1.0, a.sklearn_seconds - (time.perf_counter() - t0))))[0]
            except subprocess.TimeoutExpired:
                print("  (sklearn: %d s so far)" % (time.perf_counter() - t0), file=sys.stderr, flush=True)
        if out is None:
            child.kill()
            child.communicate()
            lines += ["%s did not end within %d s" % (head, a.sklearn_seconds)]
        else:
            got = [l for l in out.splitlines() if l.startswith("SKLEARN ")]
            lines += ["%s %s s   KL %s   n_iter %s" % ((head,) + tuple(got[-1].split()[1:])) if got else "%s failed" % head]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
