"""Times get_log_likelihood (the importance-weighted bound on the device, csrc/eval_loglik.hip) over one test set for S = 1, 10, 50
draws against a NumPy float32 restatement of the same estimate on the host, in the same process.

    python tools/loglik_bench.py [--out profiles/loglik.txt] [--rows 10000] [--batch 4096] [--latent 64] [--repeats 5] [--draws 1,10,50]

Data: the synthetic 784-column images (includes.utils.synthetic_images); DeepMixtureVAE with the reference's layer widths, K = 10,
bf16, at its initial parameters.  Device: one warm call, then the median of the repeats; every call ends in its one synchronising
read-back and the device is synchronised before the clock starts.  Host: the encoder once, then per draw the decoder and the row
sums, float32 matrix products on the parameters copied back, NumPy noise; timed once per S (its noise is another sample than the
device's: the two estimates agree to their Monte-Carlo error, which the line reports as the difference)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))


def host_loglik(p, X, S, rng, enc=2, dec=3):
    """float32 NumPy: mean over the rows of logsumexp_s w_s - log S (binary inputs, uniform prior over the clusters)"""
    f = np.float32
    relu = lambda a: np.maximum(a, f(0))
    h = X
    for i in range(enc):
        h = relu(h @ p["W_enc%d" % i] + p["b_enc%d" % i])
    hz = relu(h @ p["W_zh"] + p["b_zh"])
    mean, lv = hz @ p["W_mean"] + p["b_mean"], hz @ p["W_logvar"] + p["b_logvar"]
    sd = np.exp(f(0.5) * lv)
    pm, plv = p["prior_means"], p["prior_log_vars"]
    ip, ck = np.exp(-plv), plv.sum(1)
    m = s = None
    for _ in range(S):
        eps = rng.standard_normal(mean.shape, dtype=f)
        z = mean + sd * eps
        # sum_d (z - mu_k)^2 exp(-lambda_k) as three matrix products
        su = (z * z) @ ip.T - f(2) * (z @ (pm * ip).T) + (pm * pm * ip).sum(1)
        u = f(-0.5) * (su + ck)
        um = u.max(1, keepdims=True)
        lpz = um[:, 0] + np.log(np.exp(u - um).sum(1)) - f(np.log(len(pm)))
        lq = f(-0.5) * (eps * eps + lv).sum(1)
        h = z
        for i in range(dec):
            h = relu(h @ p["W_dec%d" % i] + p["b_dec%d" % i])
        l = h @ p["W_out"] + p["b_out"]
        lpx = (X * l - np.maximum(l, f(0)) - np.log1p(np.exp(-np.abs(l)))).sum(1)
        w = lpx + lpz - lq
        if m is None:
            m, s = w, np.ones_like(w)
        else:
            up = w > m
            s = np.where(up, s * np.exp(m - w) + f(1), s + np.exp(w - m))
            m = np.where(up, w, m)
    return float(np.mean((m + np.log(s) - f(np.log(S))).astype(np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--draws", type=str, default="1,10,50")
    a = ap.parse_args()
    import torch
    import base_models
    from includes.utils import Dataset, synthetic_images
    X = synthetic_images(a.rows, 784, seed=0)
    cls = np.random.RandomState(0).randint(0, 10, a.rows)
    np.random.seed(0)
    m = base_models.DeepMixtureVAE("m", "binary", 784, a.latent, 10, activation="relu", initializer="xavier", batch_size=a.batch, dtype="bf16",
                                   seed=1).build_graph()
    data = Dataset((X, cls), batch_size=a.batch)
    p = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in m.engine.get_parameters().items()}
    Xo = np.ascontiguousarray(X[data.order])
    lines = ["loglik_bench: get_log_likelihood over %d x 784 f32 rows, batch %d, K = 10, z = %d, bf16, reference widths; device: a warm call, then %d "
             "timed calls; host: NumPy float32, one timed call; seconds" % (a.rows, a.batch, a.latent, a.repeats)]
    for S in [int(v) for v in a.draws.split(",")]:
        ll = m.get_log_likelihood(None, data, k=S)              # warm call: code objects loaded, rows uploaded, scratch allocated
        t = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.get_log_likelihood(None, data, k=S)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        lh = host_loglik(p, Xo, S, np.random.default_rng(S))
        th = time.perf_counter() - t0
        med = statistics.median(t)
        lines.append("S = %-3d device median %.5f   (min %.5f max %.5f)   %.1f ns per row and draw   L = %.4f nats per row" % (
            S, med, min(t), max(t), 1e9 * med / (a.rows * S), ll))
        lines.append("S = %-3d host          %.5f   L = %.4f   (device - host %.4f)   ratio host / device %.0f" % (S, th, lh, ll - lh, th / med))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
