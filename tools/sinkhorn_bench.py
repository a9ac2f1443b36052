"""Times one dmvae_sinkhorn_softmin pass (csrc/sinkhorn.hip) against dmvae_prdc_counts on the same rows (csrc/prdc.hip: the same tile body,
so the ratio isolates the price of the exponential and the double sum) and against a torch composition of the same pass (torch.cdist^2 on
2048-row chunks + logsumexp) at the same (N = M, D) in the same process.

    python tools/sinkhorn_bench.py [--out profiles/sinkhorn.txt] [--rows 10000,65536] [--dims 64,256] [--repeats 7] [--model-rows 10000]

Expectation, written down before the first run: per pair the pass adds to the tile's 2 D vector instructions an fma, a
subtraction, a multiply and one v_exp_f32 (the issue cost of two), a conversion, two compares, a double-precision fma and add (half rate) and
five selects -- some 20 instruction slots against the counts kernel's 10 or so -- at the same 4 workgroups per CU: softmin / counts about
1.10 at D = 64 and about 1.03 at D = 256.  Data: standard normal rows against 0.5 + 0.8 x standard normal, eps = 0.05 x the mean cost, random potentials of size 3 eps.
Per shape: two warm calls of each, then --repeats calls of each IN TURN between HIP events, medians reported with min and max.  Also a whole
get_sample_distance (features, three transport problems, the read-backs) of the MNIST-sized bf16 model on --model-rows synthetic rows, wall
clock around the call, with its iteration counts."""
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
    return "%.2f ms (min %.2f max %.2f)" % (statistics.median(v), min(v), max(v))


def torch_softmin(X, Y, eps, g, torch, chunk=2048):
    """the same pass by torch.cdist on chunks of the rows (cdist expands the norms: not the same bits); uniform weights"""
    h = g / eps - float(np.log(Y.shape[0]))
    return torch.cat([-eps * torch.logsumexp(h[None, :] - torch.cdist(X[s:s + chunk], Y) ** 2 / eps, dim=1) for s in range(0, X.shape[0], chunk)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="10000,65536")
    ap.add_argument("--dims", default="64,256")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--model-rows", type=int, default=10000, help="rows of the whole get_sample_distance; 0 leaves it out")
    a = ap.parse_args()
    import torch
    from dmvae_hip import prdc, sinkhorn
    assert torch.cuda.is_available(), "sinkhorn_bench needs a GPU"
    lines = ["sinkhorn_bench: one dmvae_sinkhorn_softmin pass against dmvae_prdc_counts of the same rows and a torch.cdist + logsumexp composition; two "
             "warm calls, then %d calls of each in turn between HIP events (median, min, max)" % a.repeats]
    for n in [int(r) for r in a.rows.split(",")]:
        for D in [int(d) for d in a.dims.split(",")]:
            rng = np.random.RandomState(D)
            X = torch.as_tensor(rng.randn(n, D).astype(np.float32)).cuda()
            Y = torch.as_tensor((0.5 + 0.8 * rng.randn(n, D)).astype(np.float32)).cuda()
            eps = 0.05 * float(sinkhorn.scale_and_mean_cost(X, Y)[1])
            g = torch.as_tensor((3.0 * eps * rng.randn(n)).astype(np.float32)).cuda()
            out = torch.empty(n, dtype=torch.float32, device="cuda")
            rX2, rY2 = prdc.radii_enqueue(X, 5), prdc.radii_enqueue(Y, 5)
            run_pass = lambda: sinkhorn.softmin_enqueue(X, Y, eps, g=g, out=out)
            run_prdc = lambda: prdc.counts_enqueue(X, Y, rX2, rY2)
            run_torch = lambda: torch_softmin(X, Y, eps, g, torch)
            for _ in range(2):
                run_pass(), run_prdc(), run_torch()
            torch.cuda.synchronize()
            tp, tk, tt = [], [], []
            for _ in range(a.repeats):
                tp.append(timed(run_pass, torch))
                tk.append(timed(run_prdc, torch))
                tt.append(timed(run_torch, torch))
            mp, mk, mt = statistics.median(tp), statistics.median(tk), statistics.median(tt)
            got, ref = run_pass().double(), run_torch().double()
            lines += ["N = M = %d, D = %d, eps = %.4g:" % (n, D, eps),
                      "  dmvae_sinkhorn_softmin  %s   %.1f G pairs/s" % (fmt(tp), n * float(n) / mp / 1e6),
                      "  dmvae_prdc_counts       %s   %.1f G pairs/s" % (fmt(tk), n * float(n) / mk / 1e6),
                      "  torch.cdist + logsumexp %s" % fmt(tt),
                      "  softmin / counts  %.3f;  torch / softmin  %.1f x;  max |softmin - torch's| = %.2e of eps (cdist expands the norms)"
                      % (mp / mk, mt / mp, float((got - ref).abs().max()) / eps)]
            print("\n".join(lines[-5:]), flush=True)
            del X, Y
    if a.model_rows > 0:
        import base_models
        from includes.utils import Dataset
        rng = np.random.RandomState(0)
        X = (rng.rand(a.model_rows, 784) < 0.2).astype(np.float32)
        data = Dataset((X, rng.randint(0, 10, a.model_rows)), batch_size=1000, shuffle=False)
        m = base_models.DeepMixtureVAE("bench", "binary", 784, 10, 10, activation="relu", initializer="xavier", batch_size=1000, dtype="bf16", seed=0,
                                       eval="device").build_graph()
        for space in ("latent", "input"):
            res = m.get_sample_distance(None, data, space=space)
            torch.cuda.synchronize()
            t = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                m.get_sample_distance(None, data, space=space)
                t.append((time.perf_counter() - t0) * 1e3)
            lines.append("get_sample_distance(space=%r) of %d rows against %d samples, 784-500-500-2000-10 bf16 model, batch 1000, wall clock: %s; "
                         "S_eps = %.5g, iterations %s, residuals %s" % (space, a.model_rows, a.model_rows, fmt(t), res["divergence"], res["n_iter"],
                                                                        ["%.1e" % e for e in res["err"]]))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
