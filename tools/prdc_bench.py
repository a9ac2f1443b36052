"""Times dmvae_prdc_counts (csrc/prdc.hip) against dmvae_knn self-kNN of the same rows (csrc/knn.hip) and against a torch composition
(torch.cdist plus comparisons, chunked to fit) at the same (N = M, D) in the same process.

    python tools/prdc_bench.py [--out profiles/prdc.txt] [--rows 10000,65536] [--dims 64,256] [--k 5] [--repeats 7] [--model-rows 10000]

The pairs kernel does the same 16 x 256 x D fused multiply-adds per tile as knn_pairs_kernel on the same tile body; it replaces the select
with two compares and an occasional integer atomic and has 4 workgroups per CU against 3, so the expectation is prdc <= 1.10 x kNN (the
spread of a shared pool).  Data: standard normal real rows, generated rows 0.5 + 0.8 x standard normal; radii from dmvae_knn at k.  Per
shape: two warm calls of each, then --repeats calls of each IN TURN between HIP events, medians reported with min and max.  Also a whole
get_sample_quality (two self-kNNs, the pairs kernel, decode and re-encode) of the MNIST-sized bf16 model on --model-rows synthetic rows,
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
    return "%.2f ms (min %.2f max %.2f)" % (statistics.median(v), min(v), max(v))


def torch_counts(R, F, rR2, rF2, torch, chunk=2048):
    """the same four vectors by torch.cdist on chunks of the real rows (cdist expands the norms: not the same bits)"""
    fake_in_real = torch.zeros(F.shape[0], dtype=torch.int32, device=R.device)
    rif, mn, mj = [], [], []
    for s in range(0, R.shape[0], chunk):
        d2 = torch.cdist(R[s:s + chunk], F) ** 2
        fake_in_real += (d2 <= rR2[s:s + chunk, None]).sum(dim=0, dtype=torch.int32)
        rif.append((d2 <= rF2[None, :]).sum(dim=1, dtype=torch.int32))
        m = d2.min(dim=1)
        mn.append(m.values)
        mj.append(m.indices)
    return fake_in_real, torch.cat(rif), torch.cat(mn), torch.cat(mj)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="10000,65536")
    ap.add_argument("--dims", default="64,256")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--model-rows", type=int, default=10000, help="rows of the whole get_sample_quality; 0 leaves it out")
    a = ap.parse_args()
    import torch
    from dmvae_hip import knn, prdc
    assert torch.cuda.is_available(), "prdc_bench needs a GPU"
    lines = ["prdc_bench: dmvae_prdc_counts against dmvae_knn self-kNN (k = %d) of the real rows and a torch.cdist composition; two warm calls, "
             "then %d calls of each in turn between HIP events (median, min, max)" % (a.k, a.repeats)]
    for n in [int(r) for r in a.rows.split(",")]:
        for D in [int(d) for d in a.dims.split(",")]:
            rng = np.random.RandomState(D)
            R = torch.as_tensor(rng.randn(n, D).astype(np.float32)).cuda()
            F = torch.as_tensor((0.5 + 0.8 * rng.randn(n, D)).astype(np.float32)).cuda()
            rR2, rF2 = prdc.radii_enqueue(R, a.k), prdc.radii_enqueue(F, a.k)
            run_prdc = lambda: prdc.counts_enqueue(R, F, rR2, rF2)
            run_knn = lambda: knn.knn_enqueue(R, R, a.k, self_first=0)
            run_torch = lambda: torch_counts(R, F, rR2, rF2, torch)
            for _ in range(2):
                run_prdc(), run_knn(), run_torch()
            torch.cuda.synchronize()
            tp, tk, tt = [], [], []
            for _ in range(a.repeats):
                tp.append(timed(run_prdc, torch))
                tk.append(timed(run_knn, torch))
                tt.append(timed(run_torch, torch))
            mp, mk, mt = statistics.median(tp), statistics.median(tk), statistics.median(tt)
            got, ref = run_prdc(), run_torch()
            same = [float((g == r).float().mean()) for g, r in zip(got[:2], ref[:2])]
            lines += ["N = M = %d, D = %d, k = %d:" % (n, D, a.k),
                      "  dmvae_prdc_counts  %s   %.1f G pairs/s" % (fmt(tp), n * float(n) / mp / 1e6),
                      "  dmvae_knn (self)   %s   %.1f G pairs/s" % (fmt(tk), n * float(n) / mk / 1e6),
                      "  torch.cdist + compares  %s" % fmt(tt),
                      "  prdc / kNN  %.3f   (expected <= 1.10);  torch / prdc  %.1f x;  %.4f / %.4f of fake_in_real / real_in_fake equal torch's "
                      "(cdist expands the norms)" % (mp / mk, mt / mp, same[0], same[1])]
            print("\n".join(lines[-5:]), flush=True)
            del R, F
    if a.model_rows > 0:
        import base_models
        from includes.utils import Dataset
        rng = np.random.RandomState(0)
        X = (rng.rand(a.model_rows, 784) < 0.2).astype(np.float32)
        data = Dataset((X, rng.randint(0, 10, a.model_rows)), batch_size=1000, shuffle=False)
        m = base_models.DeepMixtureVAE("bench", "binary", 784, 10, 10, activation="relu", initializer="xavier", batch_size=1000, dtype="bf16", seed=0,
                                       eval="device").build_graph()
        for space in ("latent", "input"):
            m.get_sample_quality(None, data, k=a.k, space=space)
            torch.cuda.synchronize()
            t = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                m.get_sample_quality(None, data, k=a.k, space=space)
                t.append((time.perf_counter() - t0) * 1e3)
            lines.append("get_sample_quality(space=%r) of %d rows against %d samples, 784-500-500-2000-10 bf16 model, batch 1000, wall clock: %s"
                         % (space, a.model_rows, a.model_rows, fmt(t)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
