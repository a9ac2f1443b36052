"""Times dmvae_knn (csrc/knn.hip) against dmvae_silhouette (csrc/cluster_metrics.hip) at the same (N, D) in the same process, and against
sklearn.neighbors.NearestNeighbors(algorithm="brute") on a subset when sklearn imports.

    python tools/knn_bench.py [--out profiles/knn.txt] [--rows 65536] [--dims 64,256] [--k 10] [--repeats 7] [--sklearn-rows 8192]

The two kernels do the same N^2 D distance arithmetic on the same tile; the silhouette adds a square root and float64 sums per pair, the
kNN one compare per pair and rare insertions, so the expectation is kNN <= 1.25 x silhouette (the margin is for the sort passes).  Data:
standard normal rows, ten random labels for the silhouette; self-kNN (M = N, the row itself left out).  Per shape: two warm calls of each,
then --repeats calls of each IN TURN between HIP events, medians reported with min and max.  Also the ranks half of trustworthiness at
(10 000, D, k = 5), the t-SNE scatter's shape, and dmvae_knn_ranks alone there at k = 5, 64 and 256 (its count of compares grows with k).
sklearn runs once in a child process that never opens the GPU."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))

SKLEARN_CHILD = ("import sys, time, numpy as np\nfrom sklearn.neighbors import NearestNeighbors\nX = np.load(sys.argv[1]); k = int(sys.argv[2])\n"
                 "t = time.perf_counter()\nd, i = NearestNeighbors(n_neighbors=k + 1, algorithm='brute').fit(X).kneighbors(X)\n"
                 "sec = time.perf_counter() - t\nnp.save(sys.argv[3], i[:, 1:])\nprint('%.4f' % sec)\n")


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def fmt(v):
    return "%.2f ms (min %.2f max %.2f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="65536")
    ap.add_argument("--dims", default="64,256")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sklearn-rows", type=int, default=8192, help="rows of the subset sklearn searches; 0 leaves sklearn out")
    a = ap.parse_args()
    import torch
    from dmvae_hip import knn, metrics
    assert torch.cuda.is_available(), "knn_bench needs a GPU"
    lines = ["knn_bench: self-kNN (k = %d) of standard normal rows against the silhouette of the same rows under 10 random labels; two warm calls, "
             "then %d calls of each in turn between HIP events (median, min, max)" % (a.k, a.repeats)]
    for n in [int(r) for r in a.rows.split(",")]:
        for D in [int(d) for d in a.dims.split(",")]:
            rng = np.random.RandomState(D)
            Xh = rng.randn(n, D).astype(np.float32)
            X = torch.as_tensor(Xh).cuda()
            labels = torch.as_tensor(rng.randint(0, 10, n).astype(np.int32)).cuda()
            run_knn = lambda: knn.knn_enqueue(X, X, a.k, self_first=0)
            run_sil = lambda: metrics.silhouette_enqueue(X, labels, 10)
            for _ in range(2):
                run_knn(), run_sil()
            torch.cuda.synchronize()
            tk, ts = [], []
            for _ in range(a.repeats):
                tk.append(timed(run_knn, torch))
                ts.append(timed(run_sil, torch))
            ratio = statistics.median(tk) / statistics.median(ts)
            lines += ["N = M = %d, D = %d, k = %d:" % (n, D, a.k),
                      "  dmvae_knn         %s   %.1f G pairs/s" % (fmt(tk), n * float(n) / statistics.median(tk) / 1e6),
                      "  dmvae_silhouette  %s   %.1f G pairs/s" % (fmt(ts), n * float(n) / statistics.median(ts) / 1e6),
                      "  kNN / silhouette  %.3f   (expected <= 1.25)" % ratio]
            print("\n".join(lines[-4:]), flush=True)
            m = min(n, a.sklearn_rows)
            if m > a.k + 1:
                try:
                    import sklearn.neighbors      # noqa: F401
                except ImportError:
                    lines.append("  sklearn NearestNeighbors(brute): not measured, sklearn does not import")
                else:
                    sub = X[:m]
                    run_sub = lambda: knn.knn_enqueue(sub, sub, a.k, self_first=0)
                    run_sub()
                    torch.cuda.synchronize()
                    tsub = [timed(run_sub, torch) for _ in range(a.repeats)]
                    idx = run_sub()[0].cpu().numpy()
                    with tempfile.TemporaryDirectory() as tmp:
                        np.save(os.path.join(tmp, "x.npy"), Xh[:m])
                        r = subprocess.run([sys.executable, "-c", SKLEARN_CHILD, os.path.join(tmp, "x.npy"), str(a.k), os.path.join(tmp, "i.npy")],
                                           capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
                        if r.returncode != 0:
                            lines.append("  sklearn NearestNeighbors(brute) on %d rows: failed: %s" % (m, r.stderr.strip()[-300:]))
                        else:
                            sec = float(r.stdout.split()[-1])
                            same = float(np.mean(np.load(os.path.join(tmp, "i.npy")) == idx))
                            lines.append("  subset of %d rows: dmvae_knn %s, sklearn NearestNeighbors(brute, OMP_NUM_THREADS=%s) %.2f s = %.0f x; %.4f of the "
                                         "indices equal (sklearn expands the norms in f32/f64 and breaks ties its own way)"
                                         % (m, fmt(tsub), os.environ.get("OMP_NUM_THREADS", "unset"), sec, sec * 1e3 / statistics.median(tsub), same))
                    print(lines[-1], flush=True)
            nt = min(n, 10000)
            Xt, Yt = X[:nt], X[:nt, :2].contiguous()
            run_tr = lambda: knn.trustworthiness_terms(Xt, Yt, 5)
            run_tr()
            torch.cuda.synchronize()
            tt = [timed(run_tr, torch) for _ in range(a.repeats)]
            lines.append("  trustworthiness terms (kNN of a 2-D embedding + dmvae_knn_ranks in X) at N = %d, k = 5: %s" % (nt, fmt(tt)))
            print(lines[-1], flush=True)
            # the ranks kernel compares every pair with the 16 k thresholds of its workgroup: its count grows with k beside the D of the distance
            for kr in (5, 64, 256):
                idx_r = knn.knn_enqueue(Yt, Yt, kr, self_first=0)[0]
                run_rk = lambda: knn.ranks_enqueue(Xt, idx_r)
                run_rk()
                torch.cuda.synchronize()
                tr = [timed(run_rk, torch) for _ in range(a.repeats)]
                lines.append("  dmvae_knn_ranks alone at N = %d, k = %d: %s" % (nt, kr, fmt(tr)))
                print(lines[-1], flush=True)
            del X, labels
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
