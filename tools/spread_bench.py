"""Times label spreading on the device (csrc/label_spread.hip, dmvae_hip/spread.py) part by part, against the same iteration composed from
torch.sparse on the same device in the same process, and against sklearn's LabelSpreading with a callable kernel on a host copy where its
dense N x N matrix still fits.

    python tools/spread_bench.py [--out profiles/label_spread.txt] [--shapes 10000x10,10000x64,70000x10,70000x64] [--repeats 7] [--sklearn_max_n 10000]

Rows: Gaussian blobs, C = 10 classes, centres 3 sigma apart, 100 labels (ten per class), k = 7, alpha = 0.8, connectivity weights.
Per shape, after two warm calls of everything, --repeats calls of each IN TURN between HIP events (median, min, max):
  the neighbour search (dmvae_knn), the symmetrisation (tsne.knn_symmetrize, torch sorts), the normalisation (two launches), one call of
  dmvae_label_spread with 64 iterations (per iteration: that over 64; the one-iteration call beside it shows the launch floor), the same 64
  iterations as torch.sparse CSR x dense + axpy + max |F' - F|, and the whole LabelSpreading.fit by the host clock around a synchronise.
sklearn runs once in a child process that never opens the GPU, with the same W handed over as CSR."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))

C_CLASSES, K_NEIGH, ALPHA, CHUNK = 10, 7, 0.8, 64

SKLEARN_CHILD = """import sys, time, numpy as np
from sklearn.semi_supervised import LabelSpreading
d = np.load(sys.argv[1])
N = len(d['y'])
W = np.zeros((N, N))
W[np.repeat(np.arange(N), np.diff(d['indptr'])), d['indices']] = d['values']
t = time.perf_counter()
ls = LabelSpreading(kernel=lambda A, B: W, alpha=float(sys.argv[2]), max_iter=1000, tol=1e-6).fit(d['X'], d['y'])
sec = time.perf_counter() - t
print('%.4f %d %.6f' % (sec, ls.n_iter_, float(np.mean(ls.transduction_ == d['cls']))))
np.save(sys.argv[3], ls.transduction_)
"""


def blobs(N, D, seed):
    rng = np.random.RandomState(seed)
    cls = np.arange(N) % C_CLASSES
    cen = np.zeros((C_CLASSES, D))
    cen[np.arange(C_CLASSES), np.arange(C_CLASSES) % D] = (3.0 / np.sqrt(2.0)) * (1 + np.arange(C_CLASSES) // D)
    return (cen[cls] + rng.randn(N, D)).astype(np.float32), cls


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def fmt(v, per=1):
    return "%.1f us (min %.1f max %.1f)" % (1e3 * statistics.median(v) / per, 1e3 * min(v) / per, 1e3 * max(v) / per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="10000x10,10000x64,70000x10,70000x64")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sklearn_max_n", type=int, default=10000)
    a = ap.parse_args()
    import torch
    from dmvae_hip import spread
    from dmvae_hip.knn import knn_enqueue
    from dmvae_hip.tsne import knn_symmetrize
    assert torch.cuda.is_available(), "spread_bench needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = ["spread_bench: C = %d, k = %d, alpha = %g, 100 labels; two warm calls, then %d calls of each in turn between HIP events (median, min, max)"
             % (C_CLASSES, K_NEIGH, ALPHA, a.repeats)]
    for N, D in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]:
        Xh, cls = blobs(N, D, D)
        yh = np.full(N, -1, dtype=np.int64)
        yh[:100] = cls[:100]
        X, y = torch.as_tensor(Xh).to(dev), torch.as_tensor(yh.astype(np.int32)).to(dev)
        idx, d2 = knn_enqueue(X, X, K_NEIGH, self_first=0)
        indptr, indices, values = knn_symmetrize(idx, torch.ones_like(d2))
        s, _, _ = spread.sym_normalize_enqueue(indptr, indices, values)
        nnz, deg = int(indices.numel()), (indptr[1:] - indptr[:-1])
        F = torch.empty((N, C_CLASSES), dtype=torch.float32, device=dev)
        change = torch.empty(CHUNK, dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = spread.workspace(N, C_CLASSES, dev)
        S = torch.sparse_csr_tensor(indptr, indices.long(), s, size=(N, N))
        base = (1.0 - ALPHA) * torch.nn.functional.one_hot(y.long().clamp(min=0), C_CLASSES).float() * (y >= 0).float()[:, None]
        tchange = torch.empty(CHUNK, dtype=torch.float32, device=dev)

        def run_torch(n):
            Ft = torch.zeros((N, C_CLASSES), dtype=torch.float32, device=dev)
            for t in range(n):
                Fn = torch.add(base, S @ Ft, alpha=ALPHA)
                tchange[t] = (Fn - Ft).abs().max()
                Ft = Fn
            return Ft

        runs = {
            "dmvae_knn (k = %d)" % K_NEIGH: lambda: knn_enqueue(X, X, K_NEIGH, self_first=0),
            "knn_symmetrize (torch sorts, one read)": lambda: knn_symmetrize(idx, torch.ones_like(d2)),
            "dmvae_graph_sym_normalize": lambda: spread.sym_normalize_enqueue(indptr, indices, values, flag),
            "dmvae_label_spread, 1 iteration": lambda: spread.spread_enqueue(indptr, indices, s, y, C_CLASSES, ALPHA, 1, F, change, ws, flag),
            "dmvae_label_spread, %d iterations" % CHUNK: lambda: spread.spread_enqueue(indptr, indices, s, y, C_CLASSES, ALPHA, CHUNK, F, change, ws, flag),
            "torch.sparse composition, %d iterations" % CHUNK: lambda: run_torch(CHUNK),
        }
        for fn in runs.values():
            fn(), fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.repeats):
            for k, fn in runs.items():
                times[k].append(timed(fn, torch))
        Ft = run_torch(CHUNK)
        agree = float((Ft - F).abs().max())
        lines.append("N = %d, D = %d: nnz = %d, degree median %d max %d" % (N, D, nnz, int(deg.median()), int(deg.max())))
        for k, v in times.items():
            lines.append("  %-44s %s" % (k, fmt(v)))
        ours, theirs = times["dmvae_label_spread, %d iterations" % CHUNK], times["torch.sparse composition, %d iterations" % CHUNK]
        mo, mt = statistics.median(ours) / CHUNK, statistics.median(theirs) / CHUNK
        lines.append("  per iteration: kernel %s, torch.sparse %s, kernel / composition %.3f; largest |F - F_torch| after %d iterations %.2e"
                     % (fmt(ours, CHUNK), fmt(theirs, CHUNK), mo / mt, CHUNK, agree))
        lines.append("  per iteration: %.1f GB/s of the CSR entries and the gathered rows (%d bytes)"
                     % ((nnz * (8.0 + 4.0 * 12) + 12.0 * 4 * N * 2) / mo / 1e6, int(nnz * (8.0 + 4.0 * 12) + 12.0 * 4 * N * 2)))
        spread.LabelSpreading(n_neighbors=K_NEIGH, alpha=ALPHA).fit(X, yh)
        fits = []
        for _ in range(max(3, a.repeats // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ls = spread.LabelSpreading(n_neighbors=K_NEIGH, alpha=ALPHA).fit(X, yh)
            torch.cuda.synchronize()
            fits.append(1e3 * (time.perf_counter() - t0))
        free = yh < 0
        lines.append("  LabelSpreading.fit (host clock, synchronised): %.1f ms (min %.1f max %.1f), %d iterations, %d rows unreached, accuracy on the "
                     "unlabelled rows %.4f" % (statistics.median(fits), min(fits), max(fits), ls.n_iter_, ls.n_unreached_, ls.score(cls, free)))
        print("\n".join(lines[-(len(times) + 4):]), flush=True)
        if N > a.sklearn_max_n:
            lines.append("  sklearn LabelSpreading: not measured, its dense N x N float64 matrix takes %.1f GB" % (8.0 * N * N / 1e9))
        else:
            try:
                import sklearn.semi_supervised      # noqa: F401
            except ImportError:
                lines.append("  sklearn LabelSpreading: not measured, sklearn does not import")
            else:
                with tempfile.TemporaryDirectory() as tmp:
                    np.savez(os.path.join(tmp, "d.npz"), X=Xh.astype(np.float64), y=yh, cls=cls, indptr=indptr.cpu().numpy(), indices=indices.cpu().numpy(),
                             values=values.cpu().numpy().astype(np.float64) * N)
                    try:
                        pr = subprocess.run([sys.executable, "-c", SKLEARN_CHILD, os.path.join(tmp, "d.npz"), str(ALPHA), os.path.join(tmp, "t.npy")],
                                            capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES=""), timeout=240)
                    except subprocess.TimeoutExpired:
                        pr = None
                    if pr is None:
                        lines.append("  sklearn LabelSpreading: not measured, no result within 240 s")
                    elif pr.returncode != 0:
                        lines.append("  sklearn LabelSpreading: failed: %s" % pr.stderr.strip()[-300:])
                    else:
                        s_sec, s_it, s_acc = pr.stdout.split()[-3:]
                        same = float(np.mean(np.load(os.path.join(tmp, "t.npy")) == ls.transduction_))
                        lines.append("  sklearn LabelSpreading(kernel=callable, OMP_NUM_THREADS=%s) on a host copy, the graph given: %.1f ms, %s iterations "
                                     "(its tol bounds the SUM of changes), accuracy %s, %.4f of the rows predicted as on the device = %.1f x the device fit"
                                     % (os.environ.get("OMP_NUM_THREADS", "unset"), 1e3 * float(s_sec), s_it, s_acc, same,
                                        1e3 * float(s_sec) / statistics.median(fits)))
        print(lines[-1], flush=True)
        del X, S, F, ws
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
