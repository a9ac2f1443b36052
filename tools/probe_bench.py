"""Times dmvae_softmax_xent (csrc/probe.hip) against a torch composition of the same evaluation on the same device in the same process,
and a whole dmvae_hip.probe.LogisticRegression fit against sklearn's on a host copy when sklearn imports.

    python tools/probe_bench.py [--out profiles/probe.txt] [--shapes 65536x64x10,65536x256x10,65536x64x256] [--fit 55000x64x10,55000x256x10] [--repeats 7]

Kernel: standard normal rows, W = 0.1 N(0, 1); two warm calls of each, then --repeats calls of each IN TURN between HIP events, medians
with min and max.  The composition is Z @ W + b, log_softmax, the picked log-probabilities' mean, Z.T @ R and the column sums of R: six
or more launches and two reads of Z against one fused pass and two launches, so the expectation is kernel <= 1.0 x composition.
Fit: the blobs of the solver tests (class centres 1.5 N(0, 1), unit noise), C = 1, tol = 1e-4, standardised; 300 held-out rows per class
count for the accuracy.  sklearn runs once in a child process that never opens the GPU, on the standardised host copy."""
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

SKLEARN_CHILD = ("import sys, time, numpy as np\nfrom sklearn.linear_model import LogisticRegression\nd = np.load(sys.argv[1])\n"
                 "t = time.perf_counter()\nclf = LogisticRegression(C=float(sys.argv[2]), tol=1e-4, max_iter=200).fit(d['X'], d['y'])\n"
                 "sec = time.perf_counter() - t\nprint('%.4f %d %.6f' % (sec, int(np.max(clf.n_iter_)), clf.score(d['Xt'], d['yt'])))\n")


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def fmt(v):
    return "%.1f us (min %.1f max %.1f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))


def shapes(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="65536x64x10,65536x256x10,65536x64x256")
    ap.add_argument("--fit", default="55000x64x10,55000x256x10")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import torch
    from dmvae_hip import probe
    assert torch.cuda.is_available(), "probe_bench needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = ["probe_bench: dmvae_softmax_xent against the torch composition of the same evaluation; two warm calls, then %d calls of each in turn "
             "between HIP events (median, min, max)" % a.repeats]
    for n, D, Cn in shapes(a.shapes):
        rng = np.random.RandomState(D + Cn)
        Z = torch.as_tensor(rng.randn(n, D).astype(np.float32)).to(dev)
        y = torch.as_tensor(rng.randint(0, Cn, n).astype(np.int32)).to(dev)
        y64 = y.long()
        W = torch.as_tensor((0.1 * rng.randn(D, Cn)).astype(np.float32)).to(dev)
        b = torch.as_tensor((0.1 * rng.randn(Cn)).astype(np.float32)).to(dev)
        ws, out, flag = probe.xent_workspace(n, D, Cn, dev)
        rows = torch.arange(n, device=dev)

        def run_kernel():
            probe.xent_enqueue(Z, y, W, b, None, None, ws, out, flag)

        def run_torch():
            logp = torch.log_softmax(Z @ W + b, dim=1)
            loss = -logp[rows, y64].mean()
            R = logp.exp()
            R[rows, y64] -= 1.0
            return loss, (Z.t() @ R) / n, R.sum(0) / n

        for _ in range(2):
            run_kernel(), run_torch()
        torch.cuda.synchronize()
        tk, tt = [], []
        for _ in range(a.repeats):
            tk.append(timed(run_kernel, torch))
            tt.append(timed(run_torch, torch))
        loss_t, gW_t, _ = run_torch()
        host = out.cpu().numpy()
        agree = max(abs(host[0] - float(loss_t)), float(np.abs(host[1:1 + D * Cn].reshape(D, Cn) - gW_t.double().cpu().numpy()).max()))
        mk, mt = statistics.median(tk), statistics.median(tt)
        lines += ["n = %d, D = %d, C = %d:" % (n, D, Cn),
                  "  dmvae_softmax_xent   %s   %.2f TB/s of Z" % (fmt(tk), 4.0 * n * D / mk / 1e9),
                  "  torch composition    %s" % fmt(tt),
                  "  kernel / composition %.3f   (expected <= 1.0); largest difference of loss and gW %.2e" % (mk / mt, agree)]
        print("\n".join(lines[-4:]), flush=True)
        del Z, y, W, b, ws, out
    for n, D, Cn in shapes(a.fit):
        r = np.random.RandomState(1)
        cen = r.randn(Cn, D) * 1.5
        yh = r.randint(0, Cn, n)
        Zh = (cen[yh] + r.randn(n, D)).astype(np.float32)
        r = np.random.RandomState(2)
        yt = r.randint(0, Cn, 300 * Cn)
        Zt = (cen[yt] + r.randn(len(yt), D)).astype(np.float32)
        Zd, Ztd = torch.as_tensor(Zh).to(dev), torch.as_tensor(Zt).to(dev)
        probe.LogisticRegression(C=1.0, tol=1e-4, max_iter=200, standardize=True).fit(Zd, yh)      # warm: allocator, pinned buffers
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clf = probe.LogisticRegression(C=1.0, tol=1e-4, max_iter=200, standardize=True).fit(Zd, yh)
        sec = time.perf_counter() - t0
        acc = clf.score(Ztd, yt)
        lines += ["fit n = %d, D = %d, C = %d (C = 1, tol = 1e-4, standardised):" % (n, D, Cn),
                  "  device fit  %.1f ms, %d iterations, %d evaluations = %.0f us per evaluation with its two copies and scipy's step; accuracy %.4f"
                  % (1e3 * sec, clf.n_iter_, clf.n_fev_, 1e6 * sec / max(clf.n_fev_, 1), acc)]
        print("\n".join(lines[-2:]), flush=True)
        try:
            import sklearn.linear_model      # noqa: F401
        except ImportError:
            lines.append("  sklearn LogisticRegression: not measured, sklearn does not import")
        else:
            mean, std = Zh.astype(np.float64).mean(0), Zh.astype(np.float64).std(0)
            with tempfile.TemporaryDirectory() as tmp:
                np.savez(os.path.join(tmp, "d.npz"), X=(Zh - mean) / std, y=yh, Xt=(Zt - mean) / std, yt=yt)
                pr = subprocess.run([sys.executable, "-c", SKLEARN_CHILD, os.path.join(tmp, "d.npz"), "1.0"], capture_output=True, text=True,
                                    env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
            if pr.returncode != 0:
                lines.append("  sklearn LogisticRegression: failed: %s" % pr.stderr.strip()[-300:])
            else:
                s_sec, s_it, s_acc = pr.stdout.split()[-3:]
                lines.append("  sklearn LogisticRegression(lbfgs, OMP_NUM_THREADS=%s) on a host copy: %.1f ms, %s iterations, accuracy %s = %.1f x the device fit"
                             % (os.environ.get("OMP_NUM_THREADS", "unset"), 1e3 * float(s_sec), s_it, s_acc, float(s_sec) / sec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
