"""Times the posterior diagnostics (csrc/mixture_density.hip, dmvae_hip/density.py): dmvae_mixture_logpdf alone on N points against the N
encoder posteriors, and the whole get_posterior_diagnostics call, against two restatements of the same all-pairs log-density.

    python tools/posterior_bench.py [--out profiles/posterior_diagnostics.txt] [--rows 10000,70000] [--dims 10,64] [--repeats 5] [--numpy-limit 120]
                                    [--bench-json this.json --parent-bench-json parent.json]

Data: 784-wide binary rows around 10 prototypes (3 % of the pixels flipped), a DeepMixtureVAE with the reference's layers in bf16, batch
1000, its mean head scaled and its log-variance bias at -3 so that an untrained model has posteriors that overlap a little.  Device: one
warm call, then the median of --repeats calls -- get_posterior_diagnostics by the wall clock around the call (which ends in its own
synchronising read-back), dmvae_mixture_logpdf alone (workspace and output allocated before) between two HIP events.  Against
  (a) torch on the same GPU: the obvious restatement -- chunks of points broadcast against all components, f32, difference form,
      torch.logsumexp -- between HIP events, one warm call and the median of --repeats;
  (b) NumPy float32 on the host, the same chunked broadcast on 16 threads (NumPy releases the GIL in its loops), ONE run per shape in a
      child process that never opens the GPU; a shape whose run passes --numpy-limit seconds is reported as not finished.
Pair-dimensions per second = M J D / time: one subtract, one multiply and one fma each, beside the f32 vector peak of 157.3 TFLOP/s
(78.6 T fma/s).  The two --*-bench-json arguments name the files (comma-separated, one per run) that hold the JSON line of
`bench.py --gpus 1` of this tree and of its parent commit, measured on the same box: their ms/step are written side by side."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-mixture-vae_amd"))

NUMPY_CHILD = r"""
import sys, time, numpy as np
from concurrent.futures import ThreadPoolExecutor
z, mu, lv = (np.load(p) for p in sys.argv[1:4])
N, D = mu.shape
t0 = time.perf_counter()
iv = np.exp(-lv)
c = (-0.5 * lv.sum(axis=1) - np.float32(np.log(N))).astype(np.float32)
rows = max(1, (1 << 22) // (N * D))
def part(lo):
    e = z[lo:lo + rows, None, :] - mu[None]
    np.multiply(e, e, out=e)
    t = c[None] - np.float32(0.5) * np.einsum("ijd,jd->ij", e, iv)
    m = t.max(axis=1)
    return np.log(np.exp(t - m[:, None]).sum(axis=1)) + m - np.float32(0.5 * D * np.log(2 * np.pi))
with ThreadPoolExecutor(16) as ex:
    out = np.concatenate(list(ex.map(part, range(0, len(z), rows))))
print('%.9f %.3f' % (float(out.astype(np.float64).mean()), time.perf_counter() - t0))
"""


def rows_around_prototypes(n, seed=0):
    rng = np.random.RandomState(seed)
    protos = rng.rand(10, 784) < 0.19
    which = rng.randint(0, 10, n)
    return np.logical_xor(protos[which], rng.rand(n, 784) < 0.03).astype(np.float32), which.astype(np.int64)


def ms_per_step(path):
    rec = json.loads([l for l in open(path) if l.lstrip().startswith("{")][-1])
    for key in ("ms_per_step", "step_ms", "ms/step"):
        if key in rec:
            return float(rec[key])
    raise KeyError("no ms/step in %s: %s" % (path, sorted(rec)))


def torch_logpdf(z, mu, lv, chunk_elems=1 << 28):
    """the obvious restatement on the device: chunked broadcast, f32, difference form"""
    import torch
    N, D = mu.shape
    iv = torch.exp(-lv)
    c = -0.5 * lv.sum(dim=1) - float(np.log(N))
    rows = max(1, chunk_elems // (N * D))
    out = torch.empty(z.shape[0], dtype=torch.float32, device=z.device)
    for lo in range(0, z.shape[0], rows):
        e = z[lo:lo + rows, None, :] - mu[None]
        q = (e * e * iv[None]).sum(dim=2)
        out[lo:lo + rows] = torch.logsumexp(c[None] - 0.5 * q, dim=1)
    return out - 0.5 * D * float(np.log(2 * np.pi))


def events(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="10000,70000")
    ap.add_argument("--dims", default="10,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-limit", type=float, default=120.0, help="seconds one NumPy run may take; 0 leaves it out")
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--parent-bench-json", default=None)
    a = ap.parse_args()
    import torch
    import base_models
    from dmvae_hip import density, lib
    from includes.utils import Dataset
    assert torch.cuda.is_available(), "posterior_bench needs a GPU"
    lines = ["posterior_bench: get_posterior_diagnostics of a DeepMixtureVAE (784 -> 500,500 -> heads 2000, bf16, batch 1000, K = 10) on rows around 10 "
             "prototypes; one warm call, then the median of %d; NumPy once per shape (limit %.0f s, 16 threads)" % (a.repeats, a.numpy_limit)]
    for D in [int(d) for d in a.dims.split(",")]:
        m = base_models.DeepMixtureVAE("dmvae", "binary", 784, D, 10, activation="relu", initializer="xavier", batch_size=1000, dtype="bf16", seed=1,
                                       eval="device").build_graph()
        p = m.engine.get_parameters()
        rng = np.random.RandomState(2)
        m.engine.set_parameters({"W_mean": 3.0 * rng.randn(*p["W_mean"].shape), "b_logvar": np.full(D, -3.0)})
        for n in [int(r) for r in a.rows.split(",")]:
            X, cls = rows_around_prototypes(n)
            np.random.seed(3)
            data = Dataset((X, cls), batch_size=1000)
            res = m.get_posterior_diagnostics(None, data)                                 # the warm call
            wall = []
            for _ in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = m.get_posterior_diagnostics(None, data)
                wall.append((time.perf_counter() - t0) * 1e3)
            eng = m.engine
            mean, lv = (torch.empty((n, D), dtype=torch.float32, device="cuda") for _ in range(2))
            for s, k in m._eval_batches(data, data.order):
                eng.encode(k)
                mean[s:s + k].copy_(eng.view("mean", k))
                lv[s:s + k].copy_(eng.view("log_var", k))
            z, _ = density.posterior_sample(mean, lv, seed=m.seed, counter=0)
            ws = torch.empty(int(lib.dmvae_mixture_logpdf_ws_bytes(n, n, D)), dtype=torch.uint8, device="cuda")
            out = torch.empty(n, dtype=torch.float32, device="cuda")
            ev = events(lambda: density.mixture_logpdf(z, mean, lv, out=out, ws=ws), a.repeats)
            tv = events(lambda: torch_logpdf(z, mean, lv), a.repeats)
            diff = float((torch_logpdf(z, mean, lv).double() - out.double()).abs().max())
            pd = lambda ms: float(n) * n * D / ms / 1e9                                   # T pair-dimensions per second
            lines += ["N = %d, D = %d: mi %.4f (cap %.4f) marginal_kl %.4f rate %.4f active units %d, J split %d"
                      % (n, D, res["mi"], res["mi_cap"], res["marginal_kl"], res["rate"], res["active_units"], density.mixture_split(n, n, D)),
                      "  get_posterior_diagnostics, whole call   %.1f ms   (min %.1f max %.1f)" % (statistics.median(wall), min(wall), max(wall)),
                      "  dmvae_mixture_logpdf alone              %.2f ms   (min %.2f max %.2f; HIP events; %.2f T pair-dimensions/s, %.1f %% of 78.6 T fma/s)"
                      % (statistics.median(ev), min(ev), max(ev), pd(statistics.median(ev)), 100.0 * pd(statistics.median(ev)) / 78.6),
                      "  (a) torch, chunked broadcast f32        %.1f ms   (min %.1f max %.1f; %.3f T pair-dimensions/s; ratio torch / kernel %.0f; max |torch - kernel| %.2g)"
                      % (statistics.median(tv), min(tv), max(tv), pd(statistics.median(tv)), statistics.median(tv) / statistics.median(ev), diff)]
            print("\n".join(lines[-4:]), flush=True)
            if a.numpy_limit > 0:
                with tempfile.TemporaryDirectory() as tmp:
                    paths = [os.path.join(tmp, f) for f in ("z.npy", "mu.npy", "lv.npy")]
                    for path, t in zip(paths, (z, mean, lv)):
                        np.save(path, t.cpu().numpy())
                    try:
                        r = subprocess.run([sys.executable, "-c", NUMPY_CHILD] + paths, capture_output=True, text=True, timeout=a.numpy_limit,
                                           env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
                        if r.returncode != 0:
                            lines.append("  (b) NumPy float32, 16 threads           failed: %s" % r.stderr.strip()[-300:])
                        else:
                            v, sec = r.stdout.split()
                            lines.append("  (b) NumPy float32, 16 threads           %.1f s    mean log q(z) %.6f (kernel - NumPy = %.2g); ratio NumPy / kernel %.0f"
                                         % (float(sec), float(v), float(out.double().mean()) - float(v), float(sec) * 1e3 / statistics.median(ev)))
                    except subprocess.TimeoutExpired:
                        lines.append("  (b) NumPy float32, 16 threads           NOT MEASURED: did not finish within %.0f s" % a.numpy_limit)
                    print(lines[-1], flush=True)
            del mean, lv, z, ws, out
        del m
    if a.bench_json and a.parent_bench_json:
        fmt = lambda paths: " / ".join("%.4f" % ms_per_step(p) for p in paths.split(","))
        lines.append("bench.py --gpus 1, same box, runs in alternating order: this tree %s ms/step, parent commit %s ms/step (the step path "
                     "launches nothing new)" % (fmt(a.bench_json), fmt(a.parent_bench_json)))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
