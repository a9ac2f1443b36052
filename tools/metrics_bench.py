"""Times get_cluster_metrics (NMI / ARI / purity from the device confusion matrix and the all-pairs silhouette of csrc/cluster_metrics.hip)
against sklearn.metrics.silhouette_score on the host on the same encoder means.

    python tools/metrics_bench.py [--out profiles/cluster_metrics.txt] [--rows 10000,70000] [--dims 10,64] [--repeats 5] [--sklearn-limit 120]
                                  [--bench-json this.json --parent-bench-json parent.json]

Data: 784-wide binary rows around 10 prototypes (3 % of the pixels flipped), a DeepMixtureVAE with the reference's layers in bf16, batch
1000, its logits and mean heads scaled so that an untrained model spreads the rows over several clusters.  Device: one warm call, then the
median of --repeats calls of get_cluster_metrics (wall clock around the call, which ends in its own synchronising read-back), and the
silhouette call alone on the resident means between two HIP events.  sklearn runs ONCE per shape in a child process that never opens the
GPU; a shape whose sklearn run passes --sklearn-limit seconds is reported as not finished.  The two --*-bench-json arguments name the files
(comma-separated, one per run) that hold the JSON line of `bench.py --gpus 1` of this tree and of its parent commit, measured on the same
box: their ms/step are written side by side."""
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

SKLEARN_CHILD = ("import sys, time, numpy as np\nfrom sklearn.metrics import silhouette_score\nZ, l = np.load(sys.argv[1]), np.load(sys.argv[2])\n"
                 "t = time.perf_counter()\ns = silhouette_score(Z, l)\nprint('%.9f %.3f' % (s, time.perf_counter() - t))\n")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="10000,70000")
    ap.add_argument("--dims", default="10,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn-limit", type=float, default=120.0, help="seconds one sklearn run may take; 0 leaves sklearn out")
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--parent-bench-json", default=None)
    a = ap.parse_args()
    import torch
    import base_models
    from dmvae_hip import metrics
    from includes.utils import Dataset
    assert torch.cuda.is_available(), "metrics_bench needs a GPU"
    lines = ["metrics_bench: get_cluster_metrics of a DeepMixtureVAE (784 -> 500,500 -> heads 2000, bf16, batch 1000, K = 10) on rows around 10 "
             "prototypes; one warm call, then the median of %d synchronised calls; sklearn once per shape (limit %.0f s, OMP_NUM_THREADS=%s)"
             % (a.repeats, a.sklearn_limit, os.environ.get("OMP_NUM_THREADS", "unset"))]
    for D in [int(d) for d in a.dims.split(",")]:
        m = base_models.DeepMixtureVAE("dmvae", "binary", 784, D, 10, activation="relu", initializer="xavier", batch_size=1000, dtype="bf16", seed=1,
                                       eval="device").build_graph()
        p = m.engine.get_parameters()
        rng = np.random.RandomState(2)
        m.engine.set_parameters({"W_logits": 4.0 * rng.randn(*p["W_logits"].shape), "W_mean": 3.0 * rng.randn(*p["W_mean"].shape)})
        for n in [int(r) for r in a.rows.split(",")]:
            X, cls = rows_around_prototypes(n)
            np.random.seed(3)
            data = Dataset((X, cls), batch_size=1000)
            res, labels = m.get_cluster_metrics(None, data, return_labels=True)          # the warm call
            wall = []
            for _ in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = m.get_cluster_metrics(None, data)
                wall.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            m.get_cluster_metrics(None, data, silhouette=False)
            rest = (time.perf_counter() - t0) * 1e3
            Z = m.encode_means_device(data.data)
            ld = torch.as_tensor(labels).cuda()
            metrics.silhouette_enqueue(Z, ld, 10)
            torch.cuda.synchronize()
            ev = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                metrics.silhouette_enqueue(Z, ld, 10)
                e1.record()
                torch.cuda.synchronize()
                ev.append(e0.elapsed_time(e1))
            lines += ["N = %d, D = %d: %d clusters in use, acc %.4f nmi %.4f ari %.4f purity %.4f silhouette %.6f"
                      % (n, D, res["n_clusters_used"], res["acc"], res["nmi"], res["ari"], res["purity"], res["silhouette"]),
                      "  get_cluster_metrics, whole call   %.1f ms   (min %.1f max %.1f; without the silhouette, one call: %.1f ms)"
                      % (statistics.median(wall), min(wall), max(wall), rest),
                      "  dmvae_silhouette alone            %.2f ms   (min %.2f max %.2f; HIP events, %.1f G pairs/s)"
                      % (statistics.median(ev), min(ev), max(ev), n * float(n) / statistics.median(ev) / 1e6)]
            if a.sklearn_limit > 0 and res["n_clusters_used"] >= 2:
                with tempfile.TemporaryDirectory() as tmp:
                    np.save(os.path.join(tmp, "z.npy"), Z.cpu().numpy())
                    np.save(os.path.join(tmp, "l.npy"), labels)
                    try:
                        r = subprocess.run([sys.executable, "-c", SKLEARN_CHILD, os.path.join(tmp, "z.npy"), os.path.join(tmp, "l.npy")],
                                           capture_output=True, text=True, timeout=a.sklearn_limit, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
                        if r.returncode != 0:
                            lines.append("  sklearn silhouette_score          failed: %s" % r.stderr.strip()[-300:])
                        else:
                            s, sec = r.stdout.split()
                            lines.append("  sklearn silhouette_score          %.1f s    value %.6f (device - sklearn = %.2g); ratio sklearn / device silhouette %.0f"
                                         % (float(sec), float(s), res["silhouette"] - float(s), float(sec) * 1e3 / statistics.median(ev)))
                    except subprocess.TimeoutExpired:
                        lines.append("  sklearn silhouette_score          NOT MEASURED: did not finish within %.0f s" % a.sklearn_limit)
                    print(lines[-1], flush=True)
            elif a.sklearn_limit > 0:
                lines.append("  sklearn silhouette_score          not run: fewer than 2 clusters in use")
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
