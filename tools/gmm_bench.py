"""Times the prior tables' mixture fit on one data set: dmvae_hip.gmm.DiagGMM (seeding on the host and the device part apart, both
synchronised) against the sklearn call pretrain_prior makes with gmm="host", in the same process.

    python tools/gmm_bench.py [--out profiles/gmm_fit.txt] [--repeats 5] [--sklearn-repeats 1] [--seeding host|device] [--local_trials T]

--seeding device draws the k-means++ centres with dmvae_gmm_seed (--local_trials: 1 plain D^2 sampling, 0 sklearn's 2 + int(ln K)
greedy trials, 2..8); the seeding part is then timed with a synchronise of its own.  --sklearn-repeats 0 leaves the sklearn fit out.

Data: 65 000 x 10 float32, ten overlapping diagonal Gaussians from a seed (tests/helpers/gmm_oracle.overlapping); K = 10, n_init = 20,
max_iter = 200, uniform weights_init.  One warm run first, then the median of the repeats."""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-mixture-vae_amd"), os.path.join(ROOT, "tests", "helpers")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn-repeats", type=int, default=1)
    ap.add_argument("--rows", type=int, default=65000)
    ap.add_argument("--seeding", default="host", choices=["host", "device"])
    ap.add_argument("--local_trials", type=int, default=1)
    a = ap.parse_args()
    import torch
    import gmm_oracle as G
    from dmvae_hip.gmm import DiagGMM
    from sklearn.mixture import GaussianMixture
    K, D = 10, 10
    X, _ = G.overlapping(a.rows, D, K, seed=1)
    Xd = torch.as_tensor(X).cuda()
    kw = dict(max_iter=200, n_init=20, weights_init=np.ones(K) / K)
    dkw = dict(kw, seeding=a.seeding, local_trials=a.local_trials, time_parts=True) if a.seeding == "device" else kw

    DiagGMM(K, seed=0, **dkw).fit(Xd)                     # warm run: code objects loaded, allocator primed
    seed_s, dev_s, tot_s = [], [], []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = DiagGMM(K, seed=0, **dkw).fit(Xd)             # fit synchronises before it reads the result back
        tot_s.append(time.perf_counter() - t0)
        seed_s.append(g.seed_seconds_)
        dev_s.append(g.device_seconds_)
    sk_s, sk = [], None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(a.sklearn_repeats):
            np.random.seed(0)
            t0 = time.perf_counter()
            sk = GaussianMixture(n_components=K, covariance_type="diag", **kw).fit(X)       # random_state=None, as pretrain_prior calls it
            sk_s.append(time.perf_counter() - t0)
    med = statistics.median
    where = ("host NumPy, incl. the copy of Z to the host" if a.seeding == "host" else
             "device, %d trial(s) per centre, synchronised" % (a.local_trials or 2 + int(np.log(K))))
    lines = [
        "gmm_bench: %d x %d f32, K = %d, n_init = 20, max_iter = 200, tol = 1e-3; seeding %s; %d device repeats after a warm run, %d sklearn run(s); medians" % (
            a.rows, D, K, a.seeding, a.repeats, a.sklearn_repeats),
        "device fit, whole   %.4f s   (min %.4f max %.4f)" % (med(tot_s), min(tot_s), max(tot_s)),
        "  k-means++ seeding (%s)   %.4f s   (min %.4f max %.4f)" % (where, med(seed_s), min(seed_s), max(seed_s)),
        "  device part (%sLloyd, EM, select, read-back)     %.4f s   (min %.4f max %.4f)" % (
            "upload of centres, " if a.seeding == "host" else "", med(dev_s), min(dev_s), max(dev_s)),
    ]
    if sk is not None:
        lines += [
            "sklearn fit         %.4f s   (OMP_NUM_THREADS=%s)" % (med(sk_s), os.environ.get("OMP_NUM_THREADS", "unset")),
            "ratio sklearn / device whole   %.1f" % (med(sk_s) / med(tot_s)),
        ]
    lines += [
        "lower bound: device %.6f (restart %d, n_iter %d, converged %s)%s" % (
            g.lower_bound_, g.best_restart_, g.n_iter_, g.converged_,
            "" if sk is None else "   sklearn %.6f (n_iter %d)" % (sk.lower_bound_, sk.n_iter_)),
        "Lloyd iterations per restart: %s" % [int(v) for v in g.restarts_["kmeans_iter"]],
        "EM iterations per restart:    %s" % [int(v) for v in g.restarts_["n_iter"]],
    ]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
