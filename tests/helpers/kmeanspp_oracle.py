"""Float64 NumPy k-means++ seeding that takes its uniforms as an argument: the yardstick of the device seeding (dmvae_gmm_seed,
csrc/gmm_seed.hip).  Plain D^2 sampling (one trial per centre; Arthur & Vassilvitskii 2007) and the greedy form with T trials per
centre that sklearn's _kmeans_plusplus runs.  Selection rule: the first row whose running sum of d2 exceeds u * tot, never past the
last row with d2 > 0; of T candidates the first with the smallest potential.  tests/test_gmm_seed_host.py holds it against
dmvae_hip.gmm.kmeans_plusplus (T = 1) and against a restatement of sklearn's function (greedy), itself held against sklearn."""
import numpy as np


def trials(K, local_trials):
    """T: local_trials, or sklearn's 2 + int(ln K) when it is 0"""
    return int(local_trials) if local_trials else 2 + int(np.log(K))


def dist2(X, row):
    X = np.asarray(X, dtype=np.float64)
    return ((X - X[row]) ** 2).sum(1)


def uniform_row(u, n):
    return min(int(np.floor(np.float64(u) * n)), n - 1)


def select(d2, u):
    """(row, cum, tot) of one draw u in [0, 1) on the squared distances d2 (float64)"""
    cum = np.cumsum(d2)
    tot = float(cum[-1])
    if not tot > 0:
        return uniform_row(u, len(d2)), cum, tot
    i = int(np.searchsorted(cum, np.float64(u) * tot, side="right"))          # the first cum[i] > target
    return min(i, int(np.flatnonzero(d2 > 0)[-1])), cum, tot


def potentials(X, d2, rows):
    """sum_n min(d2_n, ||x_n - x_row||^2) of every candidate row"""
    return np.array([np.minimum(d2, dist2(X, r)).sum() for r in rows])


def kmeanspp(X, K, u, local_trials=1):
    """u [K][T] uniforms of ONE restart.  Returns (rows [K], candidates [K][T] (round 0: trial 0, the others -1), potentials [K][T])."""
    X = np.asarray(X, dtype=np.float64)
    T = trials(K, local_trials)
    u = np.asarray(u, dtype=np.float64).reshape(K, T)
    rows = np.zeros(K, dtype=np.int64)
    cands = np.full((K, T), -1, dtype=np.int64)
    pots = np.full((K, T), np.nan)
    rows[0] = cands[0, 0] = uniform_row(u[0, 0], len(X))
    d2 = dist2(X, rows[0])
    for k in range(1, K):
        cands[k] = [select(d2, u[k, t])[0] for t in range(T)]
        pots[k] = potentials(X, d2, cands[k])
        rows[k] = cands[k, int(np.argmin(pots[k]))]
        d2 = np.minimum(d2, dist2(X, rows[k]))
    return rows, cands, pots


def sklearn_restated(X, K, u, local_trials=0):
    """sklearn.cluster._kmeans._kmeans_plusplus (1.7) restated in float64 NumPy with unit sample weights, its random draws replaced by
    u [K][T]: the first centre floor(u[0][0] n) (what RandomState.choice does with uniform p), then per centre
    searchsorted(cumsum(closest), u * current_pot) clipped to n - 1, argmin of the candidates' potentials, and current_pot carried on from
    the winner's potential.  Returns the rows [K]."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    T = trials(K, local_trials)
    u = np.asarray(u, dtype=np.float64).reshape(K, T)
    rows = [uniform_row(u[0, 0], n)]
    closest = dist2(X, rows[0])
    pot = closest.sum()
    for k in range(1, K):
        ids = np.searchsorted(np.cumsum(closest), u[k] * pot)
        np.clip(ids, None, n - 1, out=ids)
        d = np.stack([np.minimum(closest, dist2(X, i)) for i in ids])
        cp = d.sum(axis=1)
        best = int(np.argmin(cp))
        pot, closest = cp[best], d[best]
        rows.append(int(ids[best]))
    return np.array(rows)
