"""float64 oracle of the sample-quality counts (csrc/prdc.hip, dmvae_hip/prdc.py), straight from the definitions: all-pairs squared
distances in float64 from the differences, k-th-neighbour radii with the row itself left out (or the radii as given), CLOSED balls
(d2 <= r2), improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020).  No sklearn, no prdc."""
import numpy as np

from knn_oracle import pair_d2, u_bar      # noqa: F401  (u_bar: the bound of a device d2, (D + 3) 2^-24)


def radii(X, k):
    """r2[i] = the squared distance of row i to its k-th nearest OTHER row (float64)"""
    d2 = pair_d2(X, X)
    out = np.empty(len(d2))
    for i in range(len(d2)):
        out[i] = np.sort(np.delete(d2[i], i))[k - 1]
    return out


def counts(R, F, rR2, rF2):
    """dict of what dmvae_prdc_counts returns, and the pair matrix d2 [N][M]"""
    d2 = pair_d2(R, F)
    rR2, rF2 = np.asarray(rR2, dtype=np.float64), np.asarray(rF2, dtype=np.float64)
    return dict(d2=d2,
                fake_in_real=np.count_nonzero(d2 <= rR2[:, None], axis=0).astype(np.int64),
                real_in_fake=np.count_nonzero(d2 <= rF2[None, :], axis=1).astype(np.int64),
                real_min_d2=d2.min(axis=1),
                real_min_j=np.argmin(d2, axis=1).astype(np.int64))          # (np.argmin: the first, so the lowest j on a tie)


def metrics_from_counts(c, rR2, k):
    N, M = c["d2"].shape
    return dict(precision=np.count_nonzero(c["fake_in_real"] > 0) / M, recall=np.count_nonzero(c["real_in_fake"] > 0) / N,
                density=int(c["fake_in_real"].sum()) / (k * M), coverage=np.count_nonzero(c["real_min_d2"] <= np.asarray(rR2, dtype=np.float64)) / N)


def prdc(R, F, k, rR2=None, rF2=None, real_groups=None, fake_groups=None):
    """dict(precision, recall, density, coverage, k [, the per-group vectors as arrays]); radii computed here unless given"""
    rR2 = radii(R, k) if rR2 is None else np.asarray(rR2, dtype=np.float64)
    rF2 = radii(F, k) if rF2 is None else np.asarray(rF2, dtype=np.float64)
    c = counts(R, F, rR2, rF2)
    res = dict(metrics_from_counts(c, rR2, k), k=k)
    with np.errstate(invalid="ignore", divide="ignore"):
        if real_groups is not None:
            g = np.asarray(real_groups)
            rows = np.bincount(g)
            res["coverage_per_group"] = np.bincount(g[c["real_min_d2"] <= rR2], minlength=len(rows)) / rows
            res["recall_per_group"] = np.bincount(g[c["real_in_fake"] > 0], minlength=len(rows)) / rows
        if fake_groups is not None:
            g = np.asarray(fake_groups)
            rows = np.bincount(g)
            res["precision_per_group"] = np.bincount(g[c["fake_in_real"] > 0], minlength=len(rows)) / rows
            res["density_per_group"] = np.bincount(g, weights=c["fake_in_real"], minlength=len(rows)) / (k * rows)
    return res


def undecided(d2, r2, u):
    """the pairs the f32 distance cannot decide against a radius: |d2 - r2| <= 2 u max(d2, r2) (r2 broadcast against d2)"""
    r2 = np.broadcast_to(np.asarray(r2, dtype=np.float64), d2.shape)
    with np.errstate(invalid="ignore"):
        return np.isfinite(r2) & (np.abs(d2 - r2) <= 2.0 * u * np.maximum(d2, r2))          # (every finite d2 is inside an infinite radius)
