"""float64 oracle of the silhouette coefficient, straight from the definition (Rousseeuw 1987; dmvae_silhouette of include/dmvae_hip.h),
with the distances in the DIFFERENCE form, chunked over the rows -- and the cases the GPU test and the host test share.

    d_ij = sqrt(sum_c (z_ic - z_jc)^2),  a_i = sum_{l_j = l_i} d_ij / (n_{l_i} - 1),  b_i = min_{k != l_i, n_k > 0} sum_{l_j = k} d_ij / n_k,
    s_i = (b_i - a_i) / max(a_i, b_i);  0 when n_{l_i} = 1 or max(a_i, b_i) = 0

The contingency-matrix scores (NMI / ARI / purity) are not re-derived here: tests/test_cluster_metrics_host.py holds them to sklearn."""
import numpy as np

FILLER = 1e30            # what lies between the rows where ldz > D: never read


def silhouette_samples(Z, labels, n_clusters=None, chunk=128):
    Z = np.asarray(Z, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    n = len(Z)
    K = int(labels.max()) + 1 if n_clusters is None else int(n_clusters)
    counts = np.bincount(labels, minlength=K).astype(np.float64)
    onehot = np.zeros((n, K))
    onehot[np.arange(n), labels] = 1.0
    S = np.empty((n, K))
    for s in range(0, n, chunk):
        diff = Z[s:s + chunk, None, :] - Z[None, :, :]
        S[s:s + chunk] = np.sqrt((diff * diff).sum(axis=-1)) @ onehot
    own = counts[labels]
    a = S[np.arange(n), labels] / np.maximum(own - 1.0, 1.0)
    other = np.where(counts[None, :] > 0, S / np.maximum(counts[None, :], 1.0), np.inf)
    other[np.arange(n), labels] = np.inf
    b = other.min(axis=1)
    m = np.maximum(a, b)
    ok = (own > 1) & (m > 0) & np.isfinite(b)
    return np.where(ok, (b - a) / np.where(ok, m, 1.0), 0.0)


def bar(D):
    """per sample and for the mean: 4 (D + 70) 2^-24.  A distance carries at most D / 2 + 2 ulp, a 64-term f32 sum of positive terms 64
    more, so a cluster mean is relatively off by eps < (D + 68) 2^-24; s = 1 - a / b moves by at most 2 eps, taking another cluster at a
    near-tie of b by at most 2 eps more, and the final rounding adds one ulp."""
    return 4.0 * (D + 70) * 2.0 ** -24


def _blobs(rng, N, D, labels, K, sep):
    centers = sep * rng.randn(K, D)
    return (centers[labels] + rng.randn(N, D)).astype(np.float32)


def _store(Z, ldz):
    """the rows inside an [N][ldz] buffer whose other columns hold FILLER; returns (buffer, the [N][D] view of it)"""
    N, D = Z.shape
    buf = np.full((N, ldz), FILLER, dtype=np.float32)
    buf[:, :D] = Z
    return buf


def cases():
    """[(name, buffer f32 [N][ldz], D, labels int32 [N], K)]: the shapes (N, D, K, ldz) of the GPU test"""
    out = []

    def add(name, N, D, K, ldz, labels, seed, sep=2.0, edit=None):
        rng = np.random.RandomState(seed)
        labels = np.asarray(labels, dtype=np.int32)
        assert labels.shape == (N,) and labels.min() >= 0 and labels.max() < K
        Z = _blobs(rng, N, D, labels, K, sep)
        if edit is not None:
            edit(Z)
        out.append((name, _store(Z, ldz), D, labels, K))

    # one label never used (3), one singleton cluster (5), one pair of identical rows (7 and 8, one cluster)
    rng = np.random.RandomState(1)
    lab = rng.choice([0, 1, 2, 4], size=301).astype(np.int32)
    lab[100] = 5
    lab[7] = lab[8]

    def twins(Z):
        Z[8] = Z[7]
    add("N301-D10-K6", 301, 10, 6, 10, lab, 11, edit=twins)
    add("N257-D3-K7-ld5", 257, 3, 7, 5, np.random.RandomState(2).randint(0, 7, 257), 12)
    add("N130-D64-K4", 130, 64, 4, 64, np.random.RandomState(3).randint(0, 4, 130), 13, sep=0.5)
    add("N200-D130-K3", 200, 130, 3, 130, np.random.RandomState(4).randint(0, 3, 200), 14, sep=0.3)      # D past one LDS chunk, not a multiple of 4
    add("N65-D1-K2", 65, 1, 2, 1, np.random.RandomState(5).randint(0, 2, 65), 15)
    add("N1030-D2-K10", 1030, 2, 10, 2, np.random.RandomState(6).randint(0, 10, 1030), 16)               # a few past every tile edge
    add("N66-D10-K64", 66, 10, 64, 10, list(range(62)) + [62] * 4, 17)                                   # 62 singletons and one cluster of 4
    add("N700-D4-K300", 700, 4, 300, 4, np.random.RandomState(8).randint(0, 300, 700), 18)               # K past 256
    add("N4097-D8-K3", 4097, 8, 3, 8, np.random.RandomState(9).randint(0, 3, 4097), 19, sep=1.0)         # clusters spanning many tiles
    return out


_CACHE = {}


def reference(name):
    """(buffer, D, labels, K, float64 samples) of a case: computed once per process, not to be modified"""
    if not _CACHE:
        for nm, buf, D, labels, K in cases():
            _CACHE[nm] = (buf, D, labels, K, None)
    buf, D, labels, K, ref = _CACHE[name]
    if ref is None:
        ref = silhouette_samples(buf[:, :D], labels, K)
        ref.setflags(write=False)
        _CACHE[name] = (buf, D, labels, K, ref)
    return _CACHE[name]


CASE_NAMES = ["N301-D10-K6", "N257-D3-K7-ld5", "N130-D64-K4", "N200-D130-K3", "N65-D1-K2", "N1030-D2-K10", "N66-D10-K64", "N700-D4-K300",
              "N4097-D8-K3"]
