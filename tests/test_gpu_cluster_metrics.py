"""GPU tests of the cluster-metric kernels (csrc/cluster_metrics.hip): dmvae_argmax_labels against np.argmax, exactly, and
dmvae_silhouette against the float64 oracle of tests/helpers/cluster_metrics_oracle.py, every sample and the mean.

Bar, per sample and for the mean: 4 (D + 70) 2^-24 (cluster_metrics_oracle.bar: it follows from the arithmetic contract of the
header -- f32 differences, correctly rounded sqrt, at most 64 distances per f32 running sum, a / b / s in double).  No sample is
excluded.  Properties (singletons, duplicates, the cluster count, reproducibility, the error flag, refused arguments): exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import cluster_metrics_oracle as CO      # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def run(buf, D, labels, K):
    """one dmvae_silhouette call on the rows buf[:, :D] where they lie: (samples f32 [n], out f64 [2], flag) on the host"""
    from dmvae_hip import metrics
    Zd = dev(buf)[:, :D]
    s, out, flag = metrics.silhouette_enqueue(Zd, dev(labels, torch.int32), K)
    return s.cpu().numpy(), out.cpu().numpy(), int(flag.item())


@pytest.mark.parametrize("K", [1, 5, 10, 50, 256, 4096])
def test_argmax_labels_equal_numpy_argmax(K):
    from dmvae_hip import metrics
    rng = np.random.RandomState(K)
    for n in (1, 17, 1003):
        sc = rng.randint(0, 3, (n, K)).astype(np.float32)            # three values: every row of K > 3 scores holds exact ties of its maximum
        sc[0] = 0.5                                                  # a whole row of one value: index 0
        if n > 4 and K > 20:
            sc[3] = -1.0
            sc[3, [K - 1, 17]] = 7.0                                 # a tie between two lanes' last and an early column: 17
            sc[4] = np.arange(K, dtype=np.float32) * 1e-3            # the last column
        buf = np.full((n, K + 3), 1e30, dtype=np.float32)            # ld > K, 1e30 between the rows
        buf[:, :K] = sc
        got = metrics.argmax_labels(dev(buf)[:, :K]).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, np.argmax(sc, axis=1)), (K, n)
        out = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
        metrics.argmax_labels(dev(sc), out=out[1:n + 1])             # a contiguous matrix, into a slice: nothing outside it is written
        assert np.array_equal(out.cpu().numpy(), np.concatenate([[-7], np.argmax(sc, axis=1), [-7]]))


@pytest.mark.parametrize("name", CO.CASE_NAMES)
def test_silhouette_against_the_oracle(name):
    buf, D, labels, K, ref = CO.reference(name)
    got, out, flag = run(buf, D, labels, K)
    n = len(labels)
    err = np.abs(got.astype(np.float64) - ref)
    mean_err = abs(out[0] / n - ref.mean())
    print("%s: max |s - oracle| = %.3g at row %d, |mean - oracle| = %.3g (bar %.3g)" % (name, err.max(), int(err.argmax()), mean_err, CO.bar(D)))
    assert flag == 0 and out[1] == np.count_nonzero(np.bincount(labels, minlength=K))
    assert np.all(np.isfinite(got)) and err.max() <= CO.bar(D), (name, float(err.max()), int(err.argmax()))
    assert mean_err <= CO.bar(D), (name, mean_err)
    single = np.bincount(labels, minlength=K)[labels] == 1
    assert not got[single].any()                                     # singleton rows: exactly 0
    got2, out2, _ = run(buf, D, labels, K)                           # a second call: the same bits
    assert got.tobytes() == got2.tobytes() and out.tobytes() == out2.tobytes()


def test_python_surface_returns_the_samples_and_the_score():
    from dmvae_hip import metrics
    buf, D, labels, K, ref = CO.reference("N257-D3-K7-ld5")
    s = metrics.silhouette_samples(dev(buf)[:, :D], dev(labels, torch.int32))           # device tensors; n_clusters from the labels
    assert s.is_cuda and s.dtype == torch.float32 and np.abs(s.cpu().numpy() - ref).max() <= CO.bar(D)
    score = metrics.silhouette_score(buf[:, :D], labels, n_clusters=K)                   # arrays that are uploaded
    assert isinstance(score, float) and abs(score - ref.mean()) <= CO.bar(D)
    assert score == metrics.silhouette_score(dev(buf)[:, :D], dev(labels, torch.int32), n_clusters=K)
    with pytest.raises(ValueError, match="Number of labels is 1"):                       # counted on the device
        metrics.silhouette_score(dev(buf)[:, :D], torch.zeros(len(labels), dtype=torch.int32, device="cuda"))


def test_all_duplicate_rows_give_exactly_zero():
    Z = np.tile(np.array([[0.3, -1.7, 2.5]], dtype=np.float32), (300, 1))
    labels = (np.arange(300) % 3).astype(np.int32)
    got, out, flag = run(Z, 3, labels, 3)
    assert flag == 0 and not got.any() and out[0] == 0.0 and out[1] == 3.0


@pytest.mark.parametrize("bad", [-1, 6])
def test_a_label_outside_the_range_sets_the_flag_and_is_left_out(bad):
    """an argument check on memory that is in range: the kernels compare the label with [0, K) before they index anything with it"""
    from dmvae_hip import metrics
    buf, D, labels, K, _ = CO.reference("N301-D10-K6")
    assert K == 6
    lab = labels.copy()
    lab[41] = bad
    got, out, flag = run(buf, D, lab, K)
    keep = np.arange(len(lab)) != 41
    ref = CO.silhouette_samples(buf[keep, :D], lab[keep], K)         # the row is in no sum
    assert flag == 1 and got[41] == 0.0 and np.abs(got[keep] - ref).max() <= CO.bar(D)
    assert abs(out[0] - ref.sum()) <= len(lab) * CO.bar(D) and out[1] == 5.0
    with pytest.raises(IndexError):
        metrics.silhouette_samples(dev(buf)[:, :D], dev(lab, torch.int32), n_clusters=K)
    with pytest.raises(IndexError):
        metrics.silhouette_score(dev(buf)[:, :D], dev(lab, torch.int32), n_clusters=K)


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    from dmvae_hip import _lib as L
    n, D, K = 64, 5, 4
    rng = np.random.RandomState(0)
    Z, lab = dev(rng.randn(n, D).astype(np.float32)), dev(rng.randint(0, K, n), torch.int32)
    need = int(L.lib.dmvae_silhouette_ws_bytes(n, K))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    samples = torch.full((n,), -5.0, device="cuda")
    out = torch.full((2,), -5.0, dtype=torch.float64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(n_=n, D_=D, K_=K, ldz=D, ws_ptr=ws.data_ptr(), nbytes=need, Zp=Z.data_ptr()):
        return L.lib.dmvae_silhouette(stream, Zp, ldz, n_, D_, lab.data_ptr(), K_, ws_ptr, nbytes, samples.data_ptr(), out.data_ptr(), flag.data_ptr())

    for kw, text in ((dict(n_=1), "n=1"), (dict(K_=0), "K=0"), (dict(K_=4097), "K=4097"), (dict(ldz=D - 1), "ldz=4"), (dict(D_=0, ldz=0), "D=0"),
                     (dict(nbytes=need - 1), "%d bytes" % need), (dict(ws_ptr=None), "%d bytes" % need), (dict(Zp=None), "must be given")):
        assert call(**kw) == -1, kw                                  # DMVAE_EINVAL
        assert text.encode() in L.lib.dmvae_last_error(), (kw, L.lib.dmvae_last_error())
    assert L.lib.dmvae_argmax_labels(stream, Z.data_ptr(), D - 1, n, D, lab.data_ptr()) == -1      # ld < K
    assert L.lib.dmvae_argmax_labels(stream, Z.data_ptr(), D, n, 0, lab.data_ptr()) == -1
    assert L.lib.dmvae_argmax_labels(stream, Z.data_ptr(), D, -1, D, lab.data_ptr()) == -1
    torch.cuda.synchronize()
    assert not ws.any() and (samples == -5.0).all() and (out == -5.0).all() and int(flag.item()) == 0
    assert call() == 0                                               # and the same buffers still run
    torch.cuda.synchronize()
    assert np.isfinite(samples.cpu().numpy()).all() and out[1].item() == K
