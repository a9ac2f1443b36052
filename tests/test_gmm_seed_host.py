"""CPU tests of the device k-means++ seeding's yardstick and host surface: the float64 oracle (tests/helpers/kmeanspp_oracle.py) against
the host seeding of dmvae_hip.gmm (one trial) and against sklearn's greedy function (restated, and the restatement against sklearn itself
with its random stream replaced), the C boundary of the new entries (struct layout, the limits, which need no GPU) and the options."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import gmm_oracle as G           # noqa: E402
import kmeanspp_oracle as KPP    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [("separated", 2000, 4, 6, 5), ("overlapping", 3001, 33, 3, 2), ("overlapping", 5000, 16, 50, 7), ("overlapping", 1000, 10, 10, 1)]


def data(kind, N, D, K, seed):
    return (G.separated if kind == "separated" else G.overlapping)(N, D, K, seed=seed)[0]


@pytest.mark.parametrize("case", CASES)
def test_oracle_with_one_trial_picks_the_rows_of_the_host_seeding(case):
    from dmvae_hip.gmm import kmeans_plusplus
    kind, N, D, K, seed = case
    X = data(kind, N, D, K, seed)
    X64 = X.astype(np.float64)
    centers = kmeans_plusplus(X, K, np.random.RandomState(seed))
    # the same stream in the order the host function consumes it: randint(n) for the first centre, one random_sample() per further one
    rs = np.random.RandomState(seed)
    u = np.empty((K, 1))
    u[0, 0] = (rs.randint(N) + 0.5) / N              # floor(u n) is that row
    u[1:, 0] = [rs.random_sample() for _ in range(K - 1)]
    rows, _, _ = KPP.kmeanspp(X, K, u, local_trials=1)
    # u * tot is off every boundary: the oracle's "first running sum > target" and the host's searchsorted (first >= target) agree, with
    # the oracle's total (the last running sum) as with the host's (d2.sum()), and neither needs its clamp
    d2 = KPP.dist2(X64, rows[0])
    for k in range(1, K):
        cum = np.cumsum(d2)
        for tot in (cum[-1], d2.sum()):
            t = u[k, 0] * tot
            i = int(np.searchsorted(cum, t, side="left"))
            assert tot > 0 and i == int(np.searchsorted(cum, t, side="right")) and i <= np.flatnonzero(d2 > 0)[-1], (k, i)
        d2 = np.minimum(d2, KPP.dist2(X64, rows[k]))
    assert np.array_equal(X64[rows], centers), (rows,)


class FedStream(np.random.RandomState):
    """a RandomState whose draws inside sklearn's _kmeans_plusplus come from u [K][T]"""

    def __init__(self, u):
        super().__init__(0)
        self.u, self.k = np.asarray(u, dtype=np.float64), 1

    def choice(self, n, p=None, **kw):
        return KPP.uniform_row(self.u[0, 0], n)

    def uniform(self, low=0.0, high=1.0, size=None):
        v = self.u[self.k, :size].copy()
        self.k += 1
        return v


@pytest.mark.parametrize("case", CASES)
def test_greedy_oracle_picks_the_rows_of_sklearns_function(case):
    kind, N, D, K, seed = case
    X = data(kind, N, D, K, seed)
    T = KPP.trials(K, 0)
    assert T == 2 + int(np.log(K))
    u = np.random.RandomState(100 + seed).random_sample((K, T))
    rows, cands, pots = KPP.kmeanspp(X, K, u, local_trials=0)
    restated = KPP.sklearn_restated(X, K, u)
    assert np.array_equal(rows, restated), (rows, restated)
    assert all(len(set(c)) > 1 for c in cands[1:])            # the trials are real alternatives, not T copies of one row
    from sklearn.cluster import kmeans_plusplus
    centers, idx = kmeans_plusplus(X.astype(np.float64), K, random_state=FedStream(u))
    assert np.array_equal(idx, restated), (idx, restated)
    assert np.array_equal(centers, X.astype(np.float64)[rows])


def test_first_smallest_potential_wins_a_tie():
    X = np.array([[0.0], [1.0], [1.0], [5.0]])
    # round 1 from row 0: d2 = [0, 1, 1, 25]; both trials land on the equal rows 1 and 2, whose potentials tie: the first is kept
    u = np.array([[0.1, 0.0], [0.5 / 27, 1.5 / 27]])
    rows, cands, pots = KPP.kmeanspp(X, 2, u, local_trials=2)
    assert list(cands[1]) == [1, 2] and pots[1, 0] == pots[1, 1] and list(rows) == [0, 1]
    # all rows equal: tot = 0, every draw is floor(u n)
    rows, cands, _ = KPP.kmeanspp(np.ones((4, 2)), 3, np.array([[0.3], [0.99], [0.5]]), local_trials=1)
    assert list(rows) == [1, 3, 2]
    # never a row with d2 = 0, also with u at the top of its range
    row, cum, tot = KPP.select(np.array([0.0, 2.0, 0.0, 0.0]), np.float32(1.0 - 2.0 ** -24))
    assert row == 1 and tot == 2.0


def test_seed_struct_matches_the_header_as_a_c_compiler_lays_it_out(tmp_path):
    from dmvae_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dmvae_hip.h"', 'int main(void) {']
    want = {}
    for cname, cls in (("dmvae_gmm_seed_config", _lib.GmmSeedConfig),):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        fields = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1)
                  for decl in body.split(";") if decl.strip() for part in decl.strip().split(",")]
        py = [f[0] for f in cls._fields_]
        assert fields == py, (cname, fields, py)
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f in fields]
        lines.append('printf("\\n");')
        want[cname] = [C.sizeof(cls)] + [getattr(cls, f).offset for f in py]
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines()}
    assert got == want
    # the mixture's own structs keep the layout tests/test_gmm_host.py pins
    assert C.sizeof(_lib.GmmConfig) == 36 and C.sizeof(_lib.GmmResult) == 16 * C.sizeof(C.c_void_p)


def test_seed_workspace_size_and_limits():
    """dmvae_gmm_seed_ws_bytes is host arithmetic: the shapes the models need are accepted, bad arguments are DMVAE_EINVAL, and what does
    not fit is refused with the limit named"""
    from dmvae_hip import _lib, DmvaeError, check

    def ws(N, D, K, R=1, T=1, flags=0):
        cfg = _lib.GmmSeedConfig(N=N, D=D, K=K, n_init=R, local_trials=T, seed=0, flags=flags)
        return _lib.lib.dmvae_gmm_seed_ws_bytes(C.byref(cfg))
    for D, K in ((64, 50), (256, 10), (10, 10), (1, 1), (33, 3), (3328, 4)):
        for T in (0, 1, 4):
            assert ws(65000, D, K, T=T) > 0, (D, K, T)
    assert ws(65000, 10, 10, 20) > ws(65000, 10, 10, 1)
    assert ws(65000, 10, 10, 1, 8) > ws(65000, 10, 10, 1, 1)
    assert ws(65000, 10, 10, 1, 0) == ws(65000, 10, 10, 1, 4)          # 2 + int(ln 10) = 4
    assert ws(10, 3, 10) > 0                                           # K = N
    # at least the state the kernels keep: d2 [R][N] f32, the candidates [R][K][T] and the rows [R][K] int32
    assert ws(65000, 10, 10, 20, 4) >= 20 * (65000 * 4 + 10 * 4 * 4 + 10 * 4)
    for bad in (ws(0, 10, 1), ws(100, 0, 10), ws(100, 10, 0), ws(100, 10, 10, 0), ws(9, 3, 10), ws(100, 10, 10, T=-1), ws(100, 10, 10, T=9),
                ws(100, 10, 10, flags=1)):
        assert bad == -1
    for args, pat in (((5000, 8, 1100, 1, 0), r"9 trials needs trials <= 8"), ((1000, 20000, 4), r"<= 65536 B of LDS"),
                      ((1000, 3328, 4, 1, 8), r"4 \* trials \* D \+ 4096 = 110592 <= 65536 B of LDS")):
        n = ws(*args)              # (the error text is the last call's)
        assert n == _lib.EUNSUPPORTED
        with pytest.raises(DmvaeError, match=pat):
            check(int(n), "dmvae_gmm_seed_ws_bytes")


def test_header_and_binding_name_the_new_entries():
    from dmvae_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "dmvae_hip.h")).read()
    for name in ("dmvae_gmm_seed_ws_bytes", "dmvae_gmm_seed", "dmvae_philox_uniform"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib, name)
    assert "dmvae_gmm_seed_config" in hdr


def test_seeding_options_default_to_host_and_reject_other_values():
    from dmvae_hip.gmm import DiagGMM, kmeans_plusplus_device      # noqa: F401  (the function exists)
    g = DiagGMM(6)
    assert g.seeding == "host" and g.local_trials == 1
    g = DiagGMM(6, seeding="device", local_trials=0)
    assert g.seeding == "device" and g.local_trials == 0
    for kw in (dict(seeding="gpu"), dict(seeding="device", local_trials=9), dict(seeding="device", local_trials=-1), dict(local_trials=0)):
        with pytest.raises(ValueError):
            DiagGMM(6, **kw)
    # the host seeding is what it was: a function of the seed, drawn from RandomState(seed)
    X, _ = G.separated(500, 4, 6, seed=5)
    from dmvae_hip.gmm import kmeans_plusplus
    rs = np.random.RandomState(3)
    want = np.stack([kmeans_plusplus(X, 6, rs) for _ in range(2)]).astype(np.float32)
    assert np.array_equal(DiagGMM(6, n_init=2, seed=3).seed_centers(X), want)


def test_cli_gmm_seeding_flag_defaults_to_host_and_rejects_other_values():
    sys.argv = ["train.py"]
    import importlib
    train = importlib.import_module("train")
    assert train.parser.parse_args([]).gmm_seeding == "host"
    assert train.parser.parse_args(["--gmm", "device", "--gmm_seeding", "device"]).gmm_seeding == "device"
    with pytest.raises(SystemExit):
        train.parser.parse_args(["--gmm_seeding", "sklearn"])
    assert "--gmm_seeding" in train.__doc__


def test_models_take_the_gmm_seeding_option():
    import base_models
    kw = dict(activation="relu", initializer="xavier")
    assert base_models.DeepMixtureVAE("a", "binary", 40, 6, 5, **kw).gmm_seeding == "host"
    assert base_models.DeepMixtureVAE("a", "binary", 40, 6, 5, gmm="device", gmm_seeding="device", **kw).gmm_seeding == "device"
    assert base_models.VaDE("a", "binary", 40, 6, 5, **kw).gmm_seeding == "host"
    assert base_models.VaDE("a", "binary", 40, 6, 5, gmm="device", gmm_seeding="device", **kw).gmm_seeding == "device"
    with pytest.raises(ValueError):
        base_models.VaDE("a", "binary", 40, 6, 5, gmm_seeding="gpu", **kw)
