"""bench.py as the driver launches it for N > 1 -- rehearsed on ONE GPU with two gloo ranks (RCCL needs one GPU per rank; gloo lets the ranks
share the card).  It exercises what no single-process test reaches: the rank spawn, capture_step under the sharded exchange, the settle loop's
and the timed regions' collectives, the exchange diagnostics, the fp32-master sync in front of the per-kernel profiling leg, and the contract
itself: exit code 0 and exactly ONE JSON line on stdout.  (Round 4: the stale-master guard of the engine broke this path in two places -- in
capture_step and in the profiling leg -- and nothing but a rehearsal by hand noticed.)  Timings of such a run mean nothing.
The plain one-GPU run is checked as well: exactly --steps timed steps, none of the --full legs, and --dump-outputs files that do not
depend on how many untimed settle steps ran."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_line(cmd):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DMVAE_DP_FORCE"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.parametrize("form", ["weak", "strong"])
def test_bench_two_ranks_over_gloo_prints_one_json_line(form, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "6", "--warmup", "2", "--stable-warmup", "2",
           "--profile-steps", "2", "--no-cpu-baseline", "--elbo-epochs", "0", "--full", "--dump-outputs", str(tmp_path)]
    if form == "strong":
        cmd += ["--global-batch", "1024", "--rows", "4096"]           # 512 rows per rank
    else:
        cmd += ["--batch", "512", "--rows", "4096"]
    d = _bench_line(cmd)
    assert d["n_gpus"] == 2 and d["scaling"] == form and d["steps"] == 6 and d["warmup"] == 2
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "images/sec" and d["higher_is_better"] is True and d["data"] == "synthetic"
    assert d["config"]["per_gpu_batch"] == 512 and d["config"]["global_batch"] == 1024 and d["config"]["parallelism"] == "dp2"
    assert d["config"]["collective_backend"].startswith("gloo") and d["config"]["rccl_ranks"] == 0          # a rehearsal says so
    assert "reduce-scatter" in d["config"]["update"] and "one collective after the backward pass" in d["config"]["update"]
    assert len(d["rank_ms_per_step_min_max"]) == 3 and all(a <= b for a, b in d["rank_ms_per_step_min_max"])
    ex = d["exchange"]
    assert ex["exposed_us"] > 0 and ex["step_us"] >= ex["exposed_us"] and ex["exposed_us_min_over_ranks"] <= ex["exposed_us_max_over_ranks"]
    assert ex["self_check"] == "ok"              # the replicas' checksums after the first sharded step agreed (parallel.ShardedExchange.self_check)
    assert d["roofline"]["frac"] <= 1.0 and d["kernels_per_step"] >= 10            # the profiling leg ran (behind sync_master)
    assert d["outputs"]["arrays"] > 1 and os.path.exists(os.path.join(str(tmp_path), "loss_terms.npy"))      # dumped behind sync_master


def test_bench_plain_run_times_its_steps_and_dumps_reproducible_outputs(tmp_path):
    """The plain run: one region of exactly --steps steps, none of the --full legs.  Its --dump-outputs files hold the last timed
    step's loss terms and every trained parameter, and the untimed settle regions (whose count depends on the clock) leave them
    unchanged: the step path is bit-reproducible (no float atomics), so the dumps with and without settle regions are equal."""
    import numpy as np
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--batch", "512", "--rows", "4096"]
    dumps = {}
    for settle in (0, 4):
        out = str(tmp_path / ("settle%d" % settle))
        d = _bench_line(base + ["--stable-warmup", str(settle), "--dump-outputs", out])
        assert d["n_gpus"] == 1 and d["steps"] == 7 and d["warmup"] == 3 and d["unit"] == "images/sec" and d["higher_is_better"] is True
        assert d["ms_per_step"] > 0 and len(d["repeat_ms_per_step"]) == 1 and d["ms_per_step"] == d["repeat_ms_per_step"][0]
        assert (2 <= len(d["settle_ms_per_step"]) <= settle) if settle else d["settle_ms_per_step"] == []
        for k in ("roofline", "kernels", "exchange", "elbo50", "elbo", "cpu_baseline"):
            assert k not in d, k
        names = sorted(f[:-4] for f in os.listdir(out))
        assert d["outputs"]["arrays"] == len(names) and not d["outputs"]["sampled"] and "loss_terms" in names
        assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64 << 20
        dumps[settle] = {n: np.load(os.path.join(out, n + ".npy")) for n in names}
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in dumps[settle].values())
        assert abs(float(dumps[settle]["loss_terms"][0]) - d["last_loss"]) <= 1e-3 * abs(d["last_loss"])
    assert sorted(dumps[0]) == sorted(dumps[4])
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], dumps[4][n]), n
