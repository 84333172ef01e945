"""bench.py without --full: the timed days, --dump-outputs and the one line, nothing else.  What the dump holds is what the
timed days computed: every sampled replica's orders equal the CPU oracle's day for that replica."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle
from vehicles_dispatch_simulator_amd import workloads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("roofline", "cpu_baseline", "cpu_baseline_all_cores", "per_replica_days", "neighbour_search", "stress", "hooked_slot",
             "episode_reset", "episode_turnover", "fallbacks", "parity_check_vs_oracle")


def test_plain_bench_run_prints_the_headline_and_dumps_the_last_day(tmp_path):
    R, steps, warmup = 128, 2, 1
    dump = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--replicas", str(R), "--dump-outputs", dump]
    res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    out = json.loads([l for l in res.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert out["full"] is False
    assert out["metric"] == "env-steps x replicas / sec (192-cluster, 10k vehicles)" and out["unit"] == "env-steps*replicas/s"
    assert out["higher_is_better"] is True and out["dtype"] == "int32" and out["n_gpus"] == 1
    assert out["steps"] == steps and out["warmup"] == warmup
    T = out["config"]["ticks_per_step"]
    assert T == 148 and out["config"]["replicas_per_gpu"] == R
    assert out["value"] > 0 and abs(out["value"] - T * R / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert out["aggregate_counters_last_day"]["order_num"] == R * 199999
    assert not [k for k in FULL_ONLY if k in out] and "collective" not in out
    assert list(out["leg_seconds"]) == ["import, workload, handle, warm-up, timed days", "dump_outputs"]
    assert out["dump_outputs"]["dir"] == dump and out["dump_outputs"]["replicas_sampled"] == 16

    w = workloads.didi_day("cfg2")
    init = w.vehicle_nodes(R)
    replicas = np.load(os.path.join(dump, "replicas.npy")).astype(np.int64)
    got = {k: np.load(os.path.join(dump, "order_%s.npy" % k)) for k in ("status", "vehicle", "wait")}
    assert replicas.shape == (16,) and got["status"].shape == (16, w.release_min.shape[0])
    for i, r in enumerate(replicas.tolist()):
        o = Oracle(w.city.cost, w.city.node2cluster, w.nbr_off, w.nbr_idx, w.depth_limit, w.neighbor_can_server,
                   w.release_min, w.pickup, w.delivery, w.vehicles)
        o.reset(init[r]); o.run_day()
        exp = o.orders()
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(got[k][i], exp[k].astype(got[k].dtype), err_msg="replica %d %s" % (r, k))
