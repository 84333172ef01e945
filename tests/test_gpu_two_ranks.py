"""Two ranks of the real engine (libvds on the GPU, one process each) under torch.distributed.run: replica sharding by global
index, per-rank device counters, one all-reduce per day - the N > 1 code path of bench.py with the engine in it, on the one GPU
the test box has (collective over gloo: RCCL does not take two ranks on one device).  The all-reduced totals must equal the
CPU oracle's sums over ALL replicas of the job."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle
from vehicles_dispatch_simulator_amd import workloads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("neighbor", [False, True])
def test_two_ranks_share_the_job(neighbor):
    total = 11                                   # 6 + 5 replicas
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "two_rank_worker.py"), str(total), "1" if neighbor else "0"]
    res = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    out = json.loads([l for l in res.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert out["world"] == 2 and out["allreduce_calls"] == 1
    assert out["kernel"] == ("k_dfs_dense" if neighbor else "k_tick_dense")
    w = workloads.tiny(neighbor=neighbor, vehicles=60 if neighbor else 150)
    init = w.vehicle_nodes(total)
    exp = np.zeros(8, dtype=np.int64)
    first_rank_orders = 0
    for r in range(total):
        o = Oracle(w.city.cost, w.city.node2cluster, w.nbr_off, w.nbr_idx, w.depth_limit, w.neighbor_can_server,
                   w.release_min, w.pickup, w.delivery, w.vehicles)
        o.reset(init[r]); o.run_day()
        oc = o.counters()
        exp[0] += oc["order_num"]; exp[1] += oc["reject_num"]; exp[2] += oc["wait_sum"]; exp[4] += oc["evals"]
        if r < 6:
            first_rank_orders += oc["order_num"]
    got = np.array(out["totals"], dtype=np.int64)
    assert got[0] == exp[0] and got[1] == exp[1] and got[2] == exp[2] and got[4] == exp[4], (got.tolist(), exp.tolist())
    assert out["rank0_orders"] == first_rank_orders


def test_bench_py_itself_with_two_ranks():
    """The driver's N > 1 launch line with bench.py ITSELF as the program (not a test worker): two ranks, replicas sharded by
    global index, weak scaling (R per rank fixed), one counter all-reduce per day, max-over-ranks timing, rank 0 prints the
    line.  Both ranks sit on this box's one GPU, so the collective runs over gloo (VDS_BENCH_BACKEND); everything else is the
    code an 8-GPU node runs (scripts/run_8gpu.sh).  The all-reduced totals of the last day equal the CPU oracle's sums over all
    2 R replicas."""
    Rr = 24
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full",
           "--replicas", str(Rr), "--no-cpu-baseline", "--no-neighbour-leg", "--distinct-days", "0", "--no-hooked-leg", "--no-distinct-all"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VDS_BENCH_BACKEND="gloo")
    res = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    out = json.loads([l for l in res.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["config"]["replicas_total"] == 2 * Rr and out["config"]["replicas_per_gpu"] == Rr
    assert out["collective"]["world_size"] == 2 and out["collective"]["backend"] == "gloo" and out["collective"]["allreduce_calls"] >= 3
    assert out["value"] > 0 and abs(out["value"] - 148 * 2 * Rr * 2 / (out["ms_per_step"] * 2e-3)) < 1e-6 * out["value"]
    w = workloads.didi_day("cfg2")
    init = w.vehicle_nodes(2 * Rr)               # global replica seeds: rank 1 owns replicas Rr .. 2 Rr - 1
    # rank r's first replica is GLOBAL replica r R: its start nodes are the draws of random.Random(veh_seed + r R)
    import zlib
    pr = out["per_rank"]
    assert pr["first_replica"] == [0, Rr] and pr["first_replica_seed"] == [w.veh_seed, w.veh_seed + Rr]
    assert pr["first_replica_nodes_crc32"] == [zlib.crc32(np.ascontiguousarray(init[0]).tobytes()), zlib.crc32(np.ascontiguousarray(init[Rr]).tobytes())]
    assert pr["first_replica_nodes_crc32"][0] != pr["first_replica_nodes_crc32"][1]
    assert len(pr["ms_per_step"]) == 2 and pr["ms_per_step_max"] == max(pr["ms_per_step"]) and abs(pr["ms_per_step_max"] - out["ms_per_step"]) < 1e-6 * out["ms_per_step"]
    assert out["collective"]["allreduce_us"] > 0
    exp = dict(order_num=0, reject_num=0, wait_sum=0, evals=0)
    for r in range(2 * Rr):
        o = Oracle(w.city.cost, w.city.node2cluster, w.nbr_off, w.nbr_idx, w.depth_limit, w.neighbor_can_server,
                   w.release_min, w.pickup, w.delivery, w.vehicles)
        o.reset(init[r]); o.run_day()
        oc = o.counters()
        for k in exp: exp[k] += oc[k]
    assert out["aggregate_counters_last_day"] == exp
