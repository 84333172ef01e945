"""A dispatch policy written entirely on the IDLE ROSTER (``idle_roster_torch`` / ``run_hooked(roster=True, roster_targets=)``): every
slot, every second idle vehicle of a cluster with surplus goes to the nearest node of the HOTTEST cluster - the one with the most
orders waiting per idle vehicle in that slot - when that cluster is not its own.  A toy; what it shows is the shape of such a policy:

- it reads nothing keyed by vehicle id.  ``off`` [R, C + 1] gives the length of every idle list, ``cluster`` and ``node`` [R, V] say, by
  roster position, which list an entry belongs to and where the vehicle stands; the position inside the list is ``i - off[cluster]``;
- it answers by roster position too: ``targets[r, i]`` is the node roster entry ``i`` goes to (negative: stays), applied by
  ``apply_dispatch_roster_torch`` - or, inside the hooked day, by the day graph itself.  Entries behind ``off[r, C]`` are never read.

    python examples/roster_policy.py [replicas]

The same day is run twice - slot by slot through the entry points, and as ONE ``run_hooked`` launch with the policy captured into the
day graph - and both must end with the same counters.  The ``Simulation`` shell does not use the roster."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from vehicles_dispatch_simulator_amd import workloads
from vehicles_dispatch_simulator_amd._lib import COUNTER_NAMES


def build_policy(env, w, targets):
    """The policy as a function without arguments on the library's blocks (fixed addresses: capturable); writes `targets` [R, V]."""
    R, V, C, N = env.R, env.V, env.C, w.city.N
    n2c, cost = w.city.node2cluster, np.asarray(w.city.cost)
    # nearest[c, n]: the node of cluster c with the smallest RoadCost(n, node) = cost[node, n] (simulator.py:263-264)
    nearest = np.zeros((C, N), dtype=np.int64)
    for c in range(C):
        nodes = np.flatnonzero(n2c == c)
        nearest[c] = nodes[np.argmin(cost[nodes, :], axis=0)] if nodes.size else -1
    nearest_t = torch.from_numpy(nearest).cuda().reshape(-1)
    ob = env.obs_torch(inflight=False)                                   # [5, R, C]: idle_pre, idle_now, supply, cl_orders, inflight
    ro = env.idle_roster_torch()                                         # veh / node / cluster [R, V] by roster position, off [R, C + 1]
    iota = torch.arange(V, device="cuda", dtype=torch.int64)[None, :]

    def policy():
        off = ro["off"].to(torch.int64)
        n_idle = off[:, 1:] - off[:, :-1]                                 # [R, C] = len(Clusters[c].IdleVehicles)
        orders = ob[3].to(torch.int64)
        heat = orders * 1024 // (n_idle + 1)                              # orders of the slot per idle vehicle, fixed point
        hot = heat.argmax(dim=1)                                          # [R] the hottest cluster of every city
        surplus = n_idle + ob[2].to(torch.int64) - orders                 # as in examples/nearest_vehicle_policy.py
        live = ro["cluster"] >= 0                                         # entries of the roster (the tail reads -1)
        cl = ro["cluster"].to(torch.int64).clamp(min=0)
        node = ro["node"].to(torch.int64).clamp(min=0)
        pos = iota - off.gather(1, cl)                                    # position in the entry's own list
        go = live & (pos % 2 == 1) & (surplus.gather(1, cl) > 0) & (cl != hot[:, None]) & (heat.gather(1, hot[:, None]) > 0)
        to = nearest_t[hot[:, None] * N + node]
        targets.copy_(torch.where(go & (to >= 0), to, torch.full_like(to, -1)).to(torch.int32))

    return policy


def counters_line(cn):
    tot = cn.sum(axis=0)
    return ", ".join("%s %d" % (k, tot[i]) for i, k in enumerate(COUNTER_NAMES) if k != "evals")


if __name__ == "__main__":
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    w = workloads.tiny(vehicles=150)
    stream = torch.cuda.current_stream()
    cap = (w.vehicles + 63) // 64 * 64                                    # mass moves: tables of V entries, not the defaults sized for the order flow
    env = w.make_env(R, stream=stream.cuda_stream, idle_cap=cap, ring_cap=cap, far_cap=cap)
    init = w.vehicle_nodes(R)
    targets = torch.full((R, env.V), -1, dtype=torch.int32, device="cuda")
    env.reset(init)
    policy = build_policy(env, w, targets)

    # 1. slot by slot: refresh the roster, decide, apply (the roster must be fresh: nothing may change a list in between)
    for t in range(env.T):
        env.step()
        env.obs_torch(inflight=False)
        env.idle_roster_torch()
        policy()
        env.apply_dispatch_roster_torch(targets)
        env.advance()
    env.sync()
    stepwise = env.counters()

    # 2. one launch: the policy captured, the roster refresh and the dispatch as nodes of the day graph
    side = torch.cuda.Stream()
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        policy()
    stream.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        policy()
    env.reset(init)
    env.run_hooked(env.T, policy_graph=graph, inflight=False, roster=True, roster_targets=targets)
    env.sync()
    hooked = env.counters()
    env.close()

    print("slot by slot : " + counters_line(stepwise))
    print("one launch   : " + counters_line(hooked))
    same = bool((stepwise == hooked).all())
    print("%d cities x %d slots, %d dispatches: both days end with %s counters" % (R, env.T, int(hooked[:, 4].sum()), "the SAME" if same else "DIFFERENT"))
    sys.exit(0 if same and hooked[:, 4].sum() > 0 else 1)
