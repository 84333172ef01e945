"""A dispatch policy that decides PER VEHICLE, written on the per-vehicle planes (``vehicles_torch``) and answered with one target node
per vehicle (``apply_dispatch_vehicles_torch`` / ``run_hooked(vehicle_planes=, vehicle_targets=)``): every slot, every idle vehicle whose
cluster has surplus (``idle_now + supply - cl_orders > 0``, as in ``examples/nearest_vehicle_policy.py``) goes to the nearest node of
the poorest neighbouring cluster, when that neighbour is poorer than its own cluster.  No list positions, no cap on the moves of a slot.

    python examples/per_vehicle_policy.py [replicas]

The learning signal of such a policy is what each vehicle earned: every slot the policy adds the ``value`` word of the per-vehicle
outcome block (``vehicle_outcomes_torch``, ``run_hooked(vehicle_outcomes=True)``) into a running per-vehicle return ``[R, V]`` on the
device, where the ``order`` word says the vehicle was matched.  Summed over the vehicles the day's return is the matched order value
of ``counters_torch`` (word 3), which the example checks.

The same day is run twice - slot by slot through the entry points, and as ONE ``run_hooked`` launch with the policy captured into the
day graph - and both must end with the same counters and the same returns."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from vehicles_dispatch_simulator_amd import workloads
from vehicles_dispatch_simulator_amd._lib import COUNTER_NAMES


def build_policy(env, w, targets, returns):
    """The policy as a function without arguments on the library's blocks (fixed addresses: capturable); writes `targets` [R, V] and
    adds the slot's earnings into `returns` [R, V] (int64)."""
    R, V, C, N = env.R, env.V, env.C, w.city.N
    n2c, cost = w.city.node2cluster, np.asarray(w.city.cost)
    # nearest[c, n]: the node of cluster c with the smallest RoadCost(n, node) = cost[node, n] (simulator.py:263-264)
    nearest = np.zeros((C, N), dtype=np.int64)
    for c in range(C):
        nodes = np.flatnonzero(n2c == c)
        nearest[c] = nodes[np.argmin(cost[nodes, :], axis=0)] if nodes.size else -1
    deg = max(len(nb) for nb in w.city.neighbors)
    nbr = np.full((C, max(deg, 1)), -1, dtype=np.int64)
    for c, nb in enumerate(w.city.neighbors):
        nbr[c, :len(nb)] = nb
    nearest_t, nbr_t = torch.from_numpy(nearest).cuda().reshape(-1), torch.from_numpy(nbr).cuda()
    ob = env.obs_torch(inflight=False)                                   # [5, R, C]: idle_pre, idle_now, supply, cl_orders, inflight
    pl = env.vehicles_torch(state=True, node=True, cluster=True, arrive_min=False, order=False)
    earned = env.vehicle_outcomes_torch()                                # [R, V, 4]: order, wait, value, pickup of the slot's match
    BIG = 1 << 30
    cidx = torch.arange(C, device="cuda")

    def policy():
        returns.add_(torch.where(earned[..., 0] >= 0, earned[..., 2], torch.zeros_like(earned[..., 2])).to(torch.int64))
        surplus = (ob[1] + ob[2] - ob[3]).to(torch.int64)                 # [R, C]
        around = torch.where(nbr_t >= 0, surplus[:, nbr_t.clamp(min=0)], torch.full((R,) + tuple(nbr_t.shape), BIG, device="cuda"))   # [R, C, deg]
        best = around.argmin(dim=2)                                       # the poorest neighbour of every cluster
        dst = nbr_t[cidx[None, :], best]                                  # [R, C]
        send = (surplus > 0) & (around.min(dim=2).values < surplus) & (dst >= 0)       # [R, C]
        cl = pl["cluster"].to(torch.int64).clamp(min=0)                   # [R, V]
        node = pl["node"].to(torch.int64).clamp(min=0)
        go = (pl["state"] == 0) & send.gather(1, cl)
        to = nearest_t[dst.gather(1, cl).clamp(min=0) * N + node]
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
    returns = torch.zeros((R, env.V), dtype=torch.int64, device="cuda")
    env.reset(init)
    policy = build_policy(env, w, targets, returns)

    # 1. slot by slot
    for t in range(env.T):
        env.step()
        env.obs_torch(inflight=False)
        env.vehicles_torch(state=True, node=True, cluster=True, arrive_min=False, order=False)
        env.vehicle_outcomes_torch()
        policy()
        env.apply_dispatch_vehicles_torch(targets)
        env.advance()
    env.sync()
    stepwise = env.counters()
    stepwise_returns = returns.clone()

    # 2. one launch: the policy captured, planes and targets as nodes of the day graph
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
    returns.zero_()
    env.run_hooked(env.T, policy_graph=graph, inflight=False, vehicle_planes=dict(state=True, node=True, cluster=True), vehicle_targets=targets,
                   vehicle_outcomes=True)
    env.sync()
    hooked = env.counters()
    matched_value = env.counters_torch()[:, 3].clone()                   # matched OrderValue per replica
    torch.cuda.synchronize()
    earned_ok = bool(torch.equal(returns.sum(dim=1), matched_value)) and bool(torch.equal(returns, stepwise_returns))
    total, best = int(returns.sum().item()), int(returns.max().item())
    env.close()

    print("slot by slot : " + counters_line(stepwise))
    print("one launch   : " + counters_line(hooked))
    print("per-vehicle return of the day: total %d (matched order value %d), best vehicle %d: %s" %
          (total, int(matched_value.sum().item()), best, "the vehicles' returns add up to the counters" if earned_ok else "MISMATCH"))
    same = bool((stepwise == hooked).all()) and earned_ok
    print("%d cities x %d slots, %d dispatches: both days end with %s counters" % (R, env.T, int(hooked[:, 4].sum()), "the SAME" if same else "DIFFERENT"))
    sys.exit(0 if same else 1)
