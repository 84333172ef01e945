"""Reject rate against fleet size in ONE handle: R cities of the tiny workload, city r with a fleet of its own from 0 to V vehicles
(``set_fleet``; the reference: one ``Simulation(VehiclesNumber=...)`` per fleet size, ``simulator.py:101, :347``).  One reset, one
day, one table of rejects and mean pickup wait per fleet size - then a second day that starts where the vehicles ended the first,
without the start nodes passing through the host (``reset_torch(vehicles_torch(...)["node"])``).  The city with the full fleet must
equal a plain handle of one city: the example exits non-zero otherwise.

    python examples/fleet_sweep.py [replicas]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from vehicles_dispatch_simulator_amd import workloads


def table(title, fleet, cn):
    print(title)
    print("  fleet  orders  rejects  reject share  mean wait (min)")
    for f, c in zip(fleet, cn):
        served = c[0] - c[1]
        print("  %5d  %6d  %7d  %11.1f%%  %s" % (f, c[0], c[1], 100.0 * c[1] / max(c[0], 1), "%15.2f" % (c[3] / served) if served else "              -"))


if __name__ == "__main__":
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    w = workloads.tiny()
    V = w.vehicles
    fleet = np.linspace(0, V, R).round().astype(np.int32)                 # city r has fleet[r] vehicles; the last one all of them
    nodes = np.repeat(w.vehicle_nodes(1), R, axis=0)                      # one row of start nodes: city r uses its first fleet[r]
    env = w.make_env(R, stream=torch.cuda.current_stream().cuda_stream)
    env.set_fleet(fleet)
    env.reset(nodes)
    env.run(env.T)
    env.sync()
    day1 = env.counters().copy()
    table("day 1 (every city from the same start nodes)", fleet, day1)
    # day 2 from where day 1 ended: the node plane of the handle's own block is the start-node tensor (absent vehicles read -1 and
    # are not looked at)
    env.reset_torch(env.vehicles_torch(state=False, cluster=False, arrive_min=False, order=False)["node"])
    env.run(env.T)
    env.sync()
    day2 = env.counters().copy()
    table("day 2 (every city from where its vehicles ended day 1)", fleet, day2)
    env.close()
    # the full fleet against a handle that never had a map
    plain = w.make_env(1)
    plain.reset(nodes[:1])
    plain.run(plain.T)
    ref = plain.counters()[0].copy()
    plain.close()
    ok = bool((day1[-1] == ref).all()) and int(fleet[-1]) == V and bool((day1[0, 1] == day1[0, 0]))
    print("%d cities, fleets %d .. %d: the full fleet's counters %s a plain handle's" % (R, fleet[0], fleet[-1], "EQUAL" if ok else "DIFFER FROM"))
    sys.exit(0 if ok else 1)
