"""Generator of the fleet-size fixtures.  Runs ONLY in the build container (needs the reference).

    python tests/golden/make_fleet_golden.py

A replica with a fleet of its own (vds_set_fleet) has to behave like ``Simulation(VehiclesNumber = fleet[r])``
(simulator.py:101, :347, :249-258).  The tests reach that claim through an oracle built with ``V = fleet[r]``; this file pins it
to the unmodified reference itself: ONE city, ONE order day and ONE seed run at several ``VehiclesNumber``, each run recorded like
a case of the fuzz corpus (make_fuzz_golden.generate: per-tick counters, observation planes, lists in container order, per-order
results).  Data only.

    case A   12 clusters, no neighbour search, about 600 orders: VehiclesNumber 0, 1, 2, 33, 64, 65, 139, 140
    case B   12 clusters, neighbour search of depth 2:            VehiclesNumber 1, 20, 50

Both cities take the corpus' "mul" cost style with factor 8: with plain costs 139 and 140 vehicles reject the same 7 of 599
orders (tried: plain, 3, 5), with trips eight times as long the 140th vehicle still serves two orders more.

Asserted here (and again by tests/test_fleet_expect.py):
  * the start nodes of a smaller run are a prefix of the largest run's - one seed draws one node per vehicle, in vehicle order;
  * any two sizes of a case reject a different number of orders, so a replica run at the wrong size cannot pass.

File: tests/golden/fleetpack_0.npz, keys "<run>/<array>" with <run> = fleetA_140, ...; what a run shares with its case's largest
run (the city, the order day, the settings) is stored with the largest run only, helpers of the tests merge it back.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import ref_harness as rh  # noqa: E402
import make_fuzz_golden as mf  # noqa: E402

CASES = {
    "fleetA": dict(sizes=(0, 1, 2, 33, 64, 65, 139, 140), depth=0, neighbor=False, O=600, seeds=(7301, 8301, 9301)),
    "fleetB": dict(sizes=(1, 20, 50), depth=2, neighbor=True, O=700, seeds=(7302, 8302, 9302)),
}
# per-run arrays: everything else must equal the largest run's and is stored there only
OWN = ("V", "veh_node", "order_num", "reject_num", "wait_sum", "dispatch_num", "dispatch_cost", "sum_order_value", "dispatch_log",
       "o_status", "o_vehicle", "o_wait")


def spec(case, V):
    c = CASES[case]
    return dict(side_m=3200, C=12, N=120, style="mul", style_k=8, depth=c["depth"], neighbor=c["neighbor"], tick=10, window=None,
                dispatch=False, city_seed=c["seeds"][0], order_seed=c["seeds"][1], veh_seed=c["seeds"][2], V=V, O=c["O"], extra=0,
                empty=[], cluster_mode="KmeansClustering", focus=None)


def own_key(k):
    return k in OWN or k.startswith("t_") or k.startswith("l_")


def main():
    if not rh.reference_available():
        raise SystemExit("reference not mounted: golden fixtures can only be generated in the build container")
    pack = {}
    for case, c in CASES.items():
        runs = {V: mf.generate("%s_%d" % (case, V), spec(case, V)) for V in c["sizes"]}
        top = max(c["sizes"])
        base = runs[top]
        rejects = {}
        for V, g in runs.items():
            assert int(g["V"]) == V and len(g["veh_node"]) == V
            assert (np.asarray(g["veh_node"]) == np.asarray(base["veh_node"])[:V]).all(), "start nodes of %d are no prefix" % V
            rejects[V] = int(g["reject_num"])
            for k, a in g.items():
                if V == top or own_key(k):
                    pack["%s_%d/%s" % (case, V, k)] = a
                else:
                    assert np.array_equal(np.asarray(a), np.asarray(base[k])), (case, V, k)
        assert len(set(rejects.values())) == len(rejects), rejects
        print(case, "rejects by VehiclesNumber:", rejects, "orders:", int(base["order_num"]))
    path = os.path.join(HERE, "fleetpack_0.npz")
    np.savez_compressed(path, **pack)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("fuzzpack_"))
    print("%s: %d bytes (largest fuzzpack: %d)" % (os.path.basename(path), os.path.getsize(path), largest))
    assert os.path.getsize(path) <= largest


if __name__ == "__main__":
    main()
