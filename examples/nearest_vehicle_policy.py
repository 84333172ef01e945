"""A dispatch policy in the reference's own terms - ``for vehicle in cluster.IdleVehicles: ... RoadCost(vehicle.LocationNode, target)`` -
running INSIDE the engine's day graph: ``BatchedHooks=True`` + ``BatchedIdleHeads=L`` + ``BatchedPolicy``.  Every
slot each city finds its poorest cluster (waiting orders against idle vehicles and expected arrivals) and sends, from each of its K
richest clusters, the idle vehicle NEAREST to it among the first L of the cluster's list - not blindly the head of the list, which is all a
policy could name before it could see what stands at an ``idle_pos``.

    python examples/nearest_vehicle_policy.py [replicas]

Uses the small synthetic city of ``examples/demo_simulation.py`` (written to a temporary directory in the reference's ./data layout)."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from vehicles_dispatch_simulator_amd.config.setting import *          # noqa: F401,F403  (same names as the reference)
from vehicles_dispatch_simulator_amd.simulation import Simulation
from demo_simulation import write_synthetic_data_dir


class NearestVehicleAgent(Simulation):
    K = 3
    L = 8
    BatchedPolicyPlanes = ("idle_now", "supply", "cl_orders")

    def BatchedPolicy(self, ob):
        R, C = ob["idle_now"].shape
        surplus = ob["idle_now"] + ob["supply"] - ob["cl_orders"]                     # [R, C] int32
        src = torch.topk(surplus, self.K, dim=1).indices                              # the K richest clusters
        dst = torch.argmin(surplus, dim=1)                                            # the poorest
        target = self.node_of_cluster[dst].long()                                     # [R] a node of it
        node = ob["idle_node"].long().gather(1, src[:, :, None].expand(R, self.K, self.L))      # [R, K, L] LocationNode of the heads, -1 past the end
        # RoadCost(vehicle.LocationNode, target) = Map[start][end] = cost[end, start] (simulator.py:263-264)
        road = self.cost[(target[:, None, None] * self.N + node.clamp(min=0)).reshape(-1)].reshape(R, self.K, self.L)
        road = torch.where(node >= 0, road, torch.full_like(road, 1 << 40))
        pos = torch.argmin(road, dim=2)                                               # idle_pos of the nearest one
        ok = (ob["idle_now"].gather(1, src) > 0) & (surplus.gather(1, src) - surplus.gather(1, dst[:, None]) > 2) & (src != dst[:, None])
        none = torch.full_like(src, -1)
        acts = torch.stack([torch.where(ok, src, none), torch.where(ok, pos, none), torch.where(ok, target[:, None].expand(R, self.K), none)], dim=2)
        self.moves += ok.sum()                                                        # (device state, updated in place: capturable)
        self.saved += torch.where(ok, road[:, :, 0] - road.gather(2, pos[:, :, None])[:, :, 0], torch.zeros_like(pos)).sum()
        return acts.int().contiguous()

    def BatchedPolicyBegin(self):
        self.moves.zero_()
        self.saved.zero_()


if __name__ == "__main__":
    os.environ.setdefault("TZ", "UTC")
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    data_dir = write_synthetic_data_dir(tempfile.mkdtemp(prefix="vds_nearest_"))
    sim = NearestVehicleAgent(ClusterMode=ClusterMode, DemandPredictionMode=DemandPredictionMode, DispatchMode=DispatchMode, VehiclesNumber=300,
                              TimePeriods=TIMESTEP, LocalRegionBound=LocalRegionBound, SideLengthMeter=2400, VehiclesServiceMeter=VehiclesServiceMeter,
                              NeighborCanServer=NeighborCanServer, FocusOnLocalRegion=FocusOnLocalRegion, DataDir=data_dir, Replicas=R, VehicleSeed=7,
                              BatchedHooks=True, BatchedIdleHeads=NearestVehicleAgent.L, Quiet=True)
    sim.CreateAllInstantiate()
    n2c = np.asarray(sim._world.node2cluster)
    C = sim.env.C
    sim.N = int(n2c.size)
    sim.cost = torch.from_numpy(np.ascontiguousarray(sim._world.cost).astype(np.int64)).cuda().reshape(-1)
    sim.node_of_cluster = torch.tensor([int(np.flatnonzero(n2c == c)[0]) if (n2c == c).any() else 0 for c in range(C)], dtype=torch.int32, device="cuda")
    sim.moves = torch.zeros((), dtype=torch.int64, device="cuda")
    sim.saved = torch.zeros((), dtype=torch.int64, device="cuda")
    for episode in range(3):
        if episode:
            sim.Reset()
        t0 = time.perf_counter()
        sim.SimCity()
        dt = time.perf_counter() - t0
        cn = sim.BatchedCounters().cpu().numpy()
        print("episode %d: %d cities x %d slots in %.1f ms (%s); dispatches %d at cost %d - %d less than sending the list heads; rejects per city %.1f" % (
            episode, R, sim.env.T, dt * 1e3, "one graph launch" if sim.BatchedPolicyGraphError is None else "slot by slot: " + sim.BatchedPolicyGraphError,
            int(cn[:, 6].sum()), int(cn[:, 7].sum()), int(sim.saved.item()), cn[:, 1].mean()))
    sim.env.close()
