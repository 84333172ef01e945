"""The reference-compatible ``Simulation`` shell on the GPU: a subclass written the way a user of
the reference writes one (hooks + object views) must reproduce the day the unmodified reference
produced with the same dispatch policy (golden), incl. the container order the views expose."""
import random

import numpy as np
import pandas as pd
import pytest

from helpers import load_golden, make_oracle
from vehicles_dispatch_simulator_amd import world
from vehicles_dispatch_simulator_amd.config.setting import TIMESTEP
from vehicles_dispatch_simulator_amd.simulation import Simulation

pytestmark = pytest.mark.gpu


def world_from_golden(g):
    N, C = int(g["N"]), int(g["C"])
    nbr = [g["nbr_idx"][g["nbr_off"][c]:g["nbr_off"][c + 1]].tolist() for c in range(C)]
    t0 = np.datetime64("2016-11-01T00:00", "m")
    return world.World(node_id=np.arange(N) + 10**9, lon=np.linspace(104.02, 104.12, N), lat=np.linspace(30.62, 30.70, N),
                       cost=g["cost"], node2cluster=g["node2cluster"], neighbors=nbr, n_clusters=C, grid_w=4, grid_h=3,
                       depth_limit=int(g["depth_limit"]), cluster_nodes=[np.flatnonzero(g["node2cluster"] == c).tolist() for c in range(C)],
                       o_release=t0 + g["o_release_min"].astype("timedelta64[m]"), o_release_min=g["o_release_min"],
                       o_pickup=g["o_pickup"], o_delivery=g["o_delivery"], driver_ids=np.arange(int(g["V"])) + 9000)


def make_sim(g, cls, **kw):
    sim = cls(ClusterMode=str(g["cluster_mode"]), DemandPredictionMode="None", DispatchMode="Simulation",
              VehiclesNumber=int(g["V"]), TimePeriods=TIMESTEP, LocalRegionBound=(104.011, 104.125, 30.618, 30.703),
              SideLengthMeter=float(g["side_m"]), VehiclesServiceMeter=float(g["service_m"]),
              NeighborCanServer=bool(g["neighbor_can_server"]), FocusOnLocalRegion=False, Quiet=True, **kw)
    random.seed(int(g["seed"]))          # the reference's start positions come from the global stdlib RNG
    sim.CreateAllInstantiate(World=world_from_golden(g))
    return sim


class PolicySim(Simulation):
    """Same policy as tests/golden/make_golden.py::policy_factory, written against the object views."""

    def DispatchFunction(self):
        tick, N = self.step, len(self.NodeIDList)
        self.seen_idle.append([[v._index for v in c.IdleVehicles] for c in self.Clusters])
        self.seen_supply.append(self.SupplyExpect.copy())
        if tick % 3 != 0:
            return
        chosen = set()
        for c in self.Clusters:
            idle = c.IdleVehicles
            n = len(idle)
            if n >= 3:
                for m in range(min(2, n - 1)):
                    veh = idle[(tick * 7 + m * 3 + c.ID) % n]
                    if veh._index in chosen:
                        continue
                    chosen.add(veh._index)
                    self.DispatchVehicle(veh, int((tick * 2654435761 + c.ID * 40503 + m * 17) % N))


@pytest.mark.parametrize("name", ["tiny_dispatch", "tiny_dispatch_dfs2"])
def test_subclass_with_dispatch_hook_reproduces_reference_day(name):
    g = load_golden(name)
    sim = make_sim(g, PolicySim)
    np.testing.assert_array_equal(sim._init_nodes[0], g["veh_node"])
    sim.seen_idle, sim.seen_supply = [], []
    sim.SimCity()
    assert sim.step == int(g["n_ticks"])
    assert (sim.OrderNum, sim.RejectNum, sim.TotallyWaitTime) == (int(g["order_num"]), int(g["reject_num"]), int(g["wait_sum"]))
    assert (sim.DispatchNum, sim.TotallyDispatchCost) == (int(g["dispatch_num"]), int(g["dispatch_cost"]))
    assert sim.SumOrderValue == int(g["sum_order_value"])
    for t in range(int(g["n_ticks"])):
        off = g["l_idle_off"][t]
        assert sim.seen_idle[t] == [g["l_idle_veh"][t][off[c]:off[c + 1]].tolist() for c in range(int(g["C"]))], t
        np.testing.assert_array_equal(sim.seen_supply[t], g["t_supply"][t])
    st = np.array([0 if o.ArriveInfo is None else (2 if o.ArriveInfo == "Reject" else 1) for o in sim.Orders])
    np.testing.assert_array_equal(st, g["o_status"])
    wt = np.array([-1 if o.PickupWaitTime is None else o.PickupWaitTime for o in sim.Orders])
    np.testing.assert_array_equal(wt, g["o_wait"])
    veh = np.array([-1 if o.Vehicle is None else o.Vehicle._index for o in sim.Orders])
    np.testing.assert_array_equal(veh, g["o_vehicle"])
    assert sim.RoadCost(3, 5) == int(g["cost"][5, 3])


class ViewCheckSim(Simulation):
    def GetNextStateFunction(self):
        o = self.oracle
        o.begin_tick()
        veh, L = o.vehicles(), o.lists()
        got_loc = np.array([v.LocationNode for v in self.Vehicles])
        np.testing.assert_array_equal(got_loc, veh["loc"])
        np.testing.assert_array_equal(np.array([v.Cluster.ID for v in self.Vehicles]), veh["cluster"])
        np.testing.assert_array_equal(np.array([-1 if v.DeliveryPoint is None else v.DeliveryPoint for v in self.Vehicles]), veh["dest"])
        np.testing.assert_array_equal(np.array([v.Orders[0].ID if v.Orders else -1 for v in self.Vehicles]), veh["order"])
        c = self.Clusters[self.step % len(self.Clusters)]
        a, b = L["arr_off"][c.ID], L["arr_off"][c.ID + 1]
        d = c.VehiclesArrivetime
        assert [v._index for v in d] == L["arr_veh"][a:b].tolist()
        assert [int((t - self._t0).total_seconds()) // 60 for t in d.values()] == L["arr_min"][a:b].tolist()
        assert len(c.Orders) == o.obs()["cl_orders"][c.ID] and c.PerMatchIdleVehicles == o.obs()["idle_pre"][c.ID]
        o.end_tick()


def test_object_views_follow_reference_semantics():
    g = load_golden("tiny_kmeans_dfs1")
    sim = make_sim(g, ViewCheckSim)
    sim.oracle = make_oracle(g)
    sim.SimCity()
    oo = sim.oracle.orders()
    arrived = np.array([o.ArriveInfo is not None and o.ArriveInfo.startswith("ArriveTime:") for o in sim.Orders])
    np.testing.assert_array_equal(arrived, oo["arrive_min"] >= 0)
    i = int(np.flatnonzero(arrived)[0])
    assert sim.Orders[i].ArriveInfo == "ArriveTime:" + str(sim._t0 + pd.Timedelta(minutes=int(oo["arrive_min"][i])))


def test_fast_forward_equals_hooked_loop_and_batches_replicas():
    g = load_golden("tiny_kmeans")
    sim = make_sim(g, Simulation, Replicas=5, VehicleSeed=321)
    sim.SimCity()                                 # no hook overridden -> one device run for the whole day
    assert (sim.OrderNum, sim.RejectNum, sim.TotallyWaitTime) == (int(g["order_num"]), int(g["reject_num"]), int(g["wait_sum"]))
    cn = sim.env.counters()
    assert cn.shape[0] == 5 and len(set(cn[:, 1].tolist())) > 1     # other replicas: other vehicle seeds
    sim2 = make_sim(g, Simulation)
    sim2.SimCity(FastForward=False)
    assert (sim2.OrderNum, sim2.RejectNum, sim2.TotallyWaitTime) == (sim.OrderNum, sim.RejectNum, sim.TotallyWaitTime)


def test_drop_in_from_data_directory_with_focus_region_and_reload(tmp_path):
    """The whole drop-in path: the reference's ./data layout on disk -> Simulation(...).CreateAllInstantiate()
    -> SimCity(), with FocusOnLocalRegion=True, must equal the day the unmodified reference produced from the same
    files (golden tiny_focus_grid); Reload() then runs another day from ./data/test/."""
    import os, shutil, time
    from oracle.ref_harness import write_reference_data_dir
    from test_world_loader import rebuild_inputs
    from vehicles_dispatch_simulator_amd import synth
    os.environ["TZ"] = "UTC"; time.tzset()
    g = load_golden("tiny_focus_grid")
    city, start, pick, dele = rebuild_inputs(g)
    write_reference_data_dir(str(tmp_path), city, start, pick, dele, n_drivers=int(g["V"]), cluster_mode="Grid")
    data = os.path.join(str(tmp_path), "data")
    bound = tuple(g["focus_bound"].tolist())
    sim = Simulation(ClusterMode="Grid", DemandPredictionMode="None", DispatchMode="Simulation", VehiclesNumber=int(g["V"]),
                     TimePeriods=TIMESTEP, LocalRegionBound=bound, SideLengthMeter=float(g["side_m"]),
                     VehiclesServiceMeter=float(g["service_m"]), NeighborCanServer=True, FocusOnLocalRegion=True, DataDir=data, Quiet=True)
    random.seed(int(g["seed"]))
    sim.CreateAllInstantiate("1101")
    np.testing.assert_array_equal(sim._init_nodes[0], g["veh_node"])
    assert len(sim.Orders) == g["o_pickup"].size and len(sim.Clusters) == int(g["C"])
    sim.SimCity()
    # ReadOrder's unstable sort is reproduced exactly (world.read_orders): the day is the reference's, order for order
    assert sim.step == int(g["n_ticks"]) and sim.OrderNum == int(g["order_num"])
    np.testing.assert_array_equal(sim._world.o_pickup, g["o_pickup"])
    np.testing.assert_array_equal(sim._world.o_delivery, g["o_delivery"])
    assert (sim.RejectNum, sim.TotallyWaitTime, sim.SumOrderValue) == (int(g["reject_num"]), int(g["wait_sum"]), int(g["sum_order_value"]))
    st = sim.env.orders(0, 1)
    np.testing.assert_array_equal(st["status"][0], g["o_status"])
    np.testing.assert_array_equal(st["vehicle"][0], g["o_vehicle"])
    # Reload: another day from data/test
    os.makedirs(os.path.join(data, "test"))
    start2, pick2, dele2 = synth.make_orders(77, city.N, 1500)
    write_reference_data_dir(os.path.join(str(tmp_path), "day2"), city, start2, pick2, dele2, n_drivers=int(g["V"]), cluster_mode="Grid", date="1102")
    shutil.copy(os.path.join(str(tmp_path), "day2", "data", "order_20161102.csv"), os.path.join(data, "test", "order_20161102.csv"))
    sim.Reload("1102")
    assert sim.OrderNum == 0 and 0 < len(sim.Orders) < 1500
    sim.SimCity()
    assert sim.OrderNum == len(sim.Orders) - 1
    from oracle.oracle import Oracle
    W = sim._world
    from vehicles_dispatch_simulator_amd.env import neighbors_to_csr
    off, idx = neighbors_to_csr(W.neighbors)
    o = Oracle(W.cost, W.node2cluster, off, idx, W.depth_limit, True, W.o_release_min, W.o_pickup, W.o_delivery, len(sim.Vehicles))
    o.reset(sim._init_nodes[0]); o.run_day()
    oc = o.counters()
    assert (sim.RejectNum, sim.TotallyWaitTime, sim.SumOrderValue) == (oc["reject_num"], oc["wait_sum"], oc["sum_order_value"])


class BatchedPolicySim(Simulation):
    """A policy over ALL replicas at once (``BatchedHooks=True``): every third slot, each replica sends the head of the idle
    lists of its three fullest clusters towards the cluster with the most waiting supply deficit - pure torch on the GPU."""

    def RewardFunction(self):
        self.reward_calls += 1
        self.last_rejects = self.BatchedCounters()[:, 1].clone()

    def DispatchFunction(self):
        import torch
        ob = self.BatchedObs
        idle = ob["idle_now"]                                  # [R, C]
        R, C = idle.shape
        self.action_log.append(None)
        if self.step % 3 != 0:
            return None
        K = 3
        cnt, src = torch.topk(idle, K, dim=1)                  # fullest clusters
        deficit = ob["cl_orders"] - idle + torch.arange(C, device=idle.device)[None, :] % 3   # (ties broken by id, deterministic)
        tgt_cluster = torch.argmax(deficit, dim=1)             # [R]
        tgt_node = self.first_node[tgt_cluster]                # [R]
        acts = torch.full((R, K + 2, 3), -1, dtype=torch.int32, device=idle.device)           # (with empty slots)
        ok = (cnt >= 2) & (src != tgt_cluster[:, None])
        acts[:, 1:K + 1, 0] = torch.where(ok, src, torch.full_like(src, -1)).to(torch.int32)
        acts[:, 1:K + 1, 1] = 0
        acts[:, 1:K + 1, 2] = tgt_node[:, None].to(torch.int32)
        self.action_log[-1] = acts.cpu().numpy()
        return acts


class GraphPolicySim(Simulation):
    """``BatchedPolicy``: the dispatch policy as a pure device function - every slot each replica sends the head of the idle
    lists of its two fullest clusters towards the cluster with the largest deficit (idle + expected arrivals against waiting
    orders).  Its state (a slot counter and a log of the actions) lives in CUDA tensors updated in place, so it can be captured."""

    def BatchedPolicy(self, ob):
        import torch
        idle, supply, demand = ob["idle_now"], ob["supply"], ob["cl_orders"]
        R, C = idle.shape
        K = 2
        cnt, src = torch.topk(idle, K, dim=1)
        deficit = demand - idle - supply + torch.arange(C, device=idle.device, dtype=torch.int32)[None, :] % 3
        tgt_cluster = torch.argmax(deficit, dim=1)
        tgt_node = self.first_node[tgt_cluster].to(torch.int32)
        ok = (cnt >= 2) & (src != tgt_cluster[:, None])
        acts = torch.stack([torch.where(ok, src, torch.full_like(src, -1)).to(torch.int32), torch.zeros((R, K), dtype=torch.int32, device=idle.device),
                            tgt_node[:, None].expand(R, K)], dim=2).contiguous()
        self.log.index_copy_(0, self.slot, acts[None])
        self.slot += 1
        return acts

    def BatchedPolicyBegin(self):
        self.slot.zero_()
        self.log.fill_(-1)
        self.begin_calls += 1


def test_batched_policy_runs_as_one_day_graph_and_matches_oracle_replay():
    """``BatchedHooks`` + ``BatchedPolicy``: the reference-API user reaches ``vds_run_hooked`` - the captured policy inside the day
    graph, one launch per day.  Every replica equals a CPU oracle replaying the actions the policy logged on the device; the
    slot-by-slot form of the same policy (``BatchedPolicyGraph = False``) gives the same day."""
    import torch
    g = load_golden("tiny_kmeans")
    R = 32
    n2c = g["node2cluster"]
    C = int(g["C"])
    first_node = torch.tensor([int(np.flatnonzero(n2c == c)[0]) if (n2c == c).any() else 0 for c in range(C)], device="cuda")
    days = {}
    for graph in (True, False):
        sim = make_sim(g, GraphPolicySim, Replicas=R, VehicleSeed=977, BatchedHooks=True)
        T = sim.env.T
        sim.BatchedPolicyGraph = graph
        sim.first_node, sim.begin_calls = first_node, 0
        sim.slot = torch.zeros(1, dtype=torch.int64, device="cuda")
        sim.log = torch.full((T + 4, R, 2, 3), -1, dtype=torch.int32, device="cuda")
        init = sim._init_nodes.copy()
        sim.SimCity()
        assert sim.step == T and sim.begin_calls == 1
        if graph:
            assert sim.BatchedPolicyGraphError is None, sim.BatchedPolicyGraphError
        assert int(sim.slot.item()) == T
        log = sim.log.cpu().numpy()
        assert (log[T:] == -1).all()
        got, cn = sim.env.orders(), sim.env.counters()
        days[graph] = (got, cn, log)
        if graph:
            n_dispatched = 0
            for r in range(R):
                o = make_oracle(g)
                o.reset(init[r])
                for t in range(T):
                    o.begin_tick()
                    L = o.lists()
                    vehs, tgts = [], []
                    for cl, pos, tg in log[t, r]:
                        if cl >= 0:
                            vehs.append(int(L["idle_veh"][L["idle_off"][cl] + pos])); tgts.append(int(tg))
                    if vehs:
                        o.dispatch(np.array(vehs), np.array(tgts))
                        n_dispatched += len(vehs)
                    o.end_tick()
                exp, oc = o.orders(), o.counters()
                for k in ("status", "vehicle", "wait"):
                    np.testing.assert_array_equal(got[k][r], exp[k], err_msg="replica %d %s" % (r, k))
                assert (cn[r, 0], cn[r, 1], cn[r, 3], cn[r, 4], cn[r, 5], cn[r, 7]) == (oc["order_num"], oc["reject_num"], oc["wait_sum"], oc["dispatch_num"], oc["dispatch_cost"], oc["evals"]), r
            assert n_dispatched > R * 20
            assert sim.RejectNum == cn[0, 1] and sim.DispatchNum == cn[0, 4]
            # a second episode on the same handle reuses the capture (and the library's day graph)
            st = sim._bp_state
            sim.Reset()
            sim.SimCity()
            assert sim._bp_state is st and sim.begin_calls == 2 and int(sim.slot.item()) == T and sim.step == T
            cn2 = sim.env.counters()
            assert (cn2[:, 0] == cn[:, 0]).all() and int(cn2[:, 4].sum()) > R * 20
        sim.env.close()
    for k in ("status", "vehicle", "wait"):
        np.testing.assert_array_equal(days[True][0][k], days[False][0][k])
    np.testing.assert_array_equal(days[True][1], days[False][1])
    np.testing.assert_array_equal(days[True][2], days[False][2])


class UncapturablePolicySim(GraphPolicySim):
    """The same policy with a host synchronisation inside (``.item()``): it cannot be captured."""

    def BatchedPolicy(self, ob):
        acts = GraphPolicySim.BatchedPolicy(self, ob)
        self.host_reads += int(ob["idle_now"].sum().item() >= 0)
        return acts


def test_batched_policy_that_cannot_be_captured_runs_slot_by_slot():
    """A ``BatchedPolicy`` the graph capture refuses: the reason is kept (``BatchedPolicyGraphError``) and the day runs slot by slot with
    the same results as the captured form of the same policy."""
    import torch
    g = load_golden("tiny_kmeans")
    R = 16
    n2c = g["node2cluster"]
    C = int(g["C"])
    first_node = torch.tensor([int(np.flatnonzero(n2c == c)[0]) if (n2c == c).any() else 0 for c in range(C)], device="cuda")
    out = {}
    for cls in (GraphPolicySim, UncapturablePolicySim):
        sim = make_sim(g, cls, Replicas=R, VehicleSeed=31, BatchedHooks=True)
        T = sim.env.T
        sim.first_node, sim.begin_calls, sim.host_reads = first_node, 0, 0
        sim.slot = torch.zeros(1, dtype=torch.int64, device="cuda")
        sim.log = torch.full((T + 4, R, 2, 3), -1, dtype=torch.int32, device="cuda")
        sim.SimCity()
        assert sim.step == T and int(sim.slot.item()) == T
        if cls is UncapturablePolicySim:
            assert sim.BatchedPolicyGraphError is not None and sim.host_reads >= T
        else:
            assert sim.BatchedPolicyGraphError is None
        out[cls] = (sim.env.orders(), sim.env.counters(), sim.log.cpu().numpy())
        sim.env.close()
    a, b = out[GraphPolicySim], out[UncapturablePolicySim]
    for k in ("status", "vehicle", "wait"):
        np.testing.assert_array_equal(a[0][k], b[0][k])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2][:T], b[2][:T])


def test_batched_hooks_policy_over_all_replicas_matches_oracle_replay():
    """``BatchedHooks``: hook order as SimCity's, observations / policy / actions on the device for 64 cities; every
    replica equals a CPU oracle that replays ITS action log (vehicle = head of the named idle list at that moment)."""
    import torch
    g = load_golden("tiny_kmeans")
    R = 64
    sim = make_sim(g, BatchedPolicySim, Replicas=R, VehicleSeed=4242, BatchedHooks=True)
    sim.reward_calls, sim.action_log = 0, []
    n2c = g["node2cluster"]
    C = int(g["C"])
    sim.first_node = torch.tensor([int(np.flatnonzero(n2c == c)[0]) if (n2c == c).any() else 0 for c in range(C)], device="cuda")
    init = sim._init_nodes.copy()
    sim.SimCity()
    T = sim.env.T
    assert sim.reward_calls == T and len(sim.action_log) == T and sim.step == T
    assert sum(a is not None for a in sim.action_log) == (T + 2) // 3
    got, cn = sim.env.orders(), sim.env.counters()
    n_dispatched = 0
    for r in range(R):
        o = make_oracle(g)
        o.reset(init[r])
        for t in range(T):
            o.begin_tick()
            a = sim.action_log[t]
            if a is not None:
                L = o.lists()
                vehs, tgts = [], []
                for cl, pos, tg in a[r]:
                    if cl >= 0:
                        vehs.append(int(L["idle_veh"][L["idle_off"][cl] + pos])); tgts.append(int(tg))
                if vehs:
                    o.dispatch(np.array(vehs), np.array(tgts))
                    n_dispatched += len(vehs)
            o.end_tick()
        exp, oc = o.orders(), o.counters()
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(got[k][r], exp[k], err_msg="replica %d %s" % (r, k))
        assert (cn[r, 0], cn[r, 1], cn[r, 3], cn[r, 4], cn[r, 5], cn[r, 7]) == (oc["order_num"], oc["reject_num"], oc["wait_sum"], oc["dispatch_num"], oc["dispatch_cost"], oc["evals"]), r
    assert n_dispatched > R * 20
    # the shell's own fields describe replica `Replica` (0), its views were refreshed after the day
    assert sim.RejectNum == cn[0, 1] and sim.DispatchNum == cn[0, 4] and sim.TotallyDispatchCost == cn[0, 5]
    idle_total = sum(len(c.IdleVehicles) for c in sim.Clusters)
    fly_total = sum(len(c.VehiclesArrivetime) for c in sim.Clusters)
    assert idle_total + fly_total == len(sim.Vehicles)
    assert int((sim.last_rejects.cpu().numpy() == cn[:, 1]).sum()) >= 1     # (counters of the last slot, read inside the hook)
    sim.env.close()


class CountingPolicySim(GraphPolicySim):
    """GraphPolicySim that counts the calls of ``BatchedPolicy`` made under graph capture."""

    def BatchedPolicy(self, ob):
        import torch
        self.captures += int(torch.cuda.is_current_stream_capturing())
        return GraphPolicySim.BatchedPolicy(self, ob)


@pytest.mark.parametrize("outcomes", [False, True], ids=["no-outcomes", "outcomes"])
def test_reload_recaptures_the_batched_policy(tmp_path, outcomes):
    """``Reload`` to a day whose tables make the library re-make the handle's state tables (a longer and denser day: more slots, longer
    arrival rings): the policy captured on the first day read the old observation (and outcome) blocks.  After the Reload it is captured
    again, reads the live blocks, and both days equal the CPU oracle replaying the actions the policy logged on the device."""
    import os, shutil, time
    import torch
    from oracle.oracle import Oracle
    from oracle.ref_harness import write_reference_data_dir
    from test_world_loader import rebuild_inputs
    from vehicles_dispatch_simulator_amd import synth
    from vehicles_dispatch_simulator_amd.env import neighbors_to_csr
    os.environ["TZ"] = "UTC"; time.tzset()
    g = load_golden("tiny_focus_grid")
    city, start, pick, dele = rebuild_inputs(g)
    short = start < start[0] + 2 * 3600                           # day 1: the first two hours of the fixture's day
    write_reference_data_dir(str(tmp_path), city, start[short], pick[short], dele[short], n_drivers=int(g["V"]), cluster_mode="Grid")
    data = os.path.join(str(tmp_path), "data")
    start2, pick2, dele2 = synth.make_orders(91, city.N, 6 * start.size)     # day 2: a whole day, six times the orders
    write_reference_data_dir(os.path.join(str(tmp_path), "day2"), city, start2, pick2, dele2, n_drivers=int(g["V"]), cluster_mode="Grid", date="1102")
    os.makedirs(os.path.join(data, "test"))
    shutil.copy(os.path.join(str(tmp_path), "day2", "data", "order_20161102.csv"), os.path.join(data, "test", "order_20161102.csv"))
    R = 16
    sim = CountingPolicySim(ClusterMode="Grid", DemandPredictionMode="None", DispatchMode="Simulation", VehiclesNumber=int(g["V"]),
                            TimePeriods=TIMESTEP, LocalRegionBound=tuple(g["focus_bound"].tolist()), SideLengthMeter=float(g["side_m"]),
                            VehiclesServiceMeter=float(g["service_m"]), NeighborCanServer=True, FocusOnLocalRegion=True, DataDir=data, Quiet=True,
                            Replicas=R, VehicleSeed=613, BatchedHooks=True, BatchedOutcomes=outcomes)
    random.seed(int(g["seed"]))
    sim.CreateAllInstantiate("1101")
    n2c = sim._world.node2cluster
    C = len(sim.Clusters)
    sim.first_node = torch.tensor([int(np.flatnonzero(n2c == c)[0]) if (n2c == c).any() else 0 for c in range(C)], device="cuda")
    sim.captures, sim.begin_calls = 0, 0
    sim.slot = torch.zeros(1, dtype=torch.int64, device="cuda")
    sim.log = torch.full((400, R, 2, 3), -1, dtype=torch.int32, device="cuda")
    Ts = []
    for day in (1, 2):
        if day == 2:
            sim.Reload("1102")
        T = sim.env.T
        Ts.append(T)
        init = sim._init_nodes.copy()
        sim.SimCity()
        assert sim.BatchedPolicyGraphError is None, sim.BatchedPolicyGraphError
        assert sim.step == T and int(sim.slot.item()) == T and sim.begin_calls == day
        assert sim.captures == day, "day %d: the policy was captured %d times" % (day, sim.captures)
        st = sim._bp_state
        assert st is not None and st["graph"] is not None
        planes = ("idle_pre", "idle_now", "supply", "cl_orders", "inflight")
        base = sim.env.obs_device_ptr()
        for k in sim.BatchedPolicyPlanes:
            assert st["obs"][k].data_ptr() == base + 4 * planes.index(k) * R * C, (day, k)
        if outcomes:
            oc = sim.env.outcomes_device_ptr()
            for i, k in enumerate(("served", "rejected", "wait_sum", "value_sum")):
                assert st["obs"][k].data_ptr() == oc + 8 * i * R * C, (day, k)
        # every replica against the oracle replaying the logged actions
        W = sim._world
        off, idx = neighbors_to_csr(W.neighbors)
        log = sim.log.cpu().numpy()
        got, cn = sim.env.orders(), sim.env.counters()
        n_dispatched = 0
        for r in range(R):
            o = Oracle(W.cost, W.node2cluster, off, idx, W.depth_limit, True, W.o_release_min, W.o_pickup, W.o_delivery, len(sim.Vehicles))
            o.reset(init[r])
            assert o.num_ticks == T
            for t in range(T):
                o.begin_tick()
                L = o.lists()
                vehs, tgts = [], []
                for cl, pos, tg in log[t, r]:
                    if cl >= 0:
                        vehs.append(int(L["idle_veh"][L["idle_off"][cl] + pos])); tgts.append(int(tg))
                if vehs:
                    o.dispatch(np.array(vehs), np.array(tgts))
                    n_dispatched += len(vehs)
                o.end_tick()
            exp, oc_ = o.orders(), o.counters()
            for k in ("status", "vehicle", "wait"):
                np.testing.assert_array_equal(got[k][r][:exp[k].size], exp[k], err_msg="day %d replica %d %s" % (day, r, k))
            assert (cn[r, 0], cn[r, 1], cn[r, 3], cn[r, 4], cn[r, 5], cn[r, 7]) == (oc_["order_num"], oc_["reject_num"], oc_["wait_sum"], oc_["dispatch_num"], oc_["dispatch_cost"], oc_["evals"]), (day, r)
        assert n_dispatched > 0
    assert Ts[1] > Ts[0]
    sim.env.close()
