"""Per-cluster order outcomes of each slot (vds_outcomes_device / vds_read_outcomes, vds_run_hooked with VDS_PLANE_OUTCOMES): what
RewardFunction (reference simulator.py:999-1004) reads from ``Cluster.Orders`` - served / rejected / wait_sum / value_sum per
(replica, cluster) - checked at EVERY slot against the expectation built from the goldens captured from the unmodified reference
(outcome_expect.py) or from the CPU oracle's per-order results, through every tick family, per-replica order days (regrouped storage
included), the one-graph hooked day with a captured policy, and the reference-compatible Simulation shell."""
import random

import numpy as np
import pytest

from helpers import dispatch_by_tick, load_golden, make_oracle
from outcome_expect import NAMES, expected_from_golden, expected_outcomes, tick_minutes_of
from test_gpu_parity import TINY, make_env
from test_gpu_replica_days import mk_env, mk_oracle, synth_days
from vehicles_dispatch_simulator_amd import synth, workloads

pytestmark = pytest.mark.gpu


def got_planes(env):
    oc = env.outcomes()
    return np.stack([oc[k] for k in NAMES], axis=-1)          # [R, C, 4]


def oracle_expectation(g, init_nodes, o_value):
    """Expected [T, C, 4] of one replica without dispatch: the CPU oracle's per-order results of its day."""
    o = make_oracle(g)
    o.reset(init_nodes)
    o.run_day()
    res = o.orders()
    return expected_outcomes(g["o_release_min"], g["o_pickup"], g["node2cluster"], res["status"], res["wait"], o_value,
                             tick_minutes_of(g), int(g["n_ticks"]), int(g["C"]))


def order_values(g):
    """OrderValue = RoadCost(pickup, delivery) = int(Map[pickup][delivery]) (:341-342, :263-264)."""
    return g["cost"][g["o_delivery"].astype(np.int64), g["o_pickup"].astype(np.int64)].astype(np.int64)


def check_day_stepwise(g, env, expect, dispatch=True):
    """Step the day slot by slot (dispatch_log applied to replica 0, as the reference's hook did) and compare every slot."""
    disp = dispatch_by_tick(g) if dispatch else {}
    extra = int(g["dispatch_extra_minutes"]) if "dispatch_extra_minutes" in g else 0
    assert (got_planes(env) == 0).all()                      # before the first step
    for t in range(env.T):
        env.step()
        got = got_planes(env)
        for r, e in enumerate(expect):
            np.testing.assert_array_equal(got[r], e[t], err_msg="slot %d replica %d" % (t, r))
        if t in disp:
            rows = np.array(disp[t])
            L = env.lists(0)
            pos = []
            for veh, cl in zip(rows[:, 1], rows[:, 2]):
                seg = L["idle_veh"][L["idle_off"][cl]:L["idle_off"][cl + 1]]
                pos.append(int(np.flatnonzero(seg == veh)[0]))
            rep = np.zeros(len(rows), dtype=np.int32)
            if extra:
                _, now = env.clock
                env.apply_dispatch(rep, rows[:, 2], pos, rows[:, 4], arrive_min=now + rows[:, 5] + extra)
            else:
                env.apply_dispatch(rep, rows[:, 2], pos, rows[:, 4])
            np.testing.assert_array_equal(got_planes(env), got, err_msg="slot %d: dispatch changed the planes" % t)
        env.advance()
    return env


def fixture_run(name, R=3, **kw):
    g = load_golden(name)
    V, N = int(g["V"]), int(g["N"])
    valid = g["node2cluster"] >= 0
    init = np.empty((R, V), dtype=np.int32)
    init[0] = g["veh_node"]
    for r in range(1, R):
        init[r] = synth.init_vehicle_nodes(random.Random(300 + r), N, V, valid)
    values = order_values(g)
    expect = [expected_from_golden(g)] + [oracle_expectation(g, init[r], values) for r in range(1, R)]
    env = make_env(g, R, **kw)
    env.reset(init)
    return g, env, expect


@pytest.mark.parametrize("name", TINY + ["real_spectral192_dfs2", "real_shipped_transport_dfs2"])
def test_planes_equal_reference_at_every_slot(name):
    g, env, expect = fixture_run(name, R=2 if name.startswith("real_") else 3)
    check_day_stepwise(g, env, expect)
    env.close()


# (expected vds_main_kernel, fixture, engine keywords): every tick family a handle can be forced into
FAMILIES = [
    ("k_tick_dense", "tiny_kmeans", {}),
    ("k_tick_dense", "tiny_dispatch", {"dense_debug": (16, 8, 2, 0)}),       # tiny fast-path tables: buckets take the slow path
    ("k_tick_dense", "tiny_kmeans", {"dense_debug": (16, 0, 0, 2)}),         # arrival ring instead of static arrival slots
    ("k_tick_rows", "tiny_kmeans", {"force_generic": 5}),
    ("k_tick_rows", "tiny_grid", {"force_generic": 5, "ring_ticks": 2}),     # far tables
    ("k_tick", "tiny_fraccost", {"force_generic": 1}),
    ("k_dfs_dense", "tiny_kmeans_dfs2", {}),
    ("k_dfs_hybrid", "tiny_kmeans_dfs2", {"environ": {"VDS_DENSE_DFS": "0"}}),
    ("k_dfs_hybrid", "tiny_dispatch_dfs2", {"environ": {"VDS_DENSE_DFS": "0"}}),
    ("k_tick_replica2", "tiny_kmeans_dfs2", {"force_generic": 3}),
    ("k_match_dfs", "tiny_grid_nbr_scarce", {"force_generic": 1}),
]


@pytest.mark.parametrize("kernel,name,kw", FAMILIES, ids=["%s-%s-%d" % (k, n, i) for i, (k, n, _) in enumerate(FAMILIES)])
def test_planes_through_every_tick_family(kernel, name, kw):
    g, env, expect = fixture_run(name, R=3, **kw)
    assert env.main_kernel() == kernel
    check_day_stepwise(g, env, expect)
    env.close()


def test_per_replica_order_days_and_regrouped_storage():
    """Days of different lengths per replica (vds_load_order_days), then maps that store the replicas regrouped by day
    (vds_set_replica_days): every replica's planes match its own day's expectation in the caller's order; past its day: zeros."""
    g = load_golden("tiny_kmeans")
    R, V, N = 40, int(g["V"]), int(g["N"])
    days = synth_days(g, 5, seed=5200)
    valid = g["node2cluster"] >= 0
    init = np.stack([synth.init_vehicle_nodes(random.Random(8100 + r), N, V, valid) for r in range(R)]).astype(np.int32)
    env = mk_env(g, R)
    maps = [np.arange(R) // 8, np.arange(R) % 5, (np.arange(R) * 7 + 1) % 4, np.random.default_rng(3).integers(0, 5, size=R)]
    env.load_order_days(days, maps[0].astype(np.int32))
    tick = tick_minutes_of(g)
    C = int(g["C"])
    cache = {}
    for ep, rd in enumerate(maps):
        if ep:
            env.set_replica_days(rd.astype(np.int32))
        env.reset(init)
        expect = []
        for r in range(R):
            d = int(rd[r])
            if (r, d) not in cache:
                day = days[d]
                o = mk_oracle(g, day)
                o.reset(init[r])
                T_r = o.num_ticks
                o.run_day()
                res = o.orders()
                value = g["cost"][day[2].astype(np.int64), day[1].astype(np.int64)].astype(np.int64)
                cache[(r, d)] = expected_outcomes(day[0], day[1], g["node2cluster"], res["status"], res["wait"], value, tick, T_r, C)
            expect.append(cache[(r, d)])
        Ts = [e.shape[0] for e in expect]
        assert env.T == max(Ts) and len(set(Ts)) > 1
        for t in range(env.T):
            env.step()
            got = got_planes(env)
            for r in range(R):
                exp = expect[r][t] if t < Ts[r] else np.zeros((C, 4), dtype=np.int64)
                np.testing.assert_array_equal(got[r], exp, err_msg="episode %d slot %d replica %d" % (ep, t, r))
            env.advance()
    env.close()


def test_sums_equal_the_device_counters_at_configs1_shape():
    """configs[1]-shaped city (192 clusters, 10k vehicles, ~200k orders) at 64 replicas: the planes summed over slots and clusters are
    the per-replica counters of vds_counters_device (OrderNum - RejectNum, RejectNum, TotallyWaitTime, matched OrderValue)."""
    import torch
    w = workloads.didi_day()
    R = 64
    env = w.make_env(R, stream=torch.cuda.current_stream().cuda_stream)
    env.reset(w.vehicle_nodes(R))
    acc = torch.zeros((4, R, env.C), dtype=torch.int64, device="cuda")
    for _ in range(env.T):
        env.step()
        acc += env.outcomes_torch()
        env.advance()
    cn = env.counters_torch().clone()
    tot = acc.sum(dim=2)
    assert torch.equal(tot[0], cn[:, 0] - cn[:, 1]) and torch.equal(tot[1], cn[:, 1])
    assert torch.equal(tot[2], cn[:, 2]) and torch.equal(tot[3], cn[:, 3])
    assert int(tot[0].min()) > 100000
    env.close()


def hooked_day(g, R, init, outcomes, groups, kw):
    """One run_hooked day with a captured policy that adds the outcome block into an accumulator and logs the observation block."""
    import torch
    stream = torch.cuda.current_stream()
    env = make_env(g, R, stream=stream.cuda_stream, **kw)
    if groups > 1:
        env.set_run_groups(groups, -1)
    env.reset(init)
    T = env.T
    ob = env.obs_torch(inflight=False)
    oc = env.outcomes_torch()
    acc = torch.zeros((4, R, env.C), dtype=torch.int64, device="cuda")
    log = torch.zeros((T + 1, 4, R, env.C), dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int64, device="cuda")

    def policy():
        if outcomes:
            acc.add_(oc)
        log.index_copy_(0, slot, ob[None, :4])
        slot.add_(1)

    side = torch.cuda.Stream()
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        for _ in range(2):
            policy()
    stream.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        policy()
    acc.zero_(); log.zero_(); slot.zero_()
    env.run_hooked(T, policy_graph=graph, outcomes=outcomes)
    env.sync()
    torch.cuda.synchronize()
    assert int(slot.item()) == T
    out = (acc.cpu().numpy(), log[:T].cpu().numpy(), env.counters())
    env.close()
    return out


@pytest.mark.parametrize("name,groups,kw", [("tiny_kmeans", 1, {}), ("tiny_kmeans_dfs2", 2, {}), ("tiny_kmeans", 1, {"force_generic": 1})],
                         ids=["dense-one-chain", "dfs-two-groups", "eager-generic"])
def test_run_hooked_delivers_the_planes_to_a_captured_policy(name, groups, kw):
    g = load_golden(name)
    R = 32
    init = np.stack([g["veh_node"]] + [np.random.default_rng(r).permutation(g["veh_node"]) for r in range(1, R)]).astype(np.int32)
    # stepwise reference: per-slot planes and observations
    env = make_env(g, R, **kw)
    env.reset(init)
    T = env.T
    ref_sum = np.zeros((R, env.C, 4), dtype=np.int64)
    ref_obs = np.zeros((T, 4, R, env.C), dtype=np.int32)
    for t in range(T):
        env.step()
        ref_sum += got_planes(env)
        o = env.obs()
        ref_obs[t] = np.stack([o[k] for k in ("idle_pre", "idle_now", "supply", "cl_orders")])
        env.advance()
    env.close()
    acc, log, cn = hooked_day(g, R, init, True, groups, kw)
    np.testing.assert_array_equal(np.moveaxis(acc, 0, -1), ref_sum)
    np.testing.assert_array_equal(log, ref_obs)
    acc0, log0, cn0 = hooked_day(g, R, init, False, groups, kw)
    assert (acc0 == 0).all()
    np.testing.assert_array_equal(log0, log)                  # the observation planes do not depend on the bit
    np.testing.assert_array_equal(cn0, cn)


def test_error_paths_and_plane_mask():
    g = load_golden("tiny_kmeans")
    env = make_env(g, 2)
    with pytest.raises(Exception, match="call vds_reset first"):
        env.outcomes()
    env.reset(np.tile(g["veh_node"], (2, 1)))
    p = env.outcomes_device_ptr()
    assert (got_planes(env) == 0).all()                       # reset, nothing stepped yet
    assert env._lib.vds_run_hooked(env._h, 1, 64, 0, None, None) == -1
    with pytest.raises(Exception, match="mask"):
        env.obs_device_ptr(32)                                # the observation pass keeps its five planes
    env.step()
    assert env.outcomes_device_ptr() == p                     # a fixed address
    env.close()


# ---- the reference-compatible Simulation shell -------------------------------------------------------------------------------------
from test_gpu_simulation_shell import make_sim  # noqa: E402
from vehicles_dispatch_simulator_amd.simulation import Simulation  # noqa: E402


class OutcomeRewardSim(Simulation):
    """A RewardFunction over ALL replicas (BatchedHooks): accumulates self.BatchedOutcomes and keeps replica 0's rows of every slot."""

    def RewardFunction(self):
        import torch
        oc = torch.stack([self.BatchedOutcomes[k] for k in NAMES])
        self.acc += oc
        self.rows.append(oc[:, self.Replica].cpu().numpy())


class ReferenceRewardSim(Simulation):
    """The reference's own idiom on the host-object path: for c in self.Clusters: for o in c.Orders: ...o.ArriveInfo..."""

    def RewardFunction(self):
        row = np.zeros((3, len(self.Clusters)), dtype=np.int64)
        for c in self.Clusters:
            for o in c.Orders:
                if o.ArriveInfo == "Success":
                    row[0, c.ID] += 1
                    row[2, c.ID] += o.PickupWaitTime
                elif o.ArriveInfo == "Reject":
                    row[1, c.ID] += 1
        self.rows.append(row)


def test_simulation_batched_outcomes_in_reward_function_and_reference_idiom():
    import torch
    g = load_golden("tiny_kmeans_dfs2")
    R = 8
    sim = make_sim(g, OutcomeRewardSim, Replicas=R, VehicleSeed=55, BatchedHooks=True, BatchedOutcomes=True)
    sim.acc = torch.zeros((4, R, int(g["C"])), dtype=torch.int64, device="cuda")
    sim.rows = []
    sim.SimCity()
    cn = sim.BatchedCounters().clone()
    tot = sim.acc.sum(dim=2)
    assert torch.equal(tot[0], cn[:, 0] - cn[:, 1]) and torch.equal(tot[1], cn[:, 1])
    assert torch.equal(tot[2], cn[:, 2]) and torch.equal(tot[3], cn[:, 3])
    host = make_sim(g, ReferenceRewardSim, Replicas=R, VehicleSeed=55)
    host.rows = []
    host.SimCity()
    assert len(host.rows) == len(sim.rows) == sim.env.T
    for t, (a, b) in enumerate(zip(sim.rows, host.rows)):
        np.testing.assert_array_equal(a[:3], b, err_msg="slot %d" % t)
    sim.env.close(); host.env.close()
    with pytest.raises(Exception, match="BatchedHooks"):
        make_sim(g, Simulation, BatchedOutcomes=True)


class OutcomePolicySim(Simulation):
    """A BatchedPolicy that reads the outcome planes inside the one-launch day and dispatches nothing."""

    def BatchedPolicy(self, ob):
        import torch
        self.keys = sorted(ob)
        self.acc.add_(torch.stack([ob[k] for k in NAMES]))
        return self.noop

    def BatchedPolicyBegin(self):
        self.acc.zero_()


def test_batched_policy_day_graph_receives_the_outcome_planes():
    import torch
    g = load_golden("tiny_kmeans")
    R = 16
    sim = make_sim(g, OutcomePolicySim, Replicas=R, VehicleSeed=7, BatchedHooks=True, BatchedOutcomes=True)
    sim.acc = torch.zeros((4, R, int(g["C"])), dtype=torch.int64, device="cuda")
    sim.noop = torch.full((R, 1, 3), -1, dtype=torch.int32, device="cuda")
    sim.SimCity()
    assert sim.BatchedPolicyGraphError is None, sim.BatchedPolicyGraphError
    assert set(NAMES) <= set(sim.keys) and sorted(sim.BatchedOutcomes) == sorted(NAMES)
    cn = sim.BatchedCounters().clone()
    tot = sim.acc.sum(dim=2)
    assert torch.equal(tot[0], cn[:, 0] - cn[:, 1]) and torch.equal(tot[1], cn[:, 1])
    assert torch.equal(tot[2], cn[:, 2]) and torch.equal(tot[3], cn[:, 3])
    # the second day replays the same capture
    st = sim._bp_state
    sim.Reset()
    sim.SimCity()
    assert sim._bp_state is st
    assert torch.equal(sim.acc.sum(dim=2)[1], sim.BatchedCounters()[:, 1])
    sim.env.close()
