"""Heads of every idle list as device planes (vds_idle_heads_device / vds_read_idle_heads, vds_run_hooked_idle_heads): the first L
entries of ``Clusters[c].IdleVehicles`` of every replica - Vehicle.ID and Vehicle.LocationNode (global node id), -1 past the end of a
list - checked at every slot against the CPU oracle's lists, through every tick family and both layouts, at the layout thresholds,
with order days per replica (regrouped storage included), inside the one-graph hooked day, as the input of a nearest-vehicle policy
that runs on the device, and through the reference-compatible Simulation shell.  Integer bookkeeping: bit-exact."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import threshold_cities as tc
from helpers import dispatch_by_tick, load_golden, make_oracle
from test_gpu_parity import MODES, make_env
from test_gpu_replica_days import mk_env, mk_oracle, synth_days
from vehicles_dispatch_simulator_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expected_heads(o, C, L):
    """(veh, node), each int32 [C, L], from one oracle: its lists truncated or padded with -1 to L, LocationNode of each vehicle."""
    Ls, loc = o.lists(), o.vehicles()["loc"]
    veh = np.full((C, L), -1, dtype=np.int32)
    node = np.full((C, L), -1, dtype=np.int32)
    off = Ls["idle_off"]
    for c in range(C):
        seg = Ls["idle_veh"][off[c]:off[c + 1]][:L]
        veh[c, :seg.size] = seg
        node[c, :seg.size] = loc[seg]
    return veh, node


def check_heads(env, L, oracles, tag, lists_of_replica0=True):
    got = env.idle_heads(L)
    assert got["veh"].shape == got["node"].shape == (env.R, env.C, L) and got["veh"].dtype == np.int32
    for r, o in enumerate(oracles):
        if o is None:
            continue
        veh, node = expected_heads(o, env.C, L)
        np.testing.assert_array_equal(got["veh"][r], veh, err_msg="%s replica %d veh (L = %d)" % (tag, r, L))
        np.testing.assert_array_equal(got["node"][r], node, err_msg="%s replica %d node (L = %d)" % (tag, r, L))
    if lists_of_replica0:            # ... and the synchronous one-replica read of the same lists
        G = env.lists(0)
        off = G["idle_off"]
        for c in range(env.C):
            n = min(int(off[c + 1] - off[c]), L)
            np.testing.assert_array_equal(got["veh"][0, c, :n], G["idle_veh"][off[c]:off[c] + n], err_msg=tag)
            np.testing.assert_array_equal(got["node"][0, c, :n], G["idle_node"][off[c]:off[c] + n], err_msg=tag)
            assert (got["veh"][0, c, n:] == -1).all() and (got["node"][0, c, n:] == -1).all(), tag
    return got


def seeded_init(g, R):
    """Replica 0 on the fixture's start nodes, the others seeded as test_gpu_parity.run_day seeds them."""
    V, N = int(g["V"]), int(g["N"])
    valid = g["node2cluster"] >= 0
    init = np.empty((R, V), dtype=np.int32)
    init[0] = g["veh_node"]
    for r in range(1, R):
        init[r] = synth.init_vehicle_nodes(random.Random(1000 + r), N, V, valid)
    return init


class Coverage:
    """What replica 0's oracle lists showed over the day, per L: a bucket longer than L, one with 0 < len < L, an empty one."""

    def __init__(self, Ls):
        self.seen = {L: dict(longer=False, shorter=False, empty=False) for L in Ls}
        self.longest = 0

    def add(self, o):
        n = np.diff(o.lists()["idle_off"])
        self.longest = max(self.longest, int(n.max()))
        for L, s in self.seen.items():
            s["longer"] |= bool((n > L).any())
            s["shorter"] |= bool(((n > 0) & (n < L)).any())
            s["empty"] |= bool((n == 0).any())


def heads_day(name, mode, Ls, device_dispatch=False):
    """One day slot by slot with R = 3, one handle per L (so every handle keeps one block): heads before the first step, after every
    step and - where the fixture's hook dispatched - again after the slot's dispatch (replica 0, as the reference's hook did)."""
    g = load_golden(name)
    R = 3
    kw = dict(MODES[mode])
    kw.pop("supply_inplace", None)
    if device_dispatch:
        import torch
        kw["stream"] = torch.cuda.current_stream().cuda_stream
    init = seeded_init(g, R)
    envs = {L: make_env(g, R, **kw) for L in Ls}
    oracles = []
    for r in range(R):
        o = make_oracle(g)
        o.reset(init[r])
        oracles.append(o)
    cov = Coverage(Ls)
    for L, env in envs.items():
        env.reset(init)
        check_heads(env, L, oracles, "%s %s after reset" % (name, mode))
    cov.add(oracles[0])
    disp = dispatch_by_tick(g)
    T = envs[Ls[0]].T
    assert T == oracles[0].num_ticks
    for t in range(T):
        for o in oracles:
            o.begin_tick()
        cov.add(oracles[0])
        for L, env in envs.items():
            env.step()
            check_heads(env, L, oracles, "%s %s slot %d" % (name, mode, t))
        if t in disp:
            rows = np.array(disp[t])
            Lo = oracles[0].lists()
            pos = []
            for veh, cl in zip(rows[:, 1], rows[:, 2]):
                seg = Lo["idle_veh"][Lo["idle_off"][cl]:Lo["idle_off"][cl + 1]]
                pos.append(int(np.flatnonzero(seg == veh)[0]))
            for L, env in envs.items():
                if device_dispatch:
                    acts = np.full((R, len(rows) + 2, 3), -1, dtype=np.int32)
                    acts[0, 1:len(rows) + 1, 0] = rows[:, 2]; acts[0, 1:len(rows) + 1, 1] = pos; acts[0, 1:len(rows) + 1, 2] = rows[:, 4]
                    env.apply_dispatch_torch(torch.from_numpy(acts).cuda())
                else:
                    env.apply_dispatch(np.zeros(len(rows), dtype=np.int32), rows[:, 2], pos, rows[:, 4])
            oracles[0].dispatch(rows[:, 1], rows[:, 4])
            cov.add(oracles[0])
            for L, env in envs.items():
                check_heads(env, L, oracles, "%s %s slot %d after dispatch" % (name, mode, t))
        for L, env in envs.items():
            env.advance()
        for o in oracles:
            o.end_tick()
    for env in envs.values():
        env.close()
    return g, cov


# (fixture, mode, the L run beside L = 2)
EVERY_SLOT = [
    ("tiny_kmeans", "fast", 16), ("tiny_kmeans", "generic", 3), ("tiny_kmeans", "rows", 1), ("tiny_kmeans", "dense_tiny8", 64),
    ("tiny_kmeans", "dense_alt", 3),
    ("tiny_grid", "far", 16),
    ("tiny_sort_ties", "fast", 3),
    ("tiny_window6", "fast", 16),                     # live pickup window -> k_tick
    ("tiny_kmeans_dfs2", "fast", 16),                 # stamp form + flush
    ("tiny_kmeans_dfs2", "dfs_wide", 1), ("tiny_kmeans_dfs2", "dfs_v2", 64),
    ("tiny_dispatch_dfs2", "generic", 3),             # serial form
    ("tiny_empty_clusters_dfs2", "fast", 1),
    ("tiny_dispatch", "fast", 64),                    # host dispatch (device dispatch: the test below)
    ("tiny_grid_nbr_scarce", "fast", 64), ("tiny_two_orders", "fast", 64),     # V = 24 / 30: idle_cap < L
]
TRUNCATED_AT_16 = ("tiny_kmeans", "tiny_grid", "tiny_window6")      # their longest lists pass 16 entries


def check_coverage(name, cov, Ls):
    s = cov.seen[2]
    assert s["longer"] and s["shorter"] and s["empty"], (name, s)
    if 16 in Ls and name in TRUNCATED_AT_16:
        assert cov.seen[16]["longer"] and cov.longest > 16, (name, cov.longest)
    if 64 in Ls:
        assert not cov.seen[64]["longer"], (name, cov.longest)


@pytest.mark.parametrize("name,mode,L", EVERY_SLOT, ids=["%s-%s-%d" % e for e in EVERY_SLOT])
def test_heads_equal_the_oracle_lists_at_every_slot(name, mode, L):
    g, cov = heads_day(name, mode, (2, L))
    check_coverage(name, cov, (2, L))
    if L == 64 and name in ("tiny_grid_nbr_scarce", "tiny_two_orders"):
        assert int(g["V"]) < 64                      # the lists' capacity (at most V rounded up) against L = 64: see the docstring


def test_heads_after_device_dispatch():
    g, cov = heads_day("tiny_dispatch", "fast", (2, 3), device_dispatch=True)
    check_coverage("tiny_dispatch", cov, (2, 3))
    assert int(g["dispatch_num"]) > 0


# ---- layout edges (tests/threshold_cities.py) ---------------------------------------------------------------------------------------
from test_gpu_thresholds import check_premise, make_env as make_threshold_env  # noqa: E402


def threshold_day(c, mode, Ls, tag):
    env = make_threshold_env(c, mode)
    env.reset(c["init"])
    oracles = [tc.oracle_for(c, r) for r in range(tc.R)]
    seen = []
    for L in Ls:
        seen.append(check_heads(env, L, oracles, "%s %s after reset" % (tag, mode)))
    for t in range(env.T):
        env.step()
        for o in oracles:
            o.begin_tick()
        for L in Ls:              # (one handle, alternating L: the block is made again every time)
            seen.append(check_heads(env, L, oracles, "%s %s slot %d" % (tag, mode, t)))
        env.advance()
        for o in oracles:
            o.end_tick()
    return env, seen


@pytest.mark.parametrize("side", [0, 1])
def test_cluster_of_255_and_256_nodes(side):
    """A 255-node cluster on the dense layout (loc_local is a byte: 254 must not come back negative), a 256-node one on the wide
    layout; vehicles crowd local node 254, whose global id only the cl_nodes mapping gives."""
    c = tc.cluster_size(side)
    env, seen = threshold_day(c, "fast", (3, 64), "cluster-%d" % (255 + side))
    check_premise(env, "k_tick_dense" if side == 0 else "k_tick_rows", dict(dense=1 - side), "cluster-%d" % (255 + side))
    hot = c["facts"]["hot"]
    assert any((s["node"][:, 0] == hot).any() for s in seen)      # (the crowded node heads a list of cluster 0 at some slot)
    env.close()


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("tab", [128, 256])
def test_lists_of_128_to_257_entries(side, tab):
    """Lists of 128 / 129 / 256 / 257 entries (the fast-path tables of the dense tick's two forms, both sides): L = 64 returns the
    first 64 of the list at every slot, on the dense and on the wide layout."""
    c = tc.bucket_entries(side, tab)
    n0 = c["facts"]["n0"]
    for mode in ("dense8" if tab == 128 else "dense16", "rows"):
        env, seen = threshold_day(c, mode, (64,), "entries-%d" % n0)
        assert (seen[0]["veh"][:, 0] >= 0).all()             # cluster 0 after the reset: every one of the 64 positions filled
        o = tc.oracle_for(c, 0)
        assert np.diff(o.lists()["idle_off"])[0] == n0
        env.close()


# ---- order days per replica: the block is in the caller's replica order -------------------------------------------------------------
def replica_days_case(R, replica_day, n_days, n_inits, regrouped, seed):
    """Replica r replays day replica_day[r] from start nodes init[r % n_inits]; one oracle per (day, start) pair."""
    g = load_golden("tiny_kmeans")
    V, N = int(g["V"]), int(g["N"])
    days = synth_days(g, n_days, seed=seed)
    valid = g["node2cluster"] >= 0
    starts = [synth.init_vehicle_nodes(random.Random(seed + k), N, V, valid) for k in range(n_inits)]
    init = np.stack([starts[r % n_inits] for r in range(R)]).astype(np.int32)
    env = mk_env(g, R)
    env.load_order_days(days, replica_day.astype(np.int32))
    try:
        env.obs_inplace_torch()
        stored_regrouped = False
    except Exception as e:
        assert "regrouped" in str(e), e
        stored_regrouped = True
    assert stored_regrouped == regrouped
    env.reset(init)
    oracles = {}
    for r in range(R):
        key = (int(replica_day[r]), r % n_inits)
        if key not in oracles:
            o = mk_oracle(g, days[key[0]])
            o.reset(init[r])
            oracles[key] = o
    Ts = {k: o.num_ticks for k, o in oracles.items()}
    assert env.T == max(Ts.values()) and min(Ts.values()) + 10 < env.T      # slots after the shorter day has ended are part of the run
    L = 5
    for t in range(env.T):
        env.step()
        for k, o in oracles.items():
            if t < Ts[k]:
                o.begin_tick()
        got = env.idle_heads(L)
        exp = {k: expected_heads(o, env.C, L) for k, o in oracles.items()}       # (a day that is over: its standing lists)
        for r in range(R):
            veh, node = exp[(int(replica_day[r]), r % n_inits)]
            np.testing.assert_array_equal(got["veh"][r], veh, err_msg="slot %d replica %d" % (t, r))
            np.testing.assert_array_equal(got["node"][r], node, err_msg="slot %d replica %d" % (t, r))
        env.advance()
        for k, o in oracles.items():
            if t < Ts[k]:
                o.end_tick()
    env.close()


def test_interleaved_days_twelve_replicas():
    """Two days of different length, interleaved over 12 replicas (a batch this small is never stored regrouped: the padding to 16
    replicas would pass a quarter - every row gets its own order stream instead)."""
    replica_days_case(12, np.arange(12) % 2 * 2, 3, 12, False, seed=4100)


def test_every_row_its_own_order_stream():
    replica_days_case(12, np.arange(12), 12, 12, False, seed=4200)


def test_interleaved_days_stored_regrouped():
    """Three days interleaved over 40 replicas: 14 + 13 + 13, stored as 3 x 16 with padding replicas (int2ext) - the block stays in the
    caller's order.  Two start-node sets per day, so the oracles are six."""
    replica_days_case(40, np.arange(40) % 3, 3, 2, True, seed=4300)


# ---- the hooked day ------------------------------------------------------------------------------------------------------------------
def stepwise_heads(g, R, init, L, kw):
    env = make_env(g, R, **kw)
    env.reset(init)
    ref = np.zeros((env.T, 2, R, env.C, L), dtype=np.int32)
    for t in range(env.T):
        env.step()
        h = env.idle_heads(L)
        ref[t, 0], ref[t, 1] = h["veh"], h["node"]
        env.advance()
    cn = env.counters()
    env.close()
    return ref, cn


def hooked_heads_day(g, R, init, L, groups, kw, switch_on=True):
    """One run_hooked day whose captured policy copies the heads block into a [T, 2, R, C, L] log."""
    import torch
    stream = torch.cuda.current_stream()
    env = make_env(g, R, stream=stream.cuda_stream, **kw)
    if groups > 1:
        env.set_run_groups(groups, -1)
    env.reset(init)
    T = env.T
    blk = env.idle_heads_torch(L)
    log = torch.zeros((T + 1, 2, R, env.C, L), dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int64, device="cuda")

    def policy():
        log.index_copy_(0, slot, blk[None])
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
    log.zero_(); slot.zero_()
    if not switch_on:
        blk.fill_(-7)
    env.run_hooked(T, policy_graph=graph, idle_heads=L if switch_on else 0)
    env.sync()
    torch.cuda.synchronize()
    assert int(slot.item()) == T
    out = (log[:T].cpu().numpy(), env.counters(), blk.cpu().numpy())
    assert env.idle_heads_device_ptr(L) == blk.data_ptr()
    env.close()
    return out


HOOKED = [("tiny_kmeans", 8, 1, {}, 5), ("tiny_kmeans", 40, 2, {}, 3), ("tiny_kmeans_dfs2", 8, 1, {}, 4), ("tiny_kmeans", 8, 1, {"force_generic": 1}, 2)]


@pytest.mark.parametrize("name,R,groups,kw,L", HOOKED, ids=["dense-one-chain", "dense-two-groups-R40", "dfs-stamp-flush", "eager-generic"])
def test_run_hooked_refreshes_the_block_every_slot(name, R, groups, kw, L):
    g = load_golden(name)
    init = np.stack([g["veh_node"]] + [np.random.default_rng(r).permutation(g["veh_node"]) for r in range(1, R)]).astype(np.int32)
    ref, cn_ref = stepwise_heads(g, R, init, L, kw)
    log, cn, _ = hooked_heads_day(g, R, init, L, groups, kw)
    np.testing.assert_array_equal(log, ref)
    np.testing.assert_array_equal(cn, cn_ref)
    assert (ref[:, 0] >= 0).any() and (ref[:, 0] == -1).any()
    if name == "tiny_kmeans" and groups == 1 and not kw:
        log0, cn0, blk0 = hooked_heads_day(g, R, init, L, groups, kw, switch_on=False)      # switched off: nothing touches the block
        assert (blk0 == -7).all() and (log0 == -7).all()
        np.testing.assert_array_equal(cn0, cn)


# ---- end to end: the idle vehicle nearest to a target ---------------------------------------------------------------------------------
NV_R, NV_K, NV_L = 4, 2, 8


def nearest_targets(g, T):
    valid = np.flatnonzero(g["node2cluster"] >= 0)
    return valid[(7 * np.arange(T) + 3) % valid.size].astype(np.int64)


def host_nearest_day(g, init, T):
    """The policy on the host, from each oracle's own lists: the K fullest clusters (lowest index on ties) each send, among the first L
    vehicles of their list, the one with the smallest RoadCost(LocationNode, target) (lowest position on ties).  Returns the
    actions [T, R, K, 3], the lists of every 10th slot after its dispatch, and the final counters."""
    C, cost = int(g["C"]), g["cost"]
    targets = nearest_targets(g, T)
    oracles = []
    for r in range(NV_R):
        o = make_oracle(g)
        o.reset(init[r])
        oracles.append(o)
    acts = np.full((T, NV_R, NV_K, 3), -1, dtype=np.int32)
    lists = {}
    for t in range(T):
        for r, o in enumerate(oracles):
            o.begin_tick()
            Lo, loc = o.lists(), o.vehicles()["loc"]
            off = Lo["idle_off"]
            n = np.diff(off)
            order = sorted(range(C), key=lambda c: (-int(n[c]), c))[:NV_K]
            vehs = []
            for k, c in enumerate(order):
                if n[c] == 0:
                    continue
                seg = Lo["idle_veh"][off[c]:off[c + 1]][:NV_L]
                costs = [int(cost[targets[t], loc[v]]) for v in seg]
                p = int(np.argmin(costs))                                  # (first minimum)
                acts[t, r, k] = (c, p, targets[t])
                vehs.append(int(seg[p]))
            if vehs:
                o.dispatch(np.array(vehs), np.full(len(vehs), targets[t]))
            if t % 10 == 0:
                lists[(t, r)] = {k: np.array(v) for k, v in o.lists().items()}
            o.end_tick()
    return acts, lists, [o.counters() for o in oracles]


def device_nearest_policy(g, env, T):
    """The same policy in torch on the library's blocks (fixed addresses): returns (policy, action tensor, log, slot counter)."""
    import torch
    N, C = int(g["N"]), env.C
    ob = env.obs_torch(inflight=False)
    heads = env.idle_heads_torch(NV_L)
    cost = torch.from_numpy(np.ascontiguousarray(g["cost"]).astype(np.int64)).cuda().reshape(-1)
    targets = torch.from_numpy(nearest_targets(g, T)).cuda()
    acts = torch.full((NV_R, NV_K, 3), -1, dtype=torch.int32, device="cuda")
    log = torch.full((T + 2, NV_R, NV_K, 3), -1, dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int64, device="cuda")
    cidx = torch.arange(C, device="cuda", dtype=torch.int64)
    pidx = torch.arange(NV_L, device="cuda", dtype=torch.int64)
    BIG = 1 << 40

    def policy():
        idle = ob[1].to(torch.int64)                                        # idle_now [R, C]
        key = idle * C + (C - 1 - cidx)[None, :]                            # fullest first, lowest index on ties
        src = torch.topk(key, NV_K, dim=1).indices                          # [R, K]
        cnt = torch.gather(idle, 1, src)
        tgt = targets.index_select(0, slot.clamp(max=T - 1))                # [1]
        node = torch.gather(heads[1].to(torch.int64), 1, src[:, :, None].expand(NV_R, NV_K, NV_L))      # [R, K, L]
        rc = cost[(tgt * N + node.clamp(min=0)).reshape(-1)].reshape(NV_R, NV_K, NV_L)                  # RoadCost(node, target)
        pk = torch.where(node >= 0, rc * NV_L + pidx[None, None, :], torch.full_like(rc, BIG))
        pos = torch.argmin(pk, dim=2)                                       # (the keys are distinct: lowest position on ties)
        ok = cnt > 0
        a = torch.stack([torch.where(ok, src, torch.full_like(src, -1)), torch.where(ok, pos, torch.full_like(pos, -1)),
                         torch.where(ok, tgt.expand(NV_R, NV_K), torch.full_like(src, -1))], dim=2).to(torch.int32)
        acts.copy_(a)
        log.index_copy_(0, slot, acts[None])
        slot.add_(1)

    return policy, acts, log, slot


def check_against_host(env, r_lists, t):
    for r in range(NV_R):
        G = env.lists(r)
        for k in ("idle_off", "idle_veh", "arr_off", "arr_veh", "arr_min"):
            np.testing.assert_array_equal(G[k], r_lists[(t, r)][k], err_msg="slot %d replica %d %s" % (t, r, k))


@pytest.mark.parametrize("name", ["tiny_kmeans", "tiny_kmeans_dfs2"])
def test_nearest_vehicle_policy_on_the_device_equals_the_host(name):
    import torch
    g = load_golden(name)
    init = seeded_init(g, NV_R)
    stream = torch.cuda.current_stream()
    env = make_env(g, NV_R, stream=stream.cuda_stream)
    T = env.T
    exp_acts, exp_lists, exp_cn = host_nearest_day(g, init, T)
    assert (exp_acts[:, :, :, 1] > 0).any() and (exp_acts[:, :, :, 0] >= 0).sum() > T      # some vehicle that is not the head of its list
    names = ("order_num", "reject_num", "matched", "wait_sum", "dispatch_num", "dispatch_cost")

    def check_end(tag):
        env.sync()
        cn = env.counters()
        for r in range(NV_R):
            assert [int(cn[r, i]) for i in range(6)] == [exp_cn[r][k] for k in names], (tag, r, cn[r], exp_cn[r])

    # slot by slot
    env.reset(init)
    policy, acts, log, slot = device_nearest_policy(g, env, T)
    for t in range(T):
        env.step()
        env.obs_torch(inflight=False)
        env.idle_heads_torch(NV_L)
        policy()
        env.apply_dispatch_torch(acts)
        if t % 10 == 0:
            check_against_host(env, exp_lists, t)
        env.advance()
    np.testing.assert_array_equal(log[:T].cpu().numpy(), exp_acts)
    check_end("stepwise")
    # the day as one graph
    env.reset(init)
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
    log.fill_(-1); slot.zero_(); acts.fill_(-1)
    env.run_hooked(T, actions=acts, policy_graph=graph, inflight=False, idle_heads=NV_L)
    env.sync()
    torch.cuda.synchronize()
    assert int(slot.item()) == T
    np.testing.assert_array_equal(log[:T].cpu().numpy(), exp_acts)
    check_end("one graph")
    env.close()


# ---- error paths and addresses ---------------------------------------------------------------------------------------------------------
def test_error_paths_and_block_addresses():
    g = load_golden("tiny_kmeans")
    env = make_env(g, 2)
    with pytest.raises(Exception, match="call vds_reset first"):
        env.idle_heads(4)
    assert env._lib.vds_idle_heads_device(env._h, 4, None) == -1          # VDS_EINVAL
    init = np.tile(g["veh_node"], (2, 1))
    env.reset(init)
    for bad in (0, 65, -1):
        with pytest.raises(Exception, match=r"1 \.\. 64"):
            env.idle_heads_device_ptr(bad)
        assert env._lib.vds_idle_heads_device(env._h, bad, None) == -1
    assert env._lib.vds_run_hooked_idle_heads(env._h, 65) == -1 and env._lib.vds_run_hooked_idle_heads(env._h, -1) == -1
    with pytest.raises(Exception, match=r"0 \(off\) \.\. 64"):
        env.run_hooked(1, idle_heads=65)
    assert env._lib.vds_run_hooked_idle_heads(env._h, 64) == 0 and env._lib.vds_run_hooked_idle_heads(env._h, 0) == 0
    o = make_oracle(g)
    o.reset(init[0])
    p = env.idle_heads_device_ptr(4)
    for t in range(6):
        env.step(); o.begin_tick()
        assert env.idle_heads_device_ptr(4) == p                           # the same L: a fixed address
        check_heads(env, 4, [o, o], "slot %d" % t)
        env.advance(); o.end_tick()
    check_heads(env, 7, [o, o], "another L")                                # another L: the block is made again, the values are right
    check_heads(env, 4, [o, o], "the first L again")
    env.run(5)                                                              # after a run: the lists as it left them
    for _ in range(5):
        o.begin_tick(); o.end_tick()
    check_heads(env, 4, [o, o], "after run(5)")
    env.close()


# ---- the reference-compatible Simulation shell -----------------------------------------------------------------------------------------
from test_gpu_simulation_shell import make_sim  # noqa: E402
from vehicles_dispatch_simulator_amd.simulation import Simulation  # noqa: E402


class HeadsCheckSim(Simulation):
    """DispatchFunction over all replicas: BatchedObs["idle_veh"] / ["idle_node"] of this object's replica against its own object views
    (brought up to date with the device first: the batched loop refreshes them after the day only)."""

    def DispatchFunction(self):
        self._touch(); self._advance_mirror()
        L = 4
        veh = self.BatchedObs["idle_veh"][self.Replica].cpu().numpy()
        node = self.BatchedObs["idle_node"][self.Replica].cpu().numpy()
        assert veh.shape == (len(self.Clusters), L) and tuple(self.BatchedObs["idle_veh"].shape) == (self.Replicas, len(self.Clusters), L)
        for c in self.Clusters:
            ids = [v.ID for v in c.IdleVehicles][:L]
            loc = [v.LocationNode for v in c.IdleVehicles][:L]
            assert veh[c.ID].tolist() == ids + [-1] * (L - len(ids)), (self.step, c.ID)
            assert node[c.ID].tolist() == loc + [-1] * (L - len(loc)), (self.step, c.ID)
            self.checked += len(ids)
        return None


class HeadsPolicySim(Simulation):
    def BatchedPolicy(self, ob):
        self.keys = sorted(ob)
        self.shapes = (tuple(ob["idle_veh"].shape), tuple(ob["idle_node"].shape))
        self.filled.add_((ob["idle_veh"] >= 0).sum())
        return self.noop


def test_simulation_batched_idle_heads():
    import torch
    g = load_golden("tiny_kmeans")
    R = 4
    sim = make_sim(g, HeadsCheckSim, Replicas=R, Replica=1, VehicleSeed=55, BatchedHooks=True, BatchedIdleHeads=4)
    sim.checked = 0
    sim.SimCity()
    assert sim.step == sim.env.T and sim.checked > 4 * sim.env.T
    sim.env.close()
    pol = make_sim(g, HeadsPolicySim, Replicas=R, VehicleSeed=55, BatchedHooks=True, BatchedIdleHeads=4)
    pol.filled = torch.zeros((), dtype=torch.int64, device="cuda")
    pol.noop = torch.full((R, 1, 3), -1, dtype=torch.int32, device="cuda")
    pol.SimCity()
    assert pol.BatchedPolicyGraphError is None, pol.BatchedPolicyGraphError
    assert {"idle_veh", "idle_node"} <= set(pol.keys) and pol.shapes == ((R, int(g["C"]), 4),) * 2
    assert {"idle_veh", "idle_node"} <= set(pol.BatchedObs) and int(pol.filled.item()) > 0
    pol.env.close()
    with pytest.raises(Exception, match="BatchedHooks"):
        make_sim(g, Simulation, BatchedIdleHeads=4)


# ---- guarded build ---------------------------------------------------------------------------------------------------------------------
def test_guarded_build_idle_heads():
    """This file's cases that read the most differently shaped tables (dense, stamp form + flush, idle_cap < L) under the guarded
    library: a read beyond a list's table returns the poison, a write beyond the block damages a guard (found when the handle closes)."""
    from test_gpu_debug_builds import build
    lib = build("canary", "libvds_canary.so")
    env = dict(os.environ, VDS_LIB=lib)
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "tiny_kmeans-fast or tiny_kmeans_dfs2-fast or tiny_two_orders"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "3 passed" in p.stdout, p.stdout[-500:]
