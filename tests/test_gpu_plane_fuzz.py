"""The per-slot device planes a batched policy reads, against the CPU oracle at EVERY slot of fuzzed days (the cities of
test_gpu_fuzz.py: out-of-order releases, negative costs, ties, pickup windows, 5 / 15-minute ticks, short rings):
  * the five packed observation planes (``obs`` / ``obs_torch``: ``k_pack_obs``), every replica;
  * the in-place views of the bucket records (``obs_inplace_torch``) wherever the handle offers them;
  * SupplyExpect kept in place (``supply_inplace_torch``, ``ring[slot]``) where the dense layout with one shared day takes it, VDS_ESTATE
    where the library refuses it;
  * the four outcome planes (``k_slot_outcomes``) against the orders whose oracle status turned non-zero in the slot
    (``outcome_expect.processed_planes``);
  * per-replica order days with a regrouping replica -> day map: a replica whose day is over keeps its last planes and has zero
    outcomes, with and without VDS_SUPPLY_INPLACE=1;
  * the one-launch hooked day (``run_hooked`` with a captured recorder policy that dispatches), slot by slot;
  * ``k_tick_dense_mixed`` (seeded per-(slot, cluster) forms) at fuzz shapes: partial last workgroups, ties, hot spots.
Case counts: VDS_PLANE_FUZZ_N, VDS_PLANE_FUZZ_MEDIUM_N, VDS_PLANE_FUZZ_DAYS_N, VDS_PLANE_FUZZ_HOOKED_N, VDS_PLANE_FUZZ_MIXED_N."""
import os

import numpy as np
import pytest

from oracle.oracle import Oracle
from outcome_expect import NAMES, processed_planes
from test_gpu_fuzz import days_case, medium_case, random_case
from vehicles_dispatch_simulator_amd import BatchedDispatchEnv, neighbors_to_csr, synth

pytestmark = pytest.mark.gpu

# env plane -> oracle plane right after the slot's Update + Match (before any dispatch): env idle_now is the oracle's idle_post there
OBS_MAP = (("idle_pre", "idle_pre"), ("idle_now", "idle_post"), ("supply", "supply"), ("cl_orders", "cl_orders"), ("inflight", "inflight"))
ESTATE = "libvds error -4"


class environ:
    """Library switches read when the order tables are loaded, set for the load only (as test_gpu_parity.make_env does)."""

    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_env(cost, n2c, off, idx, V, cfg, R, idle_cap=None, **kw):
    return BatchedDispatchEnv(cost, n2c, off, idx, replicas=R, vehicles=V, depth_limit=cfg["depth"], neighbor_can_server=cfg["neighbor"],
                              tick_minutes=cfg["tick"], reject_threshold=cfg["threshold"], ring_ticks=cfg["ring_ticks"],
                              force_generic=cfg["force_generic"], idle_cap=idle_cap or max(64, V), ring_cap=max(16, V), far_cap=max(64, V), **kw)


def make_oracle(cost, n2c, off, idx, V, cfg, day, init):
    o = Oracle(cost, n2c, off, idx, cfg["depth"], cfg["neighbor"], day[0], day[1], day[2], V, tick_minutes=cfg["tick"], reject_threshold=cfg["threshold"])
    o.reset(init)
    return o


def request_supply_inplace(env, expect_ok):
    """``supply_inplace_torch`` before the reset: (ring, slot) where the library keeps SupplyExpect in place, None where it refuses - and
    then it must refuse with VDS_ESTATE."""
    try:
        sup = env.supply_inplace_torch()
    except Exception as e:
        assert ESTATE in str(e), e
        assert expect_ok is not True, "supply in place refused: %s" % e
        return None
    assert expect_ok is not False, "supply in place granted where the library should refuse it"
    return sup


def inplace_views(env):
    try:
        return env.obs_inplace_torch()
    except Exception as e:
        assert ESTATE in str(e) and "regrouped" in str(e), e
        return None


class PlaneChecker:
    """Per replica: the oracle, the statuses before the slot, the planes of its last live slot."""

    def __init__(self, env, oracles, pickup_clusters, sup=None, inplace=None, tag=""):
        self.env, self.oracles, self.cl = env, oracles, pickup_clusters
        self.prev = [o.orders()["status"] for o in oracles]
        self.last = [None] * len(oracles)
        self.sup, self.inplace, self.tag = sup, inplace, tag

    def check(self, t, live):
        """Right after env.step() and the live oracles' begin_tick(), before any dispatch."""
        env, C = self.env, self.env.C
        ob = env.obs()
        oc = env.outcomes()
        got_oc = np.stack([oc[k] for k in NAMES], axis=-1)
        ip = {k: v.cpu().numpy() for k, v in self.inplace.items()} if self.inplace is not None else None
        if self.sup is not None:
            ring = self.sup[0][int(self.sup[1].item())].cpu().numpy()
            np.testing.assert_array_equal(ring, ob["supply"], err_msg="%s slot %d supply in place" % (self.tag, t))
        for r, o in enumerate(self.oracles):
            msg = "%s slot %d replica %d" % (self.tag, t, r)
            if r in live:
                oo, od = o.obs(), o.orders()
                exp = {a: oo[b] for a, b in OBS_MAP}
                exp_oc = processed_planes(self.prev[r], od["status"], self.cl[r], od["wait"], od["value"], C)
                self.prev[r] = od["status"]
                self.last[r] = exp
            else:                              # the day is over: the planes of its last slot, no outcomes
                exp = self.last[r]
                exp_oc = np.zeros((C, 4), dtype=np.int64)
            for a, _ in OBS_MAP:
                np.testing.assert_array_equal(ob[a][r], exp[a], err_msg="%s %s" % (msg, a))
            np.testing.assert_array_equal(got_oc[r], exp_oc, err_msg="%s outcomes" % msg)
            if ip is not None:
                for a in ("idle_pre", "idle_now", "cl_orders"):
                    np.testing.assert_array_equal(ip[a][r], exp[a], err_msg="%s in place %s" % (msg, a))


def check_end_of_day(env, oracles, tag):
    got, cn = env.orders(), env.counters()
    for r, o in enumerate(oracles):
        exp, oc = o.orders(), o.counters()
        n = exp["status"].size
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(got[k][r][:n], exp[k], err_msg="%s replica %d %s" % (tag, r, k))
        for i, k in enumerate(("order_num", "reject_num", "matched", "wait_sum", "dispatch_num", "dispatch_cost", "sum_order_value", "evals")):
            assert cn[r, i] == oc[k], (tag, r, k)
        L, G = o.lists(), env.lists(r)
        for k in ("idle_off", "idle_veh", "arr_off", "arr_veh", "arr_min"):
            np.testing.assert_array_equal(G[k], L[k], err_msg="%s replica %d %s" % (tag, r, k))


def pick_dispatches(rng, oracles, rows, valid_nodes):
    """As test_gpu_fuzz.run_case: a few idle vehicles of each replica in ``rows`` by their position in the slot's idle lists."""
    reps, cls, poss, tgts = [], [], [], []
    for r in rows:
        o = oracles[r]
        L = o.lists()
        nidle = int(L["idle_off"][-1])
        if nidle == 0:
            continue
        pickn = rng.choice(nidle, size=min(nidle, int(rng.integers(1, 5))), replace=False)
        vehs = L["idle_veh"][pickn]
        tg = rng.choice(valid_nodes, size=vehs.size).astype(np.int32)
        for flat, tnode in zip(pickn, tg):
            c = int(np.searchsorted(L["idle_off"], flat, side="right") - 1)
            reps.append(r); cls.append(c); poss.append(int(flat - L["idle_off"][c])); tgts.append(int(tnode))
        o.dispatch(vehs, tg)
    return reps, cls, poss, tgts


def dispatch_tensor(R, reps, cls, poss, tgts):
    import torch
    cntr = np.bincount(reps, minlength=R)
    acts = np.full((R, int(cntr.max()) + 1, 3), -1, dtype=np.int32)
    slot = np.zeros(R, dtype=np.int64)
    for r_, c_, p_, t_ in zip(reps, cls, poss, tgts):
        acts[r_, slot[r_] + (slot[r_] > 0)] = (c_, p_, t_)      # (an empty slot after the first action)
        slot[r_] += 1
    return torch.from_numpy(acts).cuda()


# ---- 1. one shared day: every plane at every slot ---------------------------------------------------------------------------------
def shared_day(seed, case, idle_cap=None, R=None, environ_kw=None, dense_debug=None, sup_request=None, expect_mixed=False):
    cost, n2c, nbr, V, rel, pick, dele, valid_nodes, cfg = case
    off, idx = neighbors_to_csr(nbr)
    R = R or cfg["R"]
    rng = np.random.default_rng(310_000 + seed)          # (this module's own streams: the cases stay what test_gpu_fuzz makes of them)
    init = rng.choice(valid_nodes, size=(R, V)).astype(np.int32) if V else np.zeros((R, 0), np.int32)
    kw = {}
    if dense_debug is not None:
        kw["dense_debug"] = dense_debug
    with environ(**(environ_kw or {})):
        env = make_env(cost, n2c, off, idx, V, cfg, R, idle_cap=idle_cap, **kw)
        env.load_orders(rel, pick, dele)
    want_sup = rng.random() < 0.7 if sup_request is None else sup_request
    sup = request_supply_inplace(env, None) if want_sup else None
    env.reset(init)
    oracles = [make_oracle(cost, n2c, off, idx, V, cfg, (rel, pick, dele), init[r]) for r in range(R)]
    assert env.T == oracles[0].num_ticks
    tag = "seed %d cfg %s" % (seed, cfg)
    chk = PlaneChecker(env, oracles, [n2c[pick.astype(np.int64)]] * R, sup=sup, inplace=inplace_views(env), tag=tag)
    everyone = range(R)
    n_disp = 0
    for t in range(env.T):
        env.step()
        for o in oracles:
            o.begin_tick()
        chk.check(t, everyone)
        if cfg["dispatch"] and t % 4 == 1:
            reps, cls, poss, tgts = pick_dispatches(rng, oracles, everyone, valid_nodes)
            if reps and n_disp % 2 == 1:          # every other dispatching slot: the same actions as a device-resident [R, K, 3] tensor
                held = dispatch_tensor(R, reps, cls, poss, tgts)
                env.apply_dispatch_torch(held)
                env.sync()
            elif reps:
                env.apply_dispatch(reps, cls, poss, tgts)
            n_disp += bool(reps)
        env.advance()
        for o in oracles:
            o.end_tick()
    check_end_of_day(env, oracles, tag)
    forms = env.cluster_forms()
    env.close()
    return sup is not None, forms


def fuzz_switches(seed, cfg):
    """Library switches of a case (the tick forms of test_gpu_fuzz.run_case), from this module's own stream."""
    lr = np.random.default_rng(320_000 + seed)
    fg, env_kw, dd = cfg["force_generic"], {}, None
    if fg == 0 and lr.random() < 0.5:
        dd = (int(lr.choice([16, 8])), int(lr.choice([0, 0, 8, 24, 40])), int(lr.choice([0, 0, 2, 5])), int(lr.random() < 0.1) | (2 if lr.random() < 0.3 else 0))
    if fg == 0 and cfg["neighbor"] and lr.random() < 0.34:
        env_kw["VDS_DENSE_DFS"] = "0"
    elif fg == 0 and lr.random() < 0.34:
        env_kw["VDS_DENSE_TICK_FORMS"] = "alt"
    return env_kw, dd


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("VDS_PLANE_FUZZ_N", "48")))))
def test_random_city_planes_every_slot(seed):
    case = random_case(seed)
    env_kw, dd = fuzz_switches(seed, case[-1])
    shared_day(seed, case, environ_kw=env_kw, dense_debug=dd)


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("VDS_PLANE_FUZZ_MEDIUM_N", "3")))))
def test_medium_city_planes_every_slot(seed):
    case = medium_case(seed)
    env_kw, dd = fuzz_switches(50_000 + seed, case[-1])
    shared_day(seed, case, idle_cap=1024, environ_kw=env_kw, dense_debug=dd, sup_request=True)


# ---- per-replica order days, maps that regroup the storage ------------------------------------------------------------------------
def regrouping_map(rng, R, n_days):
    """A map that mixes days inside aligned groups of 16 with little padding by day (16 / 16 / 8 or 16 / 24 of 40 replicas, shuffled):
    the library stores the replicas regrouped by day."""
    counts = [16, 16, 8] if n_days >= 3 else [16, 24]
    m = np.concatenate([np.full(k, d, dtype=np.int32) for d, k in enumerate(counts)])
    return rng.permutation(m).astype(np.int32)


@pytest.mark.parametrize("layout", ["case", "dense"])
@pytest.mark.parametrize("supply_env", ["0", "1"])
@pytest.mark.parametrize("seed", list(range(int(os.environ.get("VDS_PLANE_FUZZ_DAYS_N", "6")))))
def test_replica_days_planes_every_slot(seed, supply_env, layout):
    """load_order_days (days_case's days, its own map spread over 40 replicas), then a regrouping set_replica_days map; dispatches with
    explicit arrival minutes and counted flags.  A replica whose day is over keeps its last planes and has zero outcomes; SupplyExpect in
    place is refused (VDS_ESTATE) whatever VDS_SUPPLY_INPLACE says, and the `supply` plane is right with it set.  layout "dense": the
    case's city and days with what the dense tick needs (default kernels, no neighbour search or pickup window, costs in a byte)."""
    cost, n2c, nbr, V, days, rd, valid_nodes, cfg = days_case(seed)
    if layout == "dense":
        cost = np.clip(cost, 0, 200).astype(np.int32)
        cfg = dict(cfg, force_generic=0, neighbor=False, threshold=600_000_000_000)
    off, idx = neighbors_to_csr(nbr)
    rng = np.random.default_rng(330_000 + seed)
    R = 40
    maps = [rd[np.arange(R) % rd.size].astype(np.int32), regrouping_map(rng, R, len(days))]
    init = rng.choice(valid_nodes, size=(R, V)).astype(np.int32) if V else np.zeros((R, 0), np.int32)
    with environ(VDS_SUPPLY_INPLACE=supply_env):
        env = make_env(cost, n2c, off, idx, V, cfg, R)
        env.load_order_days(days, maps[0])
    regrouped = []
    for ep, m in enumerate(maps):
        tag = "seed %d episode %d supply_env %s cfg %s" % (seed, ep, supply_env, cfg)
        if ep:
            env.set_replica_days(m)
        assert request_supply_inplace(env, False) is None
        env.reset(init)
        ip = inplace_views(env)
        regrouped.append(ip is None)
        oracles = [make_oracle(cost, n2c, off, idx, V, cfg, days[m[r]], init[r]) for r in range(R)]
        Ts = [o.num_ticks for o in oracles]
        assert env.T == max(Ts)
        chk = PlaneChecker(env, oracles, [n2c[days[m[r]][1].astype(np.int64)] for r in range(R)], inplace=ip, tag=tag)
        for t in range(env.T):
            env.step()
            if t == 0 and layout == "dense":
                assert env.main_kernel() == "k_tick_dense", (tag, env.main_kernel())
            live = [r for r in range(R) if t < Ts[r]]
            for r in live:
                oracles[r].begin_tick()
            chk.check(t, set(live))
            if cfg["dispatch"] and t % 3 == 1:
                # (not on a replica's last slot: its planes are then the ones read before the dispatch, kept to the end of the batch's day)
                rows = [r for r in live if t < Ts[r] - 1]
                reps, cls, poss, tgts, arrs, cnts = [], [], [], [], [], []
                for r in rows:
                    o = oracles[r]
                    L = o.lists()
                    nidle = int(L["idle_off"][-1])
                    if nidle == 0:
                        continue
                    pickn = rng.choice(nidle, size=min(nidle, int(rng.integers(1, 4))), replace=False)
                    vehs = L["idle_veh"][pickn]
                    tg = rng.choice(valid_nodes, size=vehs.size).astype(np.int32)
                    loc = o.vehicles()["loc"][vehs]
                    arr = (o.now_min + cost[tg, loc] + rng.integers(0, 25, size=vehs.size)).astype(np.int32)
                    counted = bool(rng.random() < 0.5)
                    for flat, tnode, am in zip(pickn, tg, arr):
                        c = int(np.searchsorted(L["idle_off"], flat, side="right") - 1)
                        reps.append(r); cls.append(c); poss.append(int(flat - L["idle_off"][c])); tgts.append(int(tnode)); arrs.append(int(am)); cnts.append(int(counted))
                    o.dispatch_at(vehs, tg, arrive_min=arr, counted=counted)
                if reps:
                    env.apply_dispatch(reps, cls, poss, tgts, arrive_min=arrs, counted=cnts)
            env.advance()
            for r in live:
                oracles[r].end_tick()
        check_end_of_day(env, oracles, tag)
    if cfg["force_generic"] == 0:
        assert regrouped[1], "the second map was expected to store the replicas regrouped by day"
    env.close()


# ---- 2. the hooked day (one graph launch per day), slot by slot ------------------------------------------------------------------
HOOKED_KINDS = {
    "dense": dict(force_generic=0, neighbor=False),
    "dense_dfs": dict(force_generic=0, neighbor=True, depth=2),
    "wide_dfs": dict(force_generic=0, neighbor=True, depth=2, environ={"VDS_DENSE_DFS": "0"}),
    "generic": dict(force_generic=1),
}


def hooked_case(seed, kind):
    cost, n2c, nbr, V, rel, pick, dele, valid_nodes, cfg = random_case(seed)
    spec = dict(HOOKED_KINDS[kind])
    env_kw = spec.pop("environ", {})
    cfg = dict(cfg, **spec)
    rng = np.random.default_rng(340_000 + seed)
    cfg["R"] = int(rng.integers(3, 12))
    if cfg["threshold"] != 600_000_000_000 and kind != "generic":
        cfg["threshold"] = 600_000_000_000        # (a live pickup window keeps the wide layout: the dense kinds would not be dense)
    return (cost, n2c, nbr, max(V, 8), rel, pick, dele, valid_nodes, cfg), env_kw


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("kind", list(HOOKED_KINDS))
@pytest.mark.parametrize("seed", list(range(int(os.environ.get("VDS_PLANE_FUZZ_HOOKED_N", "3")))))
def test_hooked_day_planes_every_slot(seed, kind, groups):
    """run_hooked(T, actions, policy_graph, inflight=True, outcomes=True): a captured recorder policy copies the five observation and four
    outcome planes into per-slot history tensors (indexed by a device slot counter) and writes actions computed on the device from
    idle_now - at most one per source cluster, some slots without any, some entries -1 - into the action tensor, which it logs.  The
    oracle replays the logged actions (positions in the slot's idle lists before the dispatch); every slot's planes and the end of the
    day are compared."""
    import torch
    case, env_kw = hooked_case(seed, kind)
    cost, n2c, nbr, V, rel, pick, dele, valid_nodes, cfg = case
    off, idx = neighbors_to_csr(nbr)
    R, C = cfg["R"], int(np.asarray(off).size - 1)
    rng = np.random.default_rng(350_000 + seed)
    init = rng.choice(valid_nodes, size=(R, V)).astype(np.int32)
    stream = torch.cuda.current_stream()
    with environ(**env_kw):
        env = make_env(cost, n2c, off, idx, V, cfg, R, stream=stream.cuda_stream)
        env.load_orders(rel, pick, dele)
    if groups > 1:
        env.set_run_groups(groups, -1)
    env.reset(init)
    T = env.T
    K = min(C, 4)
    ob = env.obs_torch()
    oc = env.outcomes_torch()
    h_obs = torch.zeros((T + 1, 5, R, C), dtype=torch.int32, device="cuda")
    h_oc = torch.zeros((T + 1, 4, R, C), dtype=torch.int64, device="cuda")
    h_act = torch.zeros((T + 1, R, K, 3), dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int64, device="cuda")
    acts = torch.full((R, K, 3), -1, dtype=torch.int32, device="cuda")
    vnodes = torch.from_numpy(valid_nodes.astype(np.int64)).cuda()
    rr = torch.arange(R, device="cuda", dtype=torch.int64)[:, None]

    def policy():
        h_obs.index_copy_(0, slot, ob[None])
        h_oc.index_copy_(0, slot, oc[None])
        idle = ob[1].to(torch.int64)                                    # idle_now: [R, C]
        cnt, src = torch.topk(idle, K, dim=1)                           # K distinct source clusters per replica
        s = slot.expand(R, K)
        pos = (s * 7 + rr * 3 + src) % cnt.clamp(min=1)
        ok = (cnt > 0) & ((s + rr + src) % 3 != 0) & (s % 5 != 2)       # (every fifth slot none at all)
        tgt = vnodes[(src * 31 + s * 17 + rr) % vnodes.numel()]
        acts.copy_(torch.stack([torch.where(ok, src, torch.full_like(src, -1)), pos, tgt], dim=2).to(torch.int32))
        h_act.index_copy_(0, slot, acts[None])
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
    h_obs.zero_(); h_oc.zero_(); h_act.fill_(-1); slot.zero_()
    env.run_hooked(T, actions=acts, policy_graph=graph, inflight=True, outcomes=True)
    env.sync()
    torch.cuda.synchronize()
    assert int(slot.item()) == T
    h_obs, h_oc, h_act = h_obs[:T].cpu().numpy(), h_oc[:T].cpu().numpy(), h_act[:T].cpu().numpy()
    tag = "seed %d kind %s groups %d cfg %s" % (seed, kind, groups, cfg)
    cl = n2c[pick.astype(np.int64)]
    n_disp = 0
    oracles = []
    for r in range(R):
        o = make_oracle(cost, n2c, off, idx, V, cfg, (rel, pick, dele), init[r])
        prev = o.orders()["status"]
        for t in range(T):
            o.begin_tick()
            oo, od = o.obs(), o.orders()
            msg = "%s slot %d replica %d" % (tag, t, r)
            for i, (a, b) in enumerate(OBS_MAP):
                np.testing.assert_array_equal(h_obs[t, i, r], oo[b], err_msg="%s %s" % (msg, a))
            np.testing.assert_array_equal(np.moveaxis(h_oc[t, :, r], 0, -1), processed_planes(prev, od["status"], cl, od["wait"], od["value"], C),
                                          err_msg="%s outcomes" % msg)
            prev = od["status"]
            L = o.lists()
            vehs, tgts = [], []
            for c_, p_, tg in h_act[t, r]:
                if c_ >= 0:
                    vehs.append(int(L["idle_veh"][L["idle_off"][c_] + p_])); tgts.append(int(tg))
            if vehs:
                o.dispatch(np.array(vehs), np.array(tgts))
                n_disp += len(vehs)
            o.end_tick()
        oracles.append(o)
    assert n_disp > 0 and (h_act[:, :, :, 0] < 0).any()
    check_end_of_day(env, oracles, tag)
    env.close()


# ---- 3. k_tick_dense_mixed at fuzz shapes --------------------------------------------------------------------------------------
def mixed_case(seed):
    rng = np.random.default_rng(360_000 + seed)
    N = int(rng.integers(60, 260))
    C = int(rng.integers(2, 25))
    city = synth.make_city(seed * 13 + 3, N=N, C=C, with_neighbors=False)
    cost = (city.cost // int(rng.choice([3, 5, 9]))).astype(np.int32)          # (byte costs, trips within the static arrival slots; ties)
    n2c = city.node2cluster.copy()
    nbr = []
    for c in range(C):
        k = int(rng.integers(0, min(C, 5)))
        nbr.append(rng.choice(C, size=k, replace=False).tolist() if k else [])
    valid_nodes = np.flatnonzero(n2c >= 0)
    V = int(rng.integers(40, 300))
    O = int(rng.integers(200, 2500))
    span = int(rng.integers(120, 1440))
    rel = np.sort(rng.integers(0, span, size=O)).astype(np.int32)
    pick = rng.choice(valid_nodes, size=O).astype(np.int32)
    dele = rng.choice(valid_nodes, size=O).astype(np.int32)
    hot = int(rng.integers(0, C))                                               # a single-cluster hot spot
    hot_nodes = np.flatnonzero(n2c == hot)
    if hot_nodes.size:
        sel = rng.random(O) < 0.6
        (dele if rng.random() < 0.5 else pick)[sel] = rng.choice(hot_nodes, size=int(sel.sum()))
    while True:
        R = int(rng.integers(64, 131))
        if R % 16:
            break
    cfg = dict(neighbor=bool(seed % 2), depth=int(rng.integers(1, 3)) if seed % 2 else 0, threshold=600_000_000_000, ring_ticks=32,
               force_generic=0, tick=int(rng.choice([10, 10, 5])), R=R, dispatch=bool(rng.random() < 0.5))
    return cost, n2c, nbr, V, rel, pick, dele, valid_nodes, cfg


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("VDS_PLANE_FUZZ_MIXED_N", "6")))))
def test_mixed_dense_forms_at_fuzz_shapes(seed):
    """R in [64, 130] and not a multiple of 16 (partial last workgroups in both forms), 2 - 24 clusters, tied costs, a hot spot, with and
    without neighbour search, VDS_DENSE_CLUSTER_SEED set: every slot runs both forms (a case that fell back does not pass); every replica's
    planes at every slot and its end of day against the oracle."""
    case = mixed_case(seed)
    ran_sup, forms = shared_day(seed, case, environ_kw={"VDS_DENSE_CLUSTER_SEED": str(seed + 1)}, sup_request=True)
    assert ran_sup, "the dense layout with one shared day keeps SupplyExpect in place"
    cfg = case[-1]
    T = forms.shape[0]
    assert T > 0 and forms.shape[1] == len(case[2]), forms.shape
    per_slot = forms.sum(axis=1)
    mixed = int(((per_slot > 0) & (per_slot < forms.shape[1])).sum())
    assert mixed == T, "seed %d R %d C %d: %d of %d slots ran both forms" % (seed, cfg["R"], forms.shape[1], mixed, T)
    print("mixed slots %d of %d (R %d, C %d, neighbour %s)" % (mixed, T, cfg["R"], forms.shape[1], cfg["neighbor"]))
