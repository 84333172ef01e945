"""The per-vehicle planes (``vehicles_all`` / ``vehicles_torch``: k_vehicle_lists, k_vehicle_pull, k_vehicle_fill) and the per-vehicle
dispatch (``apply_dispatch_vehicles_torch``, ``run_hooked(vehicle_planes=, vehicle_targets=)``: k_dispatch_vehicles) on the fuzzed
cities of test_gpu_fuzz.py - V = 0 .. 139 (0 included), negative costs, costs scaled 3 - 8 times under a ring of two slots (far list,
far inbox), force_generic 1 / 3 / 5, nodes in no cluster, 5 / 15-minute slots, out-of-order releases, R = 1 .. 8, order days per
replica with regrouped storage and padding replicas.  Every replica against its own CPU oracle, bit for bit, no tolerance:

  a. the walk: the six planes after the reset, after every step, after every dispatch call and after the last advance - against
     the oracle (helpers.check_oracle) and against ``env.vehicles(r)``; in every slot 0 .. 3 dispatch calls in random order out of the
     vehicle form, the K-form on the device and the host form (two vehicle-form calls in one slot occur), the oracle applying them in
     call order - container order, DispatchNum and TotallyDispatchCost after every call, which pins the sequence numbers across forms;
  b. the same walk from a crowded start (most vehicles of a replica in one cluster, all of them in replica 0; V = 65 .. 139: lists of
     two and of three 64-entry chunks);
  c. order days per replica (40 replicas, a spread map and a regrouping one), with and without VDS_SUPPLY_INPLACE=1: a replica whose
     day is over keeps its planes, refuses non-negative targets of its idle vehicles and ignores the others;
  d. the hooked day: a captured policy logs the requested planes of every slot and writes the slot's targets from a rule restated on
     the oracle; 1 / 2 run groups, K = 0 / K > 0, a replay with the same tensors and a rebuild with another target tensor, and the
     same calls slot by slot;
  e. two medium cities (V 150 .. 999, C 20 .. 149), planes at every 8th slot.
The reference of a vehicle-form call is include/vds.h's (helpers.oracle_apply_vehicles).  A day is cut to its first 48 slots (beyond the
ring horizon of every ring_ticks drawn); legs c run until the shortest day has been over for some slots.

Case counts: VDS_VEH_FUZZ_N (walks, default 14), VDS_VEH_FUZZ_DAYS_N (2), VDS_VEH_FUZZ_HOOKED_N (4), VDS_VEH_FUZZ_MEDIUM_N (2); the
crowded starts are the fixed list CROWDED_SEEDS.  Wall time of the file with the defaults on an MI355X: 35 s (47 tests, pytest start-up included)."""
import functools
import os

import numpy as np
import pytest

from helpers import REFUSALS, check_oracle, host_view, oracle_apply_vehicles
from test_gpu_fuzz import days_case, medium_case, random_case
from test_gpu_parity import check_lists
from test_gpu_plane_fuzz import (HOOKED_KINDS, check_end_of_day, dispatch_tensor, environ, fuzz_switches, hooked_case, make_env, make_oracle,
                                 pick_dispatches, regrouping_map)
from vehicles_dispatch_simulator_amd import neighbors_to_csr

pytestmark = pytest.mark.gpu

FIELDS = ("state", "node", "cluster", "arrive_min", "order")
NAMES = FIELDS + ("source",)
SLOTS = 48                      # of a day: past the ring horizon of every ring_ticks drawn (2, 8, 32)
DISPATCH_ERROR = "libvds error -4: dispatch of an idle position"
# random_case seeds of the walks, in the order VDS_VEH_FUZZ_N takes them (beyond the list: 1000, 1001, ...), chosen for what the city and
# the layout the library picks for it make certain - the conditions of the coverage test at the end of the file:
#   327, 261  V = 0 (generic kernels with R = 3; default kernels with R = 1)
#   0, 1, 12  wide layout, a ring of two slots: far list and far inbox; nodes in no cluster (refusals); 1 and 12 have negative costs
#   6, 58     dense layout with far tables, ring entries with and without an order; 58 has nodes in no cluster
#   5, 23     dense layout with static arrival slots; 23: lists of two chunks, nodes in no cluster
#   16, 104   force_generic 1 / 5, V = 134 / 135, nodes in no cluster
#   29, 50    wide layout with far tables: force_generic 5 with two clusters; a live pickup window
#   46        dense layout, V = 139, nodes in no cluster
WALK_SEEDS = [327, 0, 6, 5, 1, 23, 58, 12, 16, 29, 50, 104, 46, 261]
# crowded starts, V = 65 .. 139: dense (46, 40, 21 with static arrival slots, 77 with far tables, 6) and wide (104); V > 128 but for 6
CROWDED_SEEDS = [46, 40, 21, 104, 77, 6]


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def new_seen():
    return dict(dense=set(), wide=set(), ring_order=False, ring_dispatch=False, refused=dict.fromkeys(REFUSALS, 0), two_vehicle_calls=0,
                longest_list=0, moves=0, in_flight_targets=0, vehicle_calls=0, v0=0)


def merge(total, s):
    for k, v in s.items():
        if isinstance(v, set):
            total[k] |= v
        elif isinstance(v, dict):
            for kk, n in v.items():
                total[k][kk] += n
        elif k == "longest_list":
            total[k] = max(total[k], v)
        else:
            total[k] = total[k] or v if isinstance(v, bool) else total[k] + v
    return total


def settle(env, expect, tag):
    """The sticky dispatch error at the next sync exactly when a target of the call was refused, and once; nothing else (no capacity
    error: the tables hold V entries)."""
    err = None
    try:
        env.sync()
    except Exception as e:
        err = str(e)
    if expect:
        assert err is not None and DISPATCH_ERROR in err, "%s: expected the dispatch error, got %r" % (tag, err)
        env.sync()
    else:
        assert err is None, "%s: %s" % (tag, err)


def check_planes(env, oracles, tag, seen, dense, against_host=True):
    got = env.vehicles_all(source=True)
    assert set(got) == set(NAMES)
    for k, a in got.items():
        assert a.shape == (env.R, env.V) and a.dtype == np.int32, (tag, k)
    for r, o in enumerate(oracles):
        check_oracle({k: got[k][r] for k in got}, o, env.V, env.C, "%s replica %d" % (tag, r))
        if against_host:
            W = host_view(env, r)
            for k in FIELDS:
                np.testing.assert_array_equal(got[k][r], W[k], err_msg="%s replica %d %s against env.vehicles" % (tag, r, k))
    src, order = got["source"], got["order"]
    seen["dense" if dense else "wide"] |= set(np.unique(src).tolist())
    if dense:
        seen["ring_order"] |= bool(((src == 2) & (order >= 0)).any())
        seen["ring_dispatch"] |= bool(((src == 2) & (order == -1)).any())
    return got


def check_dispatched(env, oracles, t, tag):
    """Container order (the arrival dicts' insertion order: the sequence numbers), DispatchNum and TotallyDispatchCost."""
    cn = env.counters()
    for r, o in enumerate(oracles):
        check_lists(env, r, o, t)
        oc = o.counters()
        assert (cn[r, 4], cn[r, 5]) == (oc["dispatch_num"], oc["dispatch_cost"]), (tag, t, r, cn[r, 4:6].tolist(), oc)


def draw_targets(rng, oracles, n2c, valid_nodes, N, V, outside):
    """[R, V] targets: a fraction of all vehicles (idle or not) drawn from {0, 0.05, 0.3, 1.0}; in about a fifth of the draws every
    target lies in one cluster; where the city has nodes in no cluster, some draws name one of them or a node >= N."""
    R = len(oracles)
    tg = np.full((R, V), -1, dtype=np.int32)
    frac = float(rng.choice([0.0, 0.05, 0.3, 1.0]))
    pick = rng.random((R, V)) < frac
    nodes = valid_nodes
    if rng.random() < 0.2:
        nodes = np.flatnonzero(n2c == n2c[rng.choice(valid_nodes)])
    tg[pick] = rng.choice(nodes, size=int(pick.sum()))
    if outside.size and V and rng.random() < 0.35:
        for _ in range(int(rng.integers(1, 4))):
            r, v = int(rng.integers(0, R)), int(rng.integers(0, V))
            tg[r, v] = int(rng.choice(outside)) if rng.random() < 0.5 else int(rng.choice([N, N + 7, 2**31 - 1]))
    return tg


def apply_vehicle_form(env, oracles, tg, n2c, seen, tag, over=()):
    """The call on the engine and, replica by replica, on the oracles; the sticky error exactly when an entry was refused."""
    for o in oracles:
        L = o.lists()
        seen["longest_list"] = max(seen["longest_list"], int(np.diff(L["idle_off"]).max()) if L["idle_off"].size > 1 else 0)
    held = to_dev(tg)
    env.apply_dispatch_vehicles_torch(held)
    refused = 0
    for r, o in enumerate(oracles):
        L = o.lists()
        idle = np.zeros(o.V, dtype=bool); idle[L["idle_veh"][:L["idle_off"][-1]]] = True
        seen["in_flight_targets"] += int((~idle & (tg[r] >= 0)).sum())
        moves, ref = oracle_apply_vehicles(o, tg[r], n2c, over=r in over)
        seen["moves"] += moves
        for k, n in ref.items():
            seen["refused"][k] += n
            refused += n
    seen["vehicle_calls"] += 1
    settle(env, refused > 0, tag)
    del held


# ---- a / b / e. the walk ---------------------------------------------------------------------------------------------------------------
def walk(seed, case, crowded=False, idle_cap=None, every=1, stream_base=410_000):
    import torch
    cost, n2c, nbr, V, rel, pick, dele, valid_nodes, cfg = case
    off, idx = neighbors_to_csr(nbr)
    R, N, C = cfg["R"], cost.shape[0], len(nbr)
    rng = np.random.default_rng(stream_base + seed)          # (this module's own stream: the cases stay what test_gpu_fuzz makes of them)
    init = rng.choice(valid_nodes, size=(R, V)).astype(np.int32) if V else np.zeros((R, 0), np.int32)
    if crowded and V:                                        # api_script.Script.draw_init, how == 1: most vehicles of a replica in ONE cluster
        big = np.flatnonzero(n2c == np.bincount(n2c[valid_nodes]).argmax())
        for r in range(R):
            move = rng.random(V) < 0.8 if r else np.ones(V, dtype=bool)      # (replica 0: the whole fleet - a list of V entries at the reset)
            init[r, move] = rng.choice(big, size=int(move.sum()))
    env_kw, dd = fuzz_switches(seed, cfg)
    kw = dict(stream=torch.cuda.current_stream().cuda_stream)
    if dd is not None:
        kw["dense_debug"] = dd
    with environ(**env_kw):
        env = make_env(cost, n2c, off, idx, V, cfg, R, idle_cap=idle_cap, **kw)
        env.load_orders(rel, pick, dele)
    env.reset(init)
    oracles = [make_oracle(cost, n2c, off, idx, V, cfg, (rel, pick, dele), init[r]) for r in range(R)]
    assert env.T == oracles[0].num_ticks
    dense = bool(env.layout()["dense"])
    outside = np.flatnonzero(n2c < 0)
    seen = new_seen()
    seen["v0"] = int(V == 0)
    tag = "seed %d%s cfg %s" % (seed, " crowded" if crowded else "", cfg)
    T = min(env.T, SLOTS)
    got = check_planes(env, oracles, tag + " after reset", seen, dense)
    assert got["state"].shape == (R, V)
    for t in range(T):
        env.step()
        for o in oracles:
            o.begin_tick()
        at = every == 1 or t % every == every - 1 or t == T - 1
        if at:
            check_planes(env, oracles, "%s slot %d" % (tag, t), seen, dense)
        forms = [str(f) for f in rng.choice(["vehicles", "vehicles", "kform", "host"], size=int(rng.integers(0, 4)))]
        seen["two_vehicle_calls"] += forms.count("vehicles") >= 2
        for i, form in enumerate(forms):
            what = "%s slot %d call %d (%s of %s)" % (tag, t, i, form, forms)
            if form == "vehicles":
                tg = draw_targets(rng, oracles, n2c, valid_nodes, N, V, outside)
                apply_vehicle_form(env, oracles, tg, n2c, seen, what)
            else:
                reps, cls, poss, tgts = pick_dispatches(rng, oracles, range(R), valid_nodes)
                if reps and form == "kform":
                    held = dispatch_tensor(R, reps, cls, poss, tgts)
                    env.apply_dispatch_torch(held)
                    settle(env, False, what)
                    del held
                elif reps:
                    env.apply_dispatch(reps, cls, poss, tgts)
                    settle(env, False, what)
            if at:
                check_planes(env, oracles, what, seen, dense, against_host=False)
            check_dispatched(env, oracles, t, what)
        env.advance()
        for o in oracles:
            o.end_tick()
    check_planes(env, oracles, tag + " after the last advance", seen, dense)
    settle(env, False, tag + " end")
    check_end_of_day(env, oracles, tag)
    env.close()
    return seen


@functools.lru_cache(maxsize=None)
def walked(seed, crowded):
    return walk(seed, random_case(seed), crowded=crowded)


N_WALKS = int(os.environ.get("VDS_VEH_FUZZ_N", "14"))
WALKS = (WALK_SEEDS + [s for s in range(1000, 1000 + max(0, N_WALKS - len(WALK_SEEDS)))])[:N_WALKS]


@pytest.mark.parametrize("seed", WALKS)
def test_walk_planes_and_three_dispatch_forms_every_slot(seed):
    seen = walked(seed, False)
    V = random_case(seed)[3]
    if V == 0:          # both entry points are no-ops, the planes are [R, 0]
        assert seen["moves"] == 0 and seen["dense"] | seen["wide"] == set()
    else:
        assert 0 in seen["dense"] | seen["wide"]


@pytest.mark.parametrize("seed", CROWDED_SEEDS)
def test_walk_from_a_crowded_start(seed):
    V = random_case(seed)[3]
    assert 65 <= V <= 139
    seen = walked(seed, True)
    assert seen["longest_list"] > (128 if V > 128 else 64), seen["longest_list"]          # (a list of three / two chunks met a vehicle-form call)


@functools.lru_cache(maxsize=None)
def walked_medium(seed):
    return walk(seed, medium_case(seed), idle_cap=1024, every=8, stream_base=420_000)


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("VDS_VEH_FUZZ_MEDIUM_N", "2")))))
def test_walk_of_a_medium_city(seed):
    seen = walked_medium(seed)
    assert seen["moves"] > 0 and seen["vehicle_calls"] > 0, seen


# ---- c. order days per replica ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def days_walked(seed, supply_env, layout):
    import torch
    cost, n2c, nbr, V, days, rd, valid_nodes, cfg = days_case(seed)
    if layout == "dense":          # (test_gpu_plane_fuzz: the case's city and days with what the dense tick needs)
        cost = np.clip(cost, 0, 200).astype(np.int32)
        cfg = dict(cfg, force_generic=0, neighbor=False, threshold=600_000_000_000)
    off, idx = neighbors_to_csr(nbr)
    N = cost.shape[0]
    rng = np.random.default_rng(430_000 + seed)
    R = 40
    maps = [rd[np.arange(R) % rd.size].astype(np.int32), regrouping_map(rng, R, len(days))]
    init = rng.choice(valid_nodes, size=(R, V)).astype(np.int32) if V else np.zeros((R, 0), np.int32)
    with environ(VDS_SUPPLY_INPLACE=supply_env):
        env = make_env(cost, n2c, off, idx, V, cfg, R, stream=torch.cuda.current_stream().cuda_stream)
        env.load_order_days(days, maps[0])
    outside = np.flatnonzero(n2c < 0)
    seen = new_seen()
    for ep, m in enumerate(maps):
        tag = "seed %d episode %d supply_env %s layout %s cfg %s" % (seed, ep, supply_env, layout, cfg)
        if ep:
            env.set_replica_days(m)
        env.reset(init)
        dense = bool(env.layout()["dense"])
        oracles = [make_oracle(cost, n2c, off, idx, V, cfg, days[m[r]], init[r]) for r in range(R)]
        Ts = [o.num_ticks for o in oracles]
        assert env.T == max(Ts)
        T = min(env.T, max(SLOTS, min(Ts) + 6))          # (beyond the end of the shortest day, where the days differ in length)
        check_planes(env, oracles, tag + " after reset", seen, dense)
        for t in range(T):
            env.step()
            live = [r for r in range(R) if t < Ts[r]]
            over = set(range(R)) - set(live)
            for r in live:
                oracles[r].begin_tick()
            check_planes(env, oracles, "%s slot %d" % (tag, t), seen, dense, against_host=t % 4 == 0)
            if t % 2 == 1 or over:
                tg = draw_targets(rng, oracles, n2c, valid_nodes, N, V, outside)
                if over and rng.random() < 0.5:          # the replicas whose day is over name only vehicles on their way: ignored, no error
                    for r in over:
                        L = oracles[r].lists()
                        tg[r, L["idle_veh"][:L["idle_off"][-1]]] = -1
                apply_vehicle_form(env, oracles, tg, n2c, seen, "%s slot %d" % (tag, t), over=over)
                check_planes(env, oracles, "%s slot %d after the call" % (tag, t), seen, dense, against_host=False)
                if t % 4 == 1:
                    check_dispatched(env, oracles, t, tag)
            env.advance()
            for r in live:
                oracles[r].end_tick()
        check_planes(env, oracles, tag + " after the last advance", seen, dense)
        check_end_of_day(env, oracles, tag)
    env.close()
    return seen


DAYS_SEEDS = list(range(int(os.environ.get("VDS_VEH_FUZZ_DAYS_N", "2"))))


@pytest.mark.parametrize("layout", ["case", "dense"])
@pytest.mark.parametrize("supply_env", ["0", "1"])
@pytest.mark.parametrize("seed", DAYS_SEEDS)
def test_replica_days_planes_and_targets_every_slot(seed, supply_env, layout):
    days_walked(seed, supply_env, layout)


# ---- d. the hooked day -----------------------------------------------------------------------------------------------------------------
def rule_targets(o, slot, node_of, V, C):
    """The policy restated on the oracle (test_gpu_dispatch_vehicles.rule_targets): idle vehicles with v % 7 == slot % 7 in clusters
    with more than two idle vehicles go to the first node of the next cluster (-1, no move, where that cluster owns no node)."""
    L = o.lists()
    n = np.diff(L["idle_off"])
    cl = np.repeat(np.arange(C), n)
    veh = L["idle_veh"][:L["idle_off"][-1]]
    tg = np.full(V, -1, dtype=np.int32)
    go = (veh % 7 == slot % 7) & (n[cl] > 2)
    tg[veh[go]] = node_of[(cl[go] + 1) % C]
    return tg


HOOKED_N = int(os.environ.get("VDS_VEH_FUZZ_HOOKED_N", "4"))


@pytest.mark.parametrize("with_k", [False, True], ids=["K0", "K2"])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("seed", list(range(HOOKED_N)))
def test_hooked_day_logs_planes_and_dispatches_by_rule(seed, groups, with_k):
    """run_hooked(n, actions=, vehicle_planes=, vehicle_targets=, policy_graph=) on a fuzzed city (test_gpu_plane_fuzz.hooked_case; the
    kind goes round with the seed).  The captured policy copies the block of vehicle planes into row t of a [T, 6, R, V] log, writes
    the slot's targets by the rule and - K > 0 - K-form actions computed from idle_now, which it logs.  Requested planes of every slot
    against the oracle, planes not requested keep what the block held; three launches (the same tensors twice: a replay; another
    target tensor: a rebuild) and the same calls slot by slot all end in the oracle's day."""
    import torch
    kind = list(HOOKED_KINDS)[seed % len(HOOKED_KINDS)]
    case, env_kw = hooked_case(seed, kind)
    cost, n2c, nbr, V, rel, pick, dele, valid_nodes, cfg = case
    off, idx = neighbors_to_csr(nbr)
    R, C = cfg["R"], len(nbr)
    rng = np.random.default_rng(440_000 + seed)
    init = rng.choice(valid_nodes, size=(R, V)).astype(np.int32)
    first = [np.flatnonzero(n2c == c) for c in range(C)]
    node_of = np.array([f[0] if f.size else -1 for f in first], dtype=np.int64)
    mask = 1 | 4 | int(rng.integers(0, 64))                  # the rule reads state and cluster
    stream = torch.cuda.current_stream()
    with environ(**env_kw):
        env = make_env(cost, n2c, off, idx, V, cfg, R, stream=stream.cuda_stream)
        env.load_orders(rel, pick, dele)
    if groups > 1:
        env.set_run_groups(groups, -1)
    env.reset(init)
    T = min(env.T, SLOTS)
    K = min(C, 2)
    ob = env.obs_torch()
    pl = env.vehicles_torch(source=True)                       # all six planes as the reset left them; the views of the block
    planes = [pl[k] for k in NAMES]
    state, cluster = pl["state"], pl["cluster"]
    h_veh = torch.zeros((T + 1, 6, R, V), dtype=torch.int32, device="cuda")
    h_act = torch.zeros((T + 1, R, K, 3), dtype=torch.int32, device="cuda")
    h_tgt = torch.zeros((T + 1, R, V), dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int64, device="cuda")
    targets = torch.full((R, V), -1, dtype=torch.int32, device="cuda")
    targets2 = torch.full((R, V), -1, dtype=torch.int32, device="cuda")
    acts = torch.full((R, K, 3), -1, dtype=torch.int32, device="cuda")
    vmod = (torch.arange(V, device="cuda", dtype=torch.int64) % 7)[None, :]
    node_t = torch.from_numpy(node_of).cuda()
    vnodes = torch.from_numpy(valid_nodes.astype(np.int64)).cuda()
    ones = torch.ones((R, V), dtype=torch.int64, device="cuda")
    rr = torch.arange(R, device="cuda", dtype=torch.int64)[:, None]

    def policy():
        h_veh.index_copy_(0, slot, torch.stack(planes)[None])
        idle = state == 0
        cl = cluster.to(torch.int64).clamp(min=0)
        cnt = torch.zeros((R, C), dtype=torch.int64, device="cuda").scatter_add_(1, cl, ones * idle)
        go = idle & (vmod == slot % 7) & (torch.gather(cnt, 1, cl) > 2)
        tgt = node_t[(cl + 1) % C]
        targets.copy_(torch.where(go, tgt, torch.full_like(tgt, -1)).to(torch.int32))
        targets2.copy_(targets)
        h_tgt.index_copy_(0, slot, targets[None])
        # K-form actions as test_gpu_plane_fuzz's recorder policy draws them (applied only where the day is launched with them)
        cn, src = torch.topk(ob[1].to(torch.int64), K, dim=1)
        s = slot.expand(R, K)
        pos = (s * 7 + rr * 3 + src) % cn.clamp(min=1)
        ok = (cn > 0) & ((s + rr + src) % 3 != 0)
        at = vnodes[(src * 31 + s * 17 + rr) % vnodes.numel()]
        acts.copy_(torch.stack([torch.where(ok, src, torch.full_like(src, -1)), pos, at], dim=2).to(torch.int32))
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
    torch.cuda.synchronize()
    tag = "seed %d kind %s groups %d K %d mask %d cfg %s" % (seed, kind, groups, K if with_k else 0, mask, cfg)

    def start():
        env.reset(init)
        now = env.vehicles_torch(source=True)               # what the block holds when the day starts: every plane at the reset
        held = torch.stack([now[k] for k in NAMES]).cpu().numpy()
        h_veh.zero_(); h_act.fill_(-1); h_tgt.fill_(-1); slot.zero_()
        return held

    def result():
        env.sync()
        torch.cuda.synchronize()
        assert int(slot.item()) == T
        od = env.orders()
        return dict(veh=h_veh[:T].cpu().numpy(), act=h_act[:T].cpu().numpy(), tgt=h_tgt[:T].cpu().numpy(), lists=[env.lists(r) for r in range(R)],
                    counters=env.counters(), status=od["status"], vehicle=od["vehicle"], wait=od["wait"], end=env.vehicles_all(source=True))

    runs = {}
    for name, tg_tensor in (("first launch", targets), ("replay", targets), ("rebuild with another target tensor", targets2)):
        held = start()
        env.run_hooked(T, actions=acts if with_k else None, policy_graph=graph, vehicle_planes=mask, vehicle_targets=tg_tensor)
        runs[name] = dict(result(), held=held)
        assert env.vehicles_device_ptr(1) == state.data_ptr()
    # the same calls slot by slot
    held = start()
    for t in range(T):
        env.step()
        env.obs_torch()
        env.vehicles_device_ptr(mask)
        graph.replay()
        if with_k:
            env.apply_dispatch_torch(acts)
        env.apply_dispatch_vehicles_torch(targets)
        env.advance()
    runs["slot by slot"] = dict(result(), held=held)

    # the oracle: the logged K-form actions first, then the rule's targets
    oracles, exp_veh, moves = [], np.full((T, 6, R, V), -1, dtype=np.int64), 0
    log = runs["first launch"]
    for r in range(R):
        o = make_oracle(cost, n2c, off, idx, V, cfg, (rel, pick, dele), init[r])
        for t in range(T):
            o.begin_tick()
            msg = "%s slot %d replica %d" % (tag, t, r)
            for name, run in runs.items():
                P = {k: run["veh"][t, i, r] for i, k in enumerate(NAMES) if mask >> i & 1}
                check_requested(P, o, V, C, mask, "%s: %s" % (name, msg))
                for i, k in enumerate(NAMES):
                    if not mask >> i & 1:          # not requested: what the block held
                        np.testing.assert_array_equal(run["veh"][t, i, r], run["held"][i, r], err_msg="%s: %s plane %s was not requested" % (name, msg, k))
            tg = rule_targets(o, t, node_of, V, C)
            np.testing.assert_array_equal(log["tgt"][t, r], tg, err_msg=msg + " targets")
            if with_k:
                L = o.lists()
                vehs = [int(L["idle_veh"][L["idle_off"][c_] + p_]) for c_, p_, _ in log["act"][t, r] if c_ >= 0]
                if vehs:
                    o.dispatch(np.array(vehs), np.array([int(x[2]) for x in log["act"][t, r] if x[0] >= 0]))
            moves += oracle_apply_vehicles(o, tg, n2c)[0]
            o.end_tick()
        oracles.append(o)
    assert moves > 0, tag
    for name, run in runs.items():
        for k in ("act", "tgt"):
            np.testing.assert_array_equal(run[k], log[k], err_msg="%s: %s %s" % (tag, name, k))
        for r, o in enumerate(oracles):
            L, oo, oc = o.lists(), o.orders(), o.counters()
            for k in ("idle_off", "idle_veh", "arr_off", "arr_veh", "arr_min"):
                np.testing.assert_array_equal(run["lists"][r][k], L[k], err_msg="%s: %s replica %d %s" % (tag, name, r, k))
            for k in ("status", "vehicle", "wait"):
                np.testing.assert_array_equal(run[k][r], oo[k], err_msg="%s: %s replica %d %s" % (tag, name, r, k))
            for i, k in enumerate(("order_num", "reject_num", "matched", "wait_sum", "dispatch_num", "dispatch_cost", "sum_order_value", "evals")):
                assert run["counters"][r, i] == oc[k], (tag, name, r, k)
            check_oracle({k: run["end"][k][r] for k in NAMES}, o, V, C, "%s: %s end of day replica %d" % (tag, name, r))
    env.close()


def check_requested(P, o, V, C, mask, tag):
    """helpers.check_oracle's assertions on the planes the day was asked for (each needs the state plane, which the rule reads)."""
    L, veh = o.lists(), o.vehicles()
    n, na = L["idle_off"][-1], L["arr_off"][-1]
    idle = np.zeros(V, dtype=bool); idle[L["idle_veh"][:n]] = True
    fly = L["arr_veh"][:na]
    assert ((P["state"] == 0) == idle).all() and set(np.flatnonzero(P["state"] > 0)) == set(fly.tolist()), tag
    np.testing.assert_array_equal(P["state"][fly], np.where(veh["order"][fly] >= 0, 1, 2), err_msg=tag)
    if mask & 2:
        np.testing.assert_array_equal(P["node"][idle], veh["loc"][idle], err_msg=tag)
        np.testing.assert_array_equal(P["node"][fly], veh["dest"][fly], err_msg=tag)
    cl = np.empty(V, dtype=np.int64)
    cl[L["idle_veh"][:n]] = np.repeat(np.arange(C), np.diff(L["idle_off"]))
    cl[fly] = np.repeat(np.arange(C), np.diff(L["arr_off"]))
    np.testing.assert_array_equal(P["cluster"], cl, err_msg=tag)
    if mask & 8:
        np.testing.assert_array_equal(P["arrive_min"][fly], L["arr_min"][:na], err_msg=tag)
        assert (P["arrive_min"][idle] == -1).all(), tag
    if mask & 16:
        np.testing.assert_array_equal(P["order"][fly], veh["order"][fly], err_msg=tag)
        assert (P["order"][idle] == -1).all(), tag
    if mask & 32:
        assert ((P["source"] == 0) == idle).all() and (P["source"][fly] >= 1).all() and (P["source"][fly] <= 4).all(), tag


# ---- the coverage conditions -------------------------------------------------------------------------------------------------------------
def test_the_corpus_reached_every_container_refusal_and_chunk_count():
    """Over the walks, the crowded starts, the medium cities and the days (each computed once per process): from the source plane every
    container 0 .. 4 on the dense layout and 0, 2, 3, 4 on the wide one; dense ring entries with and without an order; a refused
    target of each of the three kinds; a slot with two vehicle-form calls; a vehicle-form call on an idle list of more than 128
    entries (three chunks); the V = 0 case."""
    total = new_seen()
    for seed in WALKS:
        merge(total, walked(seed, False))
    for seed in CROWDED_SEEDS:
        merge(total, walked(seed, True))
    for seed in range(int(os.environ.get("VDS_VEH_FUZZ_MEDIUM_N", "2"))):
        merge(total, walked_medium(seed))
    for seed in DAYS_SEEDS:
        for supply_env in ("0", "1"):
            for layout in ("case", "dense"):
                merge(total, days_walked(seed, supply_env, layout))
    print({k: v for k, v in total.items()})
    assert {0, 1, 2, 3, 4} <= total["dense"], total
    assert {0, 2, 3, 4} <= total["wide"], total
    assert -1 not in total["dense"] | total["wide"], total
    assert total["ring_order"] and total["ring_dispatch"], total
    assert all(total["refused"][k] > 0 for k in REFUSALS), total["refused"]
    assert total["two_vehicle_calls"] > 0 and total["longest_list"] > 128, total
    assert total["v0"] > 0 and total["moves"] > 0 and total["in_flight_targets"] > 0, total
