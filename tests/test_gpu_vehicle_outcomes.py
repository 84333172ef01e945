"""Per-vehicle order outcomes of each slot (vds_vehicle_outcomes_device / vds_read_vehicle_outcomes, vds_run_hooked with
vds_run_hooked_vehicle_outcomes: k_vehicle_outcomes_fill + k_vehicle_outcomes): the int32 [R, V, 4] block {order, wait, value, pickup}
of what MatchFunction gave each vehicle in the slot stepped last, checked bit for bit at EVERY slot against the rows built from the
goldens captured from the unmodified reference or from the CPU oracle stepped alongside (vehicle_outcome_expect.py) - through every
tick family, grids of more than one block, odd sizes, order days per replica (regrouped storage with padding replicas), the one-graph
hooked day with a captured recorder policy, snapshot / restore, the block's lifetime, and on memory that starts out dirty."""
import ctypes
import functools
import gc
import os
import random
import sys

import numpy as np
import pytest

from helpers import dispatch_by_tick, load_golden, make_oracle, oracle_apply
from outcome_expect import tick_minutes_of
from test_gpu_dispatch_vehicles import CAPS, assert_same_day, day_result, rule_targets
from test_gpu_parity import TINY, make_env
from test_gpu_replica_days import mk_env, mk_oracle, synth_days
from test_gpu_slot_outcomes import FAMILIES, order_values
from test_order_tables import replica_plan
from vehicle_outcome_expect import NAMES, ORDER, expected_from_golden, expected_vehicle_outcomes, processed_rows, slot_sums
from vehicles_dispatch_simulator_amd import _lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def got_rows(env):
    vo = env.vehicle_outcomes()
    assert tuple(vo) == NAMES and all(a.shape == (env.R, env.V) and a.dtype == np.int32 for a in vo.values())
    return np.stack([vo[k] for k in NAMES], axis=-1)          # [R, V, 4]


def torch_rows(env):
    blk = env.vehicle_outcomes_torch()
    assert tuple(blk.shape) == (env.R, env.V, 4) and str(blk.dtype) == "torch.int32" and blk.is_cuda
    env.sync()
    return blk.cpu().numpy()


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def seeded_init(g, R, first=None, seed=300):
    V, N = int(g["V"]), int(g["N"])
    valid = g["node2cluster"] >= 0
    init = np.stack([synth.init_vehicle_nodes(random.Random(seed + r), N, V, valid) for r in range(R)]).astype(np.int32).reshape(R, V)
    if first is not None:
        init[0] = first
    return init


def assert_rows(got, exp, tag):
    if not np.array_equal(got, exp):
        v = int(np.flatnonzero((got != exp).any(axis=-1))[0])
        pytest.fail("%s vehicle %d: got %s, expected %s" % (tag, v, got[v].tolist(), exp[v].tolist()))


def check_sums(env, rows, tag):
    """The two sum checks of include/vds.h against the per-cluster planes of the same slot."""
    oc = env.outcomes()
    served, wait, value = slot_sums(rows)
    np.testing.assert_array_equal(served, oc["served"].sum(axis=1), err_msg=tag)
    np.testing.assert_array_equal(wait, oc["wait_sum"].sum(axis=1), err_msg=tag)
    np.testing.assert_array_equal(value, oc["value_sum"].sum(axis=1), err_msg=tag)


def oracle_day_rows(o, release, pickup, value, tick, V):
    """Expected [T, V, 4] of one replica without dispatch: the CPU oracle's per-order results of its day."""
    T = o.num_ticks
    o.run_day()
    res = o.orders()
    return expected_vehicle_outcomes(release, pickup, res["status"], res["vehicle"], res["wait"], value, tick, T, V)


# ---- 1. every slot of every tiny fixture, stepwise ---------------------------------------------------------------------------------------
def day_walk(name, R=3, kernel=None, **kw):
    """Replica 0 replays the reference's record (its dispatch log applied in the host form); replica 1 moves one vehicle in the K-form
    and replica 2 one in the vehicle form every fourth slot, each against an oracle stepped alongside."""
    g = load_golden(name)
    V, C = int(g["V"]), int(g["C"])
    init = seeded_init(g, R, first=g["veh_node"])
    ref = expected_from_golden(g)
    disp = dispatch_by_tick(g)
    extra = int(g["dispatch_extra_minutes"]) if "dispatch_extra_minutes" in g else 0
    valid = np.flatnonzero(g["node2cluster"] >= 0)
    oracles = [None]
    for r in range(1, R):
        o = make_oracle(g)
        o.reset(init[r])
        oracles.append(o)
    before = [None] + [o.orders() for o in oracles[1:]]
    env = make_env(g, R, **kw)
    assert kernel is None or env.main_kernel() == kernel
    env.reset(init)
    assert (got_rows(env) == -1).all() and (torch_rows(env) == -1).all()          # before the first step
    matched = moved = 0
    for t in range(env.T):
        env.step()
        got = got_rows(env)
        assert_rows(got[0], ref[t], "%s slot %d replica 0" % (name, t))
        for r in range(1, R):
            o = oracles[r]
            o.begin_tick()
            after = o.orders()
            exp = processed_rows(before[r]["status"], after["status"], g["o_pickup"], after["vehicle"], after["wait"], after["value"], V)
            before[r] = after
            assert_rows(got[r], exp, "%s slot %d replica %d" % (name, t, r))
        np.testing.assert_array_equal(torch_rows(env), got, err_msg="slot %d: the torch view" % t)
        check_sums(env, got, "%s slot %d" % (name, t))
        matched += int((got[..., ORDER] >= 0).sum())
        # the slot's dispatch calls do not change the block: host form (the reference's log), K-form, vehicle form
        calls, held = 0, []          # (held: the device tensors of the slot's calls, until the sync below)
        if t in disp:
            rows = np.array(disp[t])
            L = env.lists(0)
            pos = [int(np.flatnonzero(L["idle_veh"][L["idle_off"][cl]:L["idle_off"][cl + 1]] == veh)[0]) for veh, cl in zip(rows[:, 1], rows[:, 2])]
            rep = np.zeros(len(rows), dtype=np.int32)
            if extra:
                env.apply_dispatch(rep, rows[:, 2], pos, rows[:, 4], arrive_min=env.clock[1] + rows[:, 5] + extra)
            else:
                env.apply_dispatch(rep, rows[:, 2], pos, rows[:, 4])
            calls += 1
        if t % 4 == 1 and R >= 3 and V > 0:
            node = int(valid[(7 * t + 3) % valid.size])
            L = oracles[1].lists()
            n = np.diff(L["idle_off"])
            if n.max() > 0:
                c = int(np.argmax(n))
                acts = np.full((R, 1, 3), -1, dtype=np.int32)
                acts[1, 0] = (c, 0, node)
                held.append(to_dev(acts))
                env.apply_dispatch_torch(held[-1])
                oracles[1].dispatch(L["idle_veh"][L["idle_off"][c]:L["idle_off"][c] + 1], np.array([node]))
                calls += 1
            L = oracles[2].lists()
            if L["idle_off"][-1] > 0:
                tg = np.full((R, V), -1, dtype=np.int32)
                tg[2, L["idle_veh"][L["idle_off"][-1] - 1]] = node
                held.append(to_dev(tg))
                env.apply_dispatch_vehicles_torch(held[-1])
                moved += oracle_apply(oracles[2], tg[2])[0]
                calls += 1
        if calls:
            env.sync()
            np.testing.assert_array_equal(got_rows(env), got, err_msg="slot %d: dispatch changed the block" % t)
        env.advance()
        for o in oracles[1:]:
            o.end_tick()
        np.testing.assert_array_equal(got_rows(env), got, err_msg="slot %d: advance changed the block" % t)
    # the days ended where the oracles ended: the dispatched vehicles were the oracles'
    od = env.orders()
    for r in range(1, R):
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(od[k][r], before[r][k], err_msg="%s replica %d %s" % (name, r, k))
    np.testing.assert_array_equal(od["status"][0], g["o_status"])
    assert matched == int((od["status"] == 1).sum())
    return env, dict(matched=matched, moved=moved)


@pytest.mark.parametrize("name", TINY)
def test_rows_equal_reference_at_every_slot(name):
    env, seen = day_walk(name)
    assert seen["matched"] > 0 and (seen["moved"] > 0 or name == "tiny_two_orders" or env.T < 6)
    env.close()


@pytest.mark.parametrize("kernel,name,kw", FAMILIES, ids=["%s-%s-%d" % (k, n, i) for i, (k, n, _) in enumerate(FAMILIES)])
def test_rows_through_every_tick_family(kernel, name, kw):
    env, seen = day_walk(name, kernel=kernel, **kw)
    assert env.main_kernel() == kernel and seen["matched"] > 0
    env.close()


# ---- 2. more than one block in x, a replica tail ---------------------------------------------------------------------------------------
def no_dispatch_walk(g, R, init, expect, tag, torch_every=0):
    env = make_env(g, R)
    env.reset(init)
    for t in range(env.T):
        env.step()
        got = got_rows(env)
        for r in range(R):
            assert_rows(got[r], expect[r][t], "%s slot %d replica %d" % (tag, t, r))
        if torch_every and t % torch_every == 0:
            np.testing.assert_array_equal(torch_rows(env), got)
            check_sums(env, got, "%s slot %d" % (tag, t))
        env.advance()
    env.close()


def processed_per_slot(g):
    from outcome_expect import order_slots
    return np.bincount(order_slots(g["o_release_min"], tick_minutes_of(g))[g["o_status"] != 0], minlength=int(g["n_ticks"]))


def test_six_blocks_of_orders_and_neighbour_search_at_configs1_shape():
    """real_spectral192_dfs2 at R = 2: ~1350 orders per slot (six 256-thread blocks in x), neighbour search with re-pick chains, 10 000
    vehicles; y is one group of four with two live replicas."""
    g = load_golden("real_spectral192_dfs2")
    assert processed_per_slot(g).max() > 5 * 256
    V = int(g["V"])
    init = seeded_init(g, 2, first=g["veh_node"])
    expect = []
    for r in range(2):
        o = make_oracle(g)
        o.reset(init[r])
        expect.append(oracle_day_rows(o, g["o_release_min"], g["o_pickup"], order_values(g), tick_minutes_of(g), V))
        if r == 0:          # (the fixture keeps the head of the reference's vehicle column only: replica 0's oracle is tied to the record)
            res = o.orders()
            np.testing.assert_array_equal(res["status"], g["o_status"])
            np.testing.assert_array_equal(res["wait"][res["status"] == 1], g["o_wait"][g["o_status"] == 1])
            np.testing.assert_array_equal(res["vehicle"][:g["o_vehicle_head"].size], g["o_vehicle_head"])
    no_dispatch_walk(g, 2, init, expect, "real_spectral192_dfs2", torch_every=37)


def test_two_blocks_of_orders_and_a_replica_tail_of_one():
    """tiny_sort_ties (20 000 synthetic orders on the tiny city, up to 264 in one slot) at R = 5: two blocks in x, and with four replicas
    per thread one full group and a tail of one in y."""
    g = load_golden("tiny_sort_ties")
    assert processed_per_slot(g).max() > 256
    R, V = 5, int(g["V"])
    init = seeded_init(g, R, first=g["veh_node"], seed=900)
    expect = [expected_from_golden(g)]
    for r in range(1, R):
        o = make_oracle(g)
        o.reset(init[r])
        expect.append(oracle_day_rows(o, g["o_release_min"], g["o_pickup"], order_values(g), tick_minutes_of(g), V))
    assert not np.array_equal(expect[3], expect[4])
    no_dispatch_walk(g, R, init, expect, "tiny_sort_ties R=5", torch_every=11)


# ---- 3. odd sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,R,kw", [(1, 5, {}), (13, 5, {}), (13, 7, {"force_generic": 5}), (151, 1, {}), (37, 1, {"force_generic": 1})])
def test_odd_vehicle_and_replica_counts(V, R, kw):
    """V = 1, a V that is no multiple of anything, R = 1, R with a tail of three behind a full group of four."""
    g = dict(load_golden("tiny_kmeans"))
    g["V"] = np.int64(V)
    init = seeded_init(g, R, seed=4400)
    g["veh_node"] = init[0]
    expect = []
    for r in range(R):
        o = make_oracle(g)
        o.reset(init[r])
        expect.append(oracle_day_rows(o, g["o_release_min"], g["o_pickup"], order_values(g), tick_minutes_of(g), V))
    env = make_env(g, R, **kw)
    env.reset(init)
    assert (got_rows(env) == -1).all()
    matched = 0
    for t in range(40):
        env.step()
        got = got_rows(env)
        for r in range(R):
            assert_rows(got[r], expect[r][t], "V=%d R=%d slot %d replica %d" % (V, R, t, r))
        np.testing.assert_array_equal(torch_rows(env), got)
        check_sums(env, got, "V=%d R=%d slot %d" % (V, R, t))
        matched += int((got[..., ORDER] >= 0).sum())
        env.advance()
    assert matched > 0
    env.close()


def test_no_vehicles_is_a_no_op_also_inside_the_hooked_day():
    import torch
    g = dict(load_golden("tiny_kmeans"))
    g["V"] = np.int64(0)
    R = 3
    env = make_env(g, R, stream=torch.cuda.current_stream().cuda_stream)
    with pytest.raises(Exception, match="call vds_reset first"):
        env.vehicle_outcomes()
    env.reset(np.zeros((R, 0), dtype=np.int32))
    blk = env.vehicle_outcomes_torch()
    assert tuple(blk.shape) == (R, 0, 4)
    assert all(a.shape == (R, 0) for a in env.vehicle_outcomes().values())
    env.step(); env.advance()
    env.run_hooked(5, vehicle_outcomes=True)
    env.sync()
    assert env.clock[0] == 6 and tuple(env.vehicle_outcomes_torch().shape) == (R, 0, 4)
    cn = env.counters()
    assert (cn[:, 0] == cn[:, 1]).all() and cn[0, 0] > 0          # every processed order was rejected
    env.close()


# ---- 4. order days per replica, regrouped storage -------------------------------------------------------------------------------------
def test_per_replica_order_days_and_regrouped_storage():
    """The maps of test_gpu_slot_outcomes.test_per_replica_order_days_and_regrouped_storage: each replica's rows match its own day in
    the caller's order; a replica past its day reads all -1 - also where the block held something else before the call (a day's last
    slot holds the order that is never processed and matches nothing, so the block is overwritten from torch first)."""
    import torch
    g = load_golden("tiny_kmeans")
    R, V = 40, int(g["V"])
    days = synth_days(g, 5, seed=5200)
    init = seeded_init(g, R, seed=8100)
    env = mk_env(g, R)
    maps = [np.arange(R) // 8, np.arange(R) % 5, (np.arange(R) * 7 + 1) % 4, np.arange(R) % 3]
    # np.arange(R) % 3: 14 + 13 + 13 replicas - whatever the granule of the day groups, the replicas are stored by day as 3 x 16 with
    # eight padding replicas (the two maps before it are stored that way where the day groups may be eight or four replicas)
    for gran_small in (0, 1):
        rc, plan = replica_plan(maps[3], 5, gran_small=gran_small)
        assert rc == 0 and plan["regrouped"] and plan["R"] == 48 and int((plan["int2ext"] < 0).sum()) == 8
    env.load_order_days(days, maps[0].astype(np.int32))
    tick = tick_minutes_of(g)
    cache = {}
    regrouped, cleared = [], 0
    for ep, rd in enumerate(maps):
        if ep:
            env.set_replica_days(rd.astype(np.int32))
        try:
            env.obs_inplace_torch()
            regrouped.append(False)
        except Exception as e:
            assert "regrouped" in str(e), e
            regrouped.append(True)
        env.reset(init)
        expect = []
        for r in range(R):
            d = int(rd[r])
            if (r, d) not in cache:
                day = days[d]
                o = mk_oracle(g, day)
                o.reset(init[r])
                value = g["cost"][day[2].astype(np.int64), day[1].astype(np.int64)].astype(np.int64)
                cache[(r, d)] = oracle_day_rows(o, day[0], day[1], value, tick, V)
            expect.append(cache[(r, d)])
        Ts = [e.shape[0] for e in expect]
        assert env.T == max(Ts) and len(set(Ts)) > 1
        assert (got_rows(env) == -1).all()
        for t in range(env.T):
            env.step()
            poisoned = t in Ts or t % 20 == 6
            if poisoned:
                blk = env.vehicle_outcomes_torch()
                env.sync()
                blk.fill_(-7)
                torch.cuda.synchronize()
            got = got_rows(env)
            for r in range(R):
                exp = expect[r][t] if t < Ts[r] else np.full((V, 4), -1, dtype=np.int32)
                assert_rows(got[r], exp, "episode %d slot %d replica %d" % (ep, t, r))
                if poisoned and t >= Ts[r]:
                    cleared += 1                      # the fill reached a replica whose day is over
            if t % 20 == 5:
                np.testing.assert_array_equal(torch_rows(env), got)
                check_sums(env, got, "episode %d slot %d" % (ep, t))
            env.advance()
    assert regrouped[3] and not regrouped[0] and cleared > 0, (regrouped, cleared)
    env.close()


# ---- 5. the hooked day ---------------------------------------------------------------------------------------------------------------------
HG_R = 40


@functools.lru_cache(maxsize=None)
def hooked_expectation():
    """[T, R, V, 4] of tiny_kmeans with the vehicle-form rule of test_gpu_dispatch_vehicles applied behind every slot's match, and the
    oracles' final per-order results."""
    g = load_golden("tiny_kmeans")
    V, C = int(g["V"]), int(g["C"])
    node_of = np.array([np.flatnonzero(g["node2cluster"] == c)[0] for c in range(C)], dtype=np.int32)
    init = seeded_init(g, HG_R, seed=2000)
    rows, final, moves = [], [], 0
    for r in range(HG_R):
        o = make_oracle(g)
        o.reset(init[r])
        before, day = o.orders(), []
        for t in range(o.num_ticks):
            o.begin_tick()
            after = o.orders()
            day.append(processed_rows(before["status"], after["status"], g["o_pickup"], after["vehicle"], after["wait"], after["value"], V))
            before = after
            moves += oracle_apply(o, rule_targets(g, o, t, node_of))[0]
            o.end_tick()
        rows.append(np.stack(day))
        final.append(before)
    assert moves >= 20
    return g, init, node_of, np.stack(rows, axis=1), final


# (force_generic = 1: no day graph is built for this tick family - vds_run_hooked goes slot by slot through run_hooked_eager, which
# refreshes the block on the stream before it launches the policy)
@pytest.mark.parametrize("groups,kw", [(1, {}), (2, {}), (1, {"force_generic": 1})], ids=["one-chain", "two-groups", "eager-generic"])
def test_run_hooked_refreshes_the_block_for_a_captured_policy(groups, kw):
    import torch
    g, init, node_of, expect, final = hooked_expectation()
    V, C, R = int(g["V"]), int(g["C"]), HG_R
    stream = torch.cuda.current_stream()
    env = make_env(g, R, stream=stream.cuda_stream, **CAPS, **kw)
    env.set_run_groups(groups, -1)
    assert env._lib.vds_get_run_groups(env._h) == groups
    assert env.main_kernel() == ("k_tick" if kw else "k_tick_dense")
    T = env.T
    env.reset(init)
    ptr = env.vehicle_outcomes_device_ptr()
    blk = env.vehicle_outcomes_torch()
    assert blk.data_ptr() == ptr
    pl = env.vehicles_torch(state=True, node=False, cluster=True, arrive_min=False, order=False)
    state, cluster = pl["state"], pl["cluster"]
    heads = env.idle_heads_torch(4)
    oc = env.outcomes_torch()
    targets = torch.full((R, V), -1, dtype=torch.int32, device="cuda")
    log = torch.zeros((T, R, V, 4), dtype=torch.int32, device="cuda")
    served = torch.zeros((T, R), dtype=torch.int64, device="cuda")
    head0 = torch.zeros((T, R), dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int64, device="cuda")
    vmod = (torch.arange(V, device="cuda", dtype=torch.int64) % 7)[None, :]
    node_t = torch.from_numpy(node_of.astype(np.int64)).cuda()
    ones = torch.ones((R, V), dtype=torch.int64, device="cuda")

    def policy():
        log.index_copy_(0, slot, blk[None])
        served.index_copy_(0, slot, oc[0].sum(dim=1)[None])
        head0.index_copy_(0, slot, heads[0, :, 0, 0][None])
        idle = state == 0
        cl = cluster.to(torch.int64).clamp(min=0)
        cnt = torch.zeros((R, C), dtype=torch.int64, device="cuda").scatter_add_(1, cl, ones * idle)
        go = idle & (vmod == slot % 7) & (torch.gather(cnt, 1, cl) > 2)
        tgt = node_t[(cl + 1) % C]
        targets.copy_(torch.where(go, tgt, torch.full_like(tgt, -1)).to(torch.int32))
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
    on = dict(policy_graph=graph, outcomes=True, idle_heads=4, vehicle_planes=dict(state=True, cluster=True), vehicle_targets=targets,
              idle_pre=False, idle_now=False, supply=False, cl_orders=False)

    def start():
        env.reset(init)
        log.zero_(); served.zero_(); head0.fill_(-9); slot.zero_(); targets.fill_(-1)

    def check(tag):
        env.sync()
        torch.cuda.synchronize()
        assert int(slot.item()) == T, tag
        got = log.cpu().numpy()
        for t in range(T):
            for r in range(R):
                assert_rows(got[t, r], expect[t, r], "%s slot %d replica %d" % (tag, t, r))
        np.testing.assert_array_equal(served.cpu().numpy(), (expect[..., ORDER] >= 0).sum(axis=2), err_msg=tag)
        assert int((head0 == -9).sum().item()) == 0, tag
        assert env.vehicle_outcomes_device_ptr() == ptr, tag
        assert_rows(got_rows(env).reshape(R * V, 4), expect[T - 1].reshape(R * V, 4), tag + ": after the run, the last slot")
        res = day_result(env)
        for r in range(R):
            for k in ("status", "vehicle", "wait"):
                np.testing.assert_array_equal(res[k][r], final[r][k], err_msg="%s replica %d %s" % (tag, r, k))
        return res

    start()
    env.run_hooked(T, vehicle_outcomes=True, **on)
    first = check("groups %d: one launch" % groups)
    start()
    env.run_hooked(T, vehicle_outcomes=True, **on)                  # the same graph, replayed
    assert_same_day(first, check("groups %d: replay" % groups), "replay")
    env.load_orders(g["o_release_min"], g["o_pickup"], g["o_delivery"])      # the same sizes: the state tables stay, the graph is rebuilt
    start()
    assert env.vehicle_outcomes_device_ptr() == ptr
    env.run_hooked(T, vehicle_outcomes=True, **on)
    assert_same_day(first, check("groups %d: rebuilt behind load_orders" % groups), "rebuild")
    start()
    for t in range(T):                                             # the same calls slot by slot through the entry points
        env.step()
        env.outcomes_device_ptr()
        env.idle_heads_device_ptr(4)
        env.vehicles_device_ptr(5)
        env.vehicle_outcomes_device_ptr()
        graph.replay()
        env.apply_dispatch_vehicles_torch(targets)
        env.advance()
    assert_same_day(first, check("groups %d: slot by slot" % groups), "slot by slot")
    # switched off: the day is the same, the block is not touched
    start()
    blk.fill_(-7)
    env.run_hooked(T, **on)
    env.sync()
    torch.cuda.synchronize()
    assert int((blk == -7).all().item()) == 1 and int(slot.item()) == T
    assert int((log == -7).all().item()) == 1
    assert_same_day(first, day_result(env), "switched off")
    # ... and without a policy, a day with the switch equals the day of a second handle that never heard of it
    plain = dict(outcomes=True, idle_heads=4, idle_pre=False, idle_now=False, supply=False, cl_orders=False)
    fresh = make_env(g, R, stream=stream.cuda_stream, **CAPS, **kw)
    fresh.set_run_groups(groups, -1)
    fresh.reset(init)
    fresh.run_hooked(T, **plain)
    env.reset(init)
    env.run_hooked(T, vehicle_outcomes=True, **plain)
    a, b = day_result(env), day_result(fresh)
    assert_same_day(a, b, "a second handle, switch never set")
    assert b["counters"][:, 4].sum() == 0 and (b["status"] == 1).any()
    fresh.close()
    env.close()


# ---- 6. snapshot / restore ---------------------------------------------------------------------------------------------------------------
def test_snapshot_mid_slot_and_restore_through_a_permutation():
    g = load_golden("tiny_kmeans_dfs2")
    R, V = 3, int(g["V"])
    init = seeded_init(g, R, seed=2000)
    expect = []
    for r in range(R):
        o = make_oracle(g)
        o.reset(init[r])
        expect.append(oracle_day_rows(o, g["o_release_min"], g["o_pickup"], order_values(g), tick_minutes_of(g), V))
    env = make_env(g, R)
    env.reset(init)
    env.run(20)
    rows = got_rows(env)
    for r in range(R):
        assert_rows(rows[r], expect[r][19], "after run(20): the last slot of the run, replica %d" % r)
    env.step()                                             # slot 20, stepped: a snapshot inside the slot
    env.snapshot()
    at = got_rows(env)
    for r in range(R):
        assert_rows(at[r], expect[r][20], "slot 20 replica %d" % r)
    assert (at[..., ORDER] >= 0).any() and not np.array_equal(at[0], at[1]) and not np.array_equal(at[1], at[2])
    env.advance()
    for _ in range(4):
        env.step(); env.advance()
    perm = [2, 0, 1]
    env.restore(perm)
    got = got_rows(env)
    for r in range(R):
        assert_rows(got[r], at[perm[r]], "after restore: replica %d shows replica %d" % (r, perm[r]))
    np.testing.assert_array_equal(torch_rows(env), got)
    check_sums(env, got, "after restore")
    env.advance()
    env.step()
    got = got_rows(env)
    for r in range(R):
        assert_rows(got[r], expect[perm[r]][21], "a step after the restore, replica %d" % r)
    env.close()


# ---- 7. lifetime ---------------------------------------------------------------------------------------------------------------------------
def device_blocks():
    gc.collect()          # (a handle some earlier test dropped without closing it goes now)
    out = np.zeros(2, dtype=np.int64)
    assert _lib.load().vds_debug_device_blocks(out.ctypes.data_as(ctypes.c_void_p)) == 0
    return int(out[0]), int(out[1])


def test_address_lifetime_and_device_blocks():
    before = device_blocks()
    g = load_golden("tiny_kmeans")
    R, V = 3, int(g["V"])
    init = seeded_init(g, R)
    env = make_env(g, R)
    with pytest.raises(Exception, match="call vds_reset first"):
        env.vehicle_outcomes_device_ptr()
    env.reset(init)
    env.step()
    held = device_blocks()
    p = env.vehicle_outcomes_device_ptr()
    with_block = device_blocks()
    assert p % 16 == 0 and with_block[0] == held[0] + 1 and with_block[1] >= held[1] + 16 * R * V       # one block more
    env.advance(); env.step()
    assert env.vehicle_outcomes_device_ptr() == p and device_blocks() == with_block                  # ... made once
    env.reset(init)
    assert env.vehicle_outcomes_device_ptr() == p and (got_rows(env) == -1).all()                    # stable across resets
    env.reset_again()
    assert env.vehicle_outcomes_device_ptr() == p
    # the same sizes loaded again: the state tables stay, and the block with them
    env.load_orders(g["o_release_min"], g["o_pickup"], g["o_delivery"])
    with pytest.raises(Exception, match="call vds_reset first"):
        env.vehicle_outcomes_device_ptr()
    env.reset(init)
    assert env.vehicle_outcomes_device_ptr() == p
    # other idle tables: include/vds.h lets the address change here - whatever the call returns afterwards is the block, and it works
    env.set_idle_cap(env.idle_cap * 2)
    env.reset(init)
    p2 = env.vehicle_outcomes_device_ptr()
    blk2 = env.vehicle_outcomes_torch()
    assert p2 % 16 == 0 and blk2.data_ptr() == p2 and (got_rows(env) == -1).all()
    o = make_oracle(g)
    o.reset(init[1])
    exp = oracle_day_rows(o, g["o_release_min"], g["o_pickup"], order_values(g), tick_minutes_of(g), V)
    for t in range(3):
        env.step()
        got = got_rows(env)
        assert_rows(got[1], exp[t], "after set_idle_cap slot %d" % t)
        env.sync()
        np.testing.assert_array_equal(blk2.cpu().numpy(), got)
        env.advance()
    env.close()
    assert device_blocks() == before
    # the state tables re-made: a replica -> day map that stores the 40 replicas as 3 x 16 strides every table anew.  The block goes with
    # them and the next request makes it again: the address of THAT call is the one to use, and a tensor taken after it reads the new block
    R = 40
    days = synth_days(g, 5, seed=5200)
    init = seeded_init(g, R, seed=8100)
    env = mk_env(g, R)
    env.load_order_days(days, (np.arange(R) // 8).astype(np.int32))
    env.reset(init)
    env.step()
    env.vehicle_outcomes_device_ptr()
    with_block = device_blocks()
    env.set_replica_days((np.arange(R) % 3).astype(np.int32))
    env.reset(init)
    gone = device_blocks()
    p3 = env.vehicle_outcomes_device_ptr()
    assert p3 % 16 == 0 and device_blocks()[0] == gone[0] + 1, (with_block, gone, device_blocks())      # made again by this call
    blk3 = env.vehicle_outcomes_torch()
    assert blk3.data_ptr() == p3
    o = mk_oracle(g, days[1])
    o.reset(init[1])
    day = days[1]
    value = g["cost"][day[2].astype(np.int64), day[1].astype(np.int64)].astype(np.int64)
    exp = oracle_day_rows(o, day[0], day[1], value, tick_minutes_of(g), V)
    for t in range(4):
        env.step()
        got = got_rows(env)
        assert_rows(got[1], exp[t], "after set_replica_days slot %d" % t)
        assert env.vehicle_outcomes_device_ptr() == p3
        env.sync()
        np.testing.assert_array_equal(blk3.cpu().numpy(), got, err_msg="the tensor taken after the tables were re-made reads the new block")
        env.advance()
    env.close()
    assert device_blocks() == before


# ---- 8. written in full, whatever the memory held ------------------------------------------------------------------------------------
# seconds of the selection under the product library on an MI355X, pytest start-up included; the limit follows as in
# tests/test_gpu_dirty_memory.py: ten times that + 120 s, a safety stop
SELECTION = "test_rows_equal_reference_at_every_slot or test_per_replica_order_days_and_regrouped_storage"
SELECTION_SECONDS = 10


@pytest.mark.parametrize("target,lib,fill", [("dirty", "libvds_dirty.so", None), ("dirty", "libvds_dirty.so", "5A"), ("canary", "libvds_canary.so", None)],
                         ids=["dirty-A5", "dirty-5A", "canary"])
def test_every_element_is_written_on_dirty_and_guarded_memory(target, lib, fill):
    """The tiny day walks and the per-replica-days walk of this file in one pytest subprocess under the dirty library (every byte the
    library obtains is filled with A5 / 5A before first use: a row the fill missed reads as the pattern, not as -1) and under the
    guarded one (a store outside the block damages a guard, found when the handle closes)."""
    from test_gpu_debug_builds import build
    from test_gpu_dirty_memory import dirty_env, gpu_allowed, run_limited
    gpu_allowed()
    path = build(target, lib)
    argv = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k", SELECTION]
    rc, out = run_limited(argv, dirty_env(fill, path), 10 * SELECTION_SECONDS + 120, "the walks under %s (fill %s)" % (lib, fill or "A5"))
    print(out[-800:])
    assert rc == 0 and "%d passed" % (len(TINY) + 1) in out, out[-6000:]
