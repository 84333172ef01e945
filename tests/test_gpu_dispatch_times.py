"""The device dispatch forms with a per-entry arrival minute and counted flag (vds_apply_dispatch_vehicles_device_ex /
vds_apply_dispatch_roster_device_ex, vds_run_hooked_vehicles_ex / vds_run_hooked_roster_ex: k_dispatch_vehicles_timed /
k_dispatch_roster_timed; ``env.apply_dispatch_vehicles_timed_torch``, ``env.apply_dispatch_roster_timed_torch``,
``env.run_hooked(vehicle_arrive_min=, vehicle_counted=, roster_arrive_min=, roster_counted=)``).  The oracle step of a call is
tests/dispatch_times_expect.oracle_apply_timed: one ``dispatch_at`` per mover in the form's order.  Integers: bit-exact.
tests/test_dispatch_times_expect.py asserts on the CPU what this file leans on (which of the seven delayed reference-run days
reproduce the record in which order, that the booked minutes matter, how far ahead they lie)."""
import functools
import os
import sys

import numpy as np
import pytest

from dispatch_times_expect import AHEAD_MAX, ARRIVE_ROAD, DELAYED_DAYS, POISON, oracle_apply_timed, roster_order, slot_tensors, vehicle_order
from helpers import dispatch_by_tick, engine_settings, live_window, load_golden
from test_gpu_dispatch_vehicles import (CAPS, assert_reads_equal, assert_same_day, check_all, day_result, late_orders, make_oracles, read_everything,
                                        seeded_init, to_dev, torch_stream_kw)
from test_gpu_parity import MODES, make_env
from test_gpu_replica_days import mk_env, synth_days

pytestmark = pytest.mark.gpu

R3 = 3
INT32_MIN = -2 ** 31
FORMS = ("roster", "vehicle")
OBS = (("idle_pre", "idle_pre"), ("idle_now", "idle_post"), ("supply", "supply"), ("cl_orders", "cl_orders"), ("inflight", "inflight"))
COUNTERS = ("order_num", "reject_num", "matched", "wait_sum", "dispatch_num", "dispatch_cost")


def form_order(o, form):
    return vehicle_order(o) if form == "vehicle" else roster_order(o)


def apply_timed(env, form, tg, am, ct):
    """One call of the form: the roster is refreshed first (the tensors were written against the lists as they stand)."""
    dev = [None if x is None else to_dev(x) for x in (tg, am, ct)]
    if form == "roster":
        env.idle_roster_torch()
        env.apply_dispatch_roster_timed_torch(*dev)
    else:
        env.apply_dispatch_vehicles_timed_torch(*dev)


def check_obs(env, oracles, t, tag):
    """The five observation planes and the counters of every replica against its oracle."""
    ob, cn = env.obs(), env.counters()
    for r, o in enumerate(oracles):
        oo, oc = o.obs(), o.counters()
        for a, b in OBS:
            np.testing.assert_array_equal(ob[a][r], oo[b], err_msg="%s slot %d replica %d obs %s" % (tag, t, r, a))
        for i, k in enumerate(COUNTERS):
            assert cn[r, i] == oc[k], (tag, t, r, k, cn[r, i], oc[k])
    return ob, cn


def begin(env, oracles):
    env.step()
    for o in oracles:
        o.begin_tick()


def end(env, oracles):
    env.advance()
    for o in oracles:
        o.end_tick()


# ---- 1. the seven reference-run days with a booked delay --------------------------------------------------------------------------------
DAY_MODES = {"default": {}, "generic": {"force_generic": True}, "far": {"ring_ticks": 2}, "dense16": MODES["dense16"]}
# In ascending vehicle order this day leaves the reference's record (t_idle_post / t_supply at slot 121, the waits and the counts behind
# a dispatch earlier: tests/test_dispatch_times_expect.py): its vehicle form is held against the oracle only - no slot against the record
OFF_RECORD = {("tiny_dispatch_delay", "vehicle"): 0}


def searching(g):
    return bool(g["neighbor_can_server"]) and int(g["depth_limit"]) > 0


def day_cases():
    out = []
    for name in DELAYED_DAYS:
        g = load_golden(name)
        modes = ["default", "generic", "far"] + ([] if live_window(g) or searching(g) else ["dense16"])      # (dense16: where the library runs the dense tick)
        out += [(name, m) for m in modes]
    return out


@functools.lru_cache(maxsize=None)
def delayed_day(name, mode, form):
    """The whole day, R = 3 from the recorded start nodes; returns what the coverage test asks about."""
    g = load_golden(name)
    R, V, T = R3, int(g["V"]), int(g["n_ticks"])
    extra = int(g["dispatch_extra_minutes"])
    init = np.tile(g["veh_node"], (R, 1)).astype(np.int32)
    env = make_env(g, R, **{**DAY_MODES[mode], **torch_stream_kw()})
    env.reset(init)
    oracles = make_oracles(g, init)
    assert env.T == T
    disp = dispatch_by_tick(g)
    off_record = OFF_RECORD.get((name, form), T + 1)
    tag = "%s %s %s" % (name, mode, form)
    held, calls = set(), 0
    for t in range(T):
        begin(env, oracles)
        ob, cn = check_obs(env, oracles, t, tag)
        if t < off_record:          # replica 0 against the reference's own record
            np.testing.assert_array_equal(ob["supply"][0], g["t_supply"][t], err_msg=tag)
            np.testing.assert_array_equal(ob["idle_now"][0], g["t_idle_post"][t], err_msg=tag)
            assert cn[0, 0] == g["t_order_num"][t] and cn[0, 1] == g["t_reject_num"][t] and cn[0, 3] == g["t_wait_sum"][t], (tag, t)
        if t in disp:
            tg, am = np.empty((R, V), np.int32), np.empty((R, V), np.int32)
            orders = [form_order(o, form) for o in oracles]
            for r, o in enumerate(oracles):
                tg[r], am[r] = slot_tensors(disp[t], orders[r], V, int(o.now_min), extra, fill=POISON)
            apply_timed(env, form, tg, am, None)
            for r, o in enumerate(oracles):
                got = oracle_apply_timed(o, orders[r], tg[r], am[r], None, g["node2cluster"])
                assert not any(got["refused"].values()) and (got["moves"] == len(disp[t]) or t >= off_record), (tag, t)
            held |= check_all(env, oracles, t, tag)          # container order, arrive_min of every vehicle, the two counters
            calls += 1
            if t < off_record:
                np.testing.assert_array_equal(env.obs()["idle_now"][0], g["t_idle_after_dispatch"][t], err_msg=tag)
        end(env, oracles)
    env.sync()
    od, cn = env.orders(), env.counters()
    for r, o in enumerate(oracles):
        oo, oc = o.orders(), o.counters()
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(od[k][r], oo[k], err_msg="%s replica %d %s" % (tag, r, k))
        assert cn[r, 6] == oc["sum_order_value"]
    if off_record > T:
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(od[k][0], g["o_" + k], err_msg=tag + " record " + k)
        assert cn[0, 4] == int(g["dispatch_num"]) and cn[0, 5] == int(g["dispatch_cost"]) and cn[0, 1] == int(g["reject_num"])
    dense = env.layout()["dense"]
    env.close()
    assert calls == len(disp)
    return dict(dense=dense, held=held)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,mode", day_cases())
def test_delayed_day(name, mode, form):
    facts = delayed_day(name, mode, form)
    if mode == "far":          # every one of these days books arrivals beyond a two-slot ring: posted to the far inbox (4)
        assert 4 in facts["held"], facts
    if mode == "dense16":
        assert facts["dense"] == 1, facts


# ---- 2. every kind of entry in one call --------------------------------------------------------------------------------------------------
KINDS_CITY = "fuzz_019"          # 74 vehicles in 4 clusters, 3-minute slots, neither pickup window nor neighbour search: both layouts
KIND_NAMES = ("road", "now", "past", "min_plus_1", "next_slot", "beyond_ring", "beyond_day", "max_ahead", "too_far")
COUNTED_FLAGS = (0, 1, 0, 7)


@functools.lru_cache(maxsize=None)
def kinds_case(mode, form):
    g = load_golden(KINDS_CITY)
    V, n2c = int(g["V"]), g["node2cluster"]
    tick = engine_settings(g)["tick_minutes"]
    init = seeded_init(g, R3)
    env = make_env(g, R3, **{**MODES[mode], **CAPS, **torch_stream_kw()})
    env.reset(init)
    oracles = make_oracles(g, init)
    tag = "kinds %s %s" % (mode, form)
    day_end = int(oracles[0].now_min) + env.T * tick
    for t in range(3):
        begin(env, oracles)
        if t < 2:
            end(env, oracles)
    t = 2
    rng = np.random.default_rng(9)
    valid = np.flatnonzero(n2c >= 0)
    tg = np.full((R3, V), -1, dtype=np.int32)
    am = np.full((R3, V), POISON, dtype=np.int32)          # INT32_MAX wherever no mover reads: not idle, a negative target, beyond off[r][C]
    ct = np.full((R3, V), POISON, dtype=np.int32)
    orders, kinds_used, mixed = [], set(), False
    for r, o in enumerate(oracles):
        now = int(o.now_min)
        kinds = (ARRIVE_ROAD, now, now - 5, INT32_MIN + 1, now + tick, now + tick * 40, day_end + 500, now + AHEAD_MAX, now + AHEAD_MAX + 1)
        order = form_order(o, form)
        orders.append(order)
        cl = o.vehicles()["cluster"]
        flags = {}
        m = 0
        for k, (v, j) in enumerate(order):
            if k % 4 == 3:          # stays
                continue
            tg[r, j], am[r, j], ct[r, j] = valid[rng.integers(0, valid.size)], kinds[m % 9], COUNTED_FLAGS[m % 4]
            kinds_used.add(KIND_NAMES[m % 9])
            if m % 9 != 8:
                flags.setdefault(int(cl[v]), set()).add(COUNTED_FLAGS[m % 4] != 0)
            m += 1
        mixed = mixed or any(len(s) == 2 for s in flags.values())
    assert kinds_used == set(KIND_NAMES)
    apply_timed(env, form, tg, am, ct)
    refused = moves = counted = 0
    for r, o in enumerate(oracles):
        got = oracle_apply_timed(o, orders[r], tg[r], am[r], ct[r], n2c)
        assert set(k for k, n in got["refused"].items() if n) == {"too_far"}
        refused += got["refused"]["too_far"]; moves += got["moves"]; counted += got["counted"]
    with pytest.raises(Exception, match="dispatch"):
        env.sync()
    env.sync()                                              # reported once; the refused vehicles are still idle, the rest is applied
    held = check_all(env, oracles, t, tag)
    assert 0 < counted < moves and refused >= R3
    # the past, the present and the next slot are back at the next Update, in dict order; the trip beyond the ring comes out of the far list
    for t in range(3, 45):
        end(env, oracles)
        begin(env, oracles)
        if t in (3, 4, 41, 42, 43, 44):
            held |= check_all(env, oracles, t, tag)
            check_obs(env, oracles, t, tag)
    dense = env.layout()["dense"]
    env.advance()
    env.sync()
    env.close()
    return dict(dense=dense, held=held, refused=refused, mixed=mixed)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", ["fast", "rows"])
def test_every_kind_of_entry_in_one_call(mode, form):
    facts = kinds_case(mode, form)
    assert facts["dense"] == (1 if mode == "fast" else 0), facts
    assert {2, 3, 4} <= facts["held"] and facts["mixed"] and facts["refused"] > 0, facts


# ---- 3. chunk boundaries and the replica tail -----------------------------------------------------------------------------------------
CHUNK_V, CHUNK_R = 151, 5          # three 64-entry chunks; four wavefronts per workgroup and a tail of one
CHUNK_MOVERS = (0, 5, 63, 64, 70, 127, 128, 140, 150)
CHUNK_SECOND = (1, 62, 63, 64, 126, 127)          # positions in the list as the first two calls left it


@functools.lru_cache(maxsize=None)
def chunk_case(mode, form):
    g0 = late_orders(load_golden("tiny_kmeans"))
    n2c, C = g0["node2cluster"], int(g0["C"])
    sizes = np.bincount(n2c[n2c >= 0], minlength=C)
    first_picks = set(n2c[g0["o_pickup"][g0["o_release_min"] < g0["o_release_min"].min() + 10]].tolist())      # (slot 0 takes no vehicle of the long list)
    big = int(max((c for c in range(C) if c not in first_picks), key=lambda c: sizes[c]))
    nodes_big, other = np.flatnonzero(n2c == big), np.flatnonzero((n2c != big) & (n2c >= 0))
    init = np.stack([nodes_big[(np.arange(CHUNK_V) * (r + 1) + r) % nodes_big.size] for r in range(CHUNK_R)]).astype(np.int32)
    g = dict(g0, V=CHUNK_V, veh_node=init[0])
    env = make_env(g, CHUNK_R, **{**MODES[mode], **CAPS, **torch_stream_kw()})
    env.reset(init)
    oracles = make_oracles(g, init)
    begin(env, oracles)
    tag = "chunks %s %s" % (mode, form)
    rng = np.random.default_rng(13)
    chunks = set()

    def call(positions, salt):
        tg = np.full((CHUNK_R, CHUNK_V), -1, dtype=np.int32)
        am = np.full((CHUNK_R, CHUNK_V), POISON, dtype=np.int32)
        ct = np.full((CHUNK_R, CHUNK_V), POISON, dtype=np.int32)
        orders = [form_order(o, form) for o in oracles]
        for r, o in enumerate(oracles):
            L = o.lists()
            lo, n = int(L["idle_off"][big]), int(L["idle_off"][big + 1] - L["idle_off"][big])
            assert n > max(positions)
            index = dict(orders[r])
            for k, p in enumerate(positions):
                j = index[int(L["idle_veh"][lo + p])]
                tg[r, j] = other[rng.integers(0, other.size)]
                am[r, j] = (ARRIVE_ROAD, int(o.now_min) + 7 * k + r + salt, int(o.now_min) - k)[(k + r) % 3]
                ct[r, j] = (k + r + salt) % 2
                chunks.add(p // 64)
        apply_timed(env, form, tg, am, ct)
        for r, o in enumerate(oracles):
            got = oracle_apply_timed(o, orders[r], tg[r], am[r], ct[r], n2c)
            assert got["moves"] == len(positions) and 0 < got["counted"] < got["moves"]
        check_all(env, oracles, 0, tag)

    for r, o in enumerate(oracles):
        L = o.lists()
        assert L["idle_off"][big + 1] - L["idle_off"][big] == CHUNK_V
    call(CHUNK_MOVERS, 0)
    # a K-form call, then the form again in the same slot: its sequence numbers come behind both
    acts = np.full((CHUNK_R, 2, 3), -1, dtype=np.int32)
    for r, o in enumerate(oracles):
        L = o.lists()
        seg = L["idle_veh"][L["idle_off"][big]:L["idle_off"][big + 1]]
        acts[r, 0] = (big, 2, other[1]); acts[r, 1] = (big, 0, other[1])
        o.dispatch(seg[[2, 0]], np.full(2, other[1]))
    env.apply_dispatch_torch(to_dev(acts))
    check_all(env, oracles, 0, tag + " + K-form")
    call(CHUNK_SECOND, 3)
    for t in range(1, 4):          # ... and they come back in that order
        end(env, oracles)
        begin(env, oracles)
        check_all(env, oracles, t, tag)
    env.advance()
    env.sync()
    env.close()
    return dict(chunks=chunks)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", ["fast", "rows"])
def test_chunk_boundaries_and_the_replica_tail(mode, form):
    assert chunk_case(mode, form)["chunks"] == {0, 1, 2}


# ---- 4. the hooked day ------------------------------------------------------------------------------------------------------------------
HG_R = 40


def hooked_day(form, R, groups=0, V=None, **kw):
    """One launch, a replay, the tensors switched off and on again, a rebuild behind load_orders - each against the stepwise walk."""
    import torch
    g = load_golden("tiny_dispatch")
    if V is not None:
        g = dict(g, V=V, veh_node=g["veh_node"][:V])
    V, C = int(g["V"]), int(g["C"])
    tick = engine_settings(g)["tick_minutes"]
    n2c = g["node2cluster"]
    node_of = np.array([np.flatnonzero(n2c == c)[0] for c in range(C)], dtype=np.int32)
    init = seeded_init(g, R)
    stream = torch.cuda.current_stream()
    env = make_env(g, R, stream=stream.cuda_stream, **{**CAPS, **kw})
    if groups:
        env.set_run_groups(groups, -1)
    T = env.T
    env.reset(init)
    now0 = int(make_oracles(g, init[:1])[0].now_min)
    if form == "vehicle":
        pl = env.vehicles_torch(state=True, node=False, cluster=True, arrive_min=False, order=False)
        state, cluster = pl["state"], pl["cluster"]
        veh = torch.arange(V, device="cuda", dtype=torch.int64)[None, :].expand(R, V)
    else:
        ros = env.idle_roster_torch()
        veh, cluster = ros["veh"], ros["cluster"]
    targets = torch.full((R, V), -1, dtype=torch.int32, device="cuda")
    arrive = torch.full((R, V), POISON, dtype=torch.int32, device="cuda")
    counted = torch.full((R, V), POISON, dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int64, device="cuda")
    node_t = torch.from_numpy(node_of.astype(np.int64)).cuda()
    poison = torch.full((R, V), POISON, dtype=torch.int64, device="cuda")

    def policy():
        v = veh.to(torch.int64)
        idle = (state == 0) if form == "vehicle" else (v >= 0)
        cl = cluster.to(torch.int64).clamp(min=0)
        go = idle & (v % 7 == slot % 7)
        now = now0 + slot * tick
        # by vehicle number: the road (the sentinel), 25 / 35 / 45 minutes from now, three minutes ago; every second one not counted
        a = torch.where(v % 5 == 0, torch.full_like(v, ARRIVE_ROAD), torch.where(v % 5 == 4, now - 3, now + 15 + (v % 5) * 10))
        targets.copy_(torch.where(go, node_t[(cl + 1) % C], torch.full_like(v, -1)).to(torch.int32))
        arrive.copy_(torch.where(go, a, poison).to(torch.int32))
        counted.copy_(torch.where(go, v % 2, poison).to(torch.int32))
        slot.add_(1)

    graph = None
    if V > 0:
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
    obs_off = dict(idle_pre=False, idle_now=False, supply=False, cl_orders=False)
    if form == "vehicle":
        plain_kw = dict(vehicle_planes=dict(state=True, cluster=True), vehicle_targets=targets)
        timed_kw = dict(plain_kw, vehicle_arrive_min=arrive, vehicle_counted=counted)
    else:
        plain_kw = dict(roster=True, roster_targets=targets)
        timed_kw = dict(plain_kw, roster_arrive_min=arrive, roster_counted=counted)

    def hooked(kw):
        env.reset(init); slot.zero_()
        env.run_hooked(T, policy_graph=graph, **kw, **obs_off)
        res = day_result(env)
        assert graph is None or int(slot.item()) == T
        return res

    def stepwise(timed):
        env.reset(init); slot.zero_()
        for t in range(T):
            env.step()
            if form == "vehicle":
                env.vehicles_torch(state=True, node=False, cluster=True, arrive_min=False, order=False)
            else:
                env.idle_roster_torch()
            if graph is not None:
                graph.replay()
            if form == "vehicle":
                env.apply_dispatch_vehicles_timed_torch(targets, arrive, counted) if timed else env.apply_dispatch_vehicles_torch(targets)
            else:
                env.apply_dispatch_roster_timed_torch(targets, arrive, counted) if timed else env.apply_dispatch_roster_torch(targets)
            env.advance()
        return day_result(env)

    tag = "%s R %d groups %d %s" % (form, R, groups, kw)
    want_timed, want_plain = stepwise(True), stepwise(False)
    if V > 0:          # (the minutes and the flags decide the day: the two walks differ)
        assert not np.array_equal(want_timed["counters"], want_plain["counters"])
        assert 0 < want_timed["counters"][:, 4].sum() < want_plain["counters"][:, 4].sum()
    assert_same_day(hooked(timed_kw), want_timed, tag + ": one launch")
    assert_same_day(hooked(timed_kw), want_timed, tag + ": a replay")
    assert_same_day(hooked(plain_kw), want_plain, tag + ": switched off")
    assert_same_day(hooked(timed_kw), want_timed, tag + ": switched on again")
    block = (lambda: env.vehicles_device_ptr(5)) if form == "vehicle" else env.idle_roster_device_ptr
    before = block()
    env.load_orders(g["o_release_min"], g["o_pickup"], g["o_delivery"])      # the same sizes: the state tables stay, the graph is rebuilt
    env.reset(init)
    assert block() == before          # (the captured policy reads this block)
    assert_same_day(hooked(timed_kw), want_timed, tag + ": behind load_orders")
    env.close()


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("form", FORMS)
def test_hooked_day(form, groups):
    hooked_day(form, HG_R, groups)


@pytest.mark.parametrize("form", FORMS)
def test_hooked_day_on_the_eager_path(form):
    hooked_day(form, HG_R, force_generic=1)


@pytest.mark.parametrize("form", FORMS)
def test_hooked_day_without_vehicles(form):
    hooked_day(form, 4, V=0)


def test_hooked_setters_refuse_times_without_targets():
    import torch
    g = load_golden("tiny_dispatch")
    env = make_env(g, R3, **{**CAPS, **torch_stream_kw()})
    env.reset(seeded_init(g, R3))
    t = torch.zeros((R3, int(g["V"])), dtype=torch.int32, device="cuda")
    ptr = env._vehicle_targets_ptr(t, "test")
    assert env._lib.vds_run_hooked_vehicles_ex(env._h, 0, None, ptr, None) == -1
    assert env._lib.vds_run_hooked_vehicles_ex(env._h, 0, None, None, ptr) == -1
    assert env._lib.vds_run_hooked_roster_ex(env._h, 1, None, ptr, None) == -1
    assert env._lib.vds_run_hooked_roster_ex(env._h, 1, None, None, ptr) == -1
    assert env._lib.vds_apply_dispatch_vehicles_device_ex(env._h, ptr, ptr, ptr) == -1          # before step()
    assert "vds_step" in env._lib.vds_last_error(env._h).decode()
    env.step()
    assert env._lib.vds_apply_dispatch_vehicles_device_ex(env._h, None, ptr, ptr) == -1
    assert env._lib.vds_apply_dispatch_roster_device_ex(env._h, ptr, ptr, ptr) == -4           # VDS_ESTATE: the roster is stale
    env.advance()
    env.sync()
    env.close()


# ---- 5. order days per replica ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_order_days_per_replica(form):
    g = load_golden("tiny_kmeans")
    V, R = int(g["V"]), 5
    n2c = g["node2cluster"]
    days = synth_days(g, 3, seed=321)[1:]          # a whole day and one that ends after five hours; their clocks start apart
    replica_day = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    init = seeded_init(g, R)
    env = mk_env(g, R, **{**CAPS, **torch_stream_kw()})
    env.load_order_days(days, replica_day)
    env.reset(init)
    oracles = make_oracles(g, init, [days[d] for d in replica_day])
    Ts = [o.num_ticks for o in oracles]
    assert min(Ts) < max(Ts) and len({int(o.now_min) for o in oracles}) == 2
    rng = np.random.default_rng(78)
    valid = np.flatnonzero(n2c >= 0)
    t_bad = min(Ts) + 1
    for t in range(min(Ts) + 3):
        env.step()
        live = [r for r in range(R) if t < Ts[r]]
        for r in live:
            oracles[r].begin_tick()
        dispatching = t % 5 == 0 or t >= min(Ts) - 2
        if dispatching:
            tg = np.full((R, V), -1, dtype=np.int32)
            am = np.full((R, V), POISON, dtype=np.int32)
            ct = np.full((R, V), POISON, dtype=np.int32)
            orders = [form_order(o, form) for o in oracles]
            for r, o in enumerate(oracles):
                if r not in live and t != t_bad:
                    continue
                for k, (v, j) in enumerate(orders[r][:(9 if r in live else 1)]):
                    # (the minute is on the replica's OWN clock: 20 minutes and more ahead of its now, or two minutes ago)
                    tg[r, j], am[r, j], ct[r, j] = valid[rng.integers(0, valid.size)], int(o.now_min) + (20 + 11 * k if k % 3 else -2), (k + r) % 2
            apply_timed(env, form, tg, am, ct)
            for r, o in enumerate(oracles):
                got = oracle_apply_timed(o, orders[r], tg[r], am[r], ct[r], n2c, over=r not in live)
                assert got["moves"] == (9 if r in live else 0) and got["refused"]["day_over"] == (1 if r not in live and t == t_bad else 0)
            if t == t_bad:          # a replica whose day is over refuses as before
                with pytest.raises(Exception, match="dispatch"):
                    env.sync()
                env.sync()
            check_all(env, oracles, t, "days " + form, replicas=live)
        env.advance()
        for r in live:
            oracles[r].end_tick()
    env.close()


# ---- 6. snapshot ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "rows"])
def test_snapshot_behind_a_timed_dispatch_and_restore_through_a_permutation(mode):
    g = load_golden("tiny_kmeans")
    V, n2c = int(g["V"]), g["node2cluster"]
    tick = engine_settings(g)["tick_minutes"]
    init = seeded_init(g, R3)
    perm = np.array([1, 2, 0], dtype=np.int32)
    env = make_env(g, R3, **{**MODES[mode], **CAPS, **torch_stream_kw()})
    env.reset(init)
    valid = np.flatnonzero(n2c >= 0)

    def tensors(oracles, seed):
        rng = np.random.default_rng(seed)
        tg = np.full((R3, V), -1, dtype=np.int32)
        am = np.full((R3, V), POISON, dtype=np.int32)
        ct = np.full((R3, V), POISON, dtype=np.int32)
        for r, o in enumerate(oracles):
            now = int(o.now_min)
            for k, (v, j) in enumerate(vehicle_order(o)[::3]):
                tg[r, j], ct[r, j] = valid[rng.integers(0, valid.size)], k % 2
                am[r, j] = (ARRIVE_ROAD, now + 13 + k, now - 1, now + tick * 40 + k)[k % 4]          # (the last: beyond the ring)
        return tg, am, ct

    def to_the_snapshot(oracles, drive_env):
        for t in range(3):
            if drive_env:
                env.step()
            for o in oracles:
                o.begin_tick()
            if t < 2:
                if drive_env:
                    env.advance()
                for o in oracles:
                    o.end_tick()
        tg, am, ct = tensors(oracles, 4)
        if drive_env:
            apply_timed(env, "vehicle", tg, am, ct)
        for r, o in enumerate(oracles):
            oracle_apply_timed(o, vehicle_order(o), tg[r], am[r], ct[r], n2c)

    def go_on(oracles, env_rows):
        """Three more slots with a timed call each; ``env_rows[r]``: the oracle replica r follows."""
        mine = [oracles[p] for p in env_rows]
        for t in range(3, 6):
            end(env, oracles)
            begin(env, oracles)
            tg, am, ct = tensors(mine, 10 + t)
            apply_timed(env, "vehicle", tg, am, ct)
            for r, o in enumerate(oracles):
                src = list(env_rows).index(r)          # (every oracle is followed by exactly one replica)
                oracle_apply_timed(o, vehicle_order(o), tg[src], am[src], ct[src], n2c)
            check_all(env, mine, t, "snapshot %s rows %s" % (mode, list(env_rows)))

    first = make_oracles(g, init)
    to_the_snapshot(first, True)
    env.snapshot()
    at_snapshot = read_everything(env)
    check_all(env, first, 2, "snapshot: taken")
    go_on(first, range(R3))
    env.restore()
    assert_reads_equal(read_everything(env), at_snapshot, "after restore")
    env.restore(perm)
    second = make_oracles(g, init)
    to_the_snapshot(second, False)
    check_all(env, [second[p] for p in perm], 2, "snapshot: restored through a permutation")
    go_on(second, perm)
    env.advance()
    env.sync()
    env.close()


# ---- 7. instrumented builds -------------------------------------------------------------------------------------------------------------
# the two shortest day walks of 1 (both forms, default mode) and the walks of 2: seconds under the product library on an MI355X, pytest
# start-up included; the limit follows as in tests/test_gpu_dirty_memory.py: ten times that + 120 s, a safety stop
SELECTION = "(test_delayed_day and default and (fuzz_033 or fuzz_020)) or test_every_kind_of_entry_in_one_call"
SELECTION_TESTS = 2 * 2 + 4
SELECTION_SECONDS = 20


@pytest.mark.parametrize("target,lib,fill", [("dirty", "libvds_dirty.so", None), ("canary", "libvds_canary.so", None)], ids=["dirty", "canary"])
def test_walks_on_dirty_and_guarded_memory(target, lib, fill):
    """The selection in one pytest subprocess under the dirty library (every byte the library obtains is filled with a pattern before
    first use) and under the guarded one (a store outside a table damages a guard, found when the handle closes).  One at a time."""
    from test_gpu_debug_builds import build
    from test_gpu_dirty_memory import dirty_env, gpu_allowed, run_limited
    gpu_allowed()
    path = build(target, lib)
    argv = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k", SELECTION]
    rc, out = run_limited(argv, dirty_env(fill, path), 10 * SELECTION_SECONDS + 120, "the timed dispatch walks under %s" % lib)
    print(out[-800:])
    assert rc == 0 and "%d passed" % SELECTION_TESTS in out, out[-6000:]


# ---- 8. coverage ------------------------------------------------------------------------------------------------------------------------
def test_the_cases_met_what_they_were_chosen_for():
    """(the cases are cached: behind the tests above this one runs nothing again)"""
    assert 4 in delayed_day("fuzz_033", "far", "roster")["held"] and 4 in delayed_day("fuzz_033", "far", "vehicle")["held"]
    kd, kw = kinds_case("fast", "vehicle"), kinds_case("rows", "roster")
    assert kd["dense"] == 1 and 4 in kd["held"] and kw["dense"] == 0 and 4 in kw["held"]      # a far-inbox post on both layouts
    assert 2 in kd["held"]          # a dispatched vehicle's minute read back from the dense ring (ring_min): check_all compared it
    assert kd["mixed"] and kw["mixed"]                   # an uncounted and a counted move in one bucket
    assert kd["refused"] > 0 and kw["refused"] > 0       # a refused minute
    assert chunk_case("fast", "vehicle")["chunks"] == {0, 1, 2} and chunk_case("rows", "roster")["chunks"] == {0, 1, 2}      # movers in a second and a third chunk
