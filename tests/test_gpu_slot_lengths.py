"""The slot length (``TimePeriods`` in the reference, ``tick_minutes`` here) and the length of a day, on the GPU, over the slot-length
corpus (tests/golden/make_slot_golden.py): days the unmodified reference ran with slots of 1, 2, 30, 60, 63, 64, 120 and 1440 minutes,
and two days of more than 32767 slots.  What depends on the slot length and had only run at 3 .. 15 minutes and below slot 500:

  * the division by the slot length (``ticks_until`` / ``ticks_until_fast``): multiply-high for 2 .. 63 minutes, a true division at 1 and
    from 64 on, in k_tick_dense and k_tick_rows as in the generic kernels;
  * the arrival path: with 1- and 2-minute slots most trips outlive the 32-slot ring (far list, inbox, migration) and the library picks
    the dense tick's ring form by itself; from 60 minutes on every trip is due in the next slot or two and a slot holds hundreds of orders;
  * every derived plane that turns a slot into a minute or back (k_pack_obs, the vehicle planes, the vehicle and slot outcomes);
  * the slot number packed into the upper 16 bits of a meta word, negative as an int from slot 32768 on.

1. every day per slot as test_gpu_parity.run_day (three replicas against the oracle, replica 0 against the reference's record), default
   and generic kernels in this process, the modes the day's data select (test_gpu_fuzz_golden.worker_modes) in worker processes;
2. the premise: the day meant for it runs k_tick_dense at every slot length, in its ring form at 1 and 2 minutes;
3. the per-slot device planes (observations, outcomes, idle heads, vehicle planes, vehicle outcomes, idle roster) on the dense and the
   searching day of every slot length, with the checkers of the plane tests; the hooked day against the stepwise loop;
4. the whole day as one ``run(T)``, as a graph and eagerly;
5. the long days in chunks of 1024 slots, then dispatch in all four forms from slot 32768 on and a snapshot taken before it;
6. the ``Simulation`` shell with ``TimePeriods`` of 1 and 60 minutes on a reference-style data directory.
Every expectation is an integer from the CPU oracle or the reference's record; nothing has a tolerance."""
import json
import os
import random
import sys

import numpy as np
import pytest

from helpers import SIGN_SLOT, SLOT_LENGTHS, dense_by_own_rules, live_window, load_slot, make_oracle, oracle_apply, slot_day_facts, slot_names
from test_gpu_dispatch_vehicles import check_all, random_targets, to_dev
from test_gpu_fuzz_golden import DENSE_MODES, IN_PROCESS_MODES, NPROC, SEARCH_MODES, WINDOW_MODES, worker_modes
from test_gpu_idle_heads import check_heads
from test_gpu_idle_roster import check_roster, roster_call, roster_targets
from test_gpu_parity import MODES, check_lists, make_env, run_day
from test_gpu_plane_fuzz import PlaneChecker, check_end_of_day, dispatch_tensor, pick_dispatches
from test_gpu_vehicle_fuzz import check_planes, new_seen
from test_gpu_vehicle_outcomes import assert_rows, check_sums, got_rows
from vehicle_outcome_expect import processed_rows
from vehicles_dispatch_simulator_amd import synth

pytestmark = pytest.mark.gpu

SLOT = slot_names(long_days=False)
LONG = slot_names(long_days=True)
DENSE_DAY = {k: "slot_%04d_0" % k for k in SLOT_LENGTHS}          # (make_slot_golden.case_specs: a day's role is its last digit)


def searching_day(minutes):
    """Of a slot length's days with neighbour search at depth >= 1, the one that served most orders from another cluster."""
    days = [(slot_day_facts(g)["cross"], n) for n in SLOT for g in [load_slot(n)]
            if int(g["tick_minutes"]) == minutes and bool(g["neighbor_can_server"]) and int(g["depth_limit"]) >= 1]
    return max(days)[1]


SEARCH_DAY = {k: searching_day(k) for k in SLOT_LENGTHS}
CHUNK = 1024
R3 = 3


def thin(g):
    """Containers at every slot of a short day, at every 16th (and around every dispatch) of a day of hundreds of slots."""
    return 1 if int(g["n_ticks"]) <= 200 else 16


def seeded_init(g, R):
    """Replica 0 on the fixture's start nodes, the others seeded as test_gpu_parity.run_day seeds them."""
    V, N = int(g["V"]), int(g["N"])
    init = np.empty((R, V), dtype=np.int32)
    init[0] = g["veh_node"]
    for r in range(1, R):
        init[r] = synth.init_vehicle_nodes(random.Random(1000 + r), N, V, g["node2cluster"] >= 0)
    return init


def oracles_of(g, init):
    out = []
    for row in init:
        o = make_oracle(g)
        o.reset(row)
        out.append(o)
    return out


# ---- 1. every day per slot ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", IN_PROCESS_MODES)
@pytest.mark.parametrize("name", SLOT)
def test_slot_length_day_per_slot(name, mode):
    g = load_slot(name)
    run_day(g, R=R3, same_init=bool(len(g["dispatch_log"])), list_every=thin(g), **MODES[mode])


def worker_pairs():
    return [(n, m, "tick" if thin(g) == 1 else "thin%d" % thin(g)) for n in SLOT for g in [load_slot(n)] for m in worker_modes(g)]


def test_slot_length_modes_in_worker_processes():
    """Every (day, mode) pair of test_gpu_fuzz_golden.worker_modes - the neighbour-search kernels where a search can leave the pickup's
    cluster, the dense-tick variants and the row-mapped kernel where the library runs the dense tick, the wide-layout paths under a live
    window, the far tables everywhere - as a per-slot day, dealt to four worker processes (tests/parity_worker.py)."""
    import conftest
    pairs = worker_pairs()
    assert {m for _, m, _ in pairs} == set(SEARCH_MODES + DENSE_MODES + WINDOW_MODES) - set(IN_PROCESS_MODES)
    for k in SLOT_LENGTHS:          # every family at every slot length
        at = {m for n, m, _ in pairs if int(load_slot(n)["tick_minutes"]) == k}
        assert at >= set(("dense_ring", "rows", "dfs_v2", "dfs_wide", "far", "ring64")), (k, at)
    pairs.sort(key=lambda p: -int(load_slot(p[0])["n_ticks"]))          # (the long items first, dealt round robin)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "parity_worker.py")
    conftest.start_workers("slot_length_modes", [[sys.executable, worker, json.dumps(pairs[i::NPROC])] for i in range(NPROC)])
    done = 0
    for i, (rc, out) in enumerate(conftest.collect_workers("slot_length_modes")):
        assert rc == 0 and "WORKER DONE" in out, "worker %d:\n%s" % (i, out[-3000:])
        done += int(out.split("WORKER DONE")[1].split()[0])
    assert done == len(pairs)


# ---- 2. the premise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minutes", SLOT_LENGTHS)
def test_the_library_picks_the_dense_tick_and_its_ring_form_by_itself(minutes):
    g = load_slot(DENSE_DAY[minutes])
    assert int(g["tick_minutes"]) == minutes and dense_by_own_rules(g)
    env = make_env(g, 2)
    lay = env.layout()
    assert env.main_kernel() == "k_tick_dense" and lay["dense"] == 1 and lay["dense_st"] == 0, (env.main_kernel(), lay)
    if minutes <= 2:      # arrivals spread over more than DENSE_PULL_WMAX slots (tests/test_order_tables.py asserts the verdict): the ring form
        assert lay["pull"] == 0, lay
        assert slot_day_facts(g)["far"] > 0       # ... and trips beyond the ring horizon: far list, inbox, migration
    else:
        assert lay["pull"] == 1, lay
    env.close()
    s = load_slot(SEARCH_DAY[minutes])
    assert int(s["tick_minutes"]) == minutes and bool(s["neighbor_can_server"]) and int(s["depth_limit"]) >= 1
    assert slot_day_facts(s)["cross"] >= 10, SEARCH_DAY[minutes]
    env = make_env(s, 2)
    assert env.main_kernel() != "k_tick_dense", env.main_kernel()
    env.close()


# ---- 3. the per-slot device planes ------------------------------------------------------------------------------------------------------------
PLANE_DAYS = [DENSE_DAY[k] for k in SLOT_LENGTHS] + [SEARCH_DAY[k] for k in SLOT_LENGTHS]


@pytest.mark.parametrize("name", PLANE_DAYS)
def test_device_planes_at_every_slot(name):
    """Observations and per-cluster outcomes at every slot (PlaneChecker), the idle heads, the six vehicle planes, the vehicle outcomes and
    the idle roster at every slot of a short day and every 16th slot of a day of hundreds of slots - each replica against its own oracle."""
    g = load_slot(name)
    V, C = int(g["V"]), int(g["C"])
    init = seeded_init(g, R3)
    env = make_env(g, R3)
    env.reset(init)
    oracles = oracles_of(g, init)
    cl = g["node2cluster"][g["o_pickup"].astype(np.int64)]
    chk = PlaneChecker(env, oracles, [cl] * R3, tag=name)
    dense = bool(env.layout()["dense"])
    seen = new_seen()
    before = [o.orders()["status"] for o in oracles]
    every = thin(g)
    assert env.T == int(g["n_ticks"])
    for t in range(env.T):
        env.step()
        for o in oracles:
            o.begin_tick()
        chk.check(t, range(R3))
        tag = "%s slot %d" % (name, t)
        rows = got_rows(env) if t % every == 0 else None
        for r, o in enumerate(oracles):
            after = o.orders()
            if rows is not None:
                exp = processed_rows(before[r], after["status"], g["o_pickup"], after["vehicle"], after["wait"], after["value"], V)
                assert_rows(rows[r], exp, "%s replica %d" % (tag, r))
            before[r] = after["status"]
        if t % every == 0:
            check_sums(env, rows, tag)
            check_heads(env, 4, oracles, tag)
            check_planes(env, oracles, tag, seen, dense)
            check_roster(env, oracles, tag)
        env.advance()
        for o in oracles:
            o.end_tick()
    check_planes(env, oracles, name + " after the last advance", seen, dense)
    check_end_of_day(env, oracles, name)
    env.close()


def fixed_vehicle_targets(g, R):
    """Every fifth vehicle is sent to one node of its own whenever it is idle (a target of a vehicle on its way is ignored)."""
    V = int(g["V"])
    valid = np.flatnonzero(g["node2cluster"] >= 0)
    tg = np.full((R, V), -1, dtype=np.int32)
    for r in range(R):
        v = np.arange(r % 5, V, 5)
        tg[r, v] = valid[(v * 7 + r) % valid.size]
    return tg


@pytest.mark.parametrize("name", PLANE_DAYS)
def test_hooked_day_with_fixed_actions_equals_the_stepwise_loop(name):
    """run_hooked(T) with a fixed per-vehicle target tensor and an action tensor of empty entries: one graph launch for the day against
    step / apply / advance slot by slot on a second handle, and both against the oracle given the same targets."""
    import torch
    g = load_slot(name)
    init = seeded_init(g, R3)
    tg = fixed_vehicle_targets(g, R3)
    kw = dict(stream=torch.cuda.current_stream().cuda_stream)
    held, acts = to_dev(tg), to_dev(np.full((R3, 2, 3), -1, dtype=np.int32))
    hooked = make_env(g, R3, **kw)
    hooked.reset(init)
    hooked.run_hooked(hooked.T, actions=acts, vehicle_targets=held)
    hooked.sync()
    loop = make_env(g, R3, **kw)
    loop.reset(init)
    oracles = oracles_of(g, init)
    moved = 0
    for t in range(loop.T):
        loop.step()
        loop.apply_dispatch_torch(acts)
        loop.apply_dispatch_vehicles_torch(held)
        loop.advance()
        for r, o in enumerate(oracles):
            o.begin_tick()
            moved += oracle_apply(o, tg[r])[0]
            o.end_tick()
    loop.sync()
    assert moved > 0 or int(g["V"]) == 0
    check_end_of_day(loop, oracles, name + " stepwise")
    check_end_of_day(hooked, oracles, name + " hooked")
    a, b = hooked.vehicles_all(source=True), loop.vehicles_all(source=True)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s plane %s" % (name, k))
    hooked.close()
    loop.close()


# ---- 4. the whole day as one run ----------------------------------------------------------------------------------------------------------------
RUN_DAY = {k: (DENSE_DAY if i % 2 == 0 else SEARCH_DAY)[k] for i, k in enumerate(SLOT_LENGTHS)}


@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("minutes", SLOT_LENGTHS)
def test_whole_day_in_one_run(minutes, graph, monkeypatch):
    monkeypatch.setenv("VDS_RUN_GRAPH", "1" if graph == "graph" else "0")
    g = load_slot(RUN_DAY[minutes])
    init = seeded_init(g, R3)
    env = make_env(g, R3)
    env.reset(init)
    env.run(env.T)
    env.sync()
    oracles = oracles_of(g, init)
    for o in oracles:
        o.run_day()
    check_end_of_day(env, oracles, "%s %s" % (RUN_DAY[minutes], graph))
    env.close()


# ---- 5. the days of more than 32767 slots ---------------------------------------------------------------------------------------------------
LONG_MODES = {"slot_long_pull": ("fast", "generic", "rows", "dense_ring"), "slot_long_search": ("fast", "generic", "rows", "dfs_v2", "dfs_wide")}


def step_oracles(oracles, n):
    for o in oracles:
        for _ in range(n):
            o.begin_tick()
            o.end_tick()


def run_to(env, oracles, t_from, t_to):
    """Slots t_from .. t_to - 1 in runs of at most CHUNK slots; the oracles alongside."""
    t = t_from
    while t < t_to:
        n = min(CHUNK, t_to - t)
        env.run(n)
        t += n
    step_oracles(oracles, t_to - t_from)


def check_slot(env, oracles, g, t, tag):
    """Right after the step of slot t: planes, counters and containers of every replica against its oracle, replica 0 against the reference."""
    ob, cn = env.obs(), env.counters()
    for r, o in enumerate(oracles):
        oo, oc = o.obs(), o.counters()
        for a, b in (("idle_pre", "idle_pre"), ("idle_now", "idle_post"), ("supply", "supply"), ("cl_orders", "cl_orders"), ("inflight", "inflight")):
            np.testing.assert_array_equal(ob[a][r], oo[b], err_msg="%s slot %d replica %d obs %s" % (tag, t, r, a))
        for i, k in enumerate(("order_num", "reject_num", "matched", "wait_sum", "dispatch_num", "dispatch_cost")):
            assert cn[r, i] == oc[k], (tag, t, r, k, cn[r, i], oc[k])
        assert cn[r, 7] == oc["evals"], (tag, t, r, "evals")
        check_lists(env, r, o, t)
    if g is not None:
        np.testing.assert_array_equal(ob["supply"][0], g["t_supply"][t], err_msg="%s slot %d" % (tag, t))
        np.testing.assert_array_equal(ob["idle_now"][0], g["t_idle_post"][t], err_msg="%s slot %d" % (tag, t))
        assert (cn[0, 0], cn[0, 1], cn[0, 3]) == (g["t_order_num"][t], g["t_reject_num"][t], g["t_wait_sum"][t]), (tag, t)


def check_orders(env, oracles, g, tag):
    od = env.orders()
    for r, o in enumerate(oracles):
        oo = o.orders()
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(od[k][r], oo[k], err_msg="%s replica %d %s" % (tag, r, k))
    if g is not None:
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(od[k][0], g["o_" + k], err_msg="%s %s against the reference" % (tag, k))


@pytest.mark.parametrize("name,mode", [(n, m) for n in LONG for m in LONG_MODES[n]])
def test_long_day_in_chunks(name, mode):
    """run(CHUNK - 1) + step, the comparison, advance - to the end of the day; a chunk boundary at slot 32767 and at slot 32768."""
    g = load_slot(name)
    T = int(g["n_ticks"])
    assert T > SIGN_SLOT and slot_day_facts(g)["served_late"] > 0 and slot_day_facts(g)["across"] > 0
    init = seeded_init(g, R3)
    env = make_env(g, R3, **MODES[mode])
    if name == "slot_long_pull" and mode in ("fast", "dense_ring"):      # static arrival slots beyond slot 32767 / the arrival ring
        lay = env.layout()
        assert (env.main_kernel(), lay["dense"], lay["pull"]) == ("k_tick_dense", 1, int(mode == "fast")), lay
    env.reset(init)
    oracles = oracles_of(g, init)
    assert env.T == T
    stops = sorted(set(list(range(CHUNK - 1, T, CHUNK)) + [SIGN_SLOT - 1, SIGN_SLOT, T - 1]))
    t = 0
    for stop in stops:          # slots t .. stop - 1 as runs, slot `stop` stepped and compared
        run_to(env, oracles, t, stop)
        env.step()
        for o in oracles:
            o.begin_tick()
        check_slot(env, oracles, g, stop, "%s %s" % (name, mode))
        env.advance()
        for o in oracles:
            o.end_tick()
        t = stop + 1
    env.sync()
    check_orders(env, oracles, g, "%s %s" % (name, mode))
    cn = env.counters()
    assert (cn[0, 0], cn[0, 1], cn[0, 6]) == (int(g["order_num"]), int(g["reject_num"]), int(g["sum_order_value"]))
    env.close()


def dispatch_point(env, oracles, g, rng, form, t, tag):
    """One oracle-mirrored dispatch call in the given form right after the step of slot t, then containers, vehicle planes and the
    dispatch counters of every replica."""
    valid = np.flatnonzero(g["node2cluster"] >= 0)
    R = len(oracles)
    moved = 0
    if form in ("host", "kform"):
        reps, cls, poss, tgts = pick_dispatches(rng, oracles, range(R), valid)
        moved = len(reps)
        if reps and form == "host":
            env.apply_dispatch(reps, cls, poss, tgts)
        elif reps:
            held = dispatch_tensor(R, reps, cls, poss, tgts)
            env.apply_dispatch_torch(held)
            env.sync()
    elif form == "host_at":
        # two or three idle vehicles of a replica to ONE node with ONE arrival minute five slots ahead (vds_apply_dispatch_ex): they share
        # a ring bucket, which is drained by ranking the entries' meta words - from slot 32768 on with the slot's top bit set
        reps, cls, poss, tgts, arrs = [], [], [], [], []
        for r, o in enumerate(oracles):
            L = o.lists()
            k = min(int(L["idle_off"][-1]), 2 + (t + r) % 2)
            if k < 2:
                continue
            node, arrive = int(valid[(t + 3 * r) % valid.size]), int(o.now_min) + 5 * int(g["tick_minutes"])
            for flat in range(k):
                c = int(np.searchsorted(L["idle_off"], flat, side="right") - 1)
                reps.append(r); cls.append(c); poss.append(int(flat - L["idle_off"][c])); tgts.append(node); arrs.append(arrive)
            o.dispatch_at(L["idle_veh"][:k], np.full(k, node), arrive_min=np.full(k, arrive))
        moved = len(reps)
        if reps:
            env.apply_dispatch(reps, cls, poss, tgts, arrive_min=arrs)
    elif form == "vehicles":
        tg = random_targets(rng, g, R, frac=0.4)
        held = to_dev(tg)
        env.apply_dispatch_vehicles_torch(held)
        moved = sum(oracle_apply(o, tg[r])[0] for r, o in enumerate(oracles))
    else:
        check_roster(env, oracles, tag + " roster before the call")          # (the refresh a roster call needs)
        stats = dict(moved=0, refused=dict.fromkeys(("beyond_n", "no_cluster", "day_over"), 0))
        roster_call(env, oracles, roster_targets(rng, g, oracles, frac=0.4), g, stats)
        moved = stats["moved"]
    env.sync()
    check_all(env, oracles, t, "%s %s" % (tag, form))
    return moved


FORMS = ("host", "kform", "vehicles", "roster", "host_at")
EVERY = 64          # slots between two dispatch calls of the second pass


def walk_with_dispatch(env, oracles, g, rng, t_from, t_to, tag, first_form=0):
    """Slots t_from .. t_to - 1: runs, and at every slot t with (t + 1) % EVERY == 0 - slot 32767 is one - a step, a dispatch call
    (the five forms in turn), the checks, the advance.  Returns ({form: vehicles moved, "shared_late": vehicles sent into a shared bucket from slot 32767 on}, moves from slot 32767 on)."""
    import torch  # noqa: F401 (the device forms)
    moved, late = dict.fromkeys(FORMS + ("shared_late",), 0), 0
    t, i = t_from, first_form
    while t < t_to:
        stop = min((t // EVERY + 1) * EVERY - 1, t_to)
        run_to(env, oracles, t, stop)
        t = stop
        if t >= t_to:
            break
        env.step()
        for o in oracles:
            o.begin_tick()
        form = FORMS[i % len(FORMS)]
        n = dispatch_point(env, oracles, g, rng, form, t, tag)
        moved[form] += n
        late += n if t >= SIGN_SLOT - 1 else 0
        moved["shared_late"] += n if form == "host_at" and t >= SIGN_SLOT - 1 else 0
        i += 1
        env.advance()
        for o in oracles:
            o.end_tick()
        t += 1
    return moved, late


@pytest.mark.parametrize("mode", ["fast", "rows"])
@pytest.mark.parametrize("name", LONG)
def test_long_day_dispatch_forms_and_snapshot_past_slot_32767(name, mode):
    """From shortly before slot 32768 to the end of the day: every 64 slots one dispatch call - host list, [R, K, 3] device tensor,
    per-vehicle targets, roster targets, a host list that sends several vehicles into one arrival bucket, in turn - mirrored on the oracles: the dispatched vehicles' entries carry the dispatch bit beside
    a slot number with the top bit set.  In the default kernels the pass first runs from a snapshot taken at slot 32768 - 192 to slot
    32768 + 256, restores, and starts again with oracles kept at the snapshot's slot."""
    import torch
    g = load_slot(name)
    T = int(g["n_ticks"])
    init = seeded_init(g, R3)
    env = make_env(g, R3, **{**MODES[mode], **dict(idle_cap=64, ring_cap=64, far_cap=64, stream=torch.cuda.current_stream().cuda_stream)})
    env.reset(init)
    oracles = oracles_of(g, init)
    start = SIGN_SLOT - 3 * EVERY
    tag = "%s %s" % (name, mode)
    run_to(env, oracles, 0, start)
    rng = np.random.default_rng(32768)
    if mode == "fast":
        kept = oracles_of(g, init)
        step_oracles(kept, start)
        env.snapshot()
        m, late = walk_with_dispatch(env, oracles, g, rng, start, SIGN_SLOT + 256, tag + " before the restore")
        assert late > 0 and sum(m.values()) > 0, (m, late)
        env.restore()
        env.sync()
        assert env.clock[0] == start
        oracles = kept
    moved, late = walk_with_dispatch(env, oracles, g, rng, start, T, tag, first_form=1)
    assert all(moved[f] > 0 for f in FORMS) and late > 0 and moved["shared_late"] >= 4, (moved, late)
    env.sync()
    check_orders(env, oracles, None, tag)
    check_all(env, oracles, T, tag + " after the last advance")
    env.close()


# ---- 6. the shell -------------------------------------------------------------------------------------------------------------------------------
def shell_day(g, tmp_path, cls, **kw):
    """``Simulation`` on a reference-style data directory of the fixture's day (the city from its seed, the styled cost table and the labels
    from the fixture, the release times stretched as the generator did), TimePeriods = the fixture's slot length."""
    import time
    from oracle.ref_harness import write_reference_data_dir
    from vehicles_dispatch_simulator_amd import world
    C, mode, V = int(g["C"]), str(g["cluster_mode"]), int(g["V"])
    city = synth.make_city(int(g["city_seed"]), N=int(g["N"]), C=C, with_neighbors=False)
    city.cost = g["cost"]
    city.node2cluster = g["node2cluster"]
    start, pick, dele = synth.make_orders(int(g["order_seed"]), city.N, int(g["n_orders_raw"]))
    if "span" in g:
        start = start[0] + (start - start[0]) * int(g["span"][0]) // int(g["span"][1])
    os.environ["TZ"] = "UTC"
    time.tzset()
    write_reference_data_dir(str(tmp_path), city, start, pick, dele, n_drivers=V, cluster_mode=mode)
    table = synth.neighbor_table_from_sums(*synth.cluster_cost_sums_host(city.cost, city.node2cluster, C))
    world.write_neighbor_csv(os.path.join(str(tmp_path), "data", str(tuple(city.bound)) + str(C) + mode + "Neighbor.csv"), table)
    sim = cls(ClusterMode=mode, DemandPredictionMode="None", DispatchMode="Simulation", VehiclesNumber=V,
              TimePeriods=np.timedelta64(int(g["tick_minutes"]), "m"), LocalRegionBound=synth.DEFAULT_BOUND, SideLengthMeter=float(g["side_m"]),
              VehiclesServiceMeter=float(g["service_m"]), NeighborCanServer=bool(g["neighbor_can_server"]), FocusOnLocalRegion=False,
              DataDir=os.path.join(str(tmp_path), "data"), Quiet=True, **kw)
    random.seed(int(g["seed"]))
    sim.CreateAllInstantiate("1101")
    np.testing.assert_array_equal(sim._init_nodes[0], g["veh_node"])
    np.testing.assert_array_equal(sim._world.o_release_min - sim._world.o_release_min[0], g["o_release_min"] - g["o_release_min"][0])
    np.testing.assert_array_equal(sim._world.o_pickup, g["o_pickup"])
    return sim


def policy_sim_class():
    from vehicles_dispatch_simulator_amd.simulation import Simulation

    class SlotPolicySim(Simulation):
        """oracle/dispatch_idiom.policy_factory(N, every) written against the object views (test_gpu_simulation_shell.PolicySim)."""
        every = 3

        def DispatchFunction(self):
            tick, N = self.step, len(self.NodeIDList)
            if tick % self.every != 0:
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

    return SlotPolicySim


SHELL_DAYS = {1: "slot_0001_0", 60: "slot_0060_0"}          # (no live window - the shell's is the reference's constant; whole-minute costs)


@pytest.mark.parametrize("minutes", sorted(SHELL_DAYS))
def test_shell_hooked_day_equals_the_reference(minutes, tmp_path):
    """A subclass with the dispatch hook the reference ran (the generator's policy, every max(3, 60 // minutes) slots): the day of the
    unmodified reference, counter for counter and order for order."""
    g = load_slot(SHELL_DAYS[minutes])
    assert not live_window(g) and int(g["dispatch_num"]) > 0 and "dispatch_extra_minutes" not in g and int(g["tick_minutes"]) == minutes
    cls = policy_sim_class()
    cls.every = max(3, 60 // minutes)
    sim = shell_day(g, tmp_path, cls)
    sim.SimCity()
    assert sim.step == int(g["n_ticks"])
    assert (sim.OrderNum, sim.RejectNum, sim.TotallyWaitTime) == (int(g["order_num"]), int(g["reject_num"]), int(g["wait_sum"]))
    assert (sim.DispatchNum, sim.TotallyDispatchCost, sim.SumOrderValue) == (int(g["dispatch_num"]), int(g["dispatch_cost"]), int(g["sum_order_value"]))
    st = sim.env.orders(0, 1)
    for k in ("status", "vehicle", "wait"):
        np.testing.assert_array_equal(st[k][0], g["o_" + k], err_msg=k)


@pytest.mark.parametrize("minutes", sorted(SHELL_DAYS))
def test_shell_fast_forward_day(minutes, tmp_path):
    """No hook overridden: the whole day as one device run.  The fixture's day was recorded with dispatch, so the expectation is the
    oracle - pinned to the reference on this very day by tests/test_oracle_fuzz_golden.py - run without it."""
    from vehicles_dispatch_simulator_amd.simulation import Simulation
    g = load_slot(SHELL_DAYS[minutes])
    sim = shell_day(g, tmp_path, Simulation)
    sim.SimCity()
    o = make_oracle(g)
    o.run_day()
    oc, oo = o.counters(), o.orders()
    assert sim.step == int(g["n_ticks"])
    assert (sim.OrderNum, sim.RejectNum, sim.TotallyWaitTime, sim.SumOrderValue) == (oc["order_num"], oc["reject_num"], oc["wait_sum"], oc["sum_order_value"])
    st = sim.env.orders(0, 1)
    for k in ("status", "vehicle", "wait"):
        np.testing.assert_array_equal(st[k][0], oo[k], err_msg=k)
