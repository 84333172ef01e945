"""Policy-chosen matching on the device (vds_set_match_external / vds_apply_match_device / vds_match_orders_device;
``BatchedDispatchEnv(match_external=True)``, ``env.apply_match_torch``): the handle runs Update alone and commits an int32
``[R, match_width]`` tensor of vehicles, one per order of the slot in id order.
  2  the built-in matcher replayed: every tiny fixture without neighbour search, fed its own recorded vehicles, equals the golden and
     the CPU oracle slot by slot (observations, lists and dicts with minutes, counters but evals, orders, vehicles);
  3  the reference's externally matched day (matchpack_0), and seeded random policies with dispatch calls of all three device forms
     behind the match, against tests/match_model.py;
  4  the shapes at which the three kernels can go wrong;  5  the refusals.
All comparisons are exact."""
import os
import sys

import numpy as np
import pytest

from helpers import dispatch_by_tick, golden_names, load_golden, make_oracle
from match_model import MatchModel
from test_gpu_parity import check_lists, make_env
from test_match_model import model_of

pytestmark = pytest.mark.gpu

VDS_EINVAL, VDS_ESTATE = -1, -4
CAPS = dict(idle_cap=256, ring_cap=512, far_cap=512)
PLAIN = [n for n in golden_names("tiny_") if not bool(load_golden(n)["neighbor_can_server"])]


def torch_stream_kw():
    import torch
    return dict(stream=torch.cuda.current_stream().cuda_stream)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def ext_env(g, R, **kw):
    return make_env(g, R, match_external=True, **{**torch_stream_kw(), **kw})


def rows_to_dev(env, rows):
    a = np.full((env.R, env.match_width), -1, dtype=np.int32)
    for r, row in enumerate(rows):
        a[r, :len(row)] = row
    return to_dev(a)


def check_containers(env, r, o, tag):
    """lists(r) against an oracle or a model: idle order, dict order, minutes, nodes and carried orders."""
    L, G, veh = o.lists(), env.lists(r), o.vehicles()
    for k in ("idle_off", "idle_veh", "arr_off", "arr_veh", "arr_min"):
        np.testing.assert_array_equal(G[k], L[k], err_msg="%s replica %d %s" % (tag, r, k))
    n, na = L["idle_off"][-1], L["arr_off"][-1]
    np.testing.assert_array_equal(G["idle_node"][:n], veh["loc"][L["idle_veh"][:n]], err_msg=tag)
    np.testing.assert_array_equal(G["arr_node"][:na], veh["dest"][L["arr_veh"][:na]], err_msg=tag)
    np.testing.assert_array_equal(G["arr_order"][:na], veh["order"][L["arr_veh"][:na]], err_msg=tag)


def check_state(env, refs, tag, vehicles=True, idle_key="idle_now"):
    """Every replica against its reference (oracle or model): the five observation planes, the containers (+ vehicles(r)), all
    counters but evals, orders()."""
    ob, cn, od = env.obs(), env.counters(), env.orders()
    for r, o in enumerate(refs):
        oo, oc, ord_ = o.obs(), o.counters(), o.orders()
        for k in ("idle_pre", "idle_now", "supply", "cl_orders", "inflight"):
            np.testing.assert_array_equal(ob[k][r], oo[idle_key if k == "idle_now" else k], err_msg="%s replica %d obs %s" % (tag, r, k))
        for i, k in enumerate(("order_num", "reject_num", "matched", "wait_sum", "dispatch_num", "dispatch_cost", "sum_order_value")):
            assert cn[r, i] == oc[k], (tag, r, k, cn[r, i], oc[k])
        if vehicles:
            check_lists(env, r, o, -1)
        else:
            check_containers(env, r, o, tag)
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(od[k][r], ord_[k], err_msg="%s replica %d orders %s" % (tag, r, k))


# ---- 2. the built-in matcher, replayed ------------------------------------------------------------------------------------------------
def test_fixtures_of_every_kind_are_replayed():
    for n in ("tiny_window6", "tiny_tick5", "tiny_fraccost", "tiny_sort_ties", "tiny_two_orders", "tiny_dispatch"):
        assert n in PLAIN or bool(load_golden(n)["neighbor_can_server"]), n
    assert {"tiny_window6", "tiny_fraccost", "tiny_sort_ties", "tiny_two_orders", "tiny_dispatch"} <= set(PLAIN)


@pytest.mark.parametrize("name", [n for n in golden_names("tiny_") if n in PLAIN or n == "tiny_tick5"])
def test_replaying_the_builtin_matcher(name):
    g = load_golden(name)
    if bool(g["neighbor_can_server"]):
        # (recorded with neighbour search: the external handle refuses the flag, and the recorded vehicles - some from other
        # clusters - are exactly what a policy may name; the oracle keeps the search)
        ge = dict(g, neighbor_can_server=np.bool_(False))
    else:
        ge = g
    R = 3
    env = ext_env(ge, R, **CAPS)
    assert env.main_kernel() == "k_update_external"
    mo = env.match_orders()
    n_proc = mo["rec"].shape[0]
    np.testing.assert_array_equal(mo["rec"][:, 0], g["o_pickup"][:n_proc])
    np.testing.assert_array_equal(mo["rec"][:, 1], g["o_delivery"][:n_proc])
    np.testing.assert_array_equal(mo["rec"][:, 2], g["node2cluster"][g["o_pickup"][:n_proc]])
    np.testing.assert_array_equal(mo["rec"][:, 3], np.asarray(g["o_value"])[:n_proc])
    mt = env.match_orders_torch()
    np.testing.assert_array_equal(mt["rec"].cpu().numpy(), mo["rec"])
    np.testing.assert_array_equal(mt["slot_off"].cpu().numpy(), mo["slot_off"])
    off = mo["slot_off"]
    assert off.size == env.T + 1 and env.match_width == int(np.diff(off).max()) and off[-1] == n_proc
    init = np.tile(g["veh_node"], (R, 1))
    env.reset(init)
    o = make_oracle(g)
    disp = dispatch_by_tick(g)
    extra = int(g["dispatch_extra_minutes"]) if "dispatch_extra_minutes" in g else 0
    np.testing.assert_array_equal(off[1:], g["t_order_num"])
    for t in range(env.T):
        env.step()
        o.begin_tick()
        env.apply_match_torch(rows_to_dev(env, [g["o_vehicle"][off[t]:off[t + 1]]] * R))
        check_state(env, [o] * R, "%s slot %d" % (name, t), idle_key="idle_post")
        ob, cn = env.obs(), env.counters()
        np.testing.assert_array_equal(ob["supply"][0], g["t_supply"][t])
        np.testing.assert_array_equal(ob["idle_now"][0], g["t_idle_post"][t])
        np.testing.assert_array_equal(ob["idle_pre"][0], g["t_idle_pre"][t])
        np.testing.assert_array_equal(ob["cl_orders"][0], g["t_cl_orders"][t])
        assert cn[0, 0] == g["t_order_num"][t] and cn[0, 1] == g["t_reject_num"][t] and cn[0, 3] == g["t_wait_sum"][t]
        assert (cn[:, 7] == 0).all()                     # the evaluations counter does not move
        if "l_idle_off" in g:
            G = env.lists(0)
            for k in ("idle_off", "idle_veh", "arr_off", "arr_veh", "arr_min"):
                np.testing.assert_array_equal(G[k], g["l_" + k][t], err_msg="%s slot %d %s" % (name, t, k))
        if t in disp:
            rows = np.array(disp[t])
            L = o.lists()
            pos = [int(np.flatnonzero(L["idle_veh"][L["idle_off"][cl]:L["idle_off"][cl + 1]] == veh)[0]) for veh, cl in zip(rows[:, 1], rows[:, 2])]
            rep = np.repeat(np.arange(R), len(rows))
            if extra:         # (tiny_dispatch_delay: the hook body wrote its own arrival minute)
                env.apply_dispatch(rep, np.tile(rows[:, 2], R), np.tile(pos, R), np.tile(rows[:, 4], R), arrive_min=np.tile(o.now_min + rows[:, 5] + extra, R))
                o.dispatch_at(rows[:, 1], rows[:, 4], arrive_min=o.now_min + rows[:, 5] + extra)
            else:
                env.apply_dispatch(rep, np.tile(rows[:, 2], R), np.tile(pos, R), np.tile(rows[:, 4], R))
                o.dispatch(rows[:, 1], rows[:, 4])
            check_state(env, [o] * R, "%s slot %d after dispatch" % (name, t))
            np.testing.assert_array_equal(env.obs()["idle_now"][0], g["t_idle_after_dispatch"][t])
        env.advance()
        o.end_tick()
    env.sync()
    od = env.orders()
    for k in ("status", "vehicle", "wait"):
        np.testing.assert_array_equal(od[k][0], g["o_" + k])
    env.close()


# ---- 3. the reference's externally matched day; fuzzed policies ---------------------------------------------------------------------------
def test_the_reference_day_with_an_overridden_matcher():
    from test_match_model import check_slot
    g = load_golden("matchpack_0")
    R = 3
    env = ext_env(g, R)
    env.reset(np.tile(g["veh_node"], (R, 1)))
    m = model_of(g)
    assert env.T == int(g["n_ticks"]) and env.match_width == g["assign"].shape[1]
    for t in range(env.T):
        env.step()
        m.update()
        env.apply_match_torch(to_dev(np.tile(g["assign"][t], (R, 1))))
        m.match(g["assign"][t])
        check_slot(m, g, t)
        check_state(env, [m] * R, "matchpack_0 slot %d" % t)
        G = env.lists(R - 1)
        for k in ("idle_off", "idle_veh", "arr_off", "arr_veh", "arr_min"):
            np.testing.assert_array_equal(G[k], g["l_" + k][t], err_msg="slot %d %s" % (t, k))
        env.advance()
        m.end_tick()
    od = env.orders()
    for k in ("status", "vehicle", "wait"):
        np.testing.assert_array_equal(od[k][1], g["o_" + k])
    env.close()


def fuzz_row(rng, m, n):
    """One replica's entries for n orders: -1, any vehicle number (idle or not, beyond the fleet or not), an idle vehicle of any
    cluster, or the entry before it again."""
    idle = [v for c in m.idle for v in c]
    row = []
    for j in range(n):
        u = rng.random()
        if u < 0.15:
            row.append(-1)
        elif u < 0.40 or not idle:
            row.append(int(rng.integers(0, m.V)))
        elif u < 0.50 and row:
            row.append(row[-1])
        else:
            row.append(int(idle[rng.integers(0, len(idle))]))
    return row


def check_derived(env, models, t, off):
    """outcomes_torch, vehicle_outcomes_torch and orders_torch(t, t) of the slot matched last."""
    oc = env.outcomes_torch()
    vo = env.vehicle_outcomes_torch()
    ot = env.orders_torch(t, t)
    env.sync()
    oc, vo, ot = oc.cpu().numpy(), vo.cpu().numpy(), ot.cpu().numpy()
    for r, m in enumerate(models):
        exp = np.zeros((4, m.C), dtype=np.int64)
        for o in range(off[t], off[t + 1]):
            c = m.n2c[m.pick[o]]
            if m.o_status[o] == 1:
                exp[0, c] += 1; exp[2, c] += m.o_wait[o]; exp[3, c] += m.value[o]
            else:
                exp[1, c] += 1
        np.testing.assert_array_equal(oc[:, r], exp, err_msg="slot %d replica %d outcomes" % (t, r))
        ev = np.full((m.V, 4), -1, dtype=np.int32)
        for v, rec in m.slot_results.items():
            ev[v] = rec
        np.testing.assert_array_equal(vo[r], ev, err_msg="slot %d replica %d vehicle outcomes" % (t, r))
        rows = np.array([[m.o_vehicle[o], m.o_wait[o]] for o in range(off[t], off[t + 1])], dtype=np.int32).reshape(-1, 2)
        np.testing.assert_array_equal(ot[r, off[t]:off[t + 1]], rows, err_msg="slot %d replica %d order rows" % (t, r))


@pytest.mark.parametrize("name,mode", [("tiny_kmeans", {}), ("tiny_sort_ties", {}), ("tiny_kmeans", {"ring_ticks": 2})], ids=["kmeans", "sort_ties", "kmeans_far"])
def test_fuzzed_policies_and_dispatch_behind_the_match(name, mode):
    g = load_golden(name)
    R, V, N = 4, int(g["V"]), int(g["N"])
    fleet = [V, V - 7, V // 2, V]
    env = ext_env(g, R, **{**CAPS, **mode})
    env.set_fleet(fleet)
    valid = np.flatnonzero(g["node2cluster"] >= 0)
    seeds = np.random.default_rng(77)
    init = valid[seeds.integers(0, valid.size, (R, V))].astype(np.int32)
    env.reset(init)
    models = []
    for r in range(R):
        m = MatchModel(g["cost"], g["node2cluster"], int(g["C"]), V, g["o_release_min"], g["o_pickup"], g["o_delivery"], 10, fleet=fleet[r])
        m.reset(init[r])
        models.append(m)
    rngs = [np.random.default_rng(900 + r) for r in range(R)]
    off = env.match_orders()["slot_off"]
    T = min(env.T, 36)
    seen = dict(served=0, rejected=0, dup=0, busy=0, beyond_fleet=0, cross=0, moves=0)
    for t in range(T):
        env.step()
        rows = []
        for r, m in enumerate(models):
            m.update()
            ids = m.slot_orders()
            assert len(ids) == off[t + 1] - off[t]
            row = fuzz_row(rngs[r], m, len(ids))
            idle = set(v for c in m.idle for v in c)
            seen["dup"] += len(row) - len(set(row))
            seen["busy"] += sum(1 for v in row if 0 <= v < fleet[r] and v not in idle)
            seen["beyond_fleet"] += sum(1 for v in row if v >= fleet[r])
            seen["cross"] += sum(1 for o, v in zip(ids, row) if v in idle and m.cluster[v] != m.n2c[m.pick[o]])
            assert m.match(row) == 0
            rows.append(row)
        env.apply_match_torch(rows_to_dev(env, rows))
        tag = "%s slot %d" % (name, t)
        check_state(env, models, tag, vehicles=False)
        check_derived(env, models, t, off)
        # ---- dispatch behind the match, one device form per slot
        tg = np.full((R, V), -1, dtype=np.int32)
        form = t % 3
        if form == 0:          # by vehicle number
            pick = seeds.random((R, V)) < 0.1
            tg[pick] = valid[seeds.integers(0, valid.size, int(pick.sum()))]
            env.apply_dispatch_vehicles_torch(to_dev(tg))
            for r, m in enumerate(models):
                ids = [v for v in range(V) if tg[r, v] >= 0 and m.dest[v] < 0 and m.cluster[v] >= 0]
                m.dispatch(ids, tg[r, ids]); seen["moves"] += len(ids)
        elif form == 1:        # by roster position
            ro = env.idle_roster()
            for r, m in enumerate(models):
                n = int(ro["off"][r, -1])
                pick = np.flatnonzero(seeds.random(n) < 0.1)
                tg[r, pick] = valid[seeds.integers(0, valid.size, pick.size)]
                m.dispatch(ro["veh"][r, pick], tg[r, pick]); seen["moves"] += pick.size
            env.apply_dispatch_roster_torch(to_dev(tg))
        else:                  # K-form: (from_cluster, idle_pos, target)
            acts = np.full((R, 3, 3), -1, dtype=np.int32)
            for r, m in enumerate(models):
                cs = [c for c in range(m.C) if m.idle[c]][:2]
                for k, c in enumerate(cs):
                    acts[r, k + 1] = (c, len(m.idle[c]) - 1, valid[seeds.integers(0, valid.size)])
                for k, c in enumerate(cs):
                    m.dispatch([m.idle[c][-1]], [acts[r, k + 1, 2]]); seen["moves"] += 1
            env.apply_dispatch_torch(to_dev(acts))
        check_state(env, models, tag + " after dispatch form %d" % form, vehicles=False)
        env.advance()
        for m in models:
            m.end_tick()
    for m in models:
        seen["served"] += sum(1 for s in m.o_status if s == 1); seen["rejected"] += sum(1 for s in m.o_status if s == 2)
    assert all(v > 0 for v in seen.values()), seen
    env.close()


# ---- 4. where the kernels can go wrong ---------------------------------------------------------------------------------------------------
def mini(V, batch, C=2, nodes_per=3, batches=2, seed=3, tick=10):
    """A city of C clusters x nodes_per nodes with `batches` bursts of `batch` orders, one burst per slot (+ the order that ends the
    day: quirk Q1); every cost differs, trips of 1 .. 40 minutes."""
    rng = np.random.default_rng(seed)
    N = C * nodes_per
    cost = rng.integers(1, 41, (N, N)).astype(np.int32)
    rel = np.concatenate([np.full(batch, tick * b, dtype=np.int32) for b in range(batches)] + [np.array([tick * (batches + 2)], dtype=np.int32)])
    O = rel.size
    return dict(cost=cost, node2cluster=np.repeat(np.arange(C), nodes_per).astype(np.int32), nbr_off=np.zeros(C + 1, dtype=np.int32),
                nbr_idx=np.zeros(0, dtype=np.int32), depth_limit=0, neighbor_can_server=False, V=V, C=C, N=N, tick_minutes=tick,
                o_release_min=rel, o_pickup=rng.integers(0, N, O).astype(np.int32), o_delivery=rng.integers(0, N, O).astype(np.int32),
                veh_node=rng.integers(0, nodes_per, max(V, 1)).astype(np.int32)[:V])          # every vehicle starts in cluster 0


def run_mini(g, R, plan, **kw):
    """plan(t, r, model, n) -> the row of replica r (or None for the whole call when r is None); every slot against the model."""
    env = ext_env(g, R, **{**CAPS, **kw})
    env.reset(np.tile(g["veh_node"], (R, 1)))
    models = [model_of(g) for _ in range(R)]
    for t in range(env.T):
        env.step()
        for m in models:
            m.update()
        n = len(models[0].slot_orders())
        if plan(t, None, models[0], n) is None:
            env.apply_match_torch(None)
            for m in models:
                m.match(None)
        else:
            rows = [plan(t, r, m, n) for r, m in enumerate(models)]
            for m, row in zip(models, rows):
                assert m.match(row) == 0
            env.apply_match_torch(rows_to_dev(env, rows))
        check_state(env, models, "slot %d" % t, vehicles=int(g["V"]) > 0)
        env.advance()
        for m in models:
            m.end_tick()
    return env, models


def edge_rows(t, r, m, n):
    """replica 0: the movers at the first and the last position of every chunk of 64; 1: every entry moves; 2: every second one, and
    the survivors' order is what is left; 3: nobody."""
    if r is None:
        return 0
    lst = list(m.idle[0]) + [v for c in range(1, m.C) for v in m.idle[c]]
    pick = {0: [v for i, v in enumerate(lst) if i % 64 in (0, 63) or i == len(lst) - 1], 1: lst, 2: lst[::2], 3: []}[r]
    row = list(reversed(pick))[:n]                  # (named by descending position: claims and list order are unrelated)
    return row + [-1] * (n - len(row))


@pytest.mark.parametrize("V", [63, 64, 65, 129])
@pytest.mark.parametrize("far", [False, True], ids=["ring", "far"])
def test_chunk_boundaries_and_more_orders_than_one_claim_workgroup(V, far):
    g = mini(V, 300)              # 300 orders in a slot: two workgroups of the claim kernel
    env, models = run_mini(g, 4, edge_rows, **({"ring_ticks": 2} if far else {}))
    assert env.match_width == 300
    assert models[1].counters()["matched"] >= V and models[3].counters()["matched"] == 0
    if far:                       # trips of up to 80 minutes against a horizon of 2 slots: the far inbox path
        assert max(m.o_wait[o] + m.value[o] for m in models for o in range(m.O) if m.o_status[o] == 1) >= 30
    env.close()


def test_no_vehicles_and_no_tensor():
    g = mini(0, 5)
    env, models = run_mini(g, 3, lambda t, r, m, n: 0 if r is None else [-1] * n)
    assert models[0].counters()["reject_num"] == 10
    env.close()
    g = mini(40, 5)
    env, models = run_mini(g, 3, lambda t, r, m, n: None if t == 1 else (0 if r is None else [m.idle[0][-1 - j] if j < len(m.idle[0]) else -1 for j in range(n)]))
    assert models[0].counters()["reject_num"] == 5 and models[0].counters()["matched"] == 5
    env.close()


def test_an_entry_beyond_the_vehicles_rejects_its_order_and_raises_once():
    g = mini(40, 5)
    R = 3
    env = ext_env(g, R)
    env.reset(np.tile(g["veh_node"], (R, 1)))
    models = [model_of(g) for _ in range(R)]
    for t in range(2):
        env.step()
        for m in models:
            m.update()
        n = len(models[0].slot_orders())
        rows = [[m.idle[0][j] for j in range(n)] for m in models]
        if t == 1:
            rows[1][2] = 40; rows[2][0] = 2 ** 31 - 1
        assert [m.match(row) for m, row in zip(models, rows)] == ([0, 1, 1] if t == 1 else [0, 0, 0])
        env.apply_match_torch(rows_to_dev(env, rows))
        if t == 1:
            with pytest.raises(Exception, match="assignment entry >= 40 vehicles"):
                env.sync()
            env.sync()              # reported once
        check_state(env, models, "slot %d" % t)
        env.advance()
        for m in models:
            m.end_tick()
    assert models[1].o_status[2] == 2 and models[1].o_status[1] == 1 and models[2].o_status[0] == 2
    env.close()


def test_snapshot_before_a_match_and_restore_after_it():
    g = mini(65, 70, batches=3)
    R = 3
    env = ext_env(g, R, **CAPS)
    env.reset(np.tile(g["veh_node"], (R, 1)))
    models = [model_of(g) for _ in range(R)]

    def slot(t, variant, check=True):
        rows = []
        for r, m in enumerate(models):
            n = len(m.slot_orders())
            lst = [v for c in m.idle for v in c]
            row = ((lst[r::2] if variant == 0 else lst[::-1][: 5 + r]) + [7, 7, 64])[:n]      # (and a vehicle twice, a busy one)
            row += [-1] * (n - len(row))
            m.match(row); rows.append(row)
        env.apply_match_torch(rows_to_dev(env, rows))
        if check:
            check_state(env, models, "slot %d variant %d" % (t, variant))

    for t in range(env.T):
        env.step()
        for m in models:
            m.update()
        if t == 1:
            import copy
            env.snapshot()
            saved = copy.deepcopy(models)
            slot(t, 0)
            with pytest.raises(Exception, match="matched already"):
                env.apply_match_torch(None)
            env.restore()                       # back behind the step, before the match: the slot is open again
            models[:] = saved
            with pytest.raises(Exception, match="not matched"):
                env.advance()
        slot(t, 1)
        env.advance()
        for m in models:
            m.end_tick()
    env.close()


@pytest.mark.parametrize("build_name", ["canary", "dirty"])
def test_edge_shapes_on_guarded_and_dirty_tables(build_name):
    from test_gpu_debug_builds import ROOT, build
    from test_gpu_dirty_memory import dirty_env, gpu_allowed, run_limited
    gpu_allowed()
    lib = build(build_name, "libvds_%s.so" % build_name)
    argv = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_match_external.py"), "-k",
            "chunk_boundaries or snapshot_before or beyond_the_vehicles or no_vehicles"]
    rc, out = run_limited(argv, dirty_env(None, lib), 600, "the external-match edge cases under %s" % os.path.basename(lib))
    assert rc == 0 and " passed" in out and "skipped" not in out, out[-6000:]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def raises(code, fn, *a):
    with pytest.raises(Exception) as e:
        fn(*a)
    assert "libvds error %d:" % code in str(e.value), e.value


def test_refusals():
    import torch
    g = load_golden("tiny_kmeans")
    R, V = 3, int(g["V"])
    plain = make_env(g, R, **torch_stream_kw())
    assert plain._lib.vds_set_match_external(plain._h, 1) == VDS_ESTATE and plain._lib.vds_get_match_external(plain._h) == 0
    plain.reset(np.tile(g["veh_node"], (R, 1)))
    plain.step()
    raises(VDS_ESTATE, plain.apply_match_torch, None)
    assert plain._lib.vds_match_orders_device(plain._h, None, None, None) == VDS_ESTATE
    plain.close()
    with pytest.raises(Exception, match="neighbour search is part of the built-in match"):
        make_env(dict(g, neighbor_can_server=True), R, match_external=True)
    env = ext_env(g, R)
    assert env._lib.vds_get_match_external(env._h) == 1
    day = (g["o_release_min"], g["o_pickup"], g["o_delivery"])
    raises(VDS_EINVAL, env.load_order_days, [day, day])
    raises(VDS_EINVAL, env.load_orders_strided, np.tile(day[0], R), np.tile(day[1], R), np.tile(day[2], R), day[0].size, day[0].size)
    env.load_orders(*day)
    raises(VDS_EINVAL, env.set_replica_days, [0] * R)
    env.reset(np.tile(g["veh_node"], (R, 1)))
    raises(VDS_ESTATE, env.run, 8)
    raises(VDS_ESTATE, env.run_hooked, 8)
    ok = torch.full((R, env.match_width), -1, dtype=torch.int32, device="cuda")
    raises(VDS_EINVAL, env.apply_match_torch, ok)                  # before the step
    env.step()
    tg = torch.full((R, V), -1, dtype=torch.int32, device="cuda")
    raises(VDS_ESTATE, env.advance)
    raises(VDS_ESTATE, env.apply_dispatch, [0], [0], [0], [0])
    raises(VDS_ESTATE, env.apply_dispatch_torch, torch.full((R, 2, 3), -1, dtype=torch.int32, device="cuda"))
    raises(VDS_ESTATE, env.apply_dispatch_vehicles_torch, tg)
    raises(VDS_ESTATE, env.apply_dispatch_vehicles_timed_torch, tg, tg, tg)
    env.idle_roster_torch()
    raises(VDS_ESTATE, env.apply_dispatch_roster_torch, tg)
    raises(VDS_ESTATE, env.apply_dispatch_roster_timed_torch, tg, tg, tg)
    # the tensor is checked on the host before the handle is touched: the slot stays open
    for bad in (ok.to(torch.int64), ok[:, :-1], ok[:-1], ok.t().contiguous().t() if env.match_width > 1 else ok.cpu(), ok.cpu(), np.zeros((R, env.match_width), np.int32)):
        with pytest.raises(Exception, match="apply_match_torch: expected"):
            env.apply_match_torch(bad)
    env.apply_match_torch(ok)
    raises(VDS_ESTATE, env.apply_match_torch, ok)                  # twice in a slot
    env.apply_dispatch_vehicles_torch(tg)                          # and now the slot goes on
    env.advance()
    cn = env.counters()
    assert (cn[:, 0] == cn[:, 1]).all()
    env.close()


# ---- 7. the new file is hashed with the host sources --------------------------------------------------------------------------------------
def test_kernel_part_of_the_build_id_is_the_tick_kernels_alone():
    import hashlib
    import re
    from vehicles_dispatch_simulator_amd import _lib
    csrc = _lib.CSRC
    mk = open(os.path.join(csrc, "Makefile")).read()
    ksrcs = re.search(r"^KSRCS := (.*)$", mk, re.M).group(1).split() + re.search(r"^KHDRS := (.*)$", mk, re.M).group(1).split()
    hsrcs = re.search(r"^HSRCS := (.*)$", mk, re.M).group(1).split()
    assert "vds_match_external.hip" in hsrcs and "vds_match_external.hip" not in ksrcs
    text = b"".join(open(os.path.join(csrc, f), "rb").read() for f in ksrcs)
    lines = [re.sub(rb"[ \t]", b"", re.sub(rb"//.*$", b"", l)) for l in text.split(b"\n")]
    digest = hashlib.sha1(b"".join(l + b"\n" for l in lines if l)).hexdigest()[:12]
    bid = _lib.load().vds_build_id().decode()
    assert bid.startswith("src:" + digest + "+"), (bid, digest)
