"""Fleet size per replica (vds_set_fleet) and start nodes from a device tensor (vds_reset_device; ``env.set_fleet``, ``env.fleet``,
``env.reset_torch``).  Replica ``r`` has to behave like ``Simulation(VehiclesNumber = fleet[r])``: the expectation is an
``oracle.Oracle`` built with ``V = fleet[r]`` and reset with the first ``fleet[r]`` nodes of the replica's row
(tests/fleet_expect.py), and - for the fleets the unmodified reference itself ran (tests/golden/fleetpack_0.npz) - the reference's
own record.  Bit-exact, no tolerance.  On the tiny fixtures any two fleet sizes reject a different number of orders
(tests/test_fleet_expect.py), so a replica run at the wrong size, or at the handle's ``V``, cannot pass.

Rows of start nodes are padded behind each fleet with ``-1`` and with a node id beyond ``N``: entries there may hold anything."""
import os
import sys

import numpy as np
import pytest

from fleet_expect import TINY_REJECTS, check_fleet_lists, expected_start_lists, fleet_oracle, fleet_runs, load_fleet
from helpers import dispatch_by_tick, host_view, idle_mask, load_golden, oracle_apply_vehicles
from test_gpu_parity import make_env
from test_gpu_replica_days import mk_env, synth_days
from test_gpu_slot_outcomes import FAMILIES
from vehicle_outcome_expect import processed_rows, slot_sums
from vehicles_dispatch_simulator_amd import synth, workloads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEN = dict(fleets=set(), seg_sides=set(), all_rejected=0)          # what the cases met (the last test of the file asserts it)


def standard_fleets(V):
    return [V, 0, 1, V // 2, V - 1, V]


def pad_rows(rows, fleets, N):
    """The rows with what lies behind each fleet replaced: -1 and a node id in no cluster (beyond N), alternating."""
    rows = np.array(rows, dtype=np.int32)
    V = rows.shape[1]
    junk = np.where(np.arange(V) % 2 == 0, -1, N + 5).astype(np.int32)
    for r, f in enumerate(fleets):
        rows[r, f:] = junk[f:]
    return rows


def seeded_rows(g, R, same):
    V, N = int(g["V"]), int(g["N"])
    valid = g["node2cluster"] >= 0
    rows = np.empty((R, V), dtype=np.int32)
    import random
    for r in range(R):
        rows[r] = g["veh_node"][:V] if (same or r == 0) else synth.init_vehicle_nodes(random.Random(4100 + r), N, V, valid)
    return rows


def note(fleets, V):
    SEEN["fleets"] |= {("zero" if f == 0 else "one" if f == 1 else "full" if f == V else "part") for f in fleets}


def check_counters_obs(env, oracles, tag):
    ob, cn = env.obs(), env.counters()
    for r, o in enumerate(oracles):
        oo, oc = o.obs(), o.counters()
        for a, b in (("idle_pre", "idle_pre"), ("idle_now", "idle_post"), ("supply", "supply"), ("cl_orders", "cl_orders"), ("inflight", "inflight")):
            np.testing.assert_array_equal(ob[a][r], oo[b], err_msg="%s replica %d obs %s" % (tag, r, a))
        for i, k in enumerate(("order_num", "reject_num", "matched", "wait_sum", "dispatch_num", "dispatch_cost")):
            assert cn[r, i] == oc[k], (tag, r, k, cn[r, i], oc[k])
        assert cn[r, 7] == oc["evals"], (tag, r, "evals")
    return ob, cn


def check_state(env, oracles, fleets, tag):
    for r, o in enumerate(oracles):
        check_fleet_lists(env.lists(r), env.vehicles(r), o, fleets[r], env.V, env.C, "%s replica %d (fleet %d)" % (tag, r, fleets[r]))


def check_orders(env, oracles, tag):
    od = env.orders()
    for r, o in enumerate(oracles):
        oo = o.orders()
        n = oo["status"].size
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(od[k][r][:n], oo[k], err_msg="%s replica %d %s" % (tag, r, k))
    return od


# ---- 1. day walks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_kmeans", "tiny_kmeans_dfs2", "tiny_dispatch"])
def test_day_walk_every_slot_against_each_replicas_oracle(name):
    g = load_golden(name)
    V, N = int(g["V"]), int(g["N"])
    fleets = standard_fleets(V)
    R = len(fleets)
    disp = dispatch_by_tick(g)
    rows = seeded_rows(g, R, same=True)             # one row for all: fleet_expect.TINY_REJECTS says what each size rejects
    env = make_env(g, R)
    env.set_fleet(fleets)
    assert env.fleet.tolist() == fleets
    env.reset(pad_rows(rows, fleets, N))
    oracles = [fleet_oracle(g, f, rows[r]) for r, f in enumerate(fleets)]
    note(fleets, V)
    check_state(env, oracles, fleets, name + " after reset")
    assert env.T == int(g["n_ticks"])
    moved = 0
    for t in range(env.T):
        env.step()
        for o in oracles:
            o.begin_tick()
        tag = "%s slot %d" % (name, t)
        ob, cn = check_counters_obs(env, oracles, tag)
        check_state(env, oracles, fleets, tag)
        np.testing.assert_array_equal(ob["supply"][0], g["t_supply"][t])          # replica 0 also against the reference's record
        np.testing.assert_array_equal(ob["idle_now"][0], g["t_idle_post"][t])
        assert cn[0, 0] == g["t_order_num"][t] and cn[0, 1] == g["t_reject_num"][t] and cn[0, 3] == g["t_wait_sum"][t]
        if t in disp:
            # the reference's dispatch log, applied to every replica whose fleet holds the vehicle (and has it idle)
            log = np.array(disp[t])
            a_rep, a_cl, a_pos, a_tgt = [], [], [], []
            for r, o in enumerate(oracles):
                idle = idle_mask(o)
                L = o.lists()
                ids, tg = [], []
                for veh, tgt in zip(log[:, 1], log[:, 4]):
                    if veh < fleets[r] and idle[veh]:
                        cl = int(np.searchsorted(L["idle_off"], np.flatnonzero(L["idle_veh"][:L["idle_off"][-1]] == veh)[0], side="right") - 1)
                        seg = L["idle_veh"][L["idle_off"][cl]:L["idle_off"][cl + 1]]
                        a_rep.append(r); a_cl.append(cl); a_pos.append(int(np.flatnonzero(seg == veh)[0])); a_tgt.append(int(tgt))
                        ids.append(int(veh)); tg.append(int(tgt))
                assert r != 0 or len(ids) == len(log)
                # (positions refer to the lists as they stand when the call is made: one call for all replicas below)
                if ids:
                    o.dispatch(np.array(ids), np.array(tg))
                    moved += len(ids) if r else 0
            env.apply_dispatch(a_rep, a_cl, a_pos, a_tgt)
            check_state(env, oracles, fleets, tag + " after dispatch")
            np.testing.assert_array_equal(env.obs()["idle_now"][0], g["t_idle_after_dispatch"][t])
        env.advance()
        for o in oracles:
            o.end_tick()
    env.sync()
    od = check_orders(env, oracles, name)
    for k in ("status", "vehicle", "wait"):
        np.testing.assert_array_equal(od[k][0], g["o_" + k])
    cn = env.counters()
    assert cn[0, 1] == int(g["reject_num"]) and cn[5, 1] == cn[0, 1]
    if not disp:
        assert cn[:, 1].tolist() == [TINY_REJECTS[name][f] for f in fleets]  # five fleet sizes, five reject counts
        assert len(set(cn[:5, 1].tolist())) == 5
    assert cn[1, 1] == cn[1, 0] > 0 and cn[1, 2] == 0                        # the replica without vehicles rejects every order
    SEEN["all_rejected"] += 1
    if disp:
        assert moved > 0                                                     # the log moved vehicles of the smaller fleets too
    env.close()


@pytest.mark.parametrize("kernel,name,kw", FAMILIES, ids=["%s-%s-%d" % (k, n, i) for i, (k, n, _) in enumerate(FAMILIES)])
def test_end_of_day_through_every_tick_family(kernel, name, kw):
    g = load_golden(name)
    V, N = int(g["V"]), int(g["N"])
    fleets = standard_fleets(V)
    R = len(fleets)
    rows = seeded_rows(g, R, same=False)
    env = make_env(g, R, **kw)
    assert env.main_kernel() == kernel
    env.set_fleet(fleets)
    env.reset(pad_rows(rows, fleets, N))
    oracles = [fleet_oracle(g, f, rows[r]) for r, f in enumerate(fleets)]
    for t in range(env.T):
        env.step(); env.advance()
        for o in oracles:
            o.begin_tick(); o.end_tick()
    env.sync()
    tag = "%s %s end of day" % (kernel, name)
    check_state(env, oracles, fleets, tag)
    check_orders(env, oracles, tag)
    cn = env.counters()
    for r, o in enumerate(oracles):
        oc = o.counters()
        for i, k in enumerate(("order_num", "reject_num", "matched", "wait_sum")):
            assert cn[r, i] == oc[k], (tag, r, k)
        assert cn[r, 6] == oc["sum_order_value"] and cn[r, 7] == oc["evals"], (tag, r)
    env.close()


# ---- 2. the fleets the reference ran -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(fleet_runs()))
def test_every_replica_equals_the_references_own_record(case):
    sizes = fleet_runs()[case]
    fleets = sizes if len(sizes) >= 6 else sizes + sizes            # R = 6 .. 8
    top = load_fleet(case, sizes[-1])
    V, N = sizes[-1] + 37, int(top["N"])
    R = len(fleets)
    rows = np.zeros((R, V), dtype=np.int32)
    rows[:, :sizes[-1]] = top["veh_node"]
    env = make_env(dict(top, V=np.int64(V)), R)
    env.set_fleet(fleets)
    env.reset(pad_rows(rows, fleets, N))
    note(fleets, V)
    rec = [load_fleet(case, f) for f in fleets]
    assert env.T == int(top["n_ticks"])
    for t in range(env.T):
        env.step()
        ob, cn = env.obs(), env.counters()
        for r, g in enumerate(rec):
            tag = "%s VehiclesNumber %d slot %d" % (case, fleets[r], t)
            assert cn[r, 0] == g["t_order_num"][t] and cn[r, 1] == g["t_reject_num"][t] and cn[r, 3] == g["t_wait_sum"][t], tag
            for a, b in (("idle_pre", "t_idle_pre"), ("idle_now", "t_idle_post"), ("supply", "t_supply"), ("cl_orders", "t_cl_orders"), ("inflight", "t_inflight")):
                np.testing.assert_array_equal(ob[a][r], g[b][t], err_msg=tag + " " + a)
            if t % 4 == 0:
                G = env.lists(r)
                n, na = int(g["l_idle_off"][t][-1]), int(g["l_arr_off"][t][-1])
                assert n + na == fleets[r], tag
                np.testing.assert_array_equal(G["idle_off"], g["l_idle_off"][t], err_msg=tag)
                np.testing.assert_array_equal(G["idle_veh"][:n], g["l_idle_veh"][t][:n], err_msg=tag)
                np.testing.assert_array_equal(G["arr_off"], g["l_arr_off"][t], err_msg=tag)
                np.testing.assert_array_equal(G["arr_veh"][:na], g["l_arr_veh"][t][:na], err_msg=tag)
                np.testing.assert_array_equal(G["arr_min"][:na], g["l_arr_min"][t][:na], err_msg=tag)
        env.advance()
    env.sync()
    od, cn = env.orders(), env.counters()
    for r, g in enumerate(rec):
        for k in ("status", "vehicle", "wait"):                              # per-order vehicle included
            np.testing.assert_array_equal(od[k][r], g["o_" + k], err_msg="%s VehiclesNumber %d %s" % (case, fleets[r], k))
        assert cn[r, 1] == int(g["reject_num"]) and cn[r, 6] == int(g["sum_order_value"])
        if fleets[r] == 0:
            assert cn[r, 1] == cn[r, 0]
            SEEN["all_rejected"] += 1
    env.close()


# ---- 3. reset forms ----------------------------------------------------------------------------------------------------------------------
SEG_V = 2100                   # seg = 192: wave ranges [0, 192), [192, 384) ... of k_reset_fast / k_reset_staged
SEG_FLEETS = [0, 1, 63, 64, 65, 191, 192, 193, 2047, 2048, 2049, 2099, 2100]


def start_list_check(env, n2c, rows, fleets, tag):
    for r, f in enumerate(fleets):
        off, veh, node = expected_start_lists(n2c, env.C, rows[r], f)
        G = env.lists(r)
        t = "%s replica %d (fleet %d)" % (tag, r, f)
        np.testing.assert_array_equal(G["idle_off"], off, err_msg=t)
        np.testing.assert_array_equal(G["idle_veh"][:f], veh, err_msg=t)
        np.testing.assert_array_equal(G["idle_node"][:f], node, err_msg=t)
        assert (G["idle_veh"][f:] == -1).all() and G["arr_off"][-1] == 0, t


@pytest.mark.parametrize("form", ["default", "unstaged", "host_checks"])
def test_lists_right_after_the_reset_on_both_sides_of_every_wave_segment(form, monkeypatch):
    if form == "unstaged":
        monkeypatch.setenv("VDS_RESET_UNSTAGED", "1")
    if form == "host_checks":
        monkeypatch.setenv("VDS_RESET_HOST_CHECKS", "1")
    g = dict(load_golden("tiny_kmeans"))
    g["V"] = np.int64(SEG_V)
    N = int(g["N"])
    seg = (((SEG_V + 15) // 16) + 63) // 64 * 64
    assert seg == 192
    fleets = SEG_FLEETS + SEG_FLEETS[::-1] + [SEG_V] * 3         # each on two replicas at least, in two positions of a group of 16
    R = len(fleets)
    valid = np.flatnonzero(g["node2cluster"] >= 0)
    rows = valid[np.random.default_rng(77).integers(0, valid.size, size=(R, SEG_V))].astype(np.int32)
    env = make_env(g, R)
    env.set_fleet(fleets)
    env.reset(pad_rows(rows, fleets, N))
    start_list_check(env, g["node2cluster"], rows, fleets, form)
    env.reset_again()
    start_list_check(env, g["node2cluster"], rows, fleets, form + " again")
    env.close()
    note(fleets, SEG_V)
    for f in fleets:
        for edge in (seg, 2 * seg):
            if f in (edge - 1, edge, edge + 1):
                SEEN["seg_sides"].add(("below" if f < edge else "at" if f == edge else "above"))


def test_image_form_of_a_city_too_large_for_the_staged_reset():
    """30 000 vehicles in 37 clusters (k_reset_fast + k_reset_capture, then k_reset_image): the image holds the lists of the fleets."""
    N, Cn, V, R = 700, 37, 30000, 3
    w = workloads.tiny(N=N, C=Cn, vehicles=V, orders=1500, seed=5)
    rows = w.vehicle_nodes(R)
    n2c = np.asarray(w.city.node2cluster)
    env = w.make_env(R)
    fleets = [30000, 29999, 5]
    env.set_fleet(fleets)
    env.reset(pad_rows(rows, fleets, N)); start_list_check(env, n2c, rows, fleets, "image reset")
    for k in range(2):
        env.reset_again(); start_list_check(env, n2c, rows, fleets, "image again %d" % k)
    fleets = [5, 30000, 29999]
    env.set_fleet(fleets)
    with pytest.raises(Exception, match="vds_reset_again"):
        env.reset_again()
    env.reset(pad_rows(rows, fleets, N)); start_list_check(env, n2c, rows, fleets, "image second map")
    env.reset_again(); start_list_check(env, n2c, rows, fleets, "image second map again")
    env.run(3)
    cn = env.counters()
    assert cn[0, 2] <= 5 * 3 and cn[1, 2] > cn[0, 2]               # five vehicles serve at most five orders a slot
    env.close()
    note(fleets, V)


# ---- 4. reset_random ---------------------------------------------------------------------------------------------------------------------
def lopsided_city():
    """tiny_kmeans with clusters 6 .. 11 folded into cluster 0: more than half of all start nodes land in one list."""
    g = dict(load_golden("tiny_kmeans"))
    n2c = g["node2cluster"].copy()
    n2c[n2c >= 6] = 0
    g["node2cluster"] = n2c
    g["V"] = np.int64(SEG_V)
    return g


def run_reset_random_case():
    g = lopsided_city()
    V, N, R = SEG_V, int(g["N"]), 7
    seeds = [11, 2**33 + 5, 7, 8, 9, 10, 12]
    valid = g["node2cluster"] >= 0
    full = np.stack([workloads.native_vehicle_nodes(s, N, V, 1, None if valid.all() else valid)[0] for s in seeds])
    r_up = lambda x: (x + 63) // 64 * 64
    env = make_env(g, R)
    cap0 = env.idle_cap
    want_full = min(r_up(V), r_up(2 * int(np.bincount(g["node2cluster"][full[0]]).max()) + 64))
    assert want_full > cap0                                           # (a reset at V would regrow the tables)
    for fleets in ([0] * R, [0, 0, 0, 0, 1000, 0, 0], [V, 0, 1, 63, 64, 65, V - 1]):
        env.set_fleet(fleets)
        env.reset_random(seeds)
        start_list_check(env, g["node2cluster"], full, fleets, "reset_random %s" % fleets[:5])
        fullest = max(int(np.bincount(g["node2cluster"][full[r][:f]], minlength=1).max()) if f else 0 for r, f in enumerate(fleets))
        want = min(r_up(V), r_up(2 * fullest + 64))
        assert env.idle_cap == max(cap0, want), (fleets, env.idle_cap, cap0, want)
        if max(fleets) == 0:
            assert env.idle_cap == cap0
        elif max(fleets) == 1000:
            assert cap0 < env.idle_cap < want_full                    # sized from the fleets as they are, not from V
        cap0 = env.idle_cap
        note(fleets, V)
    # the same lists as reset with the prefix nodes, and the same day
    env.run(6)
    a = (env.orders(), env.counters().copy())
    env.reset(pad_rows(full, fleets, N))
    start_list_check(env, g["node2cluster"], full, fleets, "reset with the prefix nodes")
    env.run(6)
    b = (env.orders(), env.counters().copy())
    for k in ("status", "vehicle", "wait"):
        np.testing.assert_array_equal(a[0][k], b[0][k])
    np.testing.assert_array_equal(a[1], b[1])
    env.close()


def test_reset_random_draws_the_prefix_and_sizes_the_tables_from_the_fleets():
    run_reset_random_case()


# ---- 5. reset_torch ----------------------------------------------------------------------------------------------------------------------
def test_reset_torch_is_reset_from_a_device_tensor():
    import torch
    g = load_golden("tiny_kmeans")
    V, N = int(g["V"]), int(g["N"])
    fleets = standard_fleets(V)
    R = len(fleets)
    rows = seeded_rows(g, R, same=False)
    padded = pad_rows(rows, fleets, N)
    stream = torch.cuda.current_stream()
    a, b = make_env(g, R, stream=stream.cuda_stream), make_env(g, R)
    for e in (a, b):
        e.set_fleet(fleets)
    a.reset_torch(torch.from_numpy(padded).cuda())
    b.reset(padded)
    assert a.idle_cap == b.idle_cap and a.clock == b.clock
    for r in range(R):
        A, B = a.lists(r), b.lists(r)
        for k in A:
            np.testing.assert_array_equal(A[k], B[k], err_msg="replica %d %s" % (r, k))
    b.close()
    # an offender inside a fleet: refused naming vehicle and node; the previous nodes still restart
    bad = padded.copy()
    bad[3, 5] = N + 9
    with pytest.raises(Exception, match=r"vehicle %d starts on node %d which is in no cluster" % (3 * V + 5, N + 9)):
        a.reset_torch(torch.from_numpy(bad).cuda())
    bad[3, 5] = -1
    with pytest.raises(Exception, match=r"vehicle %d starts on node -1" % (3 * V + 5)):
        a.reset_torch(torch.from_numpy(bad).cuda())
    a.reset_again()
    oracles = [fleet_oracle(g, f, rows[r]) for r, f in enumerate(fleets)]
    check_state(a, oracles, fleets, "reset_again after a refused reset_torch")
    # an offender beyond the fleet is accepted (row 3 has V // 2 vehicles)
    ok = padded.copy()
    ok[3, V // 2] = N + 9
    a.reset_torch(torch.from_numpy(ok).cuda())
    check_state(a, oracles, fleets, "offender beyond the fleet")
    # day one, then day two from where the vehicles ended: the node plane of the handle's own block as the source
    a.run(a.T)
    a.sync()
    for o in oracles:
        for _ in range(a.T):
            o.begin_tick(); o.end_tick()
    end = a.vehicles_all()["node"].copy()
    for r, f in enumerate(fleets):
        assert (end[r, f:] == -1).all() and (end[r, :f] >= 0).all()
    a.reset_torch(a.vehicles_torch(state=False, node=True, cluster=False, arrive_min=False, order=False)["node"])
    day2 = [fleet_oracle(g, f, end[r]) for r, f in enumerate(fleets)]
    check_state(a, day2, fleets, "day two after reset")
    for t in range(a.T):
        a.step(); a.advance()
        for o in day2:
            o.begin_tick(); o.end_tick()
    a.sync()
    check_state(a, day2, fleets, "day two end")
    check_orders(a, day2, "day two")
    assert not np.array_equal(end[0], rows[0])
    # wrong arguments are refused by the wrapper
    for wrong in (torch.from_numpy(padded), torch.from_numpy(padded.astype(np.int64)).cuda(), torch.from_numpy(padded[:, :-1].copy()).cuda()):
        with pytest.raises(Exception, match="reset_torch"):
            a.reset_torch(wrong)
    with pytest.raises(Exception, match="null veh_init_node"):
        a._chk(a._lib.vds_reset_device(a._h, None))
    a.close()
    note(fleets, V)


def test_reset_torch_without_vehicles():
    import torch
    g = dict(load_golden("tiny_kmeans"))
    g["V"] = np.int64(0)
    env = make_env(g, 3)
    env.reset_torch(torch.empty((3, 0), dtype=torch.int32, device="cuda"))
    assert env._lib.vds_reset_device(env._h, None) == 0               # V == 0: the pointer is not looked at
    assert env.fleet.tolist() == [0, 0, 0]
    env.run(env.T)
    cn = env.counters()
    assert (cn[:, 1] == cn[:, 0]).all() and cn[0, 0] > 0
    env.close()


# ---- 6. derived blocks and the tensor dispatch forms -------------------------------------------------------------------------------------
def test_derived_blocks_and_dispatch_forms_at_every_slot():
    import torch
    g = load_golden("tiny_kmeans")
    V, N, Cn = int(g["V"]), int(g["N"]), int(g["C"])
    n2c = g["node2cluster"]
    fleets = standard_fleets(V)
    R = len(fleets)
    rows = seeded_rows(g, R, same=False)
    env = make_env(g, R, stream=torch.cuda.current_stream().cuda_stream)
    env.set_fleet(fleets)
    env.reset(pad_rows(rows, fleets, N))
    oracles = [fleet_oracle(g, f, rows[r]) for r, f in enumerate(fleets)]
    value = g["cost"][g["o_delivery"].astype(np.int64), g["o_pickup"].astype(np.int64)]
    L_heads = 4
    tgt_nodes = np.flatnonzero(n2c >= 0)
    moves = dict(vehicle=0, roster=0)
    for t in range(env.T):
        before = [o.orders()["status"].copy() for o in oracles]
        env.step()
        for o in oracles:
            o.begin_tick()
        tag = "slot %d" % t
        planes = env.vehicles_all(source=True)
        vo = env.vehicle_outcomes()
        vrows = np.stack([vo[k] for k in ("order", "wait", "value", "pickup")], axis=-1)
        ros = env.idle_roster()
        heads = env.idle_heads(L_heads)
        blk = env.orders_torch().cpu().numpy()
        oc = env.outcomes()
        served, wait, val = slot_sums(vrows)
        np.testing.assert_array_equal(served, oc["served"].sum(axis=1), err_msg=tag)          # the two sum checks of include/vds.h
        np.testing.assert_array_equal(wait, oc["wait_sum"].sum(axis=1), err_msg=tag)
        np.testing.assert_array_equal(val, oc["value_sum"].sum(axis=1), err_msg=tag)
        for r, (o, f) in enumerate(zip(oracles, fleets)):
            rt = "%s replica %d" % (tag, r)
            W = host_view(env, r)
            check_fleet_lists(env.lists(r), env.vehicles(r), o, f, V, Cn, rt)
            for k in ("state", "node", "cluster", "arrive_min", "order"):
                np.testing.assert_array_equal(planes[k][r], W[k], err_msg=rt + " plane " + k)
            for k in planes:
                assert (planes[k][r, f:] == -1).all(), (rt, k)                                # absent: -1 in all six planes
            assert (planes["source"][r, :f] >= 0).all(), rt
            oo = o.orders()
            exp = processed_rows(before[r], oo["status"], g["o_pickup"], oo["vehicle"], oo["wait"], value, max(f, 1))[:f]
            np.testing.assert_array_equal(vrows[r, :f], exp, err_msg=rt + " vehicle outcomes")
            assert (vrows[r, f:] == -1).all(), rt
            Lo = o.lists()
            n = int(Lo["idle_off"][-1])
            np.testing.assert_array_equal(ros["off"][r], Lo["idle_off"], err_msg=rt + " roster off")
            np.testing.assert_array_equal(ros["veh"][r, :n], Lo["idle_veh"][:n], err_msg=rt + " roster veh")
            np.testing.assert_array_equal(ros["node"][r, :n], o.vehicles()["loc"][Lo["idle_veh"][:n]], err_msg=rt)
            np.testing.assert_array_equal(ros["cluster"][r, :n], np.repeat(np.arange(Cn), np.diff(Lo["idle_off"])), err_msg=rt)
            for k in ("veh", "node", "cluster"):
                assert (ros[k][r, n:] == -1).all(), (rt, k)                                   # from off[r][C] on: -1
            for c in range(Cn):
                seg = Lo["idle_veh"][Lo["idle_off"][c]:Lo["idle_off"][c + 1]][:L_heads]
                np.testing.assert_array_equal(heads["veh"][r, c, :seg.size], seg, err_msg=rt + " heads")
                assert (heads["veh"][r, c, seg.size:] == -1).all(), rt
            st = oo["status"]
            np.testing.assert_array_equal(blk[r, :, 0][st == 1], oo["vehicle"][st == 1], err_msg=rt + " orders block")
            assert (blk[r, :, 0][st == 2] == -1).all() and (blk[r, :, 0][st == 0] == -2).all(), rt
            np.testing.assert_array_equal(blk[r, :, 1][st == 1], oo["wait"][st == 1], err_msg=rt)
        if t % 3 == 0:
            # the vehicle form: non-negative targets for absent vehicles too - they are "not idle", no error
            tg = np.full((R, V), -1, dtype=np.int32)
            tg[:, (t // 3) % 5::5] = tgt_nodes[(t * 7) % tgt_nodes.size]
            env.apply_dispatch_vehicles_torch(torch.from_numpy(tg).cuda())
            for r, (o, f) in enumerate(zip(oracles, fleets)):
                n, refused = oracle_apply_vehicles(o, tg[r, :f], n2c)
                assert not any(refused.values())
                moves["vehicle"] += n
            env.sync()                                                                        # (no sticky error)
        elif t % 3 == 1:
            env.idle_roster_torch()                                                           # a fresh roster (nothing moved since)
            tg = np.full((R, V), -1, dtype=np.int32)
            tg[:, ::4] = tgt_nodes[(t * 11) % tgt_nodes.size]                                 # also positions beyond off[r][C]
            env.apply_dispatch_roster_torch(torch.from_numpy(tg).cuda())
            for r, o in enumerate(oracles):
                Lo = o.lists()
                n = int(Lo["idle_off"][-1])
                ids = Lo["idle_veh"][:n][::4]
                if ids.size:
                    o.dispatch(ids, tg[r, :n][::4])
                moves["roster"] += int(ids.size)
            env.sync()
        if t % 3 != 2:
            check_state(env, oracles, fleets, tag + " after dispatch")
        env.advance()
        for o in oracles:
            o.end_tick()
    assert moves["vehicle"] > 0 and moves["roster"] > 0
    env.sync()
    check_orders(env, oracles, "derived blocks day")
    cn = env.counters()
    for r, o in enumerate(oracles):
        assert cn[r, 4] == o.counters()["dispatch_num"] and cn[r, 1] == o.counters()["reject_num"]
    assert cn[1, 4] == 0 and cn[1, 1] == cn[1, 0]
    env.close()
    note(fleets, V)


# ---- 7. day graphs -----------------------------------------------------------------------------------------------------------------------
def test_day_graphs_replay_with_another_map():
    import torch
    g = load_golden("tiny_kmeans")
    V, N, n2c = int(g["V"]), int(g["N"]), g["node2cluster"]
    R = 6
    rows = seeded_rows(g, R, same=False)
    env = make_env(g, R, stream=torch.cuda.current_stream().cuda_stream)
    tg = np.full((R, V), -1, dtype=np.int32)
    tg[:, ::17] = int(np.flatnonzero(n2c >= 0)[3])                    # a few vehicles go back to one node whenever they are idle
    tg_dev = torch.from_numpy(tg).cuda()
    veh = None
    for fleets in (standard_fleets(V), [2, V, V - 1, 0, 37, 75]):
        env.set_fleet(fleets)
        padded = pad_rows(rows, fleets, N)
        # run(T): the hook-less day graph
        env.reset(padded)
        env.run(env.T)
        env.sync()
        oracles = [fleet_oracle(g, f, rows[r]) for r, f in enumerate(fleets)]
        for o in oracles:
            for _ in range(env.T):
                o.begin_tick(); o.end_tick()
        check_state(env, oracles, fleets, "run %s" % fleets)
        check_orders(env, oracles, "run %s" % fleets)
        rejects = env.counters()[:, 1].tolist()
        assert rejects == [o.counters()["reject_num"] for o in oracles]
        # run_hooked with vehicle planes and per-vehicle targets: the second map replays the graph of the first
        env.reset(padded)
        if veh is None:
            veh = env.vehicles_torch()
        env.run_hooked(env.T, vehicle_planes=dict(state=True, node=True, cluster=True, arrive_min=True, order=True), vehicle_targets=tg_dev)
        env.sync()
        oracles = [fleet_oracle(g, f, rows[r]) for r, f in enumerate(fleets)]
        last = None
        for t in range(env.T):
            for r, (o, f) in enumerate(zip(oracles, fleets)):
                o.begin_tick()
                if t == env.T - 1 and r == 0:
                    last = idle_mask(o)[:f].copy()
                oracle_apply_vehicles(o, tg[r, :f], n2c)
                o.end_tick()
        check_state(env, oracles, fleets, "run_hooked %s" % fleets)
        check_orders(env, oracles, "run_hooked %s" % fleets)
        cn = env.counters()
        for r, o in enumerate(oracles):
            assert cn[r, 4] == o.counters()["dispatch_num"] and cn[r, 1] == o.counters()["reject_num"], (fleets, r)
        got = {k: v.cpu().numpy() for k, v in veh.items()}                   # the planes of the last slot, before its dispatch
        for r, f in enumerate(fleets):
            for k in got:
                assert (got[k][r, f:] == -1).all(), (fleets, r, k)
        np.testing.assert_array_equal(got["state"][0, :fleets[0]] == 0, last)
        note(fleets, V)
    env.close()


# ---- 8. storage forms --------------------------------------------------------------------------------------------------------------------
def test_order_days_per_replica_stored_regrouped_with_fleets_by_the_callers_index():
    g = load_golden("tiny_kmeans")
    V, N, R = int(g["V"]), int(g["N"]), 40
    days = synth_days(g, 3, seed=6100)
    replica_day = (np.arange(R) % 3).astype(np.int32)
    fleets = [[V, 0, 1, V // 2, V - 1][r % 5] for r in range(R)]
    import random
    valid = g["node2cluster"] >= 0
    starts = [synth.init_vehicle_nodes(random.Random(6200 + k), N, V, valid) for k in range(2)]
    rows = np.stack([starts[r % 2] for r in range(R)]).astype(np.int32)
    env = mk_env(g, R)
    env.load_order_days(days, replica_day)
    with pytest.raises(Exception, match="regrouped"):
        env.obs_inplace_torch()                                        # 40 replicas stored as 3 x 16
    env.set_fleet(fleets)
    env.reset(pad_rows(rows, fleets, N))
    oracles = {}
    for r in range(R):
        key = (int(replica_day[r]), r % 2, fleets[r])
        if key not in oracles:
            d = days[key[0]]
            oracles[key] = fleet_oracle(dict(g, o_release_min=d[0], o_pickup=d[1], o_delivery=d[2]), fleets[r], rows[r])
    per = [oracles[(int(replica_day[r]), r % 2, fleets[r])] for r in range(R)]
    check_state(env, per, fleets, "days after reset")
    env.run(env.T)
    env.sync()
    for o in oracles.values():
        for _ in range(o.num_ticks):
            o.begin_tick(); o.end_tick()
    check_state(env, per, fleets, "days end")
    check_orders(env, per, "days")
    cn = env.counters()
    for r, o in enumerate(per):
        assert cn[r, 1] == o.counters()["reject_num"] and cn[r, 0] == o.counters()["order_num"], r
    # the map survives another replica -> day map
    env.set_replica_days(((np.arange(R) + 1) % 3).astype(np.int32))
    assert env.fleet.tolist() == fleets
    env.close()
    note(fleets, V)


# ---- 9. snapshot and restore -------------------------------------------------------------------------------------------------------------
def test_snapshot_restore_through_a_permutation_and_set_fleet_voids_it():
    g = load_golden("tiny_kmeans")
    V, N = int(g["V"]), int(g["N"])
    fleets = standard_fleets(V)
    R = len(fleets)
    rows = seeded_rows(g, R, same=False)
    env = make_env(g, R)
    env.set_fleet(fleets)
    env.reset(pad_rows(rows, fleets, N))
    oracles = [fleet_oracle(g, f, rows[r]) for r, f in enumerate(fleets)]
    for t in range(20):
        env.step(); env.advance()
        for o in oracles:
            o.begin_tick(); o.end_tick()
    env.snapshot()
    at = [fleet_oracle(g, f, rows[r]) for r, f in enumerate(fleets)]
    for o in at:
        for _ in range(20):
            o.begin_tick(); o.end_tick()
    for _ in range(3):
        env.step(); env.advance()
    perm = [3, 0, 4, 1, 5, 2]
    env.restore(perm)
    check_state(env, [at[s] for s in perm], [fleets[s] for s in perm], "after restore")      # replica r shows src[r]'s vehicles
    assert env.fleet.tolist() == fleets                                                       # ... the parameter is unchanged
    env.step()
    for o in at:
        o.begin_tick()
    check_state(env, [at[s] for s in perm], [fleets[s] for s in perm], "a step after the restore")
    check_counters_obs(env, [at[s] for s in perm], "a step after the restore")
    env.set_fleet(fleets[::-1])
    assert env.snapshot_info() is None
    with pytest.raises(Exception):
        env.restore()
    env.close()
    note(fleets, V)


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_way_back_to_the_default():
    g = load_golden("tiny_kmeans")
    V, N, R = int(g["V"]), int(g["N"]), 6
    rows = seeded_rows(g, R, same=False)
    env = make_env(g, R)
    assert env.fleet.tolist() == [V] * R
    env.reset(rows)
    for bad, where in (([V, -1, 0, 0, 0, 0], "replica 1"), ([0, 0, 0, 0, V + 1, 0], "replica 4")):
        with pytest.raises(Exception, match="vds_set_fleet: %s" % where):
            env.set_fleet(bad)
    env.reset_again()                                                  # a refused map changes nothing
    env.set_fleet([V] * R)                                             # V everywhere: stored as "none" ...
    assert env.fleet.tolist() == [V] * R
    with pytest.raises(Exception, match="vds_reset_again"):            # ... and still a new parameter: a reset must follow
        env.reset_again()
    with pytest.raises(Exception, match="call vds_reset first"):
        env.step()
    fleets = standard_fleets(V)
    env.set_fleet(fleets)
    with pytest.raises(Exception, match="vds_reset_again"):
        env.reset_again()
    env.reset(rows)
    env.run(env.T)
    with_map = env.counters()[:, 1].copy()
    env.set_fleet(None)
    assert env.fleet.tolist() == [V] * R
    with pytest.raises(Exception, match="vds_reset_again"):
        env.reset_again()
    env.reset(rows)
    env.run(env.T)
    a = (env.orders(), env.counters().copy(), [env.lists(r) for r in range(R)])
    env.close()
    plain = make_env(g, R)                                             # a handle that never had a map
    plain.reset(rows)
    plain.run(plain.T)
    b = (plain.orders(), plain.counters().copy(), [plain.lists(r) for r in range(R)])
    plain.close()
    for k in ("status", "vehicle", "wait"):
        np.testing.assert_array_equal(a[0][k], b[0][k])
    np.testing.assert_array_equal(a[1], b[1])
    for la, lb in zip(a[2], b[2]):
        for k in la:
            np.testing.assert_array_equal(la[k], lb[k])
    assert with_map[0] == a[1][0, 1] and with_map[1] > with_map[3] > with_map[0]
    note(fleets, V)


# ---- 11. memory --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target,lib,fill", [("dirty", "libvds_dirty.so", None), ("dirty", "libvds_dirty.so", "5A"), ("canary", "libvds_canary.so", None)])
def test_nobody_reads_behind_a_fleet_on_dirty_and_guarded_memory(target, lib, fill):
    """With a map, reset_random leaves the start nodes unwritten behind each fleet: only a build whose memory starts out dirty (or
    poisoned) can show that nobody reads them.  One day walk and the reset_random test in a pytest process of their own."""
    from test_gpu_debug_builds import build
    from test_gpu_dirty_memory import dirty_env, gpu_allowed, run_limited
    gpu_allowed()
    env = dirty_env(fill, build(target, lib))
    me = os.path.abspath(__file__)
    argv = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", me + "::test_day_walk_every_slot_against_each_replicas_oracle[tiny_kmeans]",
            me + "::test_reset_random_draws_the_prefix_and_sizes_the_tables_from_the_fleets"]
    rc, out = run_limited(argv, env, 600, "the fleet walks under %s (fill %s)" % (lib, fill or "default"))
    assert rc == 0 and "2 passed" in out, out[-4000:]


# ---- 12. coverage ------------------------------------------------------------------------------------------------------------------------
def test_the_cases_met_what_they_were_chosen_for():
    """Asserted over what the tests above recorded in this process (they run first: file order)."""
    assert {"zero", "one", "full", "part"} <= SEEN["fleets"], SEEN
    assert {"below", "at", "above"} <= SEEN["seg_sides"], SEEN           # a fleet on both sides of a wave-segment edge (and on it)
    assert SEEN["all_rejected"] >= 2, SEEN                               # a replica whose every order is rejected
