"""The tail of k_tick_dense's fast path (``vds_tick_dense.hip`` ``dense_body``): the merged list in the row's LDS table in every case,
the results ahead of the compaction, the winners' entries read from that table.  Small cities (8 clusters of 16 nodes, 12 slots, 64
replicas, one shared day) whose two probe clusters hold a list of a chosen length per replica - grouped so that every wavefront
runs the table size under test - and receive orders in bursts of 0 / 1 / 8 / 9 / 16 / 17 / 64; vehicles arrive in them from a feed
cluster in some replicas only, so the same bucket is merged with and without arrivals.  Every replica is compared with the oracle
after every slot (planes, counters, idle lists in list order, arrival tables) and at the end of the day (orders), in the 8-lane form,
with the forms mixed per (slot, cluster) and in the 16-lane form with 256-entry tables.  ``test_cities_hit_the_edges`` checks on the
oracle alone - no GPU - that the cities really contain the cases the kernel can get wrong."""
import hashlib
import os
import random

import numpy as np
import pytest

import threshold_cities as tc
from helpers import load_golden, make_oracle
from oracle.oracle import COUNTER_NAMES
from test_gpu_parity import check_lists
from vehicles_dispatch_simulator_amd import BatchedDispatchEnv, synth
from vehicles_dispatch_simulator_amd.env import neighbors_to_csr

R = 64
SLOTS = 12
NC = 16                       # nodes per cluster
PROBES, FEED = (0, 2), 1      # clusters whose lists are sized per replica; cluster the arriving vehicles come from
EQ, MIX = 0, 1                # local pickup nodes of a probe cluster: every cost equal / costs 0 and `hi` alternating
# `hi`: 20 - every order keeps its static arrival slot (the flagship forms) - or 254, next to the dead value 255: the day's orders
# then go through the arrival ring (an arrival window of 26 slots is wider than the static slots take)
HIS = (20, 254)
FAST, SLOW = 5, 9             # local delivery nodes of the feed orders: arrival in slot 3 / slot 5
# orders per slot of the probe clusters (slot t takes the releases of the ten minutes up to its own; the feed orders go in slot 1)
COUNTS = {0: [0, 0, 0, 1, 8, 9, 16, 17, 64], 2: [0, 0, 0, 64, 17, 16, 9, 8, 1]}
# list lengths (after the arrivals of slot 3) of the rows of one wavefront: every row of a wavefront in the same table size
LENGTHS = {8: [[3, 4, 5, 31, 32, 3, 5, 32], [33, 63, 64, 40, 64, 33, 63, 50], [65, 127, 128, 100, 128, 65, 127, 90]],
           16: [[129, 255, 256, 200], [3, 4, 5, 31], [32, 33, 63, 64], [65, 127, 128, 129]]}
WANTED = {8: [3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128], 16: [129, 255, 256]}
# form -> (lanes per replica the lengths are grouped for, keyword arguments, environment)
FORMS = {"lanes8": (8, {"dense_debug": (8, 0, 0, 0)}, {}),
         "mixed": (8, {}, {"VDS_DENSE_CLUSTER_SEED": "3"}),
         "lanes16": (16, {"dense_debug": (16, 0, 0, 0)}, {})}


def replica_plan(lanes):
    """(list length of the probe clusters in slot 3, whether the replica receives arrivals) per replica.  Wavefronts in pairs: one
    with arrivals in every row, one without (the table is written from the registers); in the last two, every second row."""
    rpw = 64 // lanes
    nw = R // rpw
    pat = LENGTHS[lanes]
    plan = []
    for r in range(R):
        w = r // rpw
        if w < nw - 2:
            plan.append((pat[(w // 2) % len(pat)][r % rpw], w % 2 == 0))
        else:
            plan.append((pat[w % len(pat)][r % rpw], r % 2 == 0))
    return plan


_CITIES = {}


def city(lanes, hi):
    if (lanes, hi) in _CITIES:
        return _CITIES[lanes, hi]
    cost, n2c, off = tc.block_city([NC] * 8, seed=1000 + lanes + hi)
    rng = np.random.default_rng(2000 + lanes + hi)
    cost[off[FEED]:off[FEED + 1], off[FEED]:off[FEED + 1]] = rng.integers(1, 6, size=(NC, NC))
    for c in PROBES:
        a = int(off[c])
        cost[a + EQ, a + 2:a + NC] = 7
        cost[a + MIX, a + 2:a + NC] = np.where(np.arange(NC - 2) % 2 == 0, 0, hi)
        cost[a + FAST, off[FEED]:off[FEED + 1]] = 12         # OrderValue = cost[delivery, pickup]
        cost[a + SLOW, off[FEED]:off[FEED + 1]] = 35
    np.fill_diagonal(cost, 0)
    park = np.arange(off[3], off[8])
    rel, pick, dele = [], [], []
    for c in PROBES:            # two fast and one slow arrival per probe cluster
        for d in (FAST, FAST, SLOW):
            rel.append(1); pick.append(int(off[FEED] + rng.integers(NC))); dele.append(int(off[c] + d))
    for c in PROBES:
        for t, k in enumerate(COUNTS[c]):
            for j in range(k):
                if (c, t) == (0, 3):
                    p = EQ
                elif (c, t) == (0, 4):
                    p = MIX
                else:
                    p = (EQ, MIX, int(rng.integers(2, NC)), int(rng.integers(2, NC)))[j % 4]
                rel.append((t - 1) * tc.TICK + 1 + j % 9); pick.append(int(off[c] + p)); dele.append(int(rng.choice(park)))
    for _ in range(60):
        rel.append(int(rng.integers(1, 8 * tc.TICK))); pick.append(int(rng.choice(park))); dele.append(int(rng.choice(park)))
    rel.append(8 * tc.TICK - 1); pick.append(int(park[0])); dele.append(int(park[1]))      # (the day's last order is not a probe order)
    o = np.argsort(np.array(rel), kind="stable")
    day = tuple(np.array(x, dtype=np.int32)[o] for x in (rel, pick, dele))
    plan = replica_plan(lanes)
    V = 2 * max(n for n, _ in plan) + 8
    init = np.empty((R, V), dtype=np.int32)
    for r, (n, arr) in enumerate(plan):
        n0 = n - 2 if arr else n
        row = [rng.integers(off[c] + 2, off[c] + NC, size=n0) for c in PROBES]
        row.append(rng.integers(off[FEED], off[FEED + 1], size=8 if arr else 0))
        rest = V - sum(x.size for x in row)
        row.append(off[3] + (np.arange(rest) % 5) * NC + rng.integers(0, NC, size=rest))      # spread evenly over clusters 3 .. 7
        init[r] = np.concatenate(row)
        rng.shuffle(init[r])
    c = tc.case(cost, n2c, V, day, init, plan=plan, off=off)
    _CITIES[lanes, hi] = c
    return c


def oracle_for(c, r):
    off, idx = neighbors_to_csr(c["nbr"])
    from oracle.oracle import Oracle
    o = Oracle(c["cost"], c["n2c"], off, idx, 0, False, c["rel"], c["pick"], c["dele"], c["V"], tick_minutes=tc.TICK, reject_threshold=c["threshold"])
    o.reset(c["init"][r])
    return o


def day_facts(c):
    """What the probe buckets of the city exercise, from the oracle alone.  The list a bucket is matched against is the list the slot
    before left + the vehicles that left the cluster's arrival table, in table order; a winner's position is its index in it."""
    off = c["facts"]["off"]
    slot_of, cl_of = (c["rel"] + tc.TICK - 1) // tc.TICK, c["n2c"][c["pick"]]          # (slot t opens at minute 10 t - 9: the day starts ten minutes before its first release, minute 1)
    f = dict(lens_arr=set(), lens_plain=set(), ks=set(), chunk_first=0, chunk_last=0, first=0, last=0, appended=0, emptied=0,
             outrun=0, waits=set(), eq_steps=0, k_on_empty=0)
    for r in range(R):
        o = oracle_for(c, r)
        assert o.num_ticks == SLOTS
        for t in range(SLOTS):
            before = o.lists()
            o.begin_tick()
            after, ob, od = o.lists(), o.obs(), o.orders()
            for cl in PROBES:
                prev = before["idle_veh"][before["idle_off"][cl]:before["idle_off"][cl + 1]].tolist()
                a0 = before["arr_veh"][before["arr_off"][cl]:before["arr_off"][cl + 1]].tolist()
                a1 = set(after["arr_veh"][after["arr_off"][cl]:after["arr_off"][cl + 1]].tolist())
                came = [v for v in a0 if v not in a1]
                pre = prev + came
                k = int(ob["cl_orders"][cl])
                assert len(pre) == ob["idle_pre"][cl] and k == (COUNTS[cl] + [0] * SLOTS)[t], (r, t, cl)
                if k == 0:
                    continue
                f["ks"].add(k)
                (f["lens_arr"] if came else f["lens_plain"]).add(len(pre))
                f["emptied"] += len(pre) > 0 and ob["idle_post"][cl] == 0
                f["outrun"] += k > len(pre) > 0
                f["k_on_empty"] += len(pre) == 0
                ids = np.flatnonzero((slot_of == t) & (cl_of == cl))
                taken = []
                for i in ids:
                    if od["status"][i] != 1:
                        continue
                    p = pre.index(int(od["vehicle"][i]))
                    f["waits"].add(int(od["wait"][i]))
                    f["chunk_first"] += p % 8 == 0; f["chunk_last"] += p % 8 == 7 or p % 16 == 15
                    f["first"] += p == 0; f["last"] += p == len(pre) - 1; f["appended"] += p >= len(prev)
                    if (c["pick"][ids] == off[cl] + EQ).all():          # every cost of the row equal: the lowest position left wins
                        assert p == min(set(range(len(pre))) - set(taken)), (r, t, cl, p)
                        f["eq_steps"] += 1
                    taken.append(p)
            o.end_tick()
    return f


@pytest.mark.parametrize("hi", HIS)
@pytest.mark.parametrize("lanes", [8, 16])
def test_cities_hit_the_edges(lanes, hi):
    c = city(lanes, hi)
    off = c["facts"]["off"]
    for cl in PROBES:
        a = int(off[cl])
        assert (c["cost"][a + EQ, a + 2:a + NC] == 7).all()
        row = c["cost"][a + MIX, a + 2:a + NC]
        assert set(row.tolist()) == {0, hi} and (row[:-1] != row[1:]).all()
    assert tc.in_cluster_max(c) == hi and tc.cross_cluster_max(c) <= 255
    assert c["rel"].min() == 1 and c["n2c"].max() + 1 == 8
    f = day_facts(c)
    assert set(WANTED[lanes]) <= f["lens_arr"] and set(WANTED[lanes]) <= f["lens_plain"], (sorted(f["lens_arr"]), sorted(f["lens_plain"]))
    assert f["ks"] == {1, 8, 9, 16, 17, 64}
    for key in ("chunk_first", "chunk_last", "first", "last", "appended", "emptied", "outrun", "k_on_empty", "eq_steps"):
        assert f[key] > 0, (key, f)
    assert {0, 7, hi} <= f["waits"], sorted(f["waits"])


def make_env(c, kw, environ):
    saved = {k: os.environ.get(k) for k in environ}
    os.environ.update(environ)
    try:
        off, idx = neighbors_to_csr(c["nbr"])
        env = BatchedDispatchEnv(c["cost"], c["n2c"], off, idx, replicas=R, vehicles=c["V"], depth_limit=0, neighbor_can_server=False,
                                 tick_minutes=tc.TICK, reject_threshold=c["threshold"], far_cap=c["far_cap"], **kw)
        env.load_orders(c["rel"], c["pick"], c["dele"])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return env


OBS_MAP = (("idle_pre", "idle_pre"), ("idle_now", "idle_post"), ("supply", "supply"), ("cl_orders", "cl_orders"), ("inflight", "inflight"))


@pytest.mark.gpu
@pytest.mark.parametrize("form,hi", [("lanes8", 20), ("lanes8", 254), ("mixed", 20), ("lanes16", 20), ("lanes16", 254)])
def test_every_replica_and_slot_equals_the_oracle(form, hi):
    lanes, kw, environ = FORMS[form]
    c = city(lanes, hi)
    env = make_env(c, kw, environ)
    assert env.main_kernel() == "k_tick_dense" and env.layout()["blk8"] == 1, (env.main_kernel(), env.layout())
    env.reset(c["init"])
    oracles = [oracle_for(c, r) for r in range(R)]
    assert env.T == oracles[0].num_ticks == SLOTS
    for t in range(SLOTS):
        env.step()
        ob, cn = env.obs(), env.counters()
        for r, o in enumerate(oracles):
            o.begin_tick()
            oo, oc = o.obs(), o.counters()
            for a, b in OBS_MAP:
                np.testing.assert_array_equal(ob[a][r], oo[b], err_msg="%s %d slot %d replica %d %s" % (form, hi, t, r, a))
            for i, k in enumerate(COUNTER_NAMES):
                if k != "sum_order_value":
                    assert cn[r, i] == oc[k], (form, t, r, k, int(cn[r, i]), oc[k])
            check_lists(env, r, o, t)
        env.advance()
        for o in oracles:
            o.end_tick()
    work = env.work()
    assert hi != 20 or work["slow_path_buckets"] == 0, work          # (every bucket on the fast path)
    if form == "mixed":
        per_slot = env.cluster_forms().sum(axis=1)
        assert ((per_slot > 0) & (per_slot < env.C)).any(), per_slot.tolist()

    def check_orders(tag):
        env.sync()
        od, cn = env.orders(), env.counters()
        for r, o in enumerate(oracles):
            oo, oc = o.orders(), o.counters()
            for k in ("status", "vehicle", "wait"):
                np.testing.assert_array_equal(od[k][r], oo[k], err_msg="%s %s replica %d %s" % (form, tag, r, k))
            for i, k in enumerate(COUNTER_NAMES):
                assert cn[r, i] == oc[k], (form, tag, r, k, int(cn[r, i]), oc[k])

    check_orders("stepped")
    env.reset(c["init"])
    env.run(SLOTS)          # the same day as one chain of launches
    check_orders("run")
    env.close()


@pytest.mark.gpu
def test_real_kmeans192_day_at_64_replicas():
    """One day of configs[1] at full single-replica size through vds_run: 64 replicas on four different starts."""
    g = load_golden("real_kmeans192")
    V, N = int(g["V"]), int(g["N"])
    starts = [g["veh_node"]] + [synth.init_vehicle_nodes(random.Random(500 + i), N, V) for i in range(1, 4)]
    init = np.stack([starts[r % 4] for r in range(R)]).astype(np.int32)
    env = BatchedDispatchEnv(g["cost"], g["node2cluster"], g["nbr_off"], g["nbr_idx"], replicas=R, vehicles=V,
                             depth_limit=int(g["depth_limit"]), neighbor_can_server=bool(g["neighbor_can_server"]))
    env.load_orders(g["o_release_min"], g["o_pickup"], g["o_delivery"])
    assert env.main_kernel() == "k_tick_dense"
    env.reset(init)
    env.run(env.T)
    env.sync()
    od, cn = env.orders(), env.counters()
    assert hashlib.sha256(np.ascontiguousarray(od["vehicle"][0]).tobytes()).hexdigest() == str(g["sha_vehicle"])      # the reference's own day
    for i in range(4):
        o = make_oracle(g)
        o.reset(starts[i])
        o.run_day()
        oo, oc = o.orders(), o.counters()
        L = o.lists()
        for r in range(i, R, 4):
            for k in ("status", "vehicle", "wait"):
                np.testing.assert_array_equal(od[k][r], oo[k], err_msg="replica %d %s" % (r, k))
            for j, k in enumerate(COUNTER_NAMES):
                assert cn[r, j] == oc[k], (r, k, int(cn[r, j]), oc[k])
            G = env.lists(r)
            np.testing.assert_array_equal(G["idle_off"], L["idle_off"], err_msg="replica %d" % r)
            np.testing.assert_array_equal(G["idle_veh"], L["idle_veh"], err_msg="replica %d idle order" % r)
    env.close()
