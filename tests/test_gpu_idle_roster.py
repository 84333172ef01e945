"""The idle roster (vds_idle_roster_device / vds_read_idle_roster: k_idle_roster) and dispatch by roster position
(vds_apply_dispatch_roster_device, vds_run_hooked_roster: k_dispatch_roster).  The block - int32 [3][R][V] {veh, node, cluster} by
roster position and the offsets int32 [R][C + 1] - is compared bit for bit with ``oracle.lists()`` of an oracle stepped alongside and
with ``env.lists(r)`` (the independent read_lists_impl); a roster call with ``oracle.dispatch`` of the movers in ROSTER order, through
the helpers the vehicle-form tests use.  Every expectation is an integer; nothing has a tolerance."""
import ctypes
import functools
import gc
import os
import sys

import numpy as np
import pytest

from helpers import REFUSALS, load_golden, oracle_apply
from test_gpu_dispatch_vehicles import (CAPS, CHUNK_CASES, assert_same_day, check_all, day_result, find_order_case, late_orders, make_oracles,
                                        seeded_init, to_dev, torch_stream_kw)
from test_gpu_parity import MODES, TINY, check_lists, make_env
from test_gpu_replica_days import mk_env, mk_oracle, synth_days
from test_order_tables import replica_plan
from vehicles_dispatch_simulator_amd import _lib, synth
from vehicles_dispatch_simulator_amd.env import IDLE_ROSTER_NAMES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R3 = 3
VDS_EINVAL, VDS_ESTATE = -1, -4
TILE = 256          # width of k_idle_roster's scan tile (IR_THREADS)


# ---- expectations ------------------------------------------------------------------------------------------------------------------------
def expect_roster(o, V, C):
    """{veh, node, cluster, off} of one replica from the oracle's lists; ``cluster`` is derived from ``idle_off``."""
    L, loc = o.lists(), o.vehicles()["loc"]
    off = L["idle_off"].astype(np.int32)
    n = int(off[-1])
    veh = np.full(V, -1, dtype=np.int32); node = veh.copy(); cl = veh.copy()
    veh[:n] = L["idle_veh"][:n]
    node[:n] = loc[veh[:n]]
    cl[:n] = np.repeat(np.arange(C, dtype=np.int32), np.diff(off))
    return dict(veh=veh, node=node, cluster=cl, off=off)


def new_stats():
    return dict(dense=set(), longest=0, empty=0, full=0, refused=dict.fromkeys(REFUSALS, 0), second_calls=0, moved=0)


def check_roster(env, oracles, tag, stats=None, replicas=None, against_lists=True, via_torch=False):
    """Refresh, then every replica's rows against its oracle (and env.lists); returns the host copy."""
    if via_torch:
        blk = env.idle_roster_torch()
        env.sync()
        ro = {k: v.cpu().numpy() for k, v in blk.items()}
    else:
        ro = env.idle_roster()
    assert set(ro) == set(IDLE_ROSTER_NAMES) | {"off"}
    assert all(ro[k].shape == (env.R, env.V) and ro[k].dtype == np.int32 for k in IDLE_ROSTER_NAMES) and ro["off"].shape == (env.R, env.C + 1)
    for r, o in enumerate(oracles):
        if o is None or (replicas is not None and r not in replicas):
            continue
        exp = expect_roster(o, env.V, env.C)
        for k in ("off",) + IDLE_ROSTER_NAMES:
            np.testing.assert_array_equal(ro[k][r], exp[k], err_msg="%s replica %d %s" % (tag, r, k))
        if against_lists:
            G = env.lists(r)
            n = int(G["idle_off"][-1])
            np.testing.assert_array_equal(ro["off"][r], G["idle_off"], err_msg=tag)
            np.testing.assert_array_equal(ro["veh"][r, :n], G["idle_veh"][:n], err_msg=tag)
            np.testing.assert_array_equal(ro["node"][r, :n], G["idle_node"][:n], err_msg=tag)
            assert (ro["veh"][r, n:] == -1).all() and (ro["node"][r, n:] == -1).all() and (ro["cluster"][r, n:] == -1).all(), tag
        if stats is not None:
            n = int(exp["off"][-1])
            stats["longest"] = max(stats["longest"], int(np.diff(exp["off"]).max()))
            stats["empty"] += n == 0 and env.V > 0
            stats["full"] += n == env.V and env.V > 0
    if stats is not None:
        stats["dense"].add(int(env.layout()["dense"]))
    return ro


def oracle_apply_roster(o, row, n2c, over=False):
    """One roster-form call of one replica as include/vds.h states it: entry i of ``row`` belongs to roster entry i; the movers leave
    in roster order.  Returns (moves, {refusal kind: refused entries})."""
    L = o.lists()
    n = int(L["idle_off"][-1])
    veh, tg = L["idle_veh"][:n], np.asarray(row)[:n]
    want = tg >= 0
    refused = dict.fromkeys(REFUSALS, 0)
    if over:
        refused["day_over"] = int(want.sum())
        return 0, refused
    beyond = want & (tg >= n2c.size)
    outside = want & ~beyond & (n2c[np.clip(tg, 0, n2c.size - 1)] < 0)
    refused["beyond_n"], refused["no_cluster"] = int(beyond.sum()), int(outside.sum())
    ok = want & ~beyond & ~outside
    if ok.any():
        o.dispatch(veh[ok], tg[ok])
    return int(ok.sum()), refused


def roster_targets(rng, g, oracles, frac=0.25):
    """About `frac` of the roster entries of every replica get a random valid node; the entries behind the roster's end hold a node
    number >= N, which would be refused (and reported) if anything looked at it."""
    V, N = int(g["V"]), int(g["N"])
    valid = np.flatnonzero(g["node2cluster"] >= 0)
    tg = np.full((len(oracles), V), -1, dtype=np.int32)
    for r, o in enumerate(oracles):
        if o is None:
            continue
        n = int(o.lists()["idle_off"][-1])
        pick = rng.random(n) < frac
        tg[r, :n][pick] = valid[rng.integers(0, valid.size, int(pick.sum()))]
        tg[r, n:] = N + 7
    return tg


def roster_call(env, oracles, tg, g, stats=None, over=()):
    env.apply_dispatch_roster_torch(to_dev(tg))
    for r, o in enumerate(oracles):
        if o is None:
            continue
        m, ref = oracle_apply_roster(o, tg[r], g["node2cluster"], over=r in over)
        if stats is not None:
            stats["moved"] += m
            for k in REFUSALS:
                stats["refused"][k] += ref[k]


def kform_call(env, oracles, g):
    """K = 2 through vds_apply_dispatch_device: the second and the first vehicle of the fullest list to the first clustered node."""
    n0 = int(np.flatnonzero(g["node2cluster"] >= 0)[0])
    acts = np.full((len(oracles), 2, 3), -1, dtype=np.int32)
    for r, o in enumerate(oracles):
        L = o.lists()
        c = int(np.argmax(np.diff(L["idle_off"])))
        if L["idle_off"][c + 1] - L["idle_off"][c] >= 2:
            acts[r, 0] = (c, 1, n0); acts[r, 1] = (c, 0, n0)
            o.dispatch(L["idle_veh"][L["idle_off"][c]:L["idle_off"][c] + 2][[1, 0]], np.full(2, n0))
    env.apply_dispatch_torch(to_dev(acts))


def vehicle_call(env, oracles, g, rng):
    V = int(g["V"])
    valid = np.flatnonzero(g["node2cluster"] >= 0)
    tg = np.full((len(oracles), V), -1, dtype=np.int32)
    pick = rng.random(tg.shape) < 0.1
    tg[pick] = valid[rng.integers(0, valid.size, int(pick.sum()))]
    env.apply_dispatch_vehicles_torch(to_dev(tg))
    for r, o in enumerate(oracles):
        oracle_apply(o, tg[r])


# ---- 1. the day walks --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk(name, mode, slots=None, seed=5):
    g = load_golden(name)
    env = make_env(g, R3, **{**MODES[mode], **CAPS, **torch_stream_kw()})
    init = seeded_init(g, R3)
    env.reset(init)
    oracles = make_oracles(g, init)
    rng = np.random.default_rng(seed)
    stats = new_stats()
    tag = "%s %s" % (name, mode)
    check_roster(env, oracles, tag + " after the reset", stats)
    T = env.T if slots is None else min(slots, env.T)
    for t in range(T):
        env.step()
        for o in oracles:
            o.begin_tick()
        check_roster(env, oracles, "%s slot %d after the step" % (tag, t), stats, via_torch=t % 5 == 1)
        if t % 2 == 0:
            roster_call(env, oracles, roster_targets(rng, g, oracles), g, stats)
            check_all(env, oracles, t, tag + " roster call")
            check_roster(env, oracles, "%s slot %d after the roster call" % (tag, t), stats, against_lists=False)
        if t % 4 == 0:          # roster -> K-form -> vehicle form -> refreshed roster -> a second roster call: sequence numbers across the forms
            kform_call(env, oracles, g)
            check_roster(env, oracles, "%s slot %d after the K-form call" % (tag, t), stats, against_lists=False)
            vehicle_call(env, oracles, g, rng)
            check_roster(env, oracles, "%s slot %d after the vehicle-form call" % (tag, t), stats, against_lists=False)
            roster_call(env, oracles, roster_targets(rng, g, oracles, frac=0.15), g, stats)
            stats["second_calls"] += 1
            check_all(env, oracles, t, tag + " second roster call")
            check_roster(env, oracles, "%s slot %d after the second roster call" % (tag, t), stats, against_lists=False)
        env.advance()
        for o in oracles:
            o.end_tick()
    check_roster(env, oracles, tag + " after the last advance", stats)
    check_all(env, oracles, T, tag + " after the last advance")
    od = env.orders()
    for r, o in enumerate(oracles):
        oo = o.orders()
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(od[k][r], oo[k], err_msg="%s replica %d %s" % (tag, r, k))
    stats["dense_st"] = int(env.layout()["dense_st"])
    env.close()
    return stats


WALKS = [(n, m) for n in TINY for m in ("fast", "rows", "generic")] + [("tiny_kmeans_dfs2", "dfs_wide")]


@pytest.mark.parametrize("name,mode", WALKS)
def test_day_walk(name, mode):
    stats = walk(name, mode)
    assert stats["moved"] > 0 and stats["second_calls"] > 0, stats
    if name == "tiny_kmeans":
        assert stats["dense"] == ({1} if mode == "fast" else {0}), stats


def test_the_walks_cover_the_stamp_form_neighbour_search():
    assert walk("tiny_kmeans_dfs2", "fast")["dense_st"] == 1 and walk("tiny_kmeans_dfs2", "dfs_wide")["dense_st"] == 0


# ---- 2. insertion order ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "rows"])
def test_insertion_order_is_roster_order_not_vehicle_number(mode):
    g = late_orders(load_golden("tiny_kmeans"))
    V = int(g["V"])
    init = seeded_init(g, R3)
    env = make_env(g, R3, **{**MODES[mode], **CAPS, **torch_stream_kw()})
    got = {}
    for form in ("roster", "vehicle"):
        env.reset(init)
        oracles = make_oracles(g, init)
        env.step()
        for o in oracles:
            o.begin_tick()
        # v_hi idles in cluster 0, v_lo < v_hi in a higher cluster: roster order is (v_hi, v_lo), vehicle-number order the reverse
        n, v_lo, v_hi, _, d = find_order_case(g, oracles[0])
        ct = int(g["node2cluster"][n])
        tg = np.full((R3, V), -1, dtype=np.int32)
        if form == "roster":
            ro = check_roster(env, oracles, "order")
            i_hi, i_lo = int(np.flatnonzero(ro["veh"][0] == v_hi)[0]), int(np.flatnonzero(ro["veh"][0] == v_lo)[0])
            assert i_hi < i_lo and ro["cluster"][0, i_hi] == 0 < ro["cluster"][0, i_lo]
            tg[0, [i_hi, i_lo]] = n
            env.apply_dispatch_roster_torch(to_dev(tg))
            oracles[0].dispatch(np.array([v_hi, v_lo]), np.array([n, n]))
        else:
            tg[0, [v_lo, v_hi]] = n
            env.apply_dispatch_vehicles_torch(to_dev(tg))
            oracles[0].dispatch(np.array([v_lo, v_hi]), np.array([n, n]))
        check_all(env, oracles, 0, "order " + form)
        G = env.lists(0)
        arr = G["arr_veh"][G["arr_off"][ct]:G["arr_off"][ct + 1]]
        got[form] = [v for v in arr.tolist() if v in (v_lo, v_hi)]
        expect = [v_hi, v_lo] if form == "roster" else [v_lo, v_hi]
        assert got[form] == expect, (form, got)
        for t in range(1, d + 1):      # ... and they enter the idle list in that order at the arrival slot
            env.advance()
            for o in oracles:
                o.end_tick()
            env.step()
            for o in oracles:
                o.begin_tick()
        check_all(env, oracles, d, "order at arrival " + form)
        check_roster(env, oracles, "order at arrival " + form)
        G = env.lists(0)
        lst = G["idle_veh"][G["idle_off"][ct]:G["idle_off"][ct + 1]]
        assert [v for v in lst.tolist() if v in (v_lo, v_hi)] == expect
        env.advance()
    assert got["roster"] == got["vehicle"][::-1]
    env.close()


# ---- 3. shapes at which the scan and the copy can go wrong --------------------------------------------------------------------------------
def synth_fixture(C, V, N=None, seed=41, orders=400):
    """A city of C clusters built with synth (no neighbour search), a short day of synthetic orders."""
    N = max(C + C // 2, 64) if N is None else N
    city = synth.make_city(seed, N=N, C=C, mode="cluster", with_neighbors=False)
    start, pick, dele = synth.make_orders(seed + 1, N, orders)
    rel = synth.release_minutes(start)
    keep = rel < rel[0] + 120
    n2c = city.node2cluster.astype(np.int32)
    ok = keep & (n2c[pick] >= 0) & (n2c[dele] >= 0)
    return dict(cost=city.cost, node2cluster=n2c, nbr_off=np.zeros(C + 1, dtype=np.int32), nbr_idx=np.zeros(0, dtype=np.int32),
                depth_limit=0, neighbor_can_server=False, V=np.int64(V), N=np.int64(N), C=np.int64(C),
                o_release_min=(rel[ok] - rel[0]).astype(np.int32), o_pickup=pick[ok].astype(np.int32), o_delivery=dele[ok].astype(np.int32),
                veh_node=np.full(V, int(np.flatnonzero(n2c >= 0)[0]), dtype=np.int32))


def nodes_of(g, c):
    return np.flatnonzero(g["node2cluster"] == c)


def spread_init(g, R, seed):
    V, N = int(g["V"]), int(g["N"])
    return synth.make_vehicle_nodes(seed, N, V, R, g["node2cluster"] >= 0).astype(np.int32).reshape(R, V)


def one_cluster_init(g, R, c):
    """Every vehicle of every replica in cluster c, on nodes that differ per replica and vehicle."""
    V = int(g["V"])
    nd = nodes_of(g, c)
    assert nd.size > 0
    return np.stack([nd[(np.arange(V) * (r + 1) + r) % nd.size] for r in range(R)]).astype(np.int32).reshape(R, V)


#              name                 C             V    R  how the vehicles start            kw
SHAPES = {
    "C1":                  (1,            37,  3, "spread",                         {}),
    "C_tile_minus_1":      (TILE - 1,     151, 3, "spread",                         {}),
    "C_tile":              (TILE,         151, 3, "spread",                         {}),
    "C_tile_plus_1":       (TILE + 1,     151, 3, "spread",                         {}),
    "C_two_tiles_and_87":  (2 * TILE + 87, 151, 3, "spread",                        {"force_generic": 5}),
    "last_cluster_2_chunks": (12,         100, 3, "last",                           {"idle_cap": 128}),
    "last_cluster_3_chunks": (12,         140, 3, "last",                           {"force_generic": 5}),
    "only_the_middle":     (TILE + 1,     70,  3, "middle",                         {}),
    "V1":                  (12,           1,   3, "spread",                         {}),
    "V13":                 (12,           13,  5, "spread",                         {}),
    "V151_R1":             (12,           151, 1, "spread",                         {"force_generic": 5}),
    "R5_tail":             (40,           151, 5, "spread",                         {}),
    "row_filled":          (12,           64,  3, "last",                           {"idle_cap": 64}),
}


@functools.lru_cache(maxsize=None)
def shape_walk(case):
    C, V, R, how, kw = SHAPES[case]
    g = synth_fixture(C, V)
    if how == "spread":
        init = spread_init(g, R, 700 + V)
    else:
        ne = np.flatnonzero(np.bincount(g["node2cluster"], minlength=C) > 0)
        c = int(ne[-1]) if how == "last" else int(ne[ne.size // 2])
        init = one_cluster_init(g, R, c)
    caps = dict(ring_cap=256, far_cap=256)
    caps["idle_cap"] = kw.get("idle_cap", 256)
    env = make_env(g, R, **{**caps, **{k: v for k, v in kw.items() if k != "idle_cap"}, **torch_stream_kw()})
    if "idle_cap" in kw:
        assert env.idle_cap == kw["idle_cap"]
    env.reset(init)
    oracles = make_oracles(g, init)
    stats = new_stats()
    rng = np.random.default_rng(9)
    check_roster(env, oracles, case + " after the reset", stats)
    for t in range(min(env.T, 6)):
        env.step()
        for o in oracles:
            o.begin_tick()
        check_roster(env, oracles, "%s slot %d" % (case, t), stats, via_torch=t == 1)
        if how != "spread" and t == 0:
            for picks in (CHUNK_CASES["chunk_edge"], CHUNK_CASES["every_second"]):
                tg = roster_targets(rng, g, oracles, frac=0.0)
                valid = np.flatnonzero(g["node2cluster"] >= 0)
                for r, o in enumerate(oracles):
                    n = int(o.lists()["idle_off"][-1])
                    idx = np.array([p for p in picks if p < n], dtype=np.int64)
                    tg[r, idx] = valid[rng.integers(0, valid.size, idx.size)]
                roster_call(env, oracles, tg, g, stats)
                check_all(env, oracles, t, case + " chunk picks")
                check_roster(env, oracles, "%s slot %d after chunk picks" % (case, t), stats)
        roster_call(env, oracles, roster_targets(rng, g, oracles), g, stats)
        check_all(env, oracles, t, case)
        check_roster(env, oracles, "%s slot %d after the call" % (case, t), stats)
        env.advance()
        for o in oracles:
            o.end_tick()
    env.sync()
    env.close()
    return stats


@pytest.mark.parametrize("case", list(SHAPES))
def test_shapes(case):
    stats = shape_walk(case)
    C, V, R, how, kw = SHAPES[case]
    assert stats["moved"] > 0 or V == 1, stats
    if how != "spread":
        assert stats["longest"] == V and stats["full"] > 0, stats
    if case == "last_cluster_3_chunks":
        assert stats["longest"] > 128 and stats["dense"] == {0}
    if case == "last_cluster_2_chunks":
        assert 64 < stats["longest"] <= 128 and stats["dense"] == {1}


def test_no_vehicles_is_a_no_op_also_inside_the_hooked_day():
    import torch
    g = dict(load_golden("tiny_kmeans"))
    g["V"] = np.int64(0)
    R, C = 3, int(g["C"])
    env = make_env(g, R, stream=torch.cuda.current_stream().cuda_stream)
    with pytest.raises(Exception, match="call vds_reset first"):
        env.idle_roster()
    env.reset(np.zeros((R, 0), dtype=np.int32))
    ro = env.idle_roster()
    assert all(ro[k].shape == (R, 0) for k in IDLE_ROSTER_NAMES) and ro["off"].shape == (R, C + 1) and (ro["off"] == 0).all()
    blk = env.idle_roster_torch()
    assert all(tuple(blk[k].shape) == (R, 0) for k in IDLE_ROSTER_NAMES)
    blk["off"].fill_(-7)
    torch.cuda.synchronize()
    env.step()
    tg = torch.zeros((R, 0), dtype=torch.int32, device="cuda")
    env.apply_dispatch_roster_torch(tg)                       # no vehicles: a no-op, whatever the freshness flag says
    assert env._lib.vds_apply_dispatch_roster_device(env._h, None) == 0
    env.advance()
    env.run_hooked(5, roster=True, roster_targets=tg)
    env.sync()
    torch.cuda.synchronize()
    assert env.clock[0] == 6 and int((blk["off"] == 0).all().item()) == 1          # the day's refresh wrote the offsets
    cn = env.counters()
    assert (cn[:, 0] == cn[:, 1]).all() and cn[0, 0] > 0          # every processed order was rejected
    env.close()


# ---- 4. refusals and argument checks -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refusal_walk():
    g = load_golden("tiny_focus_grid")
    V, N = int(g["V"]), int(g["N"])
    outside = np.flatnonzero(g["node2cluster"] < 0)
    assert outside.size == 205
    init = seeded_init(g, R3)
    env = make_env(g, R3, **{**CAPS, **torch_stream_kw()})
    env.reset(init)
    oracles = make_oracles(g, init)
    env.step()
    for o in oracles:
        o.begin_tick()
    stats = new_stats()
    good = int(np.flatnonzero(g["node2cluster"] >= 0)[17])
    for kind, bad in (("no_cluster", int(outside[3])), ("beyond_n", N)):
        check_roster(env, oracles, "refusals", stats)
        moved0 = int(env.counters()[1, 4])
        tg = np.full((R3, V), -1, dtype=np.int32)
        tg[1, 0], tg[1, 1], tg[1, 2] = bad, good, bad
        roster_call(env, oracles, tg, g, stats)
        with pytest.raises(Exception, match="dispatch"):
            env.sync()
        env.sync()                                     # reported once
        check_all(env, oracles, 0, "refusals " + kind)
        assert env.counters()[1, 4] == moved0 + 1      # the other move of the call was applied
    env.advance()
    env.close()
    return stats


def test_refused_targets_are_skipped_and_reported_once():
    stats = refusal_walk()
    assert stats["refused"]["no_cluster"] == 2 and stats["refused"]["beyond_n"] == 2 and stats["moved"] == 2, stats


def test_overwritten_offsets_apply_nothing_and_raise_the_dispatch_error():
    """The device-side backstop: the handle believes the roster fresh, but the offsets no longer describe the lists."""
    import torch
    g = load_golden("tiny_kmeans")
    V, C = int(g["V"]), int(g["C"])
    init = seeded_init(g, R3)
    env = make_env(g, R3, **{**CAPS, **torch_stream_kw()})
    env.reset(init)
    oracles = make_oracles(g, init)
    env.step()
    for o in oracles:
        o.begin_tick()
    blk = env.idle_roster_torch()
    env.sync()
    off = blk["off"].cpu().numpy()
    c = int(np.argmax(np.diff(off[2])))
    bad = off.copy()
    bad[2, c + 1:] -= 1                               # replica 2: cluster c reads one entry short, every later list is shifted
    blk["off"].copy_(to_dev(bad))
    torch.cuda.synchronize()
    tg = np.full((R3, V), -1, dtype=np.int32)
    n0 = int(np.flatnonzero(g["node2cluster"] >= 0)[0])
    tg[0, 0] = n0
    tg[2, :] = n0                                     # everything of replica 2 would move
    env.apply_dispatch_roster_torch(to_dev(tg))
    oracles[0].dispatch(oracles[0].lists()["idle_veh"][:1], np.array([n0]))
    # replica 2: the list of cluster c does not have the length its offsets give and applies nothing; every other list still has
    # (the lists behind c read their targets one entry early - all the same node here - and move in roster order all the same)
    L2 = oracles[2].lists()
    cl2 = np.repeat(np.arange(C), np.diff(L2["idle_off"]))
    movers = L2["idle_veh"][:L2["idle_off"][-1]][cl2 != c]
    oracles[2].dispatch(movers, np.full(movers.size, n0))
    with pytest.raises(Exception, match="dispatch"):
        env.sync()
    env.sync()
    G = env.lists(2)
    np.testing.assert_array_equal(G["idle_veh"][:G["idle_off"][-1]], L2["idle_veh"][:L2["idle_off"][-1]][cl2 == c])      # only that list stands
    check_all(env, oracles, 0, "backstop")
    check_roster(env, oracles, "backstop: the next refresh")
    env.advance()
    env.close()


def test_host_side_freshness_and_argument_checks():
    import torch
    g = load_golden("tiny_kmeans")
    V = int(g["V"])
    init = seeded_init(g, R3)
    env = make_env(g, R3, **{**CAPS, **torch_stream_kw()})
    env.reset(init)
    stay = torch.full((R3, V), -1, dtype=torch.int32, device="cuda")
    ptr = env._vehicle_targets_ptr(stay, "test")
    call = lambda p=ptr: env._lib.vds_apply_dispatch_roster_device(env._h, p)
    err = lambda: env._lib.vds_last_error(env._h).decode()
    env.idle_roster_device_ptr()
    assert call() == VDS_EINVAL and "vds_step" in err()                    # before a step
    env.step()
    assert call() == VDS_ESTATE and "stale" in err()                       # the step changed the lists
    assert call(None) == VDS_EINVAL and "null" in err()
    before = [env.lists(r) for r in range(R3)]
    acts = torch.full((R3, 1, 3), -1, dtype=torch.int32, device="cuda")
    host = (np.zeros(0, np.int32),) * 4

    def changers():
        yield "roster call", lambda: env.apply_dispatch_roster_torch(stay)
        yield "K-form call", lambda: env.apply_dispatch_torch(acts)
        yield "vehicle-form call", lambda: env.apply_dispatch_vehicles_torch(stay)
        yield "host call", lambda: env.apply_dispatch(np.array([0]), np.array([int(np.argmax(np.diff(before[0]["idle_off"])))]), np.array([0]),
                                                    np.array([int(np.flatnonzero(g["node2cluster"] >= 0)[0])]))
        yield "host call with arrival minutes (vds_apply_dispatch_ex)", lambda: env.apply_dispatch(
            np.array([1]), np.array([int(np.argmax(np.diff(before[1]["idle_off"])))]), np.array([0]), np.array([int(np.flatnonzero(g["node2cluster"] >= 0)[0])]),
            arrive_min=np.array([env.clock[1] + 25]), counted=np.array([1]))
        yield "snapshot + restore", lambda: (env.snapshot(), env.restore())
        yield "restore from a device map (vds_restore_device)", lambda: env.restore_torch(torch.arange(R3, dtype=torch.int32, device="cuda"))
        yield "restore through a map", lambda: env.restore([0, 1, 2])
        yield "advance + step", lambda: (env.advance(), env.step())
        yield "reset + step", lambda: (env.reset(init), env.step())
        yield "reset_again + step", lambda: (env.reset_again(), env.step())
        yield "run + step", lambda: (env.advance(), env.run(8), env.step())
        yield "run_hooked + step", lambda: (env.advance(), env.run_hooked(2), env.step())
        yield "reset_random + step", lambda: (env.reset_random(np.arange(R3) + 11), env.step())
        yield "load_orders + reset + step", lambda: (env.load_orders(g["o_release_min"], g["o_pickup"], g["o_delivery"]), env.reset(init), env.step())
        yield "set_idle_cap + reset + step", lambda: (env.set_idle_cap(env.idle_cap * 2), env.reset(init), env.step())

    def stale_after(changes):
        for what, change in changes:
            env.idle_roster_device_ptr()
            assert call() == 0, what                                       # fresh: accepted (and stale again: the call itself)
            assert call() == VDS_ESTATE, what
            env.idle_roster()                                              # (the host read refreshes too)
            change()
            assert call() == VDS_ESTATE and "vds_idle_roster_device" in err(), what

    stale_after(changers())
    env.idle_roster_device_ptr()
    moving = torch.zeros((R3, V), dtype=torch.int32, device="cuda")
    for bad in (moving.to(torch.int64), torch.zeros((R3, V + 1), dtype=torch.int32, device="cuda"), moving.cpu(),
                torch.zeros((V, R3), dtype=torch.int32, device="cuda").t(), moving.cpu().numpy()):
        with pytest.raises(Exception, match="apply_dispatch_roster_torch"):
            env.apply_dispatch_roster_torch(bad)
        with pytest.raises(Exception, match="run_hooked"):
            env.run_hooked(1, roster=True, roster_targets=bad)
    env.advance()
    assert call() == VDS_EINVAL and "vds_step" in err()                    # after the advance
    # the hooked day: targets without the refresh, targets next to another dispatch form
    assert env._lib.vds_run_hooked_roster(env._h, 0, ptr) == VDS_EINVAL
    acts2 = torch.full((R3, 2, 3), -1, dtype=torch.int32, device="cuda")
    t0 = env.clock[0]
    with pytest.raises(Exception, match="roster targets"):
        env.run_hooked(2, actions=acts2, roster=True, roster_targets=stay)
    with pytest.raises(Exception, match="roster targets"):
        env.run_hooked(2, vehicle_targets=moving, roster=True, roster_targets=stay)
    assert env.clock[0] == t0
    env.run_hooked(2, roster=True, roster_targets=stay)                    # ... alone it runs
    env.run_hooked(2, actions=acts2)                                       # ... and is off again behind a call without it
    env.sync()
    assert env.clock[0] == t0 + 4 and env.counters()[:, 4].sum() == 0      # (nothing moved since the last reset)
    env.close()
    # order days per replica: a load of days and another replica -> day map re-make or re-stride the tables
    days = synth_days(g, 2, seed=77)
    env = mk_env(g, R3, **{**CAPS, **torch_stream_kw()})
    env.load_order_days(days, np.array([0, 1, 0], dtype=np.int32))
    env.reset(init)
    env.step()
    stale_after([("load_order_days + reset + step", lambda: (env.load_order_days(days, np.array([0, 1, 0], dtype=np.int32)), env.reset(init), env.step())),
                 ("set_replica_days + reset + step", lambda: (env.set_replica_days(np.array([1, 0, 1], dtype=np.int32)), env.reset(init), env.step()))])
    env.advance()
    env.sync()
    env.close()


# ---- 5. order days per replica -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def replica_days_walk():
    import torch
    g = load_golden("tiny_kmeans")
    R, V = 40, int(g["V"])
    days = synth_days(g, 5, seed=5200)
    init = seeded_init(g, R)
    env = mk_env(g, R, **{**CAPS, **torch_stream_kw()})
    maps = [np.arange(R) // 8, np.arange(R) % 5, (np.arange(R) * 7 + 1) % 4, np.arange(R) % 3]
    rc, plan = replica_plan(maps[3], 5, gran_small=0)
    assert rc == 0 and plan["regrouped"] and plan["R"] == 48 and int((plan["int2ext"] < 0).sum()) == 8
    env.load_order_days(days, maps[0].astype(np.int32))
    stats = new_stats()
    rng = np.random.default_rng(31)
    frozen_checked = 0
    n_ok = int(np.flatnonzero(g["node2cluster"] >= 0)[5])
    for ep, rd in enumerate(maps):
        if ep:
            env.set_replica_days(rd.astype(np.int32))
        env.reset(init)
        oracles = [mk_oracle(g, days[int(d)]) for d in rd]
        for r, o in enumerate(oracles):
            o.reset(init[r])
        Ts = [o.num_ticks for o in oracles]
        t_short = min(Ts)
        frozen = {}
        slots = sorted(set(range(0, 4)) | set(range(t_short - 2, t_short + 3)))
        for t in range(t_short + 3):
            env.step()
            live = [r for r in range(R) if t < Ts[r]]
            for r in live:
                oracles[r].begin_tick()
            if t in slots:
                blk = env.idle_roster_torch()           # the block overwritten from torch ahead of the refresh
                env.sync()
                for v in blk.values():
                    v.fill_(-7)
                torch.cuda.synchronize()
                check_roster(env, oracles, "days episode %d slot %d" % (ep, t), stats, against_lists=t % 2 == 0)
                over = [r for r in range(R) if t >= Ts[r]]
                tg = roster_targets(rng, g, oracles, frac=0.1)
                for r in over:
                    tg[r] = -1
                if over and t == t_short + 1:           # a target in a replica whose day is over: refused, its lists stand
                    tg[over[0], 0] = n_ok
                roster_call(env, oracles, tg, g, stats, over=over)
                if over and t == t_short + 1:
                    with pytest.raises(Exception, match="dispatch"):
                        env.sync()
                    env.sync()
                check_all(env, oracles, t, "days episode %d" % ep, replicas=live[::5])
                ro = check_roster(env, oracles, "days episode %d slot %d after the call" % (ep, t), stats, against_lists=False)
                for r in range(R):
                    if t == Ts[r] - 1:
                        frozen[r] = {k: ro[k][r].copy() for k in ro}
                    elif t >= Ts[r] and r in frozen:          # its city stands still, whatever the call named
                        for k in ro:
                            np.testing.assert_array_equal(ro[k][r], frozen[r][k], err_msg="episode %d slot %d replica %d %s" % (ep, t, r, k))
                        frozen_checked += 1
            env.advance()
            for r in live:
                oracles[r].end_tick()
    assert frozen_checked > 0
    env.close()
    return stats


def test_order_days_per_replica_regrouped():
    stats = replica_days_walk()
    assert stats["refused"]["day_over"] == 4, stats          # one refused entry per replica map


# ---- 6. the hooked day -------------------------------------------------------------------------------------------------------------------
HG_R = 40


def rule_roster_targets(g, o, slot, node_of):
    """The policy restated on the oracle: roster entries with (position in the list) % 5 == slot % 5 in clusters with more than two
    idle vehicles go to the first node of the next cluster."""
    V, C = int(g["V"]), int(g["C"])
    off = o.lists()["idle_off"]
    n = np.diff(off)
    cl = np.repeat(np.arange(C), n)
    pos = np.arange(off[-1]) - off[cl]
    tg = np.full(V, -1, dtype=np.int32)
    go = (pos % 5 == slot % 5) & (n[cl] > 2)
    tg[:off[-1]][go] = node_of[(cl[go] + 1) % C]
    return tg


@functools.lru_cache(maxsize=None)
def hooked_expectation():
    g = load_golden("tiny_dispatch")
    C = int(g["C"])
    node_of = np.array([np.flatnonzero(g["node2cluster"] == c)[0] for c in range(C)], dtype=np.int32)
    init = seeded_init(g, HG_R)
    oracles = make_oracles(g, init)
    moves = 0
    for o in oracles:
        for t in range(o.num_ticks):
            o.begin_tick()
            moves += oracle_apply_roster(o, rule_roster_targets(g, o, t, node_of), g["node2cluster"])[0]
            o.end_tick()
    assert moves >= 20 * HG_R
    return g, init, node_of, oracles


@pytest.mark.parametrize("groups,kw", [(1, {}), (2, {}), (1, {"force_generic": 1})], ids=["one-chain", "two-groups", "eager-generic"])
def test_run_hooked_refreshes_the_roster_and_applies_roster_targets(groups, kw):
    import torch
    g, init, node_of, oracles = hooked_expectation()
    V, C, R = int(g["V"]), int(g["C"]), HG_R
    stream = torch.cuda.current_stream()
    env = make_env(g, R, stream=stream.cuda_stream, **CAPS, **kw)
    env.set_run_groups(groups, -1)
    assert env._lib.vds_get_run_groups(env._h) == groups
    T = env.T
    env.reset(init)
    ptrs = env.idle_roster_device_ptr()
    blk = env.idle_roster_torch()
    assert (blk["veh"].data_ptr(), blk["off"].data_ptr()) == ptrs
    off, cluster = blk["off"], blk["cluster"]
    targets = torch.full((R, V), -1, dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int64, device="cuda")
    idle_log = torch.zeros((T, R), dtype=torch.int32, device="cuda")
    node_t = torch.from_numpy(node_of.astype(np.int64)).cuda()
    iota = torch.arange(V, device="cuda", dtype=torch.int64)[None, :]

    def policy():
        idle_log.index_copy_(0, slot, off[:, C][None])
        o64 = off.to(torch.int64)
        cl = cluster.to(torch.int64).clamp(min=0)
        n = (o64[:, 1:] - o64[:, :-1])
        pos = iota - torch.gather(o64, 1, cl)
        go = (cluster >= 0) & (pos % 5 == slot % 5) & (torch.gather(n, 1, cl) > 2)
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
    on = dict(policy_graph=graph, roster=True, roster_targets=targets, idle_pre=False, idle_now=False, supply=False, cl_orders=False)

    def start():
        env.reset(init)
        slot.zero_(); targets.fill_(-1); idle_log.fill_(-9)

    def check(tag):
        env.sync()
        torch.cuda.synchronize()
        assert int(slot.item()) == T and int((idle_log == -9).sum().item()) == 0, tag
        assert env.idle_roster_device_ptr() == ptrs, tag
        res = day_result(env)
        res["idle_log"] = idle_log.cpu().numpy()
        return res

    start()
    env.run_hooked(T, **on)
    first = check("one launch")
    start()
    env.run_hooked(T, **on)                                          # the same graph, replayed
    second = check("replay")
    assert_same_day(first, second, "replay")
    np.testing.assert_array_equal(first["idle_log"], second["idle_log"])
    env.load_orders(g["o_release_min"], g["o_pickup"], g["o_delivery"])      # the same sizes: the state tables stay, the graph is rebuilt
    start()
    assert env.idle_roster_device_ptr() == ptrs
    env.run_hooked(T, **on)
    third = check("rebuilt behind load_orders")
    assert_same_day(first, third, "rebuild")
    start()
    for t in range(T):                                               # the same calls slot by slot through the entry points
        env.step()
        env.idle_roster_device_ptr()
        graph.replay()
        env.apply_dispatch_roster_torch(targets)
        env.advance()
    stepwise = check("slot by slot")
    assert_same_day(first, stepwise, "slot by slot")
    np.testing.assert_array_equal(first["idle_log"], stepwise["idle_log"])
    # the oracle replay of the rule
    for r, o in enumerate(oracles):
        check_lists(env, r, o, T)
        oo, oc = o.orders(), o.counters()
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(first[k][r], oo[k], err_msg="replica %d %s" % (r, k))
        assert (first["counters"][r, 4], first["counters"][r, 5]) == (oc["dispatch_num"], oc["dispatch_cost"]), r
    assert first["counters"][:, 4].sum() >= 20 * R
    # switched off again: the block is not touched, the day equals one on a handle that never switched it on
    obs_off = dict(idle_pre=False, idle_now=False, supply=False, cl_orders=False)
    env.reset(init)
    env.sync()
    for v in blk.values():
        v.fill_(-7)
    torch.cuda.synchronize()
    env.run_hooked(T, **obs_off)
    off_day = day_result(env)
    torch.cuda.synchronize()
    assert all(int((v == -7).all().item()) == 1 for v in blk.values())
    fresh = make_env(g, R, stream=stream.cuda_stream, **CAPS, **kw)
    fresh.set_run_groups(groups, -1)
    fresh.reset(init)
    fresh.run_hooked(T, **obs_off)
    assert_same_day(off_day, day_result(fresh), "switched off")
    assert off_day["counters"][:, 4].sum() == 0
    fresh.close()
    env.close()


# ---- 7. snapshot / restore ---------------------------------------------------------------------------------------------------------------
def test_snapshot_mid_slot_and_restore_through_a_permutation():
    g = load_golden("tiny_kmeans")
    R = 3
    init = seeded_init(g, R)
    env = make_env(g, R, **{**CAPS, **torch_stream_kw()})
    env.reset(init)
    oracles = make_oracles(g, init)
    rng = np.random.default_rng(3)
    for t in range(6):
        env.step()
        for o in oracles:
            o.begin_tick()
        if t < 5:
            env.advance()
            for o in oracles:
                o.end_tick()
    check_roster(env, oracles, "before the snapshot")
    roster_call(env, oracles, roster_targets(rng, g, oracles), g)
    env.snapshot()                                         # inside the slot, behind a roster call
    at = check_roster(env, oracles, "at the snapshot")
    assert not np.array_equal(at["veh"][0], at["veh"][1]) and not np.array_equal(at["veh"][1], at["veh"][2])
    env.advance()
    for _ in range(3):
        env.step(); env.advance()
    perm = [2, 0, 1]
    env.restore(perm)
    got = env.idle_roster()
    for k in got:
        for r in range(R):
            np.testing.assert_array_equal(got[k][r], at[k][perm[r]], err_msg="after restore: replica %d shows replica %d (%s)" % (r, perm[r], k))
    # ... and a roster call against that roster behaves as it would have on the source replicas
    tg = roster_targets(rng, g, [oracles[p] for p in perm], frac=0.3)
    env.apply_dispatch_roster_torch(to_dev(tg))
    env.sync()
    after = env.idle_roster()
    for r in range(R):
        n = int(at["off"][perm[r], -1])
        keep = tg[r, :n] < 0
        np.testing.assert_array_equal(after["veh"][r, :int(keep.sum())], at["veh"][perm[r], :n][keep])      # survivors keep their order
        assert after["off"][r, -1] == keep.sum()
    env.advance()
    env.close()


# ---- 8. lifetime -------------------------------------------------------------------------------------------------------------------------
def device_blocks():
    gc.collect()          # (a handle some earlier test dropped without closing it goes now)
    out = np.zeros(2, dtype=np.int64)
    assert _lib.load().vds_debug_device_blocks(out.ctypes.data_as(ctypes.c_void_p)) == 0
    return int(out[0]), int(out[1])


def test_address_lifetime_and_device_blocks():
    before = device_blocks()
    g = load_golden("tiny_kmeans")
    R, V, C = 3, int(g["V"]), int(g["C"])
    init = seeded_init(g, R)
    env = make_env(g, R)
    with pytest.raises(Exception, match="call vds_reset first"):
        env.idle_roster_device_ptr()
    env.reset(init)
    env.step()
    held = device_blocks()
    p = env.idle_roster_device_ptr()
    with_block = device_blocks()
    assert p[1] == p[0] + 4 * 3 * R * V                                                      # ONE allocation: the offsets behind the planes
    assert with_block[0] == held[0] + 1 and with_block[1] >= held[1] + 4 * (3 * R * V + R * (C + 1))
    env.advance(); env.step()
    assert env.idle_roster_device_ptr() == p and device_blocks() == with_block                # ... made once
    env.reset(init)
    assert env.idle_roster_device_ptr() == p
    env.reset_again()
    assert env.idle_roster_device_ptr() == p
    env.load_orders(g["o_release_min"], g["o_pickup"], g["o_delivery"])                       # the same sizes: the state tables stay, and the block with them
    with pytest.raises(Exception, match="call vds_reset first"):
        env.idle_roster_device_ptr()
    env.reset(init)
    assert env.idle_roster_device_ptr() == p
    env.set_idle_cap(env.idle_cap * 2)             # other idle tables: whatever the call returns afterwards is the block, and it works
    env.reset(init)
    oracles = make_oracles(g, init)
    p2 = env.idle_roster_device_ptr()
    blk = env.idle_roster_torch()
    assert (blk["veh"].data_ptr(), blk["off"].data_ptr()) == p2
    for t in range(3):
        env.step()
        for o in oracles:
            o.begin_tick()
        ro = check_roster(env, oracles, "after set_idle_cap slot %d" % t)
        env.sync()
        for k in ro:
            np.testing.assert_array_equal(blk[k].cpu().numpy(), ro[k])
        env.advance()
        for o in oracles:
            o.end_tick()
    env.close()
    assert device_blocks() == before
    # the state tables re-made by another replica -> day map: the block goes with them, the next request makes it again
    R = 40
    days = synth_days(g, 5, seed=5200)
    init = seeded_init(g, R)
    env = mk_env(g, R)
    env.load_order_days(days, (np.arange(R) // 8).astype(np.int32))
    env.reset(init)
    env.step()
    env.idle_roster_device_ptr()
    env.set_replica_days((np.arange(R) % 3).astype(np.int32))
    env.reset(init)
    gone = device_blocks()
    p3 = env.idle_roster_device_ptr()
    assert device_blocks()[0] == gone[0] + 1
    oracles = [None] * R
    oracles[1] = mk_oracle(g, days[1]); oracles[1].reset(init[1])
    oracles[38] = mk_oracle(g, days[2]); oracles[38].reset(init[38])
    for t in range(3):
        env.step()
        for o in (oracles[1], oracles[38]):
            o.begin_tick()
        check_roster(env, oracles, "after set_replica_days slot %d" % t)
        assert env.idle_roster_device_ptr() == p3
        env.advance()
        for o in (oracles[1], oracles[38]):
            o.end_tick()
    env.close()
    assert device_blocks() == before


# ---- 9. coverage -------------------------------------------------------------------------------------------------------------------------
def test_the_walks_met_what_they_are_there_for():
    """Both layouts, a list longer than 128 entries, an empty and a full replica, each refusal, two roster calls in one slot (the walks
    are cached: whatever ran before in this process is not run again)."""
    runs = [walk("tiny_kmeans", "fast"), walk("tiny_kmeans", "rows"), shape_walk("last_cluster_3_chunks"), shape_walk("last_cluster_2_chunks"),
            empty_replica_walk(), refusal_walk(), replica_days_walk()]
    assert set().union(*[s["dense"] for s in runs]) == {0, 1}
    assert max(s["longest"] for s in runs) > 128
    assert sum(s["empty"] for s in runs) > 0 and sum(s["full"] for s in runs) > 0
    for k in REFUSALS:
        assert sum(s["refused"][k] for s in runs) > 0, k
    assert sum(s["second_calls"] for s in runs) > 0


@functools.lru_cache(maxsize=None)
def empty_replica_walk():
    """Replica 1 sends every idle vehicle away in one roster call: its next roster is empty (off[r][C] == 0, all -1)."""
    g = late_orders(load_golden("tiny_kmeans"))
    V = int(g["V"])
    init = seeded_init(g, R3)
    env = make_env(g, R3, **{**CAPS, **torch_stream_kw()})
    env.reset(init)
    oracles = make_oracles(g, init)
    stats = new_stats()
    env.step()
    for o in oracles:
        o.begin_tick()
    check_roster(env, oracles, "empty: before", stats)
    tg = np.full((R3, V), -1, dtype=np.int32)
    tg[1] = int(np.flatnonzero(g["node2cluster"] >= 0)[0])
    roster_call(env, oracles, tg, g, stats)
    check_all(env, oracles, 0, "empty")
    ro = check_roster(env, oracles, "empty: after", stats)
    assert ro["off"][1, -1] == 0 and (ro["veh"][1] == -1).all() and (ro["off"][1] == 0).all()
    roster_call(env, oracles, tg, g, stats)               # ... and a call on the empty roster looks at nothing
    env.sync()
    check_all(env, oracles, 0, "empty: second call")
    env.advance()
    env.close()
    return stats


def test_a_replica_without_idle_vehicles():
    stats = empty_replica_walk()
    assert stats["empty"] >= 1 and stats["moved"] > 0, stats


# ---- 9b. one walk, two forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"force_generic": 5}], ids=["dense", "wide"])
def test_the_two_tensor_forms_differ_in_addressing_only(kw):
    """k_dispatch_vehicles and k_dispatch_roster are one walk that differs in where a list position finds its target and its
    sequence id.  With every vehicle in ONE list in ascending vehicle number, roster position == list position == vehicle number: one
    target tensor means the same in both forms, down to the arrival keys - two environments built alike, one call of either form,
    equal bit for bit from then on.  3 clusters, 2 replicas, 70 vehicles in the last cluster: two chunks, the second partial."""
    C, V, R = 3, 70, 2
    g = synth_fixture(C, V)
    n2c, N = g["node2cluster"], int(g["N"])
    last = int(np.flatnonzero(np.bincount(n2c[n2c >= 0], minlength=C) > 0)[-1])
    # slot 0 and the slots behind it take no vehicle off the list: one order elsewhere opens the day, the others come an hour later
    rel = g["o_release_min"]
    first = int(np.flatnonzero(n2c[g["o_pickup"]] != last)[0])
    keep = rel >= rel[first] + 60
    keep[first] = True
    keep[:first] = False
    for k in ("o_release_min", "o_pickup", "o_delivery"):
        g[k] = g[k][keep]
    init = one_cluster_init(g, R, last)
    caps = dict(idle_cap=128, ring_cap=256, far_cap=256)
    envs = {form: make_env(g, R, **{**caps, **kw, **torch_stream_kw()}) for form in ("vehicle", "roster")}
    for env in envs.values():
        assert int(env.layout()["dense"]) == (0 if kw else 1)
        env.reset(init)
        env.step()
    blk = envs["roster"].idle_roster_torch()
    envs["roster"].sync()
    ro = {k: v.cpu().numpy() for k, v in blk.items()}
    for r in range(R):          # roster order and vehicle-number order agree
        assert ro["off"][r].tolist() == [0] * (last + 1) + [V] * (C - last)
        np.testing.assert_array_equal(ro["veh"][r], np.arange(V))
    valid = np.flatnonzero(n2c >= 0)
    movers = [0, 5, 31, 62, 63, 64, 65, 69]
    tg = np.full((R, V), -1, dtype=np.int32)
    for r in range(R):
        tg[r, movers] = valid[(np.arange(len(movers)) * 5 + 3 * r) % valid.size]
    tg[1, [1, 68]] = valid[[7 % valid.size, 11 % valid.size]]      # (the replicas differ)
    tg[0, 40] = N + 3                                              # refused: a target >= N
    envs["vehicle"].apply_dispatch_vehicles_torch(to_dev(tg))
    envs["roster"].apply_dispatch_roster_torch(to_dev(tg))

    def same(tag):
        a, b = envs["vehicle"], envs["roster"]
        for r in range(R):
            for what, x, y in (("lists", a.lists(r), b.lists(r)), ("vehicles", a.vehicles(r), b.vehicles(r))):
                assert set(x) == set(y)
                for k in x:
                    np.testing.assert_array_equal(x[k], y[k], err_msg="%s replica %d %s %s" % (tag, r, what, k))
        np.testing.assert_array_equal(a.counters(), b.counters(), err_msg=tag)
        return a.lists(0), a.lists(1)

    for env in envs.values():       # the sticky dispatch error, in both: seen once
        with pytest.raises(Exception, match="dispatch"):
            env.sync()
        env.sync()
    L = same("behind the call")
    cn = envs["vehicle"].counters()
    assert cn[0, 4] == len(movers) and cn[1, 4] == len(movers) + 2
    for r in range(R):
        gone = set(np.flatnonzero(tg[r] >= 0).tolist()) - {40}
        assert L[r]["idle_veh"][:L[r]["idle_off"][-1]].tolist() == [v for v in range(V) if v not in gone]      # survivors keep their order
        assert set(L[r]["arr_veh"][:L[r]["arr_off"][-1]].tolist()) == gone
    # ... and on until every mover has arrived: they enter the lists in the same order
    on_the_way = lambda: sum(int((envs["vehicle"].vehicles(r)["state"] == 2).sum()) for r in range(R))
    assert on_the_way() == 2 * len(movers) + 2
    for t in range(1, envs["vehicle"].T):
        for env in envs.values():
            env.advance()
            env.step()
        same("slot %d" % t)
        if on_the_way() == 0:
            break
    assert on_the_way() == 0, "the movers have not arrived by the end of the day"
    for env in envs.values():
        env.advance()
        env.sync()
        env.close()


# ---- 10. written in full, whatever the memory held (the LAST tests of the module: a child that ends by a signal or at its limit
# stops the ones behind it, and nothing of this module may start on the GPU behind such a child) ----------------------------------------------------------------------------------------
# seconds of the selection under the product library on an MI355X, pytest start-up included; the limit follows as in
# tests/test_gpu_dirty_memory.py: ten times that + 120 s, a safety stop
SELECTION = "test_day_walk or test_shapes or test_order_days_per_replica_regrouped"
SELECTION_COUNT = len(WALKS) + len(SHAPES) + 1
SELECTION_SECONDS = 40


@pytest.mark.parametrize("target,lib,fill", [("dirty", "libvds_dirty.so", None), ("dirty", "libvds_dirty.so", "5A"), ("canary", "libvds_canary.so", None)],
                         ids=["dirty-A5", "dirty-5A", "canary"])
def test_every_element_is_written_on_dirty_and_guarded_memory(target, lib, fill):
    """The tiny walks, the shape cases and the per-replica-days walk of this file in one pytest subprocess under the dirty library
    (every byte the library obtains is filled with A5 / 5A before first use: an element the refresh missed reads as the pattern) and
    under the guarded one (a store outside the block damages a guard, found when the handle closes; a read beyond a row meets the
    poison).  "Every element is written", "nothing is read beyond a row" and "nothing is written beyond the block" can only be falsified
    here."""
    from test_gpu_debug_builds import build
    from test_gpu_dirty_memory import dirty_env, gpu_allowed, run_limited
    gpu_allowed()
    path = build(target, lib)
    argv = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k", SELECTION]
    rc, out = run_limited(argv, dirty_env(fill, path), 10 * SELECTION_SECONDS + 120, "the roster walks under %s (fill %s)" % (lib, fill or "A5"))
    print(out[-800:])
    assert rc == 0 and "%d passed" % SELECTION_COUNT in out, out[-6000:]
