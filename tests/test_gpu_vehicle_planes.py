"""Per-vehicle state of every replica as device planes (vds_vehicles_device / vds_read_vehicles_all; ``env.vehicles_torch``,
``env.vehicles_all``): int32 [6][R][V] - state, node, cluster, arrive_min, order, source - for all replicas at once.  Every checked
replica is compared, bit for bit, with (a) ``env.vehicles(r)``, the synchronous one-replica host path (itself pinned to the oracle by
``test_gpu_parity.check_lists``), and (b) the CPU oracle directly, with the assertions ``check_lists`` makes.  The ``source`` plane
(where the engine keeps the vehicle) says which container of the kernel served an element: the coverage test asserts that the day
walks reached every container on both layouts.  The corpus has no fixture with 0 vehicles, so that size is not among the odd ones."""
import ctypes
import functools
import gc
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import threshold_cities as tc
from helpers import check_oracle, dispatch_by_tick, host_view, load_golden, make_oracle
from test_gpu_parity import MODES, make_env
from test_gpu_replica_days import mk_env, mk_oracle, synth_days
from vehicles_dispatch_simulator_amd import _lib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("state", "node", "cluster", "arrive_min", "order")
VDS_EINVAL = -1


def check_planes(env, oracles, tag, seen=None):
    """Every plane of every replica against env.vehicles(r) and, where given, against the replica's oracle; returns the planes."""
    got = env.vehicles_all(source=True)
    assert set(got) == set(FIELDS) | {"source"}
    for k, a in got.items():
        assert a.shape == (env.R, env.V) and a.dtype == np.int32, (tag, k)
    for r in range(env.R):
        W = host_view(env, r)
        for k in FIELDS:
            np.testing.assert_array_equal(got[k][r], W[k], err_msg="%s replica %d %s against env.vehicles" % (tag, r, k))
        if oracles[r] is not None:
            check_oracle({k: got[k][r] for k in got}, oracles[r], env.V, env.C, "%s replica %d" % (tag, r))
    if seen is not None:
        src, order = got["source"], got["order"]
        seen["sources"] |= set(np.unique(src).tolist())
        seen["ring_order"] |= bool(((src == 2) & (order >= 0)).any())
        seen["ring_dispatch"] |= bool(((src == 2) & (order == -1)).any())
    return got


def seeded_init(g, R):
    """Replica 0 on the fixture's start nodes, the others seeded as test_gpu_parity.run_day seeds them."""
    V, N = int(g["V"]), int(g["N"])
    valid = g["node2cluster"] >= 0
    init = np.empty((R, V), dtype=np.int32)
    if V:
        init[0] = g["veh_node"][:V] if len(g["veh_node"]) >= V else synth.init_vehicle_nodes(random.Random(1000), N, V, valid)
    for r in range(1, R):
        init[r] = synth.init_vehicle_nodes(random.Random(1000 + r), N, V, valid)
    return init


# ---- 1. the day walk -----------------------------------------------------------------------------------------------------------------
# (fixture, mode, how the fixture's dispatch is applied) - the pairs that together reach every container on both layouts
DAY_WALK = [
    ("tiny_kmeans", "fast", "host"), ("tiny_kmeans", "fast_sup", "host"),                       # static arrival slots
    ("tiny_kmeans", "dense_ring", "host"),                                                     # order-carrying ring entries, dense
    ("tiny_grid", "far", "host"), ("tiny_kmeans", "dense_far", "host"), ("tiny_kmeans", "dense_ring_far", "host"),      # far list + inbox
    ("tiny_kmeans", "rows_far", "host"), ("tiny_grid", "far_generic", "host"),
    ("tiny_kmeans", "generic", "host"), ("tiny_kmeans", "rows", "host"),                        # wide layout
    ("tiny_kmeans_dfs2", "fast", "host"), ("tiny_kmeans_dfs2", "dfs_wide", "host"),             # dense stamp form / wide neighbour search
    ("tiny_dispatch", "fast", "host"), ("tiny_dispatch", "fast", "device"), ("tiny_dispatch", "rows", "host"),      # ring dispatch entries, ring_min
    ("tiny_dispatch_delay", "fast", "host"),
    ("tiny_tick5", "fast", "host"),                                                            # 5-minute slots
]


@functools.lru_cache(maxsize=None)
def day_walk(name, mode, how):
    """One day slot by slot with R = 3: the planes after the reset, after every step, after the slot's dispatch where the fixture has
    one (replica 0, as the reference's hook did) and after the advance of the last slot.  Returns what the source plane showed."""
    g = load_golden(name)
    R = 3
    kw = dict(MODES[mode])
    want_sup = kw.pop("supply_inplace", False)
    if how == "device":
        import torch
        kw["stream"] = torch.cuda.current_stream().cuda_stream
    init = seeded_init(g, R)
    env = make_env(g, R, **kw)
    if want_sup:
        env.supply_inplace_torch()
    env.reset(init)
    oracles = []
    for r in range(R):
        o = make_oracle(g)
        o.reset(init[r])
        oracles.append(o)
    seen = dict(sources=set(), ring_order=False, ring_dispatch=False, dense=int(env.layout()["dense"]), dispatched=0)
    tag = "%s %s %s" % (name, mode, how)
    check_planes(env, oracles, tag + " after reset", seen)
    disp = dispatch_by_tick(g)
    extra = int(g["dispatch_extra_minutes"]) if "dispatch_extra_minutes" in g else 0
    T = env.T
    assert T == oracles[0].num_ticks
    for t in range(T):
        env.step()
        for o in oracles:
            o.begin_tick()
        check_planes(env, oracles, "%s slot %d" % (tag, t), seen)
        if t in disp:
            rows = np.array(disp[t])
            Lo = oracles[0].lists()
            pos = []
            for veh, cl in zip(rows[:, 1], rows[:, 2]):
                seg = Lo["idle_veh"][Lo["idle_off"][cl]:Lo["idle_off"][cl + 1]]
                pos.append(int(np.flatnonzero(seg == veh)[0]))
            if how == "device":
                acts = np.full((R, len(rows) + 2, 3), -1, dtype=np.int32)
                acts[0, 1:len(rows) + 1, 0] = rows[:, 2]; acts[0, 1:len(rows) + 1, 1] = pos; acts[0, 1:len(rows) + 1, 2] = rows[:, 4]
                env.apply_dispatch_torch(torch.from_numpy(acts).cuda())
                oracles[0].dispatch(rows[:, 1], rows[:, 4])
            elif extra:
                am = oracles[0].now_min + rows[:, 5] + extra
                env.apply_dispatch(np.zeros(len(rows), dtype=np.int32), rows[:, 2], pos, rows[:, 4], arrive_min=am)
                oracles[0].dispatch_at(rows[:, 1], rows[:, 4], arrive_min=am)
            else:
                env.apply_dispatch(np.zeros(len(rows), dtype=np.int32), rows[:, 2], pos, rows[:, 4])
                oracles[0].dispatch(rows[:, 1], rows[:, 4])
            seen["dispatched"] += len(rows)
            check_planes(env, oracles, "%s slot %d after dispatch" % (tag, t), seen)
        env.advance()
        for o in oracles:
            o.end_tick()
    check_planes(env, oracles, tag + " after the last advance", seen)
    env.close()
    return seen


@pytest.mark.parametrize("name,mode,how", DAY_WALK, ids=["%s-%s-%s" % e for e in DAY_WALK])
def test_planes_equal_host_view_and_oracle_at_every_slot(name, mode, how):
    seen = day_walk(name, mode, how)
    assert 0 in seen["sources"]
    if name.startswith("tiny_dispatch"):
        assert seen["dispatched"] > 0 and seen["ring_dispatch"]


# ---- 2. the coverage condition -------------------------------------------------------------------------------------------------------
def test_every_container_was_read_on_both_layouts():
    """Over the day walks (computed once per process), from the source plane: every container 0 .. 4 at some checked slot; on the
    dense layout ring entries with and without an order; on the wide layout the idle list, the ring, the far list and the far inbox."""
    dense = dict(sources=set(), ring_order=False, ring_dispatch=False)
    wide = set()
    for e in DAY_WALK:
        s = day_walk(*e)
        if s["dense"]:
            dense["sources"] |= s["sources"]
            dense["ring_order"] |= s["ring_order"]
            dense["ring_dispatch"] |= s["ring_dispatch"]
        else:
            wide |= s["sources"]
    assert {0, 1, 2, 3, 4} <= dense["sources"] | wide, (dense, wide)
    assert {0, 1, 2, 3, 4} <= dense["sources"], dense
    assert dense["ring_order"] and dense["ring_dispatch"], dense
    assert {0, 2, 3, 4} <= wide, wide
    assert -1 not in dense["sources"] | wide


# ---- 3. long lists and full tables ------------------------------------------------------------------------------------------------------
from test_gpu_thresholds import make_env as make_threshold_env  # noqa: E402


@pytest.mark.parametrize("tab,mode", [(128, "dense8"), (256, "dense16"), (256, "rows")])
def test_idle_lists_beyond_the_fast_path_tables(tab, mode):
    """A list of tab + 1 entries in one bucket (threshold_cities.bucket_entries): more entries than the lanes of a bucket take in one step."""
    c = tc.bucket_entries(1, tab)
    env = make_threshold_env(c, mode)
    env.reset(c["init"])
    oracles = [tc.oracle_for(c, r) for r in range(tc.R)]
    assert np.diff(oracles[0].lists()["idle_off"])[0] == tab + 1
    got = check_planes(env, oracles, "entries-%d %s after reset" % (tab + 1, mode))
    assert ((got["cluster"] == 0) & (got["state"] == 0)).sum(axis=1).tolist() == [tab + 1] * tc.R
    for t in range(env.T):
        env.step()
        for o in oracles:
            o.begin_tick()
        check_planes(env, oracles, "entries-%d %s slot %d" % (tab + 1, mode, t))
        env.advance()
        for o in oracles:
            o.end_tick()
    env.close()


@pytest.mark.parametrize("mode", ["fast", "rows"])
def test_seventy_dispatches_out_of_one_bucket(mode):
    """threshold_cities.dispatch_many: 70 vehicles of cluster 0 of every replica sent to one node in slot 0 - 70 ring / far entries
    without an order in one destination bucket."""
    c = tc.dispatch_many()
    k, tgt = c["facts"]["k"], c["facts"]["target"]
    env = make_threshold_env(c, mode)
    env.reset(c["init"])
    oracles = [tc.oracle_for(c, r) for r in range(tc.R)]
    for t in range(min(env.T, 8)):
        env.step()
        for o in oracles:
            o.begin_tick()
        if t == 0:
            for o in oracles:
                L = o.lists()
                o.dispatch(L["idle_veh"][L["idle_off"][0]:L["idle_off"][1]][:k], np.full(k, tgt))
            env.apply_dispatch(np.repeat(np.arange(tc.R), k), np.zeros(tc.R * k), np.tile(np.arange(k), tc.R), np.full(tc.R * k, tgt))
        got = check_planes(env, oracles, "dispatch_many %s slot %d" % (mode, t))
        if t == 0:
            assert ((got["state"] == 2) & (got["node"] == tgt)).sum(axis=1).tolist() == [k] * tc.R
        env.advance()
        for o in oracles:
            o.end_tick()
    env.close()


# ---- 4. order days per replica ----------------------------------------------------------------------------------------------------------
def replica_days_case(R, replica_day, n_days, n_inits, regrouped, seed):
    """Replica r replays day replica_day[r] from start nodes init[r % n_inits]; one oracle per (day, start) pair.  The planes of
    every replica against its own oracle at three slots - the middle one after the shortest day has ended - and after the last advance."""
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
    assert env.T == max(Ts.values()) and min(Ts.values()) + 10 < env.T      # some days are over while others still run
    per_replica = lambda: [oracles[(int(replica_day[r]), r % n_inits)] for r in range(R)]
    at = {3, min(Ts.values()) + 5, env.T - 2}
    for t in range(env.T):
        env.step()
        for k, o in oracles.items():
            if t < Ts[k]:
                o.begin_tick()
        if t in at:
            check_planes(env, per_replica(), "days R=%d slot %d" % (R, t))
            if t == min(Ts.values()) + 5:         # (a day that is over and a running one, at the same checked slot)
                assert any(T_k <= t for T_k in Ts.values()) and any(T_k > t for T_k in Ts.values())
        env.advance()
        for k, o in oracles.items():
            if t < Ts[k]:
                o.end_tick()
    check_planes(env, per_replica(), "days R=%d after the last advance" % R)
    env.close()


def test_days_interleaved_and_stored_regrouped():
    """Three days interleaved over 40 replicas: stored as 3 x 16 with padding replicas (int2ext); the block stays in the caller's order."""
    replica_days_case(40, np.arange(40) % 3, 3, 2, True, seed=5300)


def test_every_row_its_own_order_stream():
    replica_days_case(17, np.arange(17), 17, 17, False, seed=5200)


# ---- 5. the plane mask, the error codes, the block's address ----------------------------------------------------------------------------
def test_plane_mask_errors_and_addresses():
    import torch
    g = load_golden("tiny_kmeans")
    R = 3
    stream = torch.cuda.current_stream()
    env = make_env(g, R, stream=stream.cuda_stream)
    with pytest.raises(Exception, match="call vds_reset first"):
        env.vehicles_all()
    assert env._lib.vds_vehicles_device(env._h, 31, None) == VDS_EINVAL
    init = seeded_init(g, R)
    env.reset(init)
    for bad in (0, 64, -1):
        with pytest.raises(Exception, match=r"1 \.\. 63"):
            env.vehicles_device_ptr(bad)
        assert env._lib.vds_vehicles_device(env._h, bad, None) == VDS_EINVAL
        assert env._lib.vds_read_vehicles_all(env._h, bad, None) == VDS_EINVAL
    p = env.vehicles_device_ptr(63)
    full = env.vehicles_torch(source=True)                     # all six planes, views of the block
    assert set(full) == set(FIELDS) | {"source"} and full["state"].data_ptr() == p
    assert all(v.shape == (R, env.V) and v.dtype == torch.int32 and v.is_cuda for v in full.values())
    for _ in range(6):
        env.step(); env.advance()
    before = {k: v.clone() for k, v in env.vehicles_torch(source=True).items()}
    for _ in range(4):
        env.step(); env.advance()
    part = env.vehicles_torch(state=True, node=False, cluster=False, arrive_min=False, order=False)
    assert list(part) == ["state"] and part["state"].data_ptr() == p
    torch.cuda.synchronize()
    for k in ("node", "cluster", "arrive_min", "order", "source"):      # not requested: what the block held
        assert torch.equal(full[k], before[k]), k
    state = part["state"].cpu().numpy()
    assert (state != before["state"].cpu().numpy()).any()               # requested: new
    for r in range(R):
        np.testing.assert_array_equal(state[r], host_view(env, r)["state"])
    sub = env.vehicles_all(state=False, node=True, cluster=False, arrive_min=False, order=True)      # ascending bit order on the host
    assert list(sub) == ["node", "order"]
    for r in range(R):
        W = host_view(env, r)
        np.testing.assert_array_equal(sub["node"][r], W["node"]); np.testing.assert_array_equal(sub["order"][r], W["order"])
    # the address: fixed across steps and resets ...
    env.step()
    assert env.vehicles_device_ptr(1) == p
    env.reset(init)
    assert env.vehicles_device_ptr(31) == p
    # ... and after a load with other sizes the block is whatever the new tables need: the values are right
    n = len(g["o_release_min"]) // 3
    env.load_orders(g["o_release_min"][:n], g["o_pickup"][:n], g["o_delivery"][:n])
    env.reset(init)
    env.run(5)
    env.vehicles_device_ptr(63)
    check_planes(env, [None] * R, "after a load with other sizes")
    env.close()


# ---- 6. after the other entry points ----------------------------------------------------------------------------------------------------
def test_after_run_snapshot_restore_and_reset_again():
    g = load_golden("tiny_kmeans_dfs2")
    R = 3
    init = seeded_init(g, R)
    env = make_env(g, R)
    env.reset(init)

    def fresh(n):
        os_ = []
        for r in range(R):
            o = make_oracle(g)
            o.reset(init[r])
            for _ in range(n):
                o.begin_tick(); o.end_tick()
            os_.append(o)
        return os_

    env.run(20)                                            # (the day graph, with the stamp form's flush behind its last slot)
    check_planes(env, fresh(20), "after run(20)")
    env.snapshot()
    at_snapshot = fresh(20)
    for _ in range(4):
        env.step(); env.advance()
    perm = [2, 0, 1]
    env.restore(perm)
    got = check_planes(env, [at_snapshot[s] for s in perm], "after restore(permutation)")
    assert not np.array_equal(got["state"][0], got["state"][1])          # (the replicas differ: the permutation shows)
    env.step()
    stepped = [at_snapshot[s] for s in perm]
    for o in at_snapshot:
        o.begin_tick()
    check_planes(env, stepped, "a step after the restore")
    env.reset_again()                                      # in the middle of the day (and of a slot)
    os_ = fresh(0)
    check_planes(env, os_, "after reset_again")
    for t in range(2):
        env.step()
        for o in os_:
            o.begin_tick()
        check_planes(env, os_, "reset_again slot %d" % t)
        env.advance()
        for o in os_:
            o.end_tick()
    env.close()


# ---- 7. sizes off the kernels' grain ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,R,mode", [(1, 5, "fast"), (13, 5, "fast"), (13, 67, "rows"), (151, 1, "fast"), (37, 1, "generic")])
def test_odd_vehicle_and_replica_counts(V, R, mode):
    """V = 1, V prime, R = 1, R past one workgroup's 64 replicas and no multiple of the four a thread takes."""
    g = dict(load_golden("tiny_kmeans"))
    g["V"] = np.int64(V)
    init = seeded_init(g, R)
    g["veh_node"] = init[0]                                     # (make_oracle starts from the fixture's nodes before the reset below)
    env = make_env(g, R, **MODES[mode])
    env.reset(init)
    oracles = []
    for r in range(R):
        o = make_oracle(g) if r < 6 or r >= R - 3 else None      # (every replica against the host view; these also against an oracle)
        if o is not None:
            o.reset(init[r])
        oracles.append(o)
    check_planes(env, oracles, "V=%d R=%d after reset" % (V, R))
    for t in range(12):
        env.step()
        for o in oracles:
            if o is not None:
                o.begin_tick()
        if t % 3 == 2:
            check_planes(env, oracles, "V=%d R=%d slot %d" % (V, R, t))
        env.advance()
        for o in oracles:
            if o is not None:
                o.end_tick()
    env.close()


# ---- device blocks -----------------------------------------------------------------------------------------------------------------------
def device_blocks():
    gc.collect()          # (a handle some earlier test dropped without closing it goes now)
    out = np.zeros(2, dtype=np.int64)
    assert _lib.load().vds_debug_device_blocks(out.ctypes.data_as(ctypes.c_void_p)) == 0
    return int(out[0]), int(out[1])


def test_a_handle_that_used_the_block_gives_every_device_block_back():
    before = device_blocks()
    g = load_golden("tiny_kmeans")
    env = make_env(g, 3)
    env.reset(seeded_init(g, 3))
    env.step()
    held = device_blocks()
    env.vehicles_all(source=True)
    with_block = device_blocks()
    assert with_block[0] == held[0] + 1 and with_block[1] >= held[1] + 6 * 3 * env.V * 4      # one block more: the planes
    env.advance(); env.step()
    env.vehicles_all()
    assert device_blocks() == with_block                                                     # ... made once
    env.close()
    assert device_blocks() == before


# ---- guarded and self-checking builds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target,lib", [("canary", "libvds_canary.so"), ("dbg", "libvds_dbg.so")])
def test_guarded_and_self_checking_builds(target, lib):
    """This file's cases that read the most differently shaped tables - static arrival slots, the stamp form behind its flush, the far
    tables, the dense ring with dispatched vehicles, a 257-entry list on the wide layout - under the guarded library (a read beyond a
    table returns the poison, a write beyond the block damages a guard, found when the handle closes) and under the self-checking one
    (which reports a list that is not compact where the kernel reads it)."""
    from test_gpu_debug_builds import build
    env = dict(os.environ, VDS_LIB=build(target, lib))
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "tiny_kmeans-fast-host or tiny_kmeans_dfs2-fast-host or tiny_kmeans-rows_far-host or tiny_dispatch-fast-device or 256-rows"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "5 passed" in p.stdout, p.stdout[-500:]
    assert "raw list" not in p.stdout + p.stderr
