"""A handle gives back every device block it took (``vds_debug_device_blocks``: the live blocks of the process and their bytes, as the
one allocate / free pair of csrc/vds_mem.h counts them), on the paths that replace a block or a group of blocks in the middle of a
handle's life and that the API-sequence corpus (tests/test_gpu_api_sequences.py, which asserts the same balance per case) does not
reach: the block maps of the per-cluster forms, the idle-heads block for another L, the supply planes switched on late, the idle
tables regrown, the snapshot store re-made, the reset's list image regrown, the order tables recycled by a reload.

One handle per case on ``workloads.tiny`` cities.  Every case ends by comparing ``orders()`` and ``counters()`` with the oracle, so a
balance reached by freeing a block too early shows as a wrong result, and the count after ``close()`` must be the one before the
handle was made.  tests/test_gpu_debug_builds.py and tests/test_gpu_dirty_memory.py run this file again under the guarded and the
dirty library."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest

from oracle.oracle import Oracle
from vehicles_dispatch_simulator_amd import _lib, workloads

pytestmark = pytest.mark.gpu


def device_blocks():
    gc.collect()          # (a handle some earlier test dropped without closing it goes now, not in the middle of a case)
    out = np.zeros(2, dtype=np.int64)
    assert _lib.load().vds_debug_device_blocks(out.ctypes.data_as(C.c_void_p)) == 0
    return int(out[0]), int(out[1])


@contextlib.contextmanager
def balanced_env(w, R, **kw):
    before = device_blocks()
    env = w.make_env(R, **kw)
    try:
        assert device_blocks()[0] > before[0]
        yield env
    finally:
        env.close()
    assert device_blocks() == before, "close() left (blocks, bytes) %s, before the handle was made %s" % (device_blocks(), before)


def check_against_oracle(w, env, init, days=None, replica_day=None, replicas=None):
    """orders() and counters() of a finished day, as the worker of tests/test_gpu_debug_builds.py compares them (replicas: a sample of
    them, as that worker takes one at the larger batches; default all)"""
    got, cn = env.orders(), env.counters()
    R = init.shape[0]
    for r in (range(R) if replicas is None else replicas):
        rel, pk, dl = (w.release_min, w.pickup, w.delivery) if days is None else days[0 if replica_day is None else int(replica_day[r])]
        o = Oracle(w.city.cost, w.city.node2cluster, w.nbr_off, w.nbr_idx, w.depth_limit, w.neighbor_can_server, rel, pk, dl, w.vehicles)
        o.reset(init[r]); o.run_day()
        exp, oc = o.orders(), o.counters()
        n = exp["status"].size               # (rows are as long as the longest day)
        for k in ("status", "vehicle", "wait"):
            assert np.array_equal(got[k][r][:n], exp[k]), (r, k)
        assert cn[r, 7] == oc["evals"] and cn[r, 1] == oc["reject_num"], r


def short_day(w, n):
    return w.release_min[:n], w.pickup[:n], w.delivery[:n]


def test_device_blocks_block_map_regrown_by_a_longer_day(monkeypatch):
    """compile_forms: a seeded mixed plane (64 replicas: the smallest batch that runs mixed slots; byte costs) compiles block maps for
    every slot; the longer day's maps do not fit the block of the shorter one - read off the bytes around the reset that compiles
    them: the second one replaces a block by a larger one.  Every eleventh replica is compared with the oracle: a sample."""
    monkeypatch.setenv("VDS_DENSE_CLUSTER_SEED", "3")
    for k in ("VDS_DENSE_TICK_FORMS", "VDS_DENSE_TICK_LIM"):
        monkeypatch.delenv(k, raising=False)
    R = 64
    w = workloads.tiny(vehicles=700, orders=4000)
    init = w.vehicle_nodes(R)
    with balanced_env(w, R, load=False) as env:
        slots, resets = [], []
        for day in (short_day(w, 1200), short_day(w, 4000)):
            env.load_orders(*day)
            m = device_blocks()
            env.reset(init)                                                       # (adapt_dense writes the plane, compile_forms the block maps)
            resets.append((device_blocks()[0] - m[0], device_blocks()[1] - m[1]))
            env.run(env.T)
            per_slot = env.cluster_forms().sum(axis=1)
            assert per_slot.size == env.T and ((per_slot > 0) & (per_slot < env.C)).all(), "every slot mixes both forms"
            slots.append(env.T)
            check_against_oracle(w, env, init, days=[day], replicas=range(0, R, 11))
        assert slots[1] > slots[0], slots
        assert resets[0][0] > 0 and resets[1][0] == 0 and resets[1][1] > 0, resets          # a first block; then the same blocks, one of them larger


def test_device_blocks_idle_heads_for_two_and_then_five_positions():
    R = 2
    w = workloads.tiny()
    init = w.vehicle_nodes(R)
    with balanced_env(w, R) as env:
        env.reset(init)
        env.run(4)
        h2 = env.idle_heads(2)
        n = device_blocks()
        h5 = env.idle_heads(5)
        assert device_blocks()[0] == n[0] and device_blocks()[1] > n[1]          # the block of L = 2 went when the one of L = 5 came
        for k in ("veh", "node"):
            assert np.array_equal(h5[k][:, :, :2], h2[k]), k
        assert np.array_equal(env.idle_heads(2)["veh"], h2["veh"])
        env.run(env.T - 4)
        check_against_oracle(w, env, init)


def test_device_blocks_supply_planes_switched_on_after_a_day():
    R = 2
    w = workloads.tiny()
    init = w.vehicle_nodes(R)
    with balanced_env(w, R) as env:
        env.reset(init)
        env.run(env.T)
        n = device_blocks()
        ring, slot = env.supply_inplace_torch()                                   # the first request: two blocks join the state tables
        assert device_blocks()[0] == n[0] + 2
        assert env.supply_inplace_torch()[0].data_ptr() == ring.data_ptr() and device_blocks()[0] == n[0] + 2
        env.reset_again()
        env.run(env.T)
        check_against_oracle(w, env, init)


def test_device_blocks_idle_tables_regrown_then_reset():
    R = 3
    w = workloads.tiny()
    init = w.vehicle_nodes(R)
    with balanced_env(w, R) as env:
        env.reset(init)
        env.run(5)
        n, cap = device_blocks(), env.idle_cap
        env.set_idle_cap(cap + 64)
        assert env.idle_cap == cap + 64 and device_blocks()[0] == n[0] and device_blocks()[1] > n[1]
        env.reset(init)
        env.run(env.T)
        check_against_oracle(w, env, init)


def test_device_blocks_snapshot_store_remade_for_another_day():
    R = 2
    w = workloads.tiny()
    init = w.vehicle_nodes(R)
    with balanced_env(w, R) as env:
        env.reset(init)
        env.run(3)
        env.snapshot()
        first = env.snapshot_info()["bytes"]
        day = short_day(w, 900)
        env.load_orders(*day)                                                     # (the snapshot is void: its store goes with the next one)
        assert env.snapshot_info() is None
        env.reset(init)
        env.run(3)
        env.snapshot()
        assert env.snapshot_info()["bytes"] < first                               # (the result rows of the shorter day)
        env.run(env.T - 3)
        env.restore()
        env.run(env.T - 3)
        check_against_oracle(w, env, init, days=[day])


def test_device_blocks_reset_image_regrown_by_more_stored_replicas():
    """The city shape of test_reset_again_of_a_city_too_large_for_the_staged_reset (tests/test_gpu_edge_cases.py): the reset keeps a
    packed image of the lists, [stored replicas][V].  The vehicle count of a handle is fixed, so the image regrows with the stored
    replicas: a map that mixes two days inside groups of 16 stores 40 replicas regrouped as 48.  The bytes are read between the map
    change and the reset, so the growth is the image's alone.  Every seventh replica is compared with the oracle: a sample."""
    from test_order_tables import replica_plan
    N, Cn, V, R = 700, 37, 30000, 40
    w = workloads.tiny(N=N, C=Cn, vehicles=V, orders=1500, seed=5)
    days = workloads.distinct_days(w, 2)
    init = w.vehicle_nodes(R)
    mixed = np.array([0] * 24 + [1] * 16, dtype=np.int32)[np.random.default_rng(11).permutation(R)]
    assert replica_plan(mixed, 2, gran_small=1, alloc=R)[1]["R"] == 48
    with balanced_env(w, R, load=False) as env:
        env.load_order_days(days, np.zeros(R, dtype=np.int32))
        env.reset(init)
        n = device_blocks()
        env.reset_again()                                                         # (the image copied back)
        assert device_blocks() == n
        env.run(env.T // 2)
        env.set_replica_days(mixed)                                               # (re-makes the state and result tables for 48 replicas)
        m = device_blocks()
        env.reset(init)                                                           # 48 stored replicas: another image, nothing else
        grown = 4 * (48 - R) * V + 4 * (48 - R) * (Cn + 1)                        # image [stored replicas][V] u32, bases [stored replicas][C + 1] int32
        assert device_blocks() == (m[0], m[1] + grown), (device_blocks(), m, grown)
        env.reset_again()
        env.run(env.T)
        check_against_oracle(w, env, init, days=days, replica_day=mixed, replicas=range(0, R, 7))


def test_device_blocks_steady_over_reloads_of_the_same_day():
    R = 2
    w = workloads.tiny()
    init = w.vehicle_nodes(R)
    with balanced_env(w, R, load=False) as env:
        seen = []
        for cycle in range(3):
            env.load_orders(w.release_min, w.pickup, w.delivery)
            env.reset(init)
            env.run(env.T)
            env.sync()
            seen.append(device_blocks())
        assert seen[1][0] == seen[0][0] and seen[2][0] == seen[0][0], seen        # no block more per reload
        assert seen[2][1] == seen[1][1], seen                                     # recycling has reached its steady state
        check_against_oracle(w, env, init)
