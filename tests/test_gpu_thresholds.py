"""The host's layout and kernel thresholds (vds_api.hip load_static / load_orders), each on both sides: a city exactly at the
limit and one just past it (tests/threshold_cities.py), against the CPU oracle.  For every (row, side, mode):
  * the premise: ``main_kernel()`` and ``layout()`` (vds_debug_layout) name the form the host rules select on that side;
  * no refusal: both sides load and run;
  * parity, every replica: the five observation planes, the counters and the idle / arrival lists in container order after every slot,
    per-order status / vehicle / wait and all 8 counters at the end of the day - stepping slot by slot and as one ``run(T)``.
Row 10 covers the dispatch kernels: K = 64 / 65 device actions, more than 64 host-list actions in one (replica, cluster) group, and
dispatch costs whose sum passes 2^31 (host lists, a device tensor, a hooked slot).

Out of scope, the inputs being too large for a test: V >= 2^24 vehicles and >= 2^25 orders per day (the dense layout's packed ids),
vds_reset_random's LDS limit of 15 760 clusters, and arrival minutes beyond int32 (a slot length or a day whose own minutes do not
fit is refused on the host: tests/test_order_tables.py, tests/test_slot_length_limits.py).  Every city here runs 10-minute slots; the
slot-length axis, 1 .. 1440 minutes, and days beyond slot 32767 are tests/test_gpu_slot_lengths.py."""
import os

import numpy as np
import pytest

import threshold_cities as tc
from oracle.oracle import COUNTER_NAMES
from test_gpu_parity import MODES, check_lists
from vehicles_dispatch_simulator_amd import BatchedDispatchEnv
from vehicles_dispatch_simulator_amd.env import neighbors_to_csr

pytestmark = pytest.mark.gpu

OBS_MAP = (("idle_pre", "idle_pre"), ("idle_now", "idle_post"), ("supply", "supply"), ("cl_orders", "cl_orders"), ("inflight", "inflight"))
PLAIN_MODES = ("fast", "dense16", "dense_alt", "dense_slow", "rows", "generic")
# the dense tick's 8-lane form with its full 128-entry tables and no per-slot choice of form (row 6: the 128-entry limit)
LOCAL_MODES = {"dense8": {"dense_debug": (8, 0, 0, 0)}}


def make_env(c, mode, stream=None):
    kw = dict({**MODES, **LOCAL_MODES}[mode])
    kw.pop("supply_inplace", None)
    environ = kw.pop("environ", None) or {}
    saved = {k: os.environ.get(k) for k in environ}
    os.environ.update(environ)
    try:
        off, idx = neighbors_to_csr(c["nbr"])
        env = BatchedDispatchEnv(c["cost"], c["n2c"], off, idx, replicas=tc.R, vehicles=c["V"], depth_limit=c["depth"],
                                 neighbor_can_server=c["neighbor"], tick_minutes=tc.TICK, reject_threshold=c["threshold"],
                                 idle_cap=c["idle_cap"], far_cap=c["far_cap"], ring_cap=c["ring_cap"], stream=stream, **kw)
        env.load_orders(c["rel"], c["pick"], c["dele"])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return env


def check_premise(env, kernel, layout, tag):
    assert env.main_kernel() == kernel, (tag, env.main_kernel(), env.layout())
    if layout:
        got = env.layout()
        assert {k: got[k] for k in layout} == layout, (tag, got)


def check_slot(env, oracles, t, tag):
    ob, cn = env.obs(), env.counters()
    for r, o in enumerate(oracles):
        oo, oc = o.obs(), o.counters()
        for a, b in OBS_MAP:
            np.testing.assert_array_equal(ob[a][r], oo[b], err_msg="%s slot %d replica %d obs %s" % (tag, t, r, a))
        for i, k in enumerate(COUNTER_NAMES):
            if k != "sum_order_value":         # (compared at the end of the day, as tests/test_gpu_parity.py does)
                assert cn[r, i] == oc[k], (tag, t, r, k, int(cn[r, i]), oc[k])
        check_lists(env, r, o, t)


def check_day_end(env, oracles, tag):
    env.sync()
    od, cn = env.orders(), env.counters()
    for r, o in enumerate(oracles):
        oo, oc = o.orders(), o.counters()
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(od[k][r], oo[k], err_msg="%s replica %d %s" % (tag, r, k))
        for i, k in enumerate(COUNTER_NAMES):
            assert cn[r, i] == oc[k], (tag, r, k, int(cn[r, i]), oc[k], "engine - oracle = %d" % (int(cn[r, i]) - oc[k]))


def run_parity(c, mode, kernel, layout=None, tag=""):
    """The day slot by slot (every plane and list after every slot), then again as one run(T); returns work() of the stepped day."""
    tag = "%s %s" % (tag, mode)
    env = make_env(c, mode)
    check_premise(env, kernel, layout, tag)
    env.reset(c["init"])
    oracles = [tc.oracle_for(c, r) for r in range(tc.R)]
    assert env.T == oracles[0].num_ticks
    for t in range(env.T):
        env.step()
        for o in oracles:
            o.begin_tick()
        check_slot(env, oracles, t, tag)
        env.advance()
        for o in oracles:
            o.end_tick()
    check_day_end(env, oracles, tag)
    work = env.work()
    env.reset(c["init"])
    env.run(env.T)
    check_day_end(env, oracles, tag + " run(T)")
    env.close()
    return work


def plain_kernel(mode, dense, fast_ok):
    if mode == "generic" or not fast_ok:
        return "k_tick"
    if mode == "rows" or not dense:
        return "k_tick_rows"
    return "k_tick_dense"


# (row, builder, side) -> (dense layout chosen by default, fast_ok, layout() words of the default mode)
PLAIN_ROWS = {
    ("1-cluster-255", tc.cluster_size, 0): (1, 1, dict(dense=1, blk8=1, u8_ok=1)),
    ("1-cluster-256", tc.cluster_size, 1): (0, 1, dict(dense=0, blk8=-1, u8_ok=1)),
    ("2-in-cluster-254", tc.byte_max, 0): (1, 1, dict(dense=1, blk8=1, u8_ok=1, cost8=1)),
    ("2-in-cluster-255", tc.byte_max, 1): (1, 1, dict(dense=1, blk8=0, u8_ok=1, cost8=1)),
    ("3-cross-255", lambda s: tc.cross_max(s, False), 0): (1, 1, dict(dense=1, blk8=1, u8_ok=1, cost8=1)),
    ("3-cross-256", lambda s: tc.cross_max(s, False), 1): (1, 1, dict(dense=1, blk8=0, u8_ok=0, cost8=0)),
    ("4-int-block-127", tc.lds_int_block, 0): (1, 1, dict(dense=1, blk8=0)),
    ("4-int-block-128", tc.lds_int_block, 1): (0, 1, dict(dense=0, blk8=0)),
    ("5-cmax-2^23-1", tc.fast_cmax, 0): (1, 1, dict(dense=1, fast_ok=1, blk8=0)),
    ("5-cmax-2^23", tc.fast_cmax, 1): (0, 0, dict(dense=0, fast_ok=0)),
    ("5-cmin-0", tc.fast_cmin, 0): (1, 1, dict(dense=1, fast_ok=1)),
    ("5-cmin--1", tc.fast_cmin, 1): (0, 0, dict(dense=0, fast_ok=0)),
    ("5-threshold-cmax", tc.reject_window, 0): (1, 1, dict(dense=1, fast_ok=1, window_live=0)),
    ("5-threshold-cmax-1", tc.reject_window, 1): (0, 0, dict(dense=0, fast_ok=0, window_live=1)),
}


@pytest.mark.parametrize("key", list(PLAIN_ROWS), ids=[k[0] for k in PLAIN_ROWS])
def test_plain_threshold_both_sides(key):
    name, build, side = key
    dense, fast_ok, layout = PLAIN_ROWS[key]
    c = build(side)
    for mode in PLAIN_MODES:
        run_parity(c, mode, plain_kernel(mode, dense, fast_ok), layout if mode == "fast" else None, tag=name)


@pytest.mark.parametrize("side", [0, 1])
def test_bucket_orders_64_65_fast_path(side):
    """Row 6: 64 orders of one (cluster, slot) stay on the dense tick's fast path, 65 leave it (work()["slow_path_buckets"])."""
    c = tc.bucket_orders(side)
    for mode in ("fast", "dense16"):
        work = run_parity(c, mode, "k_tick_dense", dict(dense=1, blk8=1), tag="6-orders-%d" % (64 + side))
        assert (work["slow_path_buckets"] > 0) == bool(side), (mode, work)
    for mode in ("dense_slow", "rows", "generic"):
        run_parity(c, mode, plain_kernel(mode, 1, 1), tag="6-orders-%d" % (64 + side))


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("tab", [128, 256])
def test_bucket_entries_fast_path(side, tab):
    """Row 6: a bucket whose list holds 128 / 129 entries stays on / leaves the fast path of the 8-lane form (128-entry tables), one of
    256 / 257 entries that of the 16-lane form with 256-entry tables (byte costs), on one shared day."""
    c = tc.bucket_entries(side, tab)
    form = "dense8" if tab == 128 else "dense16"
    tag = "6-entries-%d" % (tab + side)
    work = run_parity(c, form, "k_tick_dense", dict(dense=1, blk8=1), tag=tag)
    assert (work["slow_path_buckets"] > 0) == bool(side), (form, work)
    for mode in ("fast", "dense_slow", "rows", "generic"):
        run_parity(c, mode, plain_kernel(mode, 1, 1), tag=tag)


@pytest.mark.parametrize("side", [0, 1])
def test_bucket_arrivals_64_65_fast_path(side):
    """Row 6: 64 arrivals in one (cluster, slot) stay on the dense tick's fast path, 65 leave it, in both forms."""
    c = tc.bucket_arrivals(side)
    tag = "6-arrivals-%d" % (64 + side)
    for form in ("dense8", "dense16"):
        work = run_parity(c, form, "k_tick_dense", dict(dense=1, blk8=1), tag=tag)
        assert (work["slow_path_buckets"] > 0) == bool(side), (form, work)
    for mode in ("fast", "dense_slow", "rows", "generic"):
        run_parity(c, mode, plain_kernel(mode, 1, 1), tag=tag)


# neighbour search: (row, builder, side) -> ({mode: kernel}, layout() words of the default mode)
SEARCH_ROWS = {
    ("3-search-cross-255", lambda s: tc.cross_max(s, True), 0):
        (dict(fast="k_dfs_dense", dfs_v2="k_tick_replica2", dfs_wide="k_dfs_hybrid", generic="k_match_dfs"), dict(dense=1, dense_st=1, blk8=1, cost8=1)),
    ("3-search-cross-256", lambda s: tc.cross_max(s, True), 1):
        (dict(fast="k_dfs_hybrid", dfs_v2="k_tick_replica2", dfs_wide="k_dfs_hybrid", generic="k_match_dfs"), dict(dense=0, dense_st=0, u8_ok=0, cost8=0)),
    ("7-search-cost-32767", tc.search_cost, 0): (dict(fast="k_dfs_hybrid", dfs_v2="k_tick_replica2", generic="k_match_dfs"), dict(dense_st=0, fast_ok=1)),
    ("7-search-cost-32768", tc.search_cost, 1): (dict(fast="k_match_dfs", dfs_v2="k_match_dfs", generic="k_match_dfs"), dict(dense_st=0, fast_ok=1)),
    ("8-V-16384", lambda s: tc.dense_search_capacity(s, "V"), 0): (dict(fast="k_dfs_dense", dfs_v2="k_tick_replica2"), dict(dense_st=1)),
    ("8-V-16385", lambda s: tc.dense_search_capacity(s, "V"), 1): (dict(fast="k_dfs_hybrid", dfs_v2="k_tick_replica2"), dict(dense_st=0)),
    ("8-idle_cap-16384", lambda s: tc.dense_search_capacity(s, "idle_cap"), 0): (dict(fast="k_dfs_dense", dfs_v2="k_tick_replica2"), dict(dense_st=1)),
    ("8-idle_cap-16385", lambda s: tc.dense_search_capacity(s, "idle_cap"), 1): (dict(fast="k_tick_replica2"), dict(dense_st=0)),
}
for _L, _pad in ((64, 64), (65, 128), (128, 128), (129, 256), (256, 256)):
    SEARCH_ROWS[("9-sequence-%d" % _L, tc.visit_sequence, _L)] = (dict(fast="k_dfs_dense", dfs_wide="k_dfs_hybrid", dfs_v2="k_tick_replica2"),
                                                                  dict(dense_st=1, seq_pad=_pad))
SEARCH_ROWS[("9-sequence-257", tc.visit_sequence, 257)] = (dict(fast="k_tick_replica2", dfs_wide="k_tick_replica2", generic="k_match_dfs"), dict(dense_st=0))


@pytest.mark.parametrize("key", list(SEARCH_ROWS), ids=[k[0] for k in SEARCH_ROWS])
def test_search_threshold_both_sides(key):
    name, build, side = key
    kernels, layout = SEARCH_ROWS[key]
    c = build(side)
    for mode, kernel in kernels.items():
        run_parity(c, mode, kernel, layout if mode == "fast" else None, tag=name)


def test_dense_search_loads_after_the_capacity_was_raised_on_a_wide_day():
    """The refusal of vds_load_orders where the dense neighbour-search layout is chosen but the hybrid tick's tables are then refused
    (idle_cap > 16 384 allocated): a capacity raised while a wide-layout day is loaded cannot pass 16 384 for V <= 16 384 - the dense
    layout's own condition - since vds_set_idle_cap and the reset's automatic growth both stop at V rounded up to 64.  So the next day
    loads on the dense layout and runs, with the full 16 384-entry list of row 8."""
    c = dict(tc.dense_search_capacity(0, "V"), idle_cap=0)
    env = make_env(c, "fast")
    check_premise(env, "k_dfs_dense", dict(dense_st=1), "one day")
    day = (c["rel"], c["pick"], c["dele"])
    env.load_order_days([day, day])                 # (two order days: the wide layout)
    assert env.layout()["dense_st"] == 0
    env.reset(c["init"])
    env.set_idle_cap(1 << 20)
    assert env.idle_cap == 16384
    env.load_orders(c["rel"], c["pick"], c["dele"])
    check_premise(env, "k_dfs_dense", dict(dense_st=1), "reloaded")
    assert env.idle_cap == 16384
    env.reset(c["init"])
    env.run(env.T)
    oracles = [tc.oracle_for(c, r) for r in range(tc.R)]
    for o in oracles:
        o.run_day()
    check_day_end(env, oracles, "reloaded")
    env.close()


# ---- row 10: the dispatch kernels -----------------------------------------------------------------------------------------------

def dispatch_day(c, mode, how, kernel):
    """Slot 0's hook moves the first k idle vehicles of cluster 0 of every replica to the case's target node - through host lists
    (vds_apply_dispatch: k_dispatch), a device tensor (k_dispatch_dense) or a hooked slot (vds_run_hooked) - against Oracle.dispatch;
    every plane, list and counter after every later slot, orders and counters at the end of the day.  Returns the oracles."""
    import torch
    k, tgt = c["facts"]["k"], c["facts"]["target"]
    stream = torch.cuda.current_stream().cuda_stream if how != "host" else None
    env = make_env(c, mode, stream=stream)
    check_premise(env, kernel, None, (mode, how))
    env.reset(c["init"])
    oracles = [tc.oracle_for(c, r) for r in range(tc.R)]
    one = np.stack([np.zeros(k), np.arange(k), np.full(k, tgt)], 1).astype(np.int32)
    acts = torch.from_numpy(np.ascontiguousarray(np.tile(one, (tc.R, 1, 1)))).cuda()
    for t in range(env.T):
        hooked = t == 0 and how == "hooked"
        if hooked:
            env.run_hooked(1, actions=acts)          # step -> planes -> actions -> advance
        else:
            env.step()
        for o in oracles:
            o.begin_tick()
        if not hooked:
            check_slot(env, oracles, t, (mode, how))
        if t == 0:
            for o in oracles:
                L = o.lists()
                seg = L["idle_veh"][L["idle_off"][0]:L["idle_off"][1]]
                assert seg.size >= k
                o.dispatch(seg[:k], np.full(k, tgt))
            if how == "host":
                env.apply_dispatch(np.repeat(np.arange(tc.R), k), np.zeros(tc.R * k), np.tile(np.arange(k), tc.R), np.full(tc.R * k, tgt))
            elif how == "device":
                env.apply_dispatch_torch(acts)
            torch.cuda.synchronize()
            if not hooked:          # (the planes are the oracle's before the hook: lists and counters after it)
                cn = env.counters()
                for r, o in enumerate(oracles):
                    check_lists(env, r, o, t)
                    oc = o.counters()
                    assert [int(cn[r, i]) for i in (4, 5)] == [oc["dispatch_num"], oc["dispatch_cost"]], ((mode, how), r, cn[r], oc)
        if not hooked:
            env.advance()
        for o in oracles:
            o.end_tick()
    check_day_end(env, oracles, (mode, how))
    env.close()
    return oracles


@pytest.mark.parametrize("how", ["host", "device", "hooked"])
def test_dispatch_cost_sum_past_2_31(how):
    """Row 10c: 32 dispatches at RoadCost 2^26 out of one cluster in one call on the generic layout: DispatchCost = 2^31 per replica
    (a 32-bit wavefront sum wraps to -2^31: the counter ends 2^32 too low)."""
    c = tc.dispatch_wrap()
    for mode in ("fast", "generic"):
        oracles = dispatch_day(c, mode, how, "k_tick")
        assert all(o.counters()["dispatch_cost"] == 1 << 31 for o in oracles)


@pytest.mark.parametrize("how", ["host", "device"])
def test_dispatch_dense_control_64_at_2_23(how):
    """Row 10a / control: 64 dispatches at RoadCost 2^23 - 1 in one call on the dense layout (K = 64 device actions accepted)."""
    c = tc.dispatch_dense_control()
    oracles = dispatch_day(c, "fast", how, "k_tick_dense")
    assert all(o.counters()["dispatch_cost"] == 64 * ((1 << 23) - 1) for o in oracles)


def test_dispatch_device_k65_refused():
    """Row 10a: K = 65 device actions are refused."""
    import torch
    c = tc.dispatch_dense_control()
    env = make_env(c, "fast", stream=torch.cuda.current_stream().cuda_stream)
    env.reset(c["init"])
    env.step()
    with pytest.raises(Exception, match="K must be in"):
        env.apply_dispatch_torch(torch.full((tc.R, 65, 3), -1, dtype=torch.int32, device="cuda"))
    env.close()


@pytest.mark.parametrize("mode", ["fast", "generic", "rows"])
def test_dispatch_host_group_of_70(mode):
    """Row 10b: 70 host-list actions of one (replica, cluster) group: k_dispatch takes them in two 64-action chunks."""
    dispatch_day(tc.dispatch_many(), mode, "host", plain_kernel(mode, 1, 1))
