"""Per-order results of every replica as a device block in id order (vds_orders_device, vds_run_hooked with vds_run_hooked_orders:
k_orders_block): the int32 [R, O, 2] block {vehicle, wait} checked bit for bit at EVERY slot against the block built from the goldens
captured from the unmodified reference or from the CPU oracle stepped alongside (orders_block_expect.py) - whole and as the partial
refresh (t, t) over a poisoned block - through every tick family, grids of more than one block, V = 0 and a one-order day, order days
per replica (regrouped storage with padding replicas), the one-graph hooked day with a captured recorder policy, snapshot / restore,
the block's lifetime, and on memory that starts out dirty."""
import ctypes
import gc
import os
import sys

import numpy as np
import pytest

from helpers import dispatch_by_tick, load_golden, make_oracle, oracle_apply
from orders_block_expect import PENDING, REJECTED, VEHICLE, WAIT, block_from_results, expected_after_slot, record_ranges, slot_ranges
from test_gpu_dispatch_vehicles import CAPS, assert_same_day, day_result
from test_gpu_parity import TINY, make_env
from test_gpu_replica_days import mk_env, mk_oracle, synth_days
from test_gpu_slot_outcomes import FAMILIES
from test_gpu_vehicle_outcomes import HG_R, hooked_expectation, seeded_init, to_dev
from test_order_tables import replica_plan
from vehicles_dispatch_simulator_amd import _lib
from vehicles_dispatch_simulator_amd.env import ORDER_PENDING, ORDER_REJECTED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -7
DENSE_KERNELS = ("k_tick_dense", "k_dfs_dense")

# what the cases of this file met (test_the_cases_met_what_they_were_chosen_for)
SEEN = dict(kernels=set(), day_modes=set(), regrouped=0, wide_range=0, empty_slot=0, rejected=0, neighbour_served=0, poison_kept=0,
            untouched_replica=0, padding_written=0)


def raw(env, blk):
    """The block as it stands, without a refresh."""
    import torch
    env.sync()
    torch.cuda.synchronize()
    return blk.cpu().numpy()


def refreshed(env, lo=0, hi=None):
    blk = env.orders_torch(lo, hi)
    assert tuple(blk.shape) == (env.R, env.O, 2) and str(blk.dtype) == "torch.int32" and blk.is_cuda
    return raw(env, blk)


def poison(env, blk):
    import torch
    env.sync()
    blk.fill_(POISON)
    torch.cuda.synchronize()


def assert_block(got, exp, tag):
    if not np.array_equal(got, exp):
        i = int(np.flatnonzero((got != exp).any(axis=-1))[0])
        pytest.fail("%s order %d: got %s, expected %s" % (tag, i, got[i].tolist(), exp[i].tolist()))


def assert_partial(got, exp, lo, hi, tag):
    """After a refresh of the id range [lo, hi) over a poisoned block: the range reads the expectation, every other row the poison."""
    assert_block(got[lo:hi], exp[lo:hi], tag + " (inside the range, from id %d)" % lo)
    assert (got[:lo] == POISON).all() and (got[hi:] == POISON).all(), tag + ": rows outside ids [%d, %d) were written" % (lo, hi)
    if lo > 0 or hi < got.shape[0]:
        SEEN["poison_kept"] += 1


def slot_range(off, t, T, O):
    """Ids the refresh (t, t) owns: the slot's own, and from the day's last slot on to the end of the row."""
    return int(off[t]), (O if t == T - 1 else int(off[t + 1]))


def note_day(env, g, off):
    SEEN["kernels"].add(env.main_kernel())
    SEEN["wide_range"] += int(np.diff(off).max() > 256)
    SEEN["empty_slot"] += int((np.diff(off) == 0).any())


# ---- 1. / 2. every slot of every tiny fixture, stepwise, through every tick family --------------------------------------------------------
def day_walk(name, R=3, kernel=None, **kw):
    """Replica 0 replays the reference's record (its dispatch log applied in the host form); replica 1 moves one vehicle in the K-form
    and replica 2 one in the vehicle form every fourth slot, each against an oracle stepped alongside."""
    g = load_golden(name)
    V, O = int(g["V"]), int(g["o_status"].size)
    init = seeded_init(g, R, first=g["veh_node"])
    off = record_ranges(g)                       # (one shared day: the slots' id ranges are every replica's)
    disp = dispatch_by_tick(g)
    extra = int(g["dispatch_extra_minutes"]) if "dispatch_extra_minutes" in g else 0
    valid = np.flatnonzero(g["node2cluster"] >= 0)
    oracles = [None]
    for r in range(1, R):
        o = make_oracle(g)
        o.reset(init[r])
        oracles.append(o)
    env = make_env(g, R, **kw)
    assert kernel is None or env.main_kernel() == kernel
    T = env.T
    assert env.O == O and off.size == T + 1
    note_day(env, g, off)
    env.reset(init)
    blk = env.orders_torch()                    # the first full refresh: every element, whatever the fresh block held
    got = raw(env, blk)
    assert (got[..., VEHICLE] == PENDING).all() and (got[..., WAIT] == -1).all()
    moved = 0
    for t in range(T):
        env.step()
        exp = [expected_after_slot(g, t)]
        for o in oracles[1:]:
            o.begin_tick()
            res = o.orders()
            exp.append(block_from_results(res["status"], res["vehicle"], res["wait"]))
        exp = np.stack(exp)
        got = refreshed(env)
        for r in range(R):
            assert_block(got[r], exp[r], "%s slot %d replica %d" % (name, t, r))
        # the partial refresh over a poisoned block: slot t's id range alone
        poison(env, blk)
        part = refreshed(env, t, t)
        lo, hi = slot_range(off, t, T, O)
        for r in range(R):
            assert_partial(part[r], exp[r], lo, hi, "%s slot %d replica %d, refresh (t, t)" % (name, t, r))
        got = refreshed(env)
        # the slot's dispatch calls do not change the block: host form (the reference's log), K-form, vehicle form
        held = []          # (the device tensors of the slot's calls, until the sync below)
        if t in disp:
            rows = np.array(disp[t])
            L = env.lists(0)
            pos = [int(np.flatnonzero(L["idle_veh"][L["idle_off"][cl]:L["idle_off"][cl + 1]] == veh)[0]) for veh, cl in zip(rows[:, 1], rows[:, 2])]
            rep = np.zeros(len(rows), dtype=np.int32)
            if extra:
                env.apply_dispatch(rep, rows[:, 2], pos, rows[:, 4], arrive_min=env.clock[1] + rows[:, 5] + extra)
            else:
                env.apply_dispatch(rep, rows[:, 2], pos, rows[:, 4])
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
            L = oracles[2].lists()
            if L["idle_off"][-1] > 0:
                tg = np.full((R, V), -1, dtype=np.int32)
                tg[2, L["idle_veh"][L["idle_off"][-1] - 1]] = node
                held.append(to_dev(tg))
                env.apply_dispatch_vehicles_torch(held[-1])
                moved += oracle_apply(oracles[2], tg[2])[0]
        np.testing.assert_array_equal(raw(env, blk), got, err_msg="slot %d: dispatch changed the block" % t)
        np.testing.assert_array_equal(refreshed(env), got, err_msg="slot %d: a refresh behind the dispatch calls differs" % t)
        env.advance()
        for o in oracles[1:]:
            o.end_tick()
        np.testing.assert_array_equal(raw(env, blk), got, err_msg="slot %d: advance changed the block" % t)
        np.testing.assert_array_equal(refreshed(env), got, err_msg="slot %d: a refresh behind advance differs" % t)
    check_day_end(env, refreshed(env), name)
    np.testing.assert_array_equal(env.orders()["status"][0], g["o_status"])
    SEEN["day_modes"].add("shared")
    if int(g["depth_limit"]) >= 1 and bool(g["neighbor_can_server"]):
        from helpers import recorded_day_facts
        SEEN["neighbour_served"] += int(recorded_day_facts(g)["cross"] > 0)
    return env, dict(moved=moved, rejected=int((got[..., VEHICLE] == REJECTED).sum()), matched=int((got[..., VEHICLE] >= 0).sum()))


def check_day_end(env, got, tag):
    """Word for word against vds_read_orders, and the served / rejected / wait sums against the counters."""
    od = env.orders()
    st = od["status"]
    np.testing.assert_array_equal(got[..., VEHICLE] >= 0, st == 1, err_msg=tag)
    np.testing.assert_array_equal(got[..., VEHICLE] == ORDER_REJECTED, st == 2, err_msg=tag)
    np.testing.assert_array_equal(got[..., VEHICLE] == ORDER_PENDING, st == 0, err_msg=tag)
    np.testing.assert_array_equal(got[..., VEHICLE][st != 0], od["vehicle"][st != 0], err_msg=tag)
    np.testing.assert_array_equal(got[..., WAIT], od["wait"], err_msg=tag)
    cn = env.counters()          # order_num, reject_num, matched, wait_sum, ...
    served = got[..., VEHICLE] >= 0
    np.testing.assert_array_equal(served.sum(axis=1), cn[:, 0] - cn[:, 1], err_msg=tag)
    np.testing.assert_array_equal((got[..., VEHICLE] == REJECTED).sum(axis=1), cn[:, 1], err_msg=tag)
    np.testing.assert_array_equal((got[..., WAIT].astype(np.int64) * served).sum(axis=1), cn[:, 3], err_msg=tag)
    SEEN["rejected"] += int((st == 2).sum() > 0)


@pytest.mark.parametrize("name", TINY)
def test_block_equals_reference_at_every_slot(name):
    env, seen = day_walk(name)
    assert seen["matched"] > 0 and (seen["moved"] > 0 or name == "tiny_two_orders" or env.T < 6)
    env.close()


@pytest.mark.parametrize("kernel,name,kw", FAMILIES, ids=["%s-%s-%d" % (k, n, i) for i, (k, n, _) in enumerate(FAMILIES)])
def test_block_through_every_tick_family(kernel, name, kw):
    env, seen = day_walk(name, kernel=kernel, **kw)
    assert env.main_kernel() == kernel and seen["matched"] > 0
    env.close()


# ---- 3. more than one workgroup in x, a replica tail behind the replicas-per-thread grouping ------------------------------------------------
def oracle_day(o):
    """(slot in which each order was processed, -1: never; the day's final results; the slots' id ranges) from stepping an oracle."""
    statuses = [o.orders()["status"].copy()]
    for _ in range(o.num_ticks):
        o.begin_tick()
        statuses.append(o.orders()["status"].copy())
        o.end_tick()
    off = slot_ranges(statuses)
    slot = np.full(statuses[0].size, -1, dtype=np.int64)
    for t in range(len(statuses) - 1):
        slot[off[t]:off[t + 1]] = t
    return slot, o.orders(), off


def day_block(day, t, O=None):
    """The block of one replica once slot t is stepped, from oracle_day's triple."""
    slot, res, _ = day
    done = (slot >= 0) & (slot <= t)
    return block_from_results(np.where(done, res["status"], 0), res["vehicle"], res["wait"], O)


@pytest.mark.parametrize("R", [5, 1])
def test_two_workgroups_of_ids_and_a_replica_tail_of_one(R):
    """tiny_sort_ties (20 000 synthetic orders on the tiny city, up to 264 in one slot): a slot of more than 256 ids - every thread of a
    workgroup at work, some on a second id - ten tiles of 2048 ids per replica for the full refresh, ranges of four slots that start
    and end inside a tile; R = 5 (an odd count, replicas that differ) and R = 1."""
    g = load_golden("tiny_sort_ties")
    off = record_ranges(g)
    assert np.diff(off).max() > 256
    O = int(g["o_status"].size)
    init = seeded_init(g, R, first=g["veh_node"], seed=900)
    days = [None]
    for r in range(1, R):
        o = make_oracle(g)
        o.reset(init[r])
        days.append(oracle_day(o))
    env = make_env(g, R)
    note_day(env, g, off)
    T = env.T
    env.reset(init)
    blk = env.orders_torch()
    for t in range(T):
        env.step()
        exp = np.stack([expected_after_slot(g, t)] + [day_block(d, t) for d in days[1:]])
        wide = off[t + 1] - off[t] > 256
        if wide or t % 9 == 0 or t == T - 1:
            got = refreshed(env)
            for r in range(R):
                assert_block(got[r], exp[r], "tiny_sort_ties R=%d slot %d replica %d" % (R, t, r))
            poison(env, blk)
            part = refreshed(env, t, t)
            lo, hi = slot_range(off, t, T, O)
            for r in range(R):
                assert_partial(part[r], exp[r], lo, hi, "tiny_sort_ties R=%d slot %d replica %d, refresh (t, t)" % (R, t, r))
            if t >= 3:          # a range of several slots: ids [off[t - 3], ..)
                poison(env, blk)
                part = refreshed(env, t - 3, t)
                for r in range(R):
                    assert_partial(part[r], exp[r], int(off[t - 3]), hi, "tiny_sort_ties R=%d slots %d .. %d replica %d" % (R, t - 3, t, r))
        env.advance()
    got = refreshed(env)
    assert R == 1 or not np.array_equal(got[3], got[4])
    check_day_end(env, got, "tiny_sort_ties R=%d" % R)
    env.close()


# ---- 4. V = 0 and a single-order day ---------------------------------------------------------------------------------------------------------
def test_no_vehicles_every_processed_order_is_rejected():
    g = dict(load_golden("tiny_kmeans"))
    g["V"] = np.int64(0)
    R, O = 3, int(g["o_status"].size)
    env = make_env(g, R)
    env.reset(np.zeros((R, 0), dtype=np.int32))
    off = record_ranges(g)
    blk = env.orders_torch()
    for t in range(env.T):
        env.step()
        if t % 7 == 0 or t == env.T - 1:
            got = refreshed(env)
            n = int(off[t + 1])
            assert (got[:, :n] == -1).all() and (got[:, n:, VEHICLE] == PENDING).all() and (got[:, n:, WAIT] == -1).all(), t
        env.advance()
    got = raw(env, blk)
    assert off[-1] == O - 1 and (got[:, :O - 1, VEHICLE] == REJECTED).all() and (got[:, O - 1, VEHICLE] == PENDING).all()
    check_day_end(env, got, "V = 0")
    env.close()


def test_a_day_of_one_order_reads_pending_also_inside_the_hooked_day():
    import torch
    g = load_golden("tiny_kmeans")
    R = 3
    init = seeded_init(g, R)
    env = mk_env(g, R, stream=torch.cuda.current_stream().cuda_stream)
    env.load_orders(g["o_release_min"][:1], g["o_pickup"][:1], g["o_delivery"][:1])
    assert env.O == 1 and env.T >= 1
    env.reset(init)
    blk = env.orders_torch()
    assert tuple(blk.shape) == (R, 1, 2)
    exp = np.tile(np.array([PENDING, -1], dtype=np.int32), (R, 1, 1))
    np.testing.assert_array_equal(raw(env, blk), exp)
    env.step()
    poison(env, blk)
    np.testing.assert_array_equal(refreshed(env), exp)
    for t in range(env.T):                               # the row is the tail of the day's LAST slot alone
        poison(env, blk)
        got = refreshed(env, t, t)
        assert (got == (exp if t == env.T - 1 else POISON)).all(), t
    env.advance()
    poison(env, blk)
    env.run_hooked(env.T - 1, orders=True)
    np.testing.assert_array_equal(raw(env, blk), exp)
    assert env.clock[0] == env.T
    check_day_end(env, refreshed(env), "one order")
    env.close()


# ---- 5. order days per replica over four maps, regrouped storage -------------------------------------------------------------------------------
MAPS = [np.arange(40) // 8, np.arange(40) % 5, (np.arange(40) * 7 + 1) % 4, np.arange(40) % 3]
_DAYS = {}          # (replica, day) -> oracle_day: the two layouts walk the same days from the same start nodes


# (the dense layout groups order days per replica in granules of eight or four replicas: every map is one day per workgroup there; on
# the wide layout the granule is 16, so the mixed maps run one order stream per row)
@pytest.mark.parametrize("kw,maps", [({}, (0, 1, 2, 3)), ({"force_generic": 5}, (1, 3))], ids=["dense-four-maps", "rows-two-maps"])
def test_per_replica_order_days_and_regrouped_storage(kw, maps):
    """The maps of test_gpu_slot_outcomes.test_per_replica_order_days_and_regrouped_storage: each replica's rows follow its own day in
    the caller's order.  The block is overwritten from torch before the refreshes, so that "past a shorter day's orders reads pending"
    and "a replica whose day is over is untouched by (t, t)" are the kernel's doing."""
    g = load_golden("tiny_kmeans")
    R = 40
    days = synth_days(g, 5, seed=5200)
    init = seeded_init(g, R, seed=8100)
    env = mk_env(g, R, **kw)
    # np.arange(R) % 3: 14 + 13 + 13 replicas - whatever the granule of the day groups, the replicas are stored by day as 3 x 16 with
    # eight padding replicas
    for gran_small in (0, 1):
        rc, plan = replica_plan(MAPS[3], 5, gran_small=gran_small)
        assert rc == 0 and plan["regrouped"] and plan["R"] == 48 and int((plan["int2ext"] < 0).sum()) == 8
    env.load_order_days(days, MAPS[maps[0]].astype(np.int32))
    O = env.O
    assert O == max(d[0].size for d in days) and len({d[0].size for d in days}) > 1
    cache = _DAYS
    for ep, rd in enumerate(MAPS[m] for m in maps):
        if ep:
            env.set_replica_days(rd.astype(np.int32))
        try:
            env.obs_inplace_torch()
            regrouped = False
        except Exception as e:
            assert "regrouped" in str(e), e
            regrouped = True
        # the plan the library made: granules of 16 replicas, or of eight / four on the dense layout at 16 lanes per replica; no
        # regrouping on a forced tick family.  Told apart by what the handle shows where the two differ in it
        lay = env.layout()
        plans = [replica_plan(rd, 5, gran_small=gs, regroup=int(not kw))[1] for gs in (0, 1)]
        fit = [p for p in plans if bool(p["regrouped"]) == regrouped]
        assert fit, (ep, regrouped)
        plan = fit[0] if len(fit) == 1 else plans[int(lay["dense"] == 1 and lay["dense_lpr"] == 16 and not kw)]
        SEEN["day_modes"].add("one day per workgroup" if plan["chunk_days"] else "one day per row")
        SEEN["regrouped"] += int(regrouped)
        SEEN["kernels"].add(env.main_kernel())
        env.reset(init)
        rep = []
        for r in range(R):
            d = int(rd[r])
            if (r, d) not in cache:
                o = mk_oracle(g, days[d])
                o.reset(init[r])
                cache[(r, d)] = oracle_day(o)
            rep.append(cache[(r, d)])
        Ts = [d[2].size - 1 for d in rep]
        assert env.T == max(Ts) and len(set(Ts)) > 1
        blk = env.orders_torch()
        poison(env, blk)
        got = refreshed(env)                               # nothing stepped: every element pending, the padding included
        assert (got[..., VEHICLE] == PENDING).all() and (got[..., WAIT] == -1).all()
        SEEN["padding_written"] += int(min(d[1]["status"].size for d in rep) < O)
        for t in range(env.T):
            env.step()
            exp = [day_block(rep[r], t, O) for r in range(R)]
            if t in Ts or t + 1 in Ts or t % 20 == 6:
                # over a poisoned block: a replica whose day is over stays as it was, a live one gets its slot's ids (and, in its last
                # slot, the rest of its row: the order never processed and the padding behind a shorter day)
                poison(env, blk)
                part = refreshed(env, t, t)
                for r in range(R):
                    tag = "episode %d slot %d replica %d, refresh (t, t)" % (ep, t, r)
                    if t >= Ts[r]:
                        assert (part[r] == POISON).all(), tag + ": a replica whose day is over was written"
                        SEEN["untouched_replica"] += 1
                    else:
                        lo, hi = slot_range(rep[r][2], t, Ts[r], O)
                        assert_partial(part[r], exp[r], lo, hi, tag)
                got = refreshed(env)                       # (0, INT32_MAX): every element again
            else:
                got = refreshed(env, t, t)                 # the block accumulates
            for r in range(R):
                assert_block(got[r], exp[r], "episode %d slot %d replica %d" % (ep, t, r))
            env.advance()
        check_day_end(env, got, "episode %d" % ep)
    env.close()


# ---- 6. the hooked day -------------------------------------------------------------------------------------------------------------------------
# (force_generic = 1: no day graph is built for this tick family - vds_run_hooked goes slot by slot through run_hooked_eager, which
# refreshes the range on the stream before it launches the policy)
@pytest.mark.parametrize("groups,kw", [(1, {}), (2, {}), (1, {"force_generic": 1})], ids=["one-chain", "two-groups", "eager-generic"])
def test_run_hooked_refreshes_the_slots_rows_for_a_captured_policy(groups, kw):
    """tiny_kmeans at R = 40 with the vehicle-form rule of test_gpu_vehicle_outcomes.hooked_expectation applied by the captured policy,
    which also copies slot t's rows of the block out, next to the per-cluster outcomes, the per-vehicle outcomes, the idle heads and
    two vehicle planes."""
    import torch
    g, init, node_of, vexpect, final = hooked_expectation()
    V, C, R = int(g["V"]), int(g["C"]), HG_R
    O = int(g["o_status"].size)
    off = record_ranges(g)                       # (dispatch moves no order to another slot)
    W = int(np.diff(off).max())
    full = np.stack([block_from_results(f["status"], f["vehicle"], f["wait"]) for f in final])          # [R, O, 2] at day end
    stream = torch.cuda.current_stream()
    env = make_env(g, R, stream=stream.cuda_stream, **CAPS, **kw)
    env.set_run_groups(groups, -1)
    assert env._lib.vds_get_run_groups(env._h) == groups
    assert env.main_kernel() == ("k_tick" if kw else "k_tick_dense")
    SEEN["kernels"].add(env.main_kernel())
    T = env.T
    env.reset(init)
    pl = env.vehicles_torch(state=True, node=False, cluster=True, arrive_min=False, order=False)
    state, cluster = pl["state"], pl["cluster"]
    heads = env.idle_heads_torch(4)
    oc = env.outcomes_torch()
    vout = env.vehicle_outcomes_torch()
    targets = torch.full((R, V), -1, dtype=torch.int32, device="cuda")
    # ids of slot t, padded to the widest slot with the id O - 1 (never processed)
    ids = np.full((T, W), O - 1, dtype=np.int64)
    for t in range(T):
        ids[t, :off[t + 1] - off[t]] = np.arange(off[t], off[t + 1])
    ids_t = torch.from_numpy(ids).cuda()
    log = torch.zeros((T, R, W, 2), dtype=torch.int32, device="cuda")
    served = torch.zeros((T, R), dtype=torch.int64, device="cuda")
    vserved = torch.zeros((T, R), dtype=torch.int64, device="cuda")
    head0 = torch.zeros((T, R), dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int64, device="cuda")
    vmod = (torch.arange(V, device="cuda", dtype=torch.int64) % 7)[None, :]
    node_t = torch.from_numpy(node_of.astype(np.int64)).cuda()
    ones = torch.ones((R, V), dtype=torch.int64, device="cuda")
    cur = {}

    def capture():
        """(Re-)capture the policy against the block as it stands: vds_load_orders* drops the block, the next request makes it again."""
        slot.zero_()
        cur["ptr"] = env.orders_device_ptr()
        blk = cur["blk"] = env.orders_torch()
        assert blk.data_ptr() == cur["ptr"]

        def policy():
            log.index_copy_(0, slot, blk.index_select(1, ids_t.index_select(0, slot)[0])[None])
            served.index_copy_(0, slot, oc[0].sum(dim=1)[None])
            vserved.index_copy_(0, slot, (vout[..., 0] >= 0).sum(dim=1)[None])
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
        cur["graph"] = graph
        env.run_hooked_invalidate()          # (the day graph is keyed by addresses: a re-captured policy may live where the last one did)

    capture()
    on = dict(outcomes=True, idle_heads=4, vehicle_planes=dict(state=True, cluster=True), vehicle_outcomes=True, vehicle_targets=targets,
              idle_pre=False, idle_now=False, supply=False, cl_orders=False)

    def start():
        env.reset(init)
        log.fill_(POISON); served.zero_(); vserved.zero_(); head0.fill_(-9); slot.zero_(); targets.fill_(-1)
        poison(env, cur["blk"])
        got = refreshed(env)                 # the full refresh the accumulation starts from
        assert (got[..., VEHICLE] == PENDING).all() and (got[..., WAIT] == -1).all()

    def check(tag):
        env.sync()
        torch.cuda.synchronize()
        assert int(slot.item()) == T, tag
        got = log.cpu().numpy()
        for t in range(T):
            n = int(off[t + 1] - off[t])
            for r in range(R):
                assert_block(got[t, r, :n], full[r, off[t]:off[t + 1]], "%s slot %d replica %d" % (tag, t, r))
            assert (got[t, :, n:, VEHICLE] == PENDING).all() and (got[t, :, n:, WAIT] == -1).all(), (tag, t)
        exp_served = (vexpect[..., 0] >= 0).sum(axis=2)
        np.testing.assert_array_equal(served.cpu().numpy(), exp_served, err_msg=tag)
        np.testing.assert_array_equal(vserved.cpu().numpy(), exp_served, err_msg=tag)
        assert int((head0 == -9).sum().item()) == 0, tag
        acc = raw(env, cur["blk"])           # accumulated over the day's (t, t) refreshes ...
        for r in range(R):
            assert_block(acc[r], full[r], "%s: the accumulated block, replica %d" % (tag, r))
        assert env.orders_device_ptr() == cur["ptr"], tag
        np.testing.assert_array_equal(raw(env, cur["blk"]), acc, err_msg=tag + ": ... equals the full refresh of the finished day")
        res = day_result(env)
        for r in range(R):
            for k in ("status", "vehicle", "wait"):
                np.testing.assert_array_equal(res[k][r], final[r][k], err_msg="%s replica %d %s" % (tag, r, k))
        return res

    start()
    env.run_hooked(T, policy_graph=cur["graph"], orders=True, **on)
    first = check("groups %d: one launch" % groups)
    start()
    env.run_hooked(T, policy_graph=cur["graph"], orders=True, **on)                  # the same graph, replayed
    assert_same_day(first, check("groups %d: replay" % groups), "replay")
    env.load_orders(g["o_release_min"], g["o_pickup"], g["o_delivery"])      # the block goes with the load: made again, policy re-captured
    env.reset(init)
    capture()
    start()
    env.run_hooked(T, policy_graph=cur["graph"], orders=True, **on)
    assert_same_day(first, check("groups %d: rebuilt behind load_orders" % groups), "rebuild")
    # switched off: the day is the same, a poisoned block stays poisoned
    start()
    poison(env, cur["blk"])
    env.run_hooked(T, policy_graph=cur["graph"], **on)
    env.sync()
    torch.cuda.synchronize()
    assert int((cur["blk"] == POISON).all().item()) == 1 and int(slot.item()) == T
    assert int((log == POISON).all().item()) == 1
    SEEN["poison_kept"] += 1
    assert_same_day(first, day_result(env), "switched off")
    # ... and without a policy, a day with the switch equals the day of a second handle that never heard of it
    plain = dict(outcomes=True, idle_heads=4, idle_pre=False, idle_now=False, supply=False, cl_orders=False)
    fresh = make_env(g, R, stream=stream.cuda_stream, **CAPS, **kw)
    fresh.set_run_groups(groups, -1)
    fresh.reset(init)
    fresh.run_hooked(T, **plain)
    env.reset(init)
    env.run_hooked(T, orders=True, **plain)
    a, b = day_result(env), day_result(fresh)
    assert_same_day(a, b, "a second handle, switch never set")
    assert (b["status"] == 1).any()
    fresh.close()
    env.close()


# ---- 7. snapshot / restore -------------------------------------------------------------------------------------------------------------------
def test_snapshot_mid_slot_and_restore_through_a_permutation():
    g = load_golden("tiny_kmeans_dfs2")
    R = 3
    init = seeded_init(g, R, seed=2000)
    days = []
    for r in range(R):
        o = make_oracle(g)
        o.reset(init[r])
        days.append(oracle_day(o))
    env = make_env(g, R)
    env.reset(init)
    env.run(20)
    got = refreshed(env)
    for r in range(R):
        assert_block(got[r], day_block(days[r], 19), "after run(20), replica %d" % r)
    env.step()                                             # slot 20, stepped: a snapshot inside the slot
    env.snapshot()
    at = refreshed(env)
    for r in range(R):
        assert_block(at[r], day_block(days[r], 20), "slot 20 replica %d" % r)
    assert (at[..., VEHICLE] >= 0).any() and not np.array_equal(at[0], at[1]) and not np.array_equal(at[1], at[2])
    env.advance()
    for _ in range(4):
        env.step(); env.advance()
    later = refreshed(env)
    assert not np.array_equal(later, at)
    perm = [2, 0, 1]
    env.restore(perm)
    blk = env.orders_torch(0, 0)
    poison(env, blk)
    got = refreshed(env)
    for r in range(R):
        assert_block(got[r], at[perm[r]], "after restore: replica %d shows replica %d" % (r, perm[r]))
    env.advance()
    env.step()
    got = refreshed(env, 21, 21)
    for r in range(R):
        assert_block(got[r], day_block(days[perm[r]], 21), "a step after the restore, replica %d" % r)
    env.close()


# ---- 8. address and lifetime -------------------------------------------------------------------------------------------------------------------
def device_blocks():
    gc.collect()          # (a handle some earlier test dropped without closing it goes now)
    out = np.zeros(2, dtype=np.int64)
    assert _lib.load().vds_debug_device_blocks(out.ctypes.data_as(ctypes.c_void_p)) == 0
    return int(out[0]), int(out[1])


def test_address_lifetime_refusals_and_device_blocks():
    before = device_blocks()
    g = load_golden("tiny_kmeans")
    R = 3
    O = int(g["o_status"].size)
    init = seeded_init(g, R)
    env = make_env(g, R)
    with pytest.raises(Exception, match="call vds_reset first"):
        env.orders_device_ptr()
    env.reset(init)
    for lo, hi in ((-1, 3), (4, 3), (-5, -6)):
        with pytest.raises(Exception, match="slot_lo <= slot_hi"):
            env.orders_device_ptr(lo, hi)
    env.step()
    held = device_blocks()
    p = env.orders_device_ptr()
    with_block = device_blocks()
    assert p % 8 == 0 and with_block[0] == held[0] + 1 and with_block[1] >= held[1] + 8 * R * O       # one block more
    assert env._lib.vds_orders_device(env._h, 0, 0, None) == 0                                        # dev_ptr may be NULL
    env.advance(); env.step()
    assert env.orders_device_ptr(1, 1) == p and env.orders_device_ptr(10 ** 6) == p and device_blocks() == with_block          # ... made once
    env.reset(init)
    assert env.orders_device_ptr() == p                                                               # stable across resets
    got = refreshed(env)
    assert (got[..., VEHICLE] == PENDING).all()
    env.reset_again()
    assert env.orders_device_ptr() == p
    env.set_idle_cap(env.idle_cap * 2)                                                                # other idle tables: the block lives with `out`
    env.reset(init)
    assert env.orders_device_ptr() == p and device_blocks()[0] == with_block[0]
    # another O: the block is gone with the load and made again, for the new size, by the next request
    env.load_orders(g["o_release_min"][:O // 2], g["o_pickup"][:O // 2], g["o_delivery"][:O // 2])
    with pytest.raises(Exception, match="call vds_reset first"):
        env.orders_device_ptr()
    env.reset(init)
    gone = device_blocks()
    blk = env.orders_torch()
    assert env.O == O // 2 and tuple(blk.shape) == (R, O // 2, 2) and device_blocks()[0] == gone[0] + 1
    o = make_oracle(dict(g, o_release_min=g["o_release_min"][:O // 2], o_pickup=g["o_pickup"][:O // 2], o_delivery=g["o_delivery"][:O // 2]))
    o.reset(init[1])
    day = oracle_day(o)
    for t in range(3):
        env.step()
        assert_block(refreshed(env)[1], day_block(day, t), "after load_orders with another O, slot %d" % t)
        env.advance()
    env.close()
    assert device_blocks() == before
    # the tables re-made: a replica -> day map that stores the 40 replicas as 3 x 16 strides every table anew.  The block goes with them
    # and the next request makes it again
    R = 40
    days = synth_days(g, 5, seed=5200)
    init = seeded_init(g, R, seed=8100)
    env = mk_env(g, R)
    env.load_order_days(days, (np.arange(R) // 8).astype(np.int32))
    env.reset(init)
    env.step()
    env.orders_device_ptr()
    with_block = device_blocks()
    env.set_replica_days((np.arange(R) % 3).astype(np.int32))
    env.reset(init)
    gone = device_blocks()
    p3 = env.orders_device_ptr()
    assert p3 % 8 == 0 and device_blocks()[0] == gone[0] + 1, (with_block, gone, device_blocks())      # made again by this call
    o = mk_oracle(g, days[1])
    o.reset(init[1])
    day = oracle_day(o)
    for t in range(4):
        env.step()
        assert env.orders_device_ptr(t, t) == p3
        assert_block(refreshed(env)[1], day_block(day, t, env.O), "after set_replica_days slot %d" % t)
        env.advance()
    env.close()
    assert device_blocks() == before


# ---- 9. written in full, whatever the memory held --------------------------------------------------------------------------------------------
# seconds of the selection under the product library on an MI355X, pytest start-up included; the limit follows as in
# tests/test_gpu_dirty_memory.py: ten times that + 120 s, a safety stop
SELECTION = "test_block_equals_reference_at_every_slot or test_per_replica_order_days_and_regrouped_storage"
SELECTION_SECONDS = 20


@pytest.mark.parametrize("target,lib,fill", [("dirty", "libvds_dirty.so", None), ("dirty", "libvds_dirty.so", "5A"), ("canary", "libvds_canary.so", None)],
                         ids=["dirty-A5", "dirty-5A", "canary"])
def test_every_element_is_written_on_dirty_and_guarded_memory(target, lib, fill):
    """The tiny day walks and the per-replica-days walk of this file in one pytest subprocess under the dirty library (every byte the
    library obtains is filled with A5 / 5A before first use: the block is not cleared when it is made, so the first full refresh meets
    the fill, and a row it missed reads as the pattern) and under the guarded one (a store outside the block damages a guard, found
    when the handle closes)."""
    from test_gpu_debug_builds import build
    from test_gpu_dirty_memory import dirty_env, gpu_allowed, run_limited
    gpu_allowed()
    path = build(target, lib)
    argv = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k", SELECTION]
    rc, out = run_limited(argv, dirty_env(fill, path), 10 * SELECTION_SECONDS + 120, "the walks under %s (fill %s)" % (lib, fill or "A5"))
    print(out[-800:])
    assert rc == 0 and "%d passed" % (len(TINY) + 2) in out, out[-6000:]


# ---- 10. coverage ----------------------------------------------------------------------------------------------------------------------------
def test_the_cases_met_what_they_were_chosen_for():
    """What the cases above were chosen for, counted while they ran (a run of this test alone walks what it needs itself)."""
    if not (SEEN["kernels"] & set(DENSE_KERNELS)) or SEEN["neighbour_served"] == 0:
        day_walk("tiny_kmeans_dfs2")[0].close()
    if not (SEEN["kernels"] - set(DENSE_KERNELS)):
        day_walk("tiny_kmeans", kernel="k_tick_rows", force_generic=5)[0].close()
    if not SEEN["wide_range"]:
        test_two_workgroups_of_ids_and_a_replica_tail_of_one(1)
    if len(SEEN["day_modes"]) < 3 or not SEEN["untouched_replica"]:
        test_per_replica_order_days_and_regrouped_storage({}, (3,))
        test_per_replica_order_days_and_regrouped_storage({"force_generic": 5}, (1,))
    # both layouts and all three day modes
    assert SEEN["kernels"] & set(DENSE_KERNELS) and SEEN["kernels"] - set(DENSE_KERNELS), SEEN["kernels"]
    assert SEEN["day_modes"] == {"shared", "one day per workgroup", "one day per row"} and SEEN["regrouped"] > 0, SEEN
    # a slot range spanning several workgroups, an empty slot, a rejected order, a neighbour-served order
    assert SEEN["wide_range"] > 0 and SEEN["empty_slot"] > 0 and SEEN["rejected"] > 0 and SEEN["neighbour_served"] > 0, SEEN
    # a partial refresh that left poisoned rows in place; a replica past its day left alone; the padding of a shorter day written
    assert SEEN["poison_kept"] > 0 and SEEN["untouched_replica"] > 0 and SEEN["padding_written"] > 0, SEEN
