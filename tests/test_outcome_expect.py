"""The expectation of the per-cluster outcome planes (``outcome_expect.py``) against the reference's own record, no GPU: summed over
clusters, every slot's planes are the per-slot increments of OrderNum - RejectNum, RejectNum and TotallyWaitTime the unmodified
reference logged (``t_order_num`` / ``t_reject_num`` / ``t_wait_sum``, the alignment the parity tests use: entry t after slot t),
``served + rejected`` is ``len(Cluster.Orders)`` of every bucket (``t_cl_orders``), and the served orders' values add up to
SumOrderValue without the value of the order that is never processed."""
import numpy as np
import pytest

from helpers import dispatch_by_tick, golden_names, load_golden, make_oracle, slot_names
from outcome_expect import REJECTED, SERVED, VALUE_SUM, WAIT_SUM, expected_from_golden, order_slots, processed_planes, tick_minutes_of

NAMES = golden_names("tiny_") + golden_names("real_") + slot_names()


def increments(x):
    x = np.asarray(x, dtype=np.int64)
    return np.diff(np.concatenate([[0], x]))


@pytest.mark.parametrize("name", NAMES)
def test_expected_planes_reproduce_reference_record(name):
    g = load_golden(name)
    e = expected_from_golden(g)
    T, C = int(g["n_ticks"]), int(g["C"])
    assert e.shape == (T, C, 4)
    per_slot = e.sum(axis=1)
    np.testing.assert_array_equal(per_slot[:, SERVED] + per_slot[:, REJECTED], increments(g["t_order_num"]))
    np.testing.assert_array_equal(per_slot[:, REJECTED], increments(g["t_reject_num"]))
    np.testing.assert_array_equal(per_slot[:, WAIT_SUM], increments(g["t_wait_sum"]))
    assert per_slot[:, SERVED].sum() == int(g["order_num"]) - int(g["reject_num"])
    assert per_slot[:, WAIT_SUM].sum() == int(g["wait_sum"])
    # SumOrderValue (:1095-1100) counts every order that is not rejected: the served ones and the one never processed
    q1 = np.flatnonzero(g["o_status"] == 0)
    assert q1.size == 1
    assert per_slot[:, VALUE_SUM].sum() + int(g["o_value"][q1[0]]) == int(g["sum_order_value"])
    # served + rejected == len(Cluster.Orders) (:919) in every bucket of the reference's record: the Q1 order breaks out of the loop
    # (:914-915) before it is appended, so no bucket counts it
    if "t_cl_orders" in g:
        np.testing.assert_array_equal(e[:, :, SERVED] + e[:, :, REJECTED], g["t_cl_orders"])
    # the never-processed order is the last one, and its slot lies inside the day
    assert q1[0] == len(g["o_status"]) - 1
    assert order_slots(g["o_release_min"], tick_minutes_of(g))[q1[0]] < T


def replay_steps(g):
    """The oracle's per-order results before the first slot and after each slot's Update + Match (before its dispatch)."""
    o = make_oracle(g)
    disp = dispatch_by_tick(g)
    extra = int(g["dispatch_extra_minutes"]) if "dispatch_extra_minutes" in g else 0
    out = [o.orders()]
    for t in range(o.num_ticks):
        o.begin_tick()
        out.append(o.orders())
        if t in disp:
            rows = np.array(disp[t])
            if extra:
                o.dispatch_at(rows[:, 1], rows[:, 4], arrive_min=o.now_min + rows[:, 5] + extra)
            else:
                o.dispatch(rows[:, 1], rows[:, 4])
        o.end_tick()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_status_diff_expectation_equals_golden_expectation(name):
    """``processed_planes`` - what the plane fuzz (test_gpu_plane_fuzz.py) expects at every slot: the CPU oracle stepped through the
    fixture's day (its dispatch log replayed as test_oracle_golden does), the orders whose status turned non-zero in each slot grouped
    by pickup cluster - equals the expectation built from the reference's record alone, slot for slot."""
    g = load_golden(name)
    T, C = int(g["n_ticks"]), int(g["C"])
    cl = g["node2cluster"][g["o_pickup"].astype(np.int64)]
    steps = replay_steps(g)
    assert len(steps) == T + 1
    # (wait / value of each slot's read: an order's PickupWaitTime is set when it is processed and does not change afterwards)
    got = np.stack([processed_planes(steps[t]["status"], steps[t + 1]["status"], cl, steps[t + 1]["wait"], steps[t + 1]["value"], C)
                    for t in range(T)])
    np.testing.assert_array_equal(steps[-1]["status"], g["o_status"])
    np.testing.assert_array_equal(got, expected_from_golden(g))
