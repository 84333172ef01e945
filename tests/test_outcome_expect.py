"""The expectation of the per-cluster outcome planes (``outcome_expect.py``) against the reference's own record, no GPU: summed over
clusters, every slot's planes are the per-slot increments of OrderNum - RejectNum, RejectNum and TotallyWaitTime the unmodified
reference logged (``t_order_num`` / ``t_reject_num`` / ``t_wait_sum``, the alignment the parity tests use: entry t after slot t),
``served + rejected`` is ``len(Cluster.Orders)`` of every bucket (``t_cl_orders``), and the served orders' values add up to
SumOrderValue without the value of the order that is never processed."""
import numpy as np
import pytest

from helpers import golden_names, load_golden
from outcome_expect import REJECTED, SERVED, VALUE_SUM, WAIT_SUM, expected_from_golden, order_slots, tick_minutes_of

NAMES = golden_names("tiny_") + golden_names("real_")


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
