"""Expected per-cluster order outcomes of every slot (``vds_outcomes_device``), built with numpy from a golden fixture alone
(``expected_outcomes``), or from the CPU oracle's statuses before and after each slot (``processed_planes``: any release order).

The goldens were captured from the unmodified reference, so the expectation does not rest on this engine.  In the reference an
order is processed by ``MatchFunction`` in the first slot whose window ``ReleasTime < RealExpTime + TimePeriods`` admits it
(``simulator.py:912``), with ``RealExpTime = Orders[0].ReleasTime - TimePeriods + t * TimePeriods`` at slot t (``:1037``, ``:1091``):
slot ``(release - release[0]) // tick + 1``.  It sits in ``Cluster.Orders`` of its pickup node's cluster (``:918-919``) until the
next slot's ``UpdateFunction`` clears the lists (``:1013``).  The order that is never processed (quirk Q1, ``:914-915``) has status 0
and is in no bucket."""
from __future__ import annotations

import numpy as np

SERVED, REJECTED, WAIT_SUM, VALUE_SUM = range(4)
NAMES = ("served", "rejected", "wait_sum", "value_sum")


def order_slots(release_min, tick_minutes):
    """Slot in which each order is processed (orders sorted by release, as ``self.Orders``)."""
    rel = np.asarray(release_min, dtype=np.int64)
    return (rel - rel[0]) // int(tick_minutes) + 1


def expected_outcomes(release_min, pickup, node2cluster, status, wait, value, tick_minutes, T, C):
    """int64 ``[T, C, 4]``: (served, rejected, wait_sum, value_sum) of the orders of (slot, pickup cluster).
    ``status``: 0 never processed, 1 ``ArriveInfo == "Success"``, 2 ``"Reject"``; ``wait``: ``PickupWaitTime``; ``value``: ``OrderValue``."""
    status = np.asarray(status)
    slot = order_slots(release_min, tick_minutes)
    cl = np.asarray(node2cluster, dtype=np.int64)[np.asarray(pickup, dtype=np.int64)]
    out = np.zeros((int(T), int(C), 4), dtype=np.int64)
    done = status != 0
    assert (slot[done] < T).all() and (cl[done] >= 0).all()
    s = status == 1
    r = status == 2
    np.add.at(out[:, :, SERVED], (slot[s], cl[s]), 1)
    np.add.at(out[:, :, REJECTED], (slot[r], cl[r]), 1)
    np.add.at(out[:, :, WAIT_SUM], (slot[s], cl[s]), np.asarray(wait, dtype=np.int64)[s])
    np.add.at(out[:, :, VALUE_SUM], (slot[s], cl[s]), np.asarray(value, dtype=np.int64)[s])
    return out


def processed_planes(before, after, pickup_cluster, wait, value, C):
    """int64 ``[C, 4]`` of one slot from the CPU oracle's own stepping: the orders whose status turned non-zero between ``before`` (the
    statuses read before the slot's ``begin_tick``) and ``after`` (read after it), by pickup cluster.  ``wait`` / ``value``: the oracle's
    ``PickupWaitTime`` / ``OrderValue``.  Unlike ``order_slots`` it assumes nothing about the order of the releases, and the order that is
    never processed (status 0) is in no slot."""
    before, after = np.asarray(before), np.asarray(after)
    cl = np.asarray(pickup_cluster, dtype=np.int64)
    new = (before == 0) & (after != 0)
    assert (cl[new] >= 0).all()
    out = np.zeros((int(C), 4), dtype=np.int64)
    s = new & (after == 1)
    r = new & (after == 2)
    np.add.at(out[:, SERVED], cl[s], 1)
    np.add.at(out[:, REJECTED], cl[r], 1)
    np.add.at(out[:, WAIT_SUM], cl[s], np.asarray(wait, dtype=np.int64)[s])
    np.add.at(out[:, VALUE_SUM], cl[s], np.asarray(value, dtype=np.int64)[s])
    return out


def tick_minutes_of(g):
    return int(g["tick_minutes"]) if "tick_minutes" in g else 10


def expected_from_golden(g):
    """``expected_outcomes`` of a fixture as ``load_golden`` returns it."""
    return expected_outcomes(g["o_release_min"], g["o_pickup"], g["node2cluster"], g["o_status"], g["o_wait"], g["o_value"],
                             tick_minutes_of(g), int(g["n_ticks"]), int(g["C"]))
