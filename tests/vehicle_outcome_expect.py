"""Expected per-vehicle order outcomes of every slot (``vds_vehicle_outcomes_device``), built with numpy from a golden fixture alone
(``expected_vehicle_outcomes``), or from the CPU oracle's statuses before and after a slot (``processed_rows``: any release order,
days with dispatch).

Row ``[t, v]`` is ``{order, wait, value, pickup}`` of the order ``MatchFunction`` (``simulator.py:924-975``, neighbour search
``:978-996`` included) gave vehicle ``v`` in slot ``t``: ``Order.ID``, ``PickupWaitTime`` (``:949``, ``:952``), ``OrderValue``
(``:341-342``) and the pickup node; ``-1`` in all four words where the vehicle was not matched in that slot.  An order's slot is
``outcome_expect.order_slots``.  A vehicle leaves ``IdleVehicles`` when it is matched (``:963``) and comes back only through a later
``UpdateFunction``: it is matched at most once per slot, which both builders assert."""
from __future__ import annotations

import numpy as np

from outcome_expect import order_slots, tick_minutes_of

ORDER, WAIT, VALUE, PICKUP = range(4)
NAMES = ("order", "wait", "value", "pickup")


def expected_vehicle_outcomes(release_min, pickup, status, vehicle, wait, value, tick_minutes, T, V):
    """int32 ``[T, V, 4]``.  ``status``: 0 never processed, 1 ``ArriveInfo == "Success"``, 2 ``"Reject"``; ``vehicle``: the vehicle
    of a served order."""
    status = np.asarray(status)
    slot = order_slots(release_min, tick_minutes)
    veh = np.asarray(vehicle, dtype=np.int64)
    out = np.full((int(T), int(V), 4), -1, dtype=np.int32)
    s = np.flatnonzero(status == 1)
    assert (slot[s] < T).all() and (veh[s] >= 0).all() and (veh[s] < V).all()
    key = slot[s] * int(V) + veh[s]
    assert np.unique(key).size == key.size, "a vehicle matched twice in one slot"
    out[slot[s], veh[s], ORDER] = s
    out[slot[s], veh[s], WAIT] = np.asarray(wait, dtype=np.int64)[s]
    out[slot[s], veh[s], VALUE] = np.asarray(value, dtype=np.int64)[s]
    out[slot[s], veh[s], PICKUP] = np.asarray(pickup, dtype=np.int64)[s]
    return out


def processed_rows(before, after, pickup, vehicle, wait, value, V):
    """int32 ``[V, 4]`` of one slot from the CPU oracle's own stepping: the orders whose status turned from 0 to 1 between ``before``
    (the statuses read before the slot's ``begin_tick``) and ``after`` (read after it).  ``vehicle`` / ``wait`` / ``value``: the
    oracle's results read after the slot."""
    before, after = np.asarray(before), np.asarray(after)
    veh = np.asarray(vehicle, dtype=np.int64)
    s = np.flatnonzero((before == 0) & (after == 1))
    assert (veh[s] >= 0).all() and (veh[s] < V).all()
    assert np.unique(veh[s]).size == s.size, "a vehicle matched twice in one slot"
    out = np.full((int(V), 4), -1, dtype=np.int32)
    out[veh[s], ORDER] = s
    out[veh[s], WAIT] = np.asarray(wait, dtype=np.int64)[s]
    out[veh[s], VALUE] = np.asarray(value, dtype=np.int64)[s]
    out[veh[s], PICKUP] = np.asarray(pickup, dtype=np.int64)[s]
    return out


def expected_from_golden(g):
    """``expected_vehicle_outcomes`` of a fixture as ``load_golden`` returns it."""
    return expected_vehicle_outcomes(g["o_release_min"], g["o_pickup"], g["o_status"], g["o_vehicle"], g["o_wait"], g["o_value"],
                                     tick_minutes_of(g), int(g["n_ticks"]), int(g["V"]))


def slot_sums(rows):
    """``(served, wait_sum, value_sum)`` over the vehicles of ``[..., V, 4]`` rows, int64: what planes 0, 2 and 3 of
    ``vds_outcomes_device`` give summed over clusters."""
    rows = np.asarray(rows).astype(np.int64)
    m = rows[..., ORDER] >= 0
    return m.sum(axis=-1), (rows[..., WAIT] * m).sum(axis=-1), (rows[..., VALUE] * m).sum(axis=-1)
