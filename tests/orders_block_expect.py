"""Expected per-order block in id order (``vds_orders_device``), built with numpy from a golden fixture alone (``expected_after_slot``),
or from what the CPU oracle reports after a slot (``block_from_results``: any release order, days with dispatch).

Row ``i`` is ``{vehicle, wait}`` of ``Order.ID == i`` as ``MatchFunction`` (``simulator.py:924-975``) left it: ``{Vehicles index,
PickupWaitTime}`` of a matched order, ``{REJECTED, -1}`` where ``ArriveInfo == "Reject"`` (``:944``, ``:968``), ``{PENDING, -1}`` where
the order was not processed (yet): a later slot, the last order of the day (quirk Q1, ``:914-915``), the padding behind a shorter
day's own orders.  An order's slot is ``outcome_expect.order_slots``."""
from __future__ import annotations

import numpy as np

from outcome_expect import order_slots, tick_minutes_of

REJECTED, PENDING = -1, -2
VEHICLE, WAIT = 0, 1


def block_from_results(status, vehicle, wait, O=None):
    """int32 ``[O, 2]`` from per-order results as ``Oracle.orders()`` / ``env.orders()`` give them (``status``: 0 not processed, 1
    served, 2 rejected).  ``O`` longer than the day: the padding reads pending."""
    status = np.asarray(status)
    n = status.size if O is None else int(O)
    out = np.empty((n, 2), dtype=np.int32)
    out[:, VEHICLE] = PENDING
    out[:, WAIT] = -1
    s = np.flatnonzero(status == 1)
    assert (np.asarray(vehicle)[s] >= 0).all()
    out[s, VEHICLE] = np.asarray(vehicle, dtype=np.int64)[s]
    out[s, WAIT] = np.asarray(wait, dtype=np.int64)[s]
    out[np.flatnonzero(status == 2), VEHICLE] = REJECTED
    return out


def expected_after_slot(g, t):
    """The block of a fixture's day once slot ``t`` is stepped (``t = -1``: nothing stepped), from the reference's record alone: its
    final per-order results masked by the orders' slots."""
    done = order_slots(g["o_release_min"], tick_minutes_of(g)) <= int(t)
    return block_from_results(np.where(done, g["o_status"], 0), g["o_vehicle"], g["o_wait"])


def slot_ranges(statuses):
    """``[T + 1]`` first processed id of every slot (the engine's ``tick_off``) from the statuses read before the first slot and after
    each one; asserts what the block's kernel leans on - each slot's newly processed ids are ONE contiguous range that starts where the
    slot before ended."""
    off = [0]
    for before, after in zip(statuses[:-1], statuses[1:]):
        new = np.flatnonzero((np.asarray(before) == 0) & (np.asarray(after) != 0))
        assert ((np.asarray(before) != 0) <= (np.asarray(after) != 0)).all(), "a processed order became unprocessed"
        if new.size:
            assert new[0] == off[-1] and new[-1] - new[0] + 1 == new.size, "a slot's processed ids are not one contiguous range"
        off.append(off[-1] + int(new.size))
    return np.array(off, dtype=np.int64)


def record_ranges(g):
    """``slot_ranges`` of a fixture from the record alone (``order_slots`` and the final statuses)."""
    T = int(g["n_ticks"])
    slot = order_slots(g["o_release_min"], tick_minutes_of(g))
    st = np.asarray(g["o_status"])
    return slot_ranges([np.where(slot <= t, st, 0) for t in range(-1, T)])
