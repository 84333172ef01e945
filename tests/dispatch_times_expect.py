"""What the device dispatch forms with a per-entry arrival minute and counted flag (vds_apply_dispatch_vehicles_device_ex /
vds_apply_dispatch_roster_device_ex) must do, said with the oracle: one slot's tensors drive ``Oracle.dispatch_at`` the way
include/vds.h defines each form -

  - the movers in ascending vehicle number (vehicle form) or in roster order, cluster then list position (roster form);
  - a vehicle that is not idle, and an entry with a negative target, is skipped - its entries are never read;
  - one ``dispatch_at`` call per mover, with its own minute and its own ``counted``;
  - ``ARRIVE_ROAD`` means now + RoadCost; a minute more than ``AHEAD_MAX`` ahead of now is refused like a bad target.

No GPU and no library in here: tests/test_dispatch_times_expect.py holds this file against the reference-run days,
tests/test_gpu_dispatch_times.py holds the kernels against it."""
import numpy as np

from helpers import REFUSALS, dispatch_by_tick, idle_mask, make_oracle

ARRIVE_ROAD = -2 ** 31
AHEAD_MAX = 2 ** 30
TIMED_REFUSALS = REFUSALS + ("too_far",)
POISON = 2 ** 31 - 1          # what the tests put where nothing may be read

# the reference-run days whose hook body booked extra minutes on top of the road cost
DELAYED_DAYS = ("tiny_dispatch_delay", "fuzz_001", "fuzz_012", "fuzz_013", "fuzz_019", "fuzz_020", "fuzz_033")


def vehicle_order(o):
    """(vehicle, tensor index) of every idle vehicle in the vehicle form's order: ascending vehicle number, indexed by it."""
    return [(int(v), int(v)) for v in np.flatnonzero(idle_mask(o))]


def roster_order(o):
    """(vehicle, tensor index) in the roster form's order: ascending cluster, list order, indexed by roster position."""
    L = o.lists()
    return [(int(v), i) for i, v in enumerate(L["idle_veh"][:L["idle_off"][-1]])]


def oracle_apply_timed(o, order, targets, arrive_min, counted, n2c, over=False, one_call=False):
    """One call of one replica.  ``order``: ``vehicle_order(o)`` / ``roster_order(o)``; ``targets`` / ``arrive_min`` / ``counted``
    the replica's rows (the last two may be None).  Returns dict(moves, counted, refused={kind: entries}, movers=[(vehicle, index)]).
    ``one_call``: the movers in one ``dispatch_at`` call (all counted: the call takes one flag) instead of one call each."""
    n2c = np.asarray(n2c)
    now = int(o.now_min)
    out = dict(moves=0, counted=0, refused=dict.fromkeys(TIMED_REFUSALS, 0), movers=[])
    batch = []
    for v, j in order:
        n = int(targets[j])
        if n < 0:
            continue
        if over:
            out["refused"]["day_over"] += 1
        elif n >= n2c.size:
            out["refused"]["beyond_n"] += 1
        elif n2c[n] < 0:
            out["refused"]["no_cluster"] += 1
        else:
            a = ARRIVE_ROAD if arrive_min is None else int(arrive_min[j])
            if a != ARRIVE_ROAD and a > now and a - now > AHEAD_MAX:
                out["refused"]["too_far"] += 1
                continue
            k = True if counted is None else int(counted[j]) != 0
            if one_call:
                assert k
                batch.append((v, n, a))
            else:
                o.dispatch_at([v], [n], None if a == ARRIVE_ROAD else [a], counted=k)
            out["moves"] += 1
            out["counted"] += int(k)
            out["movers"].append((v, j))
    if batch:
        assert all(a != ARRIVE_ROAD for _, _, a in batch) or all(a == ARRIVE_ROAD for _, _, a in batch)
        road = batch[0][2] == ARRIVE_ROAD
        o.dispatch_at([b[0] for b in batch], [b[1] for b in batch], None if road else [b[2] for b in batch], counted=True)
    return out


def slot_tensors(rows, order, V, now, extra, fill=-1):
    """The logged moves of one slot (rows of ``dispatch_log``: slot, vehicle, from cluster, -, target, road cost) as one replica's
    ``targets`` / ``arrive_min`` rows for the form whose ``order`` is given; ``extra``: the minutes the body booked on top of the
    road cost (None: no arrive_min row).  Entries of no mover: ``fill`` in arrive_min (targets: -1).  A logged vehicle that is not
    idle (a day that has left the record) has no entry in ``order``: the vehicle form still writes its entry, which is never read."""
    index = dict(order)
    if all(v == j for v, j in order):
        index = {v: v for v in range(V)}
    targets = np.full(V, -1, dtype=np.int32)
    arrive = None if extra is None else np.full(V, fill, dtype=np.int32)
    for row in rows:
        j = index.get(int(row[1]))
        if j is None:
            continue
        targets[j] = int(row[4])
        if arrive is not None:
            arrive[j] = now + int(row[5]) + extra
    return targets, arrive


def replay_day(g, form, extra, one_call=False):
    """The recorded day ``g`` in one oracle, its dispatch log applied slot by slot through ``oracle_apply_timed`` in the order of
    ``form`` ("vehicle" / "roster").  Returns (first slot at which ``t_idle_post`` / ``t_supply`` leave the reference's record - the
    number of slots when only the end-of-day vectors or counters do - or None, the oracle)."""
    o = make_oracle(g)
    disp = dispatch_by_tick(g)
    T, V = int(g["n_ticks"]), int(g["V"])
    left = None
    for t in range(T):
        o.begin_tick()
        ob = o.obs()
        if left is None and not (np.array_equal(ob["idle_post"], g["t_idle_post"][t]) and np.array_equal(ob["supply"], g["t_supply"][t])):
            left = t
        if t in disp:
            order = vehicle_order(o) if form == "vehicle" else roster_order(o)
            targets, arrive = slot_tensors(disp[t], order, V, int(o.now_min), extra)
            got = oracle_apply_timed(o, order, targets, arrive, None, g["node2cluster"], one_call=one_call)
            assert not any(got["refused"].values()) and (got["moves"] == len(disp[t]) or left is not None)
        o.end_tick()
    if left is None:
        od, oc = o.orders(), o.counters()
        same = all(np.array_equal(od[k], g["o_" + k]) for k in ("status", "vehicle", "wait"))
        if not (same and oc["dispatch_num"] == int(g["dispatch_num"]) and oc["dispatch_cost"] == int(g["dispatch_cost"])):
            left = T
    return left, o


def slots_ahead(g):
    """The furthest booked arrival of the day's log, in slots: ceil((road cost + extra minutes) / slot length)."""
    tick, extra = int(g["tick_minutes"]) if "tick_minutes" in g else 10, int(g["dispatch_extra_minutes"])
    return max(-(-(int(row[5]) + extra) // tick) for row in g["dispatch_log"])
