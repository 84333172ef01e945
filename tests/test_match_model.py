"""tests/match_model.py against the unmodified reference's externally matched day (tests/golden/matchpack_0.npz, written by
tests/golden/make_match_golden.py): every slot's idle lists, arrival dicts with their minutes, counters, observations and the
per-order results.  No GPU."""
import numpy as np

from helpers import load_golden
from match_model import MatchModel, last_or_lowest


def model_of(g, fleet=None):
    m = MatchModel(g["cost"], g["node2cluster"], int(g["C"]), int(g["V"]), g["o_release_min"], g["o_pickup"], g["o_delivery"],
                   int(g["tick_minutes"]) if "tick_minutes" in g else 10, fleet=fleet)
    m.reset(g["veh_node"])
    return m


def check_slot(m, g, t):
    L = m.lists()
    for k in ("idle_off", "idle_veh", "arr_off", "arr_veh", "arr_min"):
        np.testing.assert_array_equal(L[k], g["l_" + k][t], err_msg="slot %d %s" % (t, k))
    ob, cn = m.obs(), m.counters()
    for k in ("idle_pre", "cl_orders", "supply"):
        np.testing.assert_array_equal(ob[k], g["t_" + k][t], err_msg="slot %d %s" % (t, k))
    assert (cn["order_num"], cn["reject_num"], cn["wait_sum"]) == (g["t_order_num"][t], g["t_reject_num"][t], g["t_wait_sum"][t]), t


def test_the_fixture_has_what_it_is_for():
    g = load_golden("matchpack_0")
    assert int((g["o_status"] == 2).sum()) > 10 and int((g["o_status"] == 1).sum()) > 50 and g["o_status"][-1] == 0
    assert int(g["slot_n"].max()) >= 4 and (g["slot_n"] == 0).any() and g["assign"].shape == (int(g["n_ticks"]), int(g["slot_n"].max()))


def test_model_replays_the_reference_day_slot_by_slot():
    g = load_golden("matchpack_0")
    m = model_of(g)
    assert m.num_ticks == int(g["n_ticks"])
    cross = 0
    for t in range(m.num_ticks):
        m.update()
        ids = m.slot_orders()
        assert len(ids) == g["slot_n"][t]
        row = g["assign"][t]
        cross += sum(1 for o, v in zip(ids, row) if v >= 0 and m.cluster[v] != m.n2c[m.pick[o]])
        assert last_or_lowest(m, ids) == row[:len(ids)].tolist(), t          # the fixture's matcher, on the model's containers
        assert m.match(row) == 0
        check_slot(m, g, t)
        m.end_tick()
    assert cross > 5
    od = m.orders()
    np.testing.assert_array_equal(od["status"], g["o_status"])
    np.testing.assert_array_equal(od["vehicle"], g["o_vehicle"])
    np.testing.assert_array_equal(od["wait"], g["o_wait"])
    np.testing.assert_array_equal(od["value"], g["o_value"])


def test_model_rejects_what_the_contract_rejects():
    g = load_golden("matchpack_0")
    m = model_of(g, fleet=10)
    t = int(np.flatnonzero(g["slot_n"] >= 3)[0])
    for _ in range(t):
        m.update(); m.match(None); m.end_tick()
    m.update()
    ids = m.slot_orders()
    idle = [v for c in m.idle for v in c]
    assert all(v < 10 for v in idle) and len(idle) == 10
    row = [idle[0], idle[0], 12] + [-1] * (len(ids) - 3)        # a vehicle, the same again, one beyond the fleet
    assert m.match(row) == 0
    assert [m.o_status[o] for o in ids[:3]] == [1, 2, 2] and m.o_vehicle[ids[0]] == idle[0]
    m.end_tick(); m.update()
    n = len(m.slot_orders())
    assert m.match([int(g["V"])] * n) == n                        # >= V: never an index, the sticky error
