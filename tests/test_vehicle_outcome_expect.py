"""The expectation of the per-vehicle outcome block (``vehicle_outcome_expect.py``) against the reference's own record, no GPU: for
every tiny fixture and the fuzz corpus the rows built from the fixture's ``o_status`` / ``o_vehicle`` / ``o_wait`` equal the rows
built by stepping the CPU oracle through the day (its dispatch log replayed), slot for slot; summed over vehicles they are the served
count and the wait and value sums of the per-cluster expectation (``outcome_expect.py``) summed over clusters; and the recorded days
hold the situations tests/test_gpu_vehicle_outcomes.py relies on."""
import numpy as np
import pytest

from helpers import fuzz_names, golden_names, load_golden, recorded_day_facts, slot_names
from outcome_expect import SERVED, VALUE_SUM, WAIT_SUM, order_slots, tick_minutes_of
from outcome_expect import expected_from_golden as cluster_expectation
from test_outcome_expect import replay_steps
from vehicle_outcome_expect import ORDER, PICKUP, VALUE, WAIT, expected_from_golden, processed_rows, slot_sums

TINY = golden_names("tiny_")
NAMES = TINY + fuzz_names() + slot_names()


@pytest.mark.parametrize("name", NAMES)
def test_rows_from_the_record_equal_rows_from_stepping_the_oracle(name):
    g = load_golden(name)
    T, V = int(g["n_ticks"]), int(g["V"])
    e = expected_from_golden(g)
    assert e.shape == (T, V, 4) and e.dtype == np.int32
    steps = replay_steps(g)
    assert len(steps) == T + 1
    np.testing.assert_array_equal(steps[-1]["status"], g["o_status"])
    for t in range(T):
        a = steps[t + 1]
        got = processed_rows(steps[t]["status"], a["status"], g["o_pickup"], a["vehicle"], a["wait"], a["value"], V)
        np.testing.assert_array_equal(got, e[t], err_msg="slot %d" % t)
    # a row is all -1 or names an order of the day in full (a wait or a value may be negative on a city with negative costs: the
    # order word alone says whether there was a match)
    m = e[:, :, ORDER] >= 0
    assert (e[~m] == -1).all() and (e[m][:, PICKUP] >= 0).all()
    o = e[m][:, ORDER].astype(np.int64)
    np.testing.assert_array_equal(e[m][:, PICKUP], g["o_pickup"][o])
    np.testing.assert_array_equal(e[m][:, VALUE], np.asarray(g["o_value"])[o])
    np.testing.assert_array_equal(e[m][:, WAIT], g["o_wait"][o])
    assert m.sum() == int((g["o_status"] == 1).sum())


@pytest.mark.parametrize("name", NAMES)
def test_sums_over_vehicles_equal_the_cluster_planes_summed_over_clusters(name):
    g = load_golden(name)
    served, wait, value = slot_sums(expected_from_golden(g))
    per_slot = cluster_expectation(g).sum(axis=1)
    np.testing.assert_array_equal(served, per_slot[:, SERVED])
    np.testing.assert_array_equal(wait, per_slot[:, WAIT_SUM])
    np.testing.assert_array_equal(value, per_slot[:, VALUE_SUM])


def facts(name):
    g = load_golden(name)
    e = expected_from_golden(g)
    T, V = int(g["n_ticks"]), int(g["V"])
    m = e[:, :, ORDER] >= 0
    processed = np.bincount(order_slots(g["o_release_min"], tick_minutes_of(g))[g["o_status"] != 0], minlength=T)
    return dict(twice=int((m.sum(axis=0) >= 2).sum()), empty_slots=int((processed == 0).sum()),
                all_matched=int((m.sum(axis=1) == V).sum()) if V else 0, none_idle=int((g["t_idle_post"].sum(axis=1) == 0).sum()),
                cross=recorded_day_facts(g)["cross"], depth=int(g["depth_limit"]), nbr=bool(g["neighbor_can_server"]),
                most=int(processed.max()))


def test_the_recorded_days_hold_what_the_gpu_tests_rely_on():
    """From the reference's record alone, over the tiny fixtures the GPU file walks slot by slot."""
    F = {n: facts(n) for n in TINY}
    # a vehicle matched in two different slots of one day: a row must be replaced, not kept
    assert F["tiny_kmeans"]["twice"] > 0 and all(f["twice"] > 0 for n, f in F.items() if n != "tiny_two_orders")
    # a served order whose vehicle idled in another cluster than the pickup's, on a depth >= 1 day
    assert F["tiny_kmeans_dfs2"]["cross"] > 0 and F["tiny_kmeans_dfs2"]["depth"] >= 1 and F["tiny_kmeans_dfs2"]["nbr"]
    assert F["tiny_kmeans_dfs1"]["cross"] > 0 and F["tiny_kmeans_dfs1"]["depth"] == 1
    # a slot without orders: the fill alone
    assert all(f["empty_slots"] > 0 for f in F.values())
    # a slot after whose match no vehicle is idle
    assert F["tiny_kmeans_dfs2"]["none_idle"] > 0 and F["tiny_grid_nbr_scarce"]["none_idle"] > 0
    # more orders in one slot than one 256-thread block takes
    assert F["tiny_sort_ties"]["most"] > 256
    # ... and a slot in which every vehicle is matched, in the fuzz corpus
    assert any(facts(n)["all_matched"] > 0 for n in fuzz_names() if int(load_golden(n)["V"]) > 0)
