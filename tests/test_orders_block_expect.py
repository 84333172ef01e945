"""The expectation of the per-order block (``orders_block_expect.py``) against the reference's own record, no GPU: for every tiny
fixture and the fuzz corpus the block built from the fixture's ``o_status`` / ``o_vehicle`` / ``o_wait`` masked by the orders' slots
equals the block built from the CPU oracle stepped through the day (its dispatch log replayed) after every slot; and the recorded
days hold the facts tests/test_gpu_orders_block.py leans on."""
import numpy as np
import pytest

from helpers import fuzz_names, golden_names, load_golden, make_oracle, recorded_day_facts
from orders_block_expect import PENDING, REJECTED, VEHICLE, WAIT, block_from_results, expected_after_slot, record_ranges, slot_ranges
from test_outcome_expect import replay_steps

TINY = golden_names("tiny_")
NAMES = TINY + fuzz_names()


def test_the_corpus_is_the_tiny_fixtures_and_the_58_fuzz_days():
    assert len(fuzz_names()) == 58 and len(TINY) > 0


@pytest.mark.parametrize("name", NAMES)
def test_block_from_the_record_equals_block_from_stepping_the_oracle(name):
    g = load_golden(name)
    T, O = int(g["n_ticks"]), g["o_status"].size
    steps = replay_steps(g)
    assert len(steps) == T + 1
    np.testing.assert_array_equal(steps[-1]["status"], g["o_status"])
    first = expected_after_slot(g, -1)
    assert first.shape == (O, 2) and first.dtype == np.int32
    assert (first[:, VEHICLE] == PENDING).all() and (first[:, WAIT] == -1).all()
    np.testing.assert_array_equal(block_from_results(steps[0]["status"], steps[0]["vehicle"], steps[0]["wait"]), first)
    for t in range(T):
        a = steps[t + 1]
        np.testing.assert_array_equal(block_from_results(a["status"], a["vehicle"], a["wait"]), expected_after_slot(g, t), err_msg="slot %d" % t)
    # the words of a row: a vehicle of the fleet and the recorded wait, or a code and -1
    e = expected_after_slot(g, T - 1)
    m = e[:, VEHICLE] >= 0
    assert (e[m, VEHICLE] < int(g["V"])).all() and (e[~m, WAIT] == -1).all() and set(np.unique(e[~m, VEHICLE])) <= {REJECTED, PENDING}
    np.testing.assert_array_equal(m, g["o_status"] == 1)
    np.testing.assert_array_equal(e[:, VEHICLE] == REJECTED, g["o_status"] == 2)
    # the slots' id ranges, from the record and from the oracle's own stepping
    np.testing.assert_array_equal(record_ranges(g), slot_ranges([s["status"] for s in steps]))


def facts(name):
    g = load_golden(name)
    off = record_ranges(g)
    O = g["o_status"].size
    return dict(O=O, tiles=bool(off[0] == 0 and off[-1] == O - 1), last_pending=bool(g["o_status"][O - 1] == 0),
                empty_slots=int((np.diff(off) == 0).sum()), most=int(np.diff(off).max()), rejected=int((g["o_status"] == 2).sum()),
                cross=recorded_day_facts(g)["cross"], depth=int(g["depth_limit"]), nbr=bool(g["neighbor_can_server"]))


def test_the_recorded_days_hold_what_the_gpu_tests_lean_on():
    """From the reference's record alone, over the tiny fixtures the GPU file walks slot by slot."""
    F = {n: facts(n) for n in TINY}
    # each slot's processed ids are one contiguous range (record_ranges asserts it) and the ranges tile [0, O - 1)
    assert all(f["tiles"] for f in F.values())
    # the last id is never processed
    assert all(f["last_pending"] for f in F.values())
    # a slot without orders
    assert all(f["empty_slots"] > 0 for f in F.values())
    # more orders in one slot than one 256-thread block takes
    assert F["tiny_sort_ties"]["most"] > 256
    # a rejected order
    assert F["tiny_kmeans"]["rejected"] > 0 and F["tiny_grid_nbr_scarce"]["rejected"] > 0
    # an order served by a vehicle of another cluster, at depth 1 and at depth 2
    assert F["tiny_kmeans_dfs1"]["cross"] > 0 and F["tiny_kmeans_dfs1"]["depth"] == 1 and F["tiny_kmeans_dfs1"]["nbr"]
    assert F["tiny_kmeans_dfs2"]["cross"] > 0 and F["tiny_kmeans_dfs2"]["depth"] == 2 and F["tiny_kmeans_dfs2"]["nbr"]


@pytest.mark.parametrize("name", ["tiny_kmeans", "tiny_kmeans_dfs1"])
def test_unsorted_release_minutes_keep_the_ranges_contiguous_on_the_oracle(name):
    """The cursor of MatchFunction (:912-973) only moves forward: with release minutes that are not sorted (the day of
    test_gpu_edge_cases.test_unsorted_release_times_follow_cursor_semantics) every slot still processes one contiguous id range, the
    processed ids are a prefix, and the last id stays unprocessed."""
    g = dict(load_golden(name))
    rel = g["o_release_min"].copy()
    rng = np.random.default_rng(3)
    idx = rng.choice(rel.size - 1, size=200, replace=False)
    rel[idx] = np.maximum(0, rel[idx] + rng.integers(-300, 300, size=200)).astype(np.int32)
    assert (np.diff(rel.astype(np.int64)) < 0).any()
    g["o_release_min"] = rel
    o = make_oracle(g)
    statuses = [o.orders()["status"].copy()]
    for _ in range(o.num_ticks):
        o.begin_tick()
        statuses.append(o.orders()["status"].copy())
        o.end_tick()
    off = slot_ranges(statuses)
    done = statuses[-1] != 0
    assert done[:off[-1]].all() and not done[off[-1]:].any() and not done[-1] and off[-1] > 0
    assert (np.diff(off) == 0).any() and (np.diff(off) > 0).any()
