"""Pins the CPU oracle (oracle/vds_oracle.c) on the axes the GPU fuzz tests vary - DFS depth -1..4, ticks of 10 / 5 / 15 / 7 / 3
minutes, raw pickup windows none / 40 / 8 / 0, tie-heavy / long / negative / fractional costs, 0..139 vehicles, 4..48 clusters,
dispatch - against days the unmodified reference ran (tests/golden/make_fuzz_golden.py).  Bit-exact, as the tiny fixtures:
per tick counters, the five observation planes, idle lists and arrival dicts in container order; then per-order status /
vehicle / wait / value and the final counters.  CPU only."""
import os

import numpy as np
import pytest

from helpers import SLOT_LENGTHS, fuzz_coverage_gaps, fuzz_names, load_fuzz, load_golden, slot_coverage_gaps, slot_names
from oracle.ref_harness import write_reference_data_dir
from test_oracle_golden import replay
from vehicles_dispatch_simulator_amd import synth, world

FUZZ = fuzz_names()
SLOT = slot_names()
LONG = slot_names(long_days=True)


@pytest.mark.parametrize("name", FUZZ + SLOT)
def test_oracle_matches_reference_fuzz(name):
    g = load_golden(name)
    o = replay(g, check_lists=name not in LONG)       # (only the two days of more than 32767 slots are recorded without lists)
    od = o.orders()
    np.testing.assert_array_equal(od["status"], g["o_status"])
    np.testing.assert_array_equal(od["vehicle"], g["o_vehicle"])
    np.testing.assert_array_equal(od["wait"], g["o_wait"])
    np.testing.assert_array_equal(od["value"], g["o_value"])
    c = o.counters()
    for k in ("order_num", "reject_num", "wait_sum", "dispatch_num", "dispatch_cost", "sum_order_value"):
        assert c[k] == int(g[k]), k
    assert c["matched"] == int((g["o_status"] == 1).sum())
    # quirk Q1: the last order of the day is never processed
    assert od["status"][-1] == 0 and c["order_num"] == g["o_status"].size - 1


def test_fuzz_corpus_covers_its_axes():
    """The corpus is only a pin where it reaches: every depth, tick and window several times, neighbour search that really
    served from another cluster at every depth >= 1, windows that really rejected a found vehicle, the cost styles with and
    without dispatch, empty fleets, clusters without nodes (conditions: helpers.fuzz_coverage_gaps, derived from the
    reference's record alone)."""
    assert 48 <= len(FUZZ) <= 64
    cases = {n: load_fuzz(n) for n in FUZZ}
    assert fuzz_coverage_gaps(cases) == []
    assert {int(g["C"]) for g in cases.values()} >= {4, 6, 12, 24, 35, 48}
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sizes = [os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f.startswith("fuzzpack_")]
    assert max(sizes) < 1_000_000 and sum(sizes) < 4_000_000


def test_slot_corpus_covers_its_axes():
    """The slot-length corpus (tests/golden/make_slot_golden.py): per slot length a day for the dense tick, a search that served from
    another cluster, dispatch, served beside rejected orders; trips beyond the ring horizon at 1 and 2 minutes; slots of more than
    256 orders and window rejects from 60 minutes on; two days that serve orders past slot 32767 with vehicles under way across it
    (conditions: helpers.slot_coverage_gaps, from the reference's record alone)."""
    cases = {n: load_golden(n) for n in SLOT}
    assert slot_coverage_gaps(cases) == []
    assert {int(g["tick_minutes"]) for g in cases.values()} == set(SLOT_LENGTHS)
    assert sorted(slot_names(long_days=True)) == ["slot_long_pull", "slot_long_search"]
    assert all(int(cases[n]["n_ticks"]) > 32767 for n in slot_names(long_days=True))
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sizes = [os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f.startswith("slotpack_")]
    assert max(sizes) < 1_000_000 and sum(sizes) < 3_000_000


def _loader_cases():
    """Two label-file cities per depth outside the tiny fixtures' 0..2, with a cluster count other than their 12."""
    by_depth = {-1: [], 3: [], 4: []}
    for n in FUZZ:
        g = load_fuzz(n)
        if not len(g["focus_bound"]) and int(g["C"]) != 12 and int(g["depth_limit"]) in by_depth:
            by_depth[int(g["depth_limit"])].append(n)
    assert all(len(v) >= 2 for v in by_depth.values()), by_depth
    return [n for v in by_depth.values() for n in v[:2]]


LOADER = _loader_cases()


@pytest.mark.parametrize("name", LOADER)
def test_loader_matches_reference_tables_fuzz(name, tmp_path):
    """world.load_world on a reference-style data directory (as tests/test_world_loader.py): cluster count from the grid shape of
    side_m, depth from service_m (-1 included), neighbour lists and the order stream, against what the reference built."""
    import time
    g = load_fuzz(name)
    C, mode = int(g["C"]), str(g["cluster_mode"])
    city = synth.make_city(int(g["city_seed"]), N=int(g["N"]), C=C, frac=str(g["style"]) == "frac", with_neighbors=False)
    if city.cost_float is None:
        city.cost = g["cost"]               # (the styled table travels in the fixture)
    city.node2cluster = g["node2cluster"]
    start, pick, dele = synth.make_orders(int(g["order_seed"]), city.N, int(g["n_orders_raw"]))
    os.environ["TZ"] = "UTC"
    time.tzset()
    write_reference_data_dir(str(tmp_path), city, start, pick, dele, n_drivers=int(g["V"]), cluster_mode=mode)
    table = synth.neighbor_table_from_sums(*synth.cluster_cost_sums_host(city.cost, city.node2cluster, C))
    world.write_neighbor_csv(os.path.join(str(tmp_path), "data", str(tuple(city.bound)) + str(C) + mode + "Neighbor.csv"), table)
    W = world.load_world(os.path.join(str(tmp_path), "data"), cluster_mode=mode, local_region_bound=synth.DEFAULT_BOUND,
                         side_length_meter=float(g["side_m"]), vehicles_service_meter=float(g["service_m"]))
    np.testing.assert_array_equal(W.cost, g["cost"])
    np.testing.assert_array_equal(W.node2cluster, g["node2cluster"])
    assert W.n_clusters == C and W.depth_limit == int(g["depth_limit"])
    nbr = [g["nbr_idx"][g["nbr_off"][c]:g["nbr_off"][c + 1]].tolist() for c in range(C)]
    assert [list(x) for x in W.neighbors] == nbr
    np.testing.assert_array_equal(W.o_release_min, g["o_release_min"])
    np.testing.assert_array_equal(W.o_pickup, g["o_pickup"])
    np.testing.assert_array_equal(W.o_delivery, g["o_delivery"])
