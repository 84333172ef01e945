"""CPU side of the fleet-size feature (vds_set_fleet): the CPU oracle replays every run of tests/golden/fleetpack_0.npz - one city,
one day, one seed run by the unmodified reference at several ``VehiclesNumber`` (tests/golden/make_fleet_golden.py) - bit for bit;
the conditions that make those runs a pin hold (start nodes of a smaller run are a prefix of the largest run's, any two sizes
reject differently); the tiny fixtures reject what the GPU tests rely on at every fleet size they use; and the start nodes
``vds_py_random_nodes`` draws for a smaller fleet are a prefix of the ``V``-draw sequence.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from fleet_expect import FLEET_PACK, TINY_REJECTS, fleet_oracle, fleet_runs, load_fleet
from helpers import GOLDEN_DIR, load_golden
from test_oracle_golden import replay

RUNS = [(case, V) for case, sizes in sorted(fleet_runs().items()) for V in sizes]


def test_the_recorded_sizes_are_the_ones_chosen():
    assert fleet_runs() == {"fleetA": [0, 1, 2, 33, 64, 65, 139, 140], "fleetB": [1, 20, 50]}
    a, b = load_fleet("fleetA", 140), load_fleet("fleetB", 50)
    assert 550 <= int(a["order_num"]) <= 650 and not bool(a["neighbor_can_server"])
    assert bool(b["neighbor_can_server"]) and int(b["depth_limit"]) == 2
    largest = max(os.path.getsize(os.path.join(GOLDEN_DIR, f)) for f in os.listdir(GOLDEN_DIR) if f.startswith("fuzzpack_"))
    assert os.path.getsize(FLEET_PACK) <= largest


@pytest.mark.parametrize("case,V", RUNS, ids=["%s-%d" % r for r in RUNS])
def test_oracle_replays_the_reference_at_every_recorded_fleet(case, V):
    g = load_fleet(case, V)
    o = replay(g, check_lists=True)
    od = o.orders()
    for k in ("status", "vehicle", "wait"):
        np.testing.assert_array_equal(od[k], g["o_" + k])
    c = o.counters()
    for k in ("order_num", "reject_num", "wait_sum", "sum_order_value"):
        assert c[k] == int(g[k]), k


@pytest.mark.parametrize("case", sorted(fleet_runs()))
def test_prefix_and_distinctness_of_the_recorded_runs(case):
    sizes = fleet_runs()[case]
    top = load_fleet(case, sizes[-1])
    rejects = []
    for V in sizes:
        g = load_fleet(case, V)
        np.testing.assert_array_equal(g["veh_node"], top["veh_node"][:V])
        rejects.append(int(g["reject_num"]))
        # the oracle a replica of that fleet is compared with (the largest run's row, cut) is the recorded run
        o = fleet_oracle(top, V, top["veh_node"])
        o.run_day()
        assert o.counters()["reject_num"] == rejects[-1] and np.array_equal(o.orders()["vehicle"], g["o_vehicle"])
    assert len(set(rejects)) == len(rejects) and rejects == sorted(rejects, reverse=True), rejects
    if 0 in sizes:
        assert rejects[0] == int(top["order_num"])            # no vehicle: every processed order is rejected


@pytest.mark.parametrize("name", sorted(TINY_REJECTS))
def test_tiny_fixtures_reject_differently_at_every_fleet_size_used(name):
    g = load_golden(name)
    got = {}
    for f in TINY_REJECTS[name]:
        o = fleet_oracle(g, f, g["veh_node"])
        o.run_day()
        got[f] = int(o.counters()["reject_num"])
    assert got == TINY_REJECTS[name]
    assert len(set(got.values())) == len(got)
    assert max(TINY_REJECTS[name]) == int(g["V"])


@pytest.mark.parametrize("seed", [3, 2**32 + 17])
def test_random_nodes_of_a_smaller_fleet_are_a_prefix(seed):
    from vehicles_dispatch_simulator_amd import _lib
    lib = _lib.load()
    N, V = 500, 130
    valid = (np.arange(N) % 3 != 0).astype(np.uint8)

    def draw(n):
        out = np.full(max(n, 1), -7, dtype=np.int32)
        assert lib.vds_py_random_nodes(C.c_uint64(seed), N, n, valid.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
        return out[:n]

    full = draw(V)
    assert (valid[full] == 1).all()
    for f in (0, 1, 63, 64, 65):
        np.testing.assert_array_equal(draw(f), full[:f])
