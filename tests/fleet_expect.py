"""What a replica with a fleet of its own (vds_set_fleet) has to show, shared by tests/test_fleet_expect.py (CPU) and
tests/test_gpu_fleet.py: the loader of the reference-run fixtures (tests/golden/make_fleet_golden.py), the oracle of one replica -
``Oracle(V = fleet[r])`` reset with the first ``fleet[r]`` nodes of the replica's row - and the comparison of a replica's lists and
vehicles with it.  No GPU is touched by importing this."""
import os

import numpy as np

from helpers import GOLDEN_DIR, engine_settings
from oracle.oracle import Oracle

FLEET_PACK = os.path.join(GOLDEN_DIR, "fleetpack_0.npz")
# (fixture, V): any two fleet sizes reject differently (the issue's table, from the CPU oracle; asserted by test_fleet_expect)
TINY_REJECTS = {
    "tiny_kmeans": {0: 2499, 1: 2465, 2: 2434, 37: 1472, 75: 751, 149: 280, 150: 279},
    "tiny_kmeans_dfs2": {0: 2999, 1: 2969, 12: 2634, 25: 2265, 49: 1659, 50: 1634},
    "tiny_dispatch": {139: 286, 140: 285},
}


def fleet_runs():
    """{case: ascending VehiclesNumber of its recorded runs}."""
    runs = {}
    with np.load(FLEET_PACK) as z:
        for k in z.files:
            case, V = k.split("/")[0].rsplit("_", 1)
            runs.setdefault(case, set()).add(int(V))
    return {c: sorted(v) for c, v in runs.items()}


def load_fleet(case, V):
    """One recorded run in the form of a tiny fixture: its own arrays over what its case's largest run stores for all of them."""
    top = fleet_runs()[case][-1]
    g = {}
    with np.load(FLEET_PACK) as z:
        for name in ("%s_%d" % (case, top), "%s_%d" % (case, V)):
            for k in z.files:
                if k.startswith(name + "/"):
                    a = z[k]
                    g[k[len(name) + 1:]] = a.astype(np.int32) if a.dtype == np.int16 else a
    assert int(g["V"]) == V
    return g


def fleet_oracle(g, f, nodes):
    """The expectation for a replica of fleet ``f`` on the city and day of fixture ``g`` whose row of start nodes is ``nodes``."""
    o = Oracle(g["cost"], g["node2cluster"], g["nbr_off"], g["nbr_idx"], int(g["depth_limit"]), bool(g["neighbor_can_server"]),
               g["o_release_min"], g["o_pickup"], g["o_delivery"], int(f), **engine_settings(g))
    o.reset(np.ascontiguousarray(np.asarray(nodes)[:f], dtype=np.int32))
    return o


def check_fleet_lists(G, W, o, f, V, C, tag):
    """``env.lists(r)`` (G) and ``env.vehicles(r)`` (W) of a replica of fleet ``f`` on a handle of ``V`` vehicles against its oracle:
    lists and arrival tables in container order, the vehicles below ``f`` field by field, the absent ones 255 / -1."""
    L, veh = o.lists(), o.vehicles()
    n, na = int(L["idle_off"][-1]), int(L["arr_off"][-1])
    assert n + na == f, tag
    for k in ("idle_off", "arr_off"):
        np.testing.assert_array_equal(G[k], L[k], err_msg="%s %s" % (tag, k))
    np.testing.assert_array_equal(G["idle_veh"][:n], L["idle_veh"][:n], err_msg=tag + " idle order")
    np.testing.assert_array_equal(G["idle_node"][:n], veh["loc"][L["idle_veh"][:n]], err_msg=tag + " idle nodes")
    for k in ("arr_veh", "arr_min"):
        np.testing.assert_array_equal(G[k][:na], L[k][:na], err_msg="%s %s" % (tag, k))
    np.testing.assert_array_equal(G["arr_node"][:na], veh["dest"][L["arr_veh"][:na]], err_msg=tag + " arr_node")
    np.testing.assert_array_equal(G["arr_order"][:na], veh["order"][L["arr_veh"][:na]], err_msg=tag + " arr_order")
    for k in ("idle_veh", "idle_node"):
        assert (G[k][n:] == -1).all(), (tag, k)
    for k in ("arr_veh", "arr_min", "arr_order", "arr_node"):
        assert (G[k][na:] == -1).all(), (tag, k)
    # vehicles: those of the fleet against the oracle, the others in no container
    idle = np.zeros(V, dtype=bool); idle[L["idle_veh"][:n]] = True
    fly = L["arr_veh"][:na]
    st = W["state"].astype(np.int32)
    assert ((st == 0) == idle).all() and sorted(np.flatnonzero((st > 0) & (st < 255)).tolist()) == sorted(fly.tolist()), tag
    assert (st[f:] == 255).all() and (st[:f] != 255).all(), tag
    for k in ("node", "cluster", "arrive_min", "order"):
        assert (W[k][f:] == -1).all(), (tag, k)
    np.testing.assert_array_equal(W["node"][:f][idle[:f]], veh["loc"][idle[:f]], err_msg=tag)
    np.testing.assert_array_equal(W["node"][fly], veh["dest"][fly], err_msg=tag)
    np.testing.assert_array_equal(W["order"][fly], veh["order"][fly], err_msg=tag)
    np.testing.assert_array_equal(st[fly], np.where(veh["order"][fly] >= 0, 1, 2), err_msg=tag)
    np.testing.assert_array_equal(W["arrive_min"][fly], L["arr_min"][:na], err_msg=tag)
    assert (W["arrive_min"][idle] == -1).all() and (W["order"][idle] == -1).all(), tag
    cl = np.full(V, -1, dtype=np.int64)
    cl[L["idle_veh"][:n]] = np.repeat(np.arange(C), np.diff(L["idle_off"]))
    cl[fly] = np.repeat(np.arange(C), np.diff(L["arr_off"]))
    np.testing.assert_array_equal(W["cluster"], cl, err_msg=tag + " cluster")


def expected_start_lists(node2cluster, C, nodes, f):
    """(idle_off [C + 1], idle_veh [f], idle_node [f]) right after a reset, by numpy: vehicles 0 .. f - 1 in vehicle order per cluster."""
    nodes = np.asarray(nodes)[:f]
    cl = np.asarray(node2cluster)[nodes]
    order = np.argsort(cl, kind="stable")
    off = np.zeros(C + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(cl, minlength=C))
    return off, order, nodes[order]
