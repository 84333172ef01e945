"""Fixture of the externally matched day.  Runs ONLY where the reference lies (oracle/ref_harness.py).

    python tests/golden/make_match_golden.py

The unmodified reference runs a tiny city with ``MatchFunction`` replaced by a matcher written in the reference's idiom - the cursor
and the bookkeeping of ``simulator.py:909-919`` and ``:948-973`` as they are, the search (``:921-943``) replaced: the LAST vehicle of
the pickup cluster's ``IdleVehicles`` if there is one, else the FIRST idle vehicle of the lowest-numbered cluster that has one, else
"Reject".  So the day has matches across clusters and rejects, and no pickup window.  Recorded per slot, behind Match and
SupplyExpect: the assignment (vehicle per processed order, -1 = reject), idle lists and arrival dicts in container order with their
minutes, counters and observations; per order the result.  ``tests/golden/matchpack_0.npz`` holds data only.
tests/test_match_model.py replays it on tests/match_model.py, tests/test_gpu_match_external.py on the GPU."""
from __future__ import annotations

import os
import random
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from vehicles_dispatch_simulator_amd import synth  # noqa: E402
import ref_harness as rh  # noqa: E402

CASE = dict(city=dict(seed=131, N=120, C=12), O=420, oseed=31, V=14, seed=41, cluster_mode="KmeansClustering", tick_minutes=10)


def install_matcher(S, setting, veh_index, rows):
    """``S.MatchFunction`` := the cursor and bookkeeping of the reference's, with the search replaced (module docstring)."""

    def match():
        for cl in S.Clusters:
            cl.PerMatchIdleVehicles = len(cl.IdleVehicles)
        row = []
        while S.NowOrder.ReleasTime < S.RealExpTime + S.TimePeriods:
            if S.NowOrder.ID == S.Orders[-1].ID:
                break
            S.OrderNum += 1
            order = S.NowOrder
            home = S.NodeID2Cluseter[order.PickupPoint]
            home.Orders.append(order)
            # ---- the search, replaced
            found = None
            if len(home.IdleVehicles):
                found = (home.IdleVehicles[-1], home)
            else:
                for cl in S.Clusters:
                    if len(cl.IdleVehicles):
                        found = (cl.IdleVehicles[0], cl)
                        break
            # ---- the bookkeeping, kept
            if found is None:
                S.RejectNum += 1
                order.ArriveInfo = "Reject"
                row.append(-1)
            else:
                veh, src = found
                wait = S.RoadCost(veh.LocationNode, order.PickupPoint)
                order.PickupWaitTime = wait
                veh.Orders.append(order)
                S.TotallyWaitTime += wait
                trip = wait + S.RoadCost(order.PickupPoint, order.DeliveryPoint)
                veh.DeliveryPoint = order.DeliveryPoint
                S.Clusters[S.NodeID2Cluseter[order.DeliveryPoint].ID].VehiclesArrivetime[veh] = S.RealExpTime + np.timedelta64(trip * setting.MINUTES)
                src.IdleVehicles.remove(veh)
                order.ArriveInfo = "Success"
                row.append(veh_index[id(veh)])
            S.NowOrder = S.Orders[order.ID + 1]
        rows.append(row)

    S.MatchFunction = match


def generate():
    setting, refsim = rh._import_reference()
    city = synth.make_city(**CASE["city"])
    start, pick, dele = synth.make_orders(CASE["oseed"], city.N, CASE["O"])
    V, tick = CASE["V"], CASE["tick_minutes"]
    root = tempfile.mkdtemp(prefix="vds_match_ref_")
    cwd, old_stdout = os.getcwd(), sys.stdout
    devnull = open(os.devnull, "w")
    try:
        rh.write_reference_data_dir(root, city, start, pick, dele, n_drivers=V, cluster_mode=CASE["cluster_mode"])
        os.chdir(root)
        sys.stdout = devnull
        random.seed(CASE["seed"])
        S = refsim.Simulation(ClusterMode=CASE["cluster_mode"], DemandPredictionMode="None", DispatchMode="Simulation", VehiclesNumber=V,
                              TimePeriods=np.timedelta64(tick * setting.MINUTES), LocalRegionBound=tuple(city.bound), SideLengthMeter=3200,
                              VehiclesServiceMeter=3200, NeighborCanServer=False, FocusOnLocalRegion=False)
        S.CreateAllInstantiate("1101")
        C, N, O = len(S.Clusters), len(S.Node), len(S.Orders)
        veh_index = {id(v): i for i, v in enumerate(S.Vehicles)}
        veh_node = np.array([v.LocationNode for v in S.Vehicles], dtype=np.int32)
        n2c = np.full(N, -1, dtype=np.int32)
        for n, c in S.NodeID2Cluseter.items():
            n2c[int(n)] = c.ID
        ep0 = S.Orders[0].ReleasTime
        minute = lambda t: int((t - ep0).total_seconds()) // 60
        rows, slots = [], []
        install_matcher(S, setting, veh_index, rows)
        orig_supply = S.SupplyExpectFunction

        def supply():
            orig_supply()
            rec = dict(order_num=S.OrderNum, reject_num=S.RejectNum, wait_sum=int(S.TotallyWaitTime),
                       idle_pre=[cl.PerMatchIdleVehicles for cl in S.Clusters], cl_orders=[len(cl.Orders) for cl in S.Clusters],
                       supply=np.asarray(S.SupplyExpect).astype(np.int64).tolist(), idle=[], idle_off=[0], arr_veh=[], arr_min=[], arr_off=[0])
            for cl in S.Clusters:
                rec["idle"].extend(veh_index[id(v)] for v in cl.IdleVehicles)
                rec["idle_off"].append(len(rec["idle"]))
                for v, t in cl.VehiclesArrivetime.items():
                    rec["arr_veh"].append(veh_index[id(v)])
                    rec["arr_min"].append(minute(t))
                rec["arr_off"].append(len(rec["arr_veh"]))
            slots.append(rec)

        S.SupplyExpectFunction = supply
        S.SimCity()
        sys.stdout = old_stdout
        T = len(slots)
        assert T == S.step == len(rows)
        M = max(len(r) for r in rows)
        pad = lambda x, n: list(x) + [-1] * (n - len(x))
        status = np.array([2 if o.ArriveInfo == "Reject" else (1 if o.ArriveInfo is not None else 0) for o in S.Orders], dtype=np.uint8)
        out = dict(
            N=np.int64(N), C=np.int64(C), V=np.int64(V), tick_minutes=np.int64(tick), cost=np.trunc(S.Map.values).astype(np.int32),
            node2cluster=n2c, veh_node=veh_node, nbr_off=np.zeros(C + 1, dtype=np.int32), nbr_idx=np.zeros(0, dtype=np.int32),
            depth_limit=np.int64(0), neighbor_can_server=np.bool_(False),
            o_release_min=np.array([minute(o.ReleasTime) for o in S.Orders], dtype=np.int32),
            o_pickup=np.array([o.PickupPoint for o in S.Orders], dtype=np.int32), o_delivery=np.array([o.DeliveryPoint for o in S.Orders], dtype=np.int32),
            o_value=np.array([o.OrderValue for o in S.Orders], dtype=np.int32), n_ticks=np.int64(T),
            slot_n=np.array([len(r) for r in rows], dtype=np.int32), assign=np.array([pad(r, M) for r in rows], dtype=np.int32).reshape(T, M),
            o_status=status, o_wait=np.array([int(o.PickupWaitTime) if s == 1 else -1 for o, s in zip(S.Orders, status)], dtype=np.int32),
            t_order_num=np.array([s["order_num"] for s in slots], dtype=np.int64), t_reject_num=np.array([s["reject_num"] for s in slots], dtype=np.int64),
            t_wait_sum=np.array([s["wait_sum"] for s in slots], dtype=np.int64),
            t_idle_pre=np.array([s["idle_pre"] for s in slots], dtype=np.int32), t_cl_orders=np.array([s["cl_orders"] for s in slots], dtype=np.int32),
            t_supply=np.array([s["supply"] for s in slots], dtype=np.int32),
            l_idle_off=np.array([s["idle_off"] for s in slots], dtype=np.int32), l_idle_veh=np.array([pad(s["idle"], V) for s in slots], dtype=np.int32),
            l_arr_off=np.array([s["arr_off"] for s in slots], dtype=np.int32), l_arr_veh=np.array([pad(s["arr_veh"], V) for s in slots], dtype=np.int32),
            l_arr_min=np.array([pad(s["arr_min"], V) for s in slots], dtype=np.int32),
        )
        o_vehicle = np.full(O, -1, dtype=np.int32)
        k = 0
        for r in rows:
            o_vehicle[k:k + len(r)] = r
            k += len(r)
        out["o_vehicle"] = o_vehicle
        assert (out["cost"] == city.cost).all() and (n2c == city.node2cluster).all()
        return out
    finally:
        sys.stdout = old_stdout
        devnull.close()
        os.chdir(cwd)
        shutil.rmtree(root, ignore_errors=True)


def main():
    g = generate()
    n2c, cross = g["node2cluster"], 0
    assert int((g["o_status"] == 2).sum()) > 10 and int((g["o_status"] == 1).sum()) > 50, "the day needs matches and rejects"
    # a match from another cluster than the pickup's: the wait is a cost no vehicle of the pickup cluster could have had ... counted on the model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from match_model import MatchModel
    m = MatchModel(g["cost"], n2c, int(g["C"]), int(g["V"]), g["o_release_min"], g["o_pickup"], g["o_delivery"], int(g["tick_minutes"]))
    m.reset(g["veh_node"])
    for t in range(int(g["n_ticks"])):
        m.update()
        for o, v in zip(m.slot_orders(), g["assign"][t]):
            cross += v >= 0 and m.cluster[v] != n2c[g["o_pickup"][o]]
        m.match(g["assign"][t])
        m.end_tick()
    assert cross > 5, "the day needs matches across clusters"
    path = os.path.join(HERE, "matchpack_0.npz")
    np.savez_compressed(path, **g)
    print("%s: %d bytes, %d slots, %d orders, %d served (%d across clusters), %d rejected" % (
        os.path.basename(path), os.path.getsize(path), int(g["n_ticks"]), int(g["t_order_num"][-1]), int((g["o_status"] == 1).sum()), cross, int((g["o_status"] == 2).sum())))


if __name__ == "__main__":
    main()
