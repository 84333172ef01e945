"""configs[1] hooked day with the two device dispatch forms, without and with the per-entry arrival-minute and counted tensors
(vds_run_hooked_vehicles_ex / vds_run_hooked_roster_ex): what DESIGN.md's k_dispatch_vehicles_timed / k_dispatch_roster_timed figures
were timed on.  Modelled on profiles/dispatch_vehicles_day.py, whose cases b / c / d are the plain vehicle form here.

    python profiles/dispatch_times_day.py [replicas=1024] [days=20] [out.json]

One process, one handle, HIP events around whole run_hooked days (one graph launch each; per-slot time = day / T).  Every case: two
untimed days (the first builds / updates the day graph), then `days` timed ones; median (min - max).  Cases:
    z        the hooked day with nothing in it
    r        the roster refresh alone (the roster form needs it in every slot: its cases are read against this one)
    v0 v1 v50    the vehicle form, plain kernel: an all-negative tensor, ~1 %, ~half of the entries a random valid node
    V0 V1 V50    ... with both tensors: k_dispatch_vehicles_timed
    p0 p1 p50    the roster form, plain kernel, the same shares by roster position
    P0 P1 P50    ... with both tensors: k_dispatch_roster_timed
The arrival-minute tensor holds the sentinel (now + RoadCost) and the counted tensor 1 everywhere: the timed days move the vehicles
the plain days move, slot for slot, so the difference is the two extra loads per mover and the variant's own code, not another day."""
import json
import os
import sys

ARRIVE_ROAD = -2 ** 31


def main(R, days, out_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from vehicles_dispatch_simulator_amd import workloads

    w = workloads.didi_day()
    stream = torch.cuda.current_stream()
    # (ring_cap: as profiles/dispatch_vehicles_day.py; idle_cap: as profiles/idle_roster_day.py - by roster position the same tensor sends
    # whoever stands at a chosen position to a random node every slot, which fills the largest clusters' lists beyond the default)
    env = w.make_env(R, stream=stream.cuda_stream, ring_cap=128, idle_cap=1024)
    env.reset(w.vehicle_nodes(R))
    V, T = env.V, env.T
    valid = np.flatnonzero(w.city.node2cluster >= 0)
    gen = torch.Generator(device="cuda").manual_seed(20)
    valid_t = torch.from_numpy(valid.astype(np.int32)).cuda()

    def tensor(frac):
        t = torch.full((R, V), -1, dtype=torch.int32, device="cuda")
        if frac > 0:
            pick = torch.rand((R, V), device="cuda", generator=gen) < frac
            node = valid_t[torch.randint(0, valid.size, (R, V), device="cuda", generator=gen)]
            t = torch.where(pick, node, t)
        return t.contiguous()

    tg = {"0": tensor(0.0), "1": tensor(0.01), "50": tensor(0.5)}          # (generated in the order of dispatch_vehicles_day.py's b / c / d)
    road = torch.full((R, V), ARRIVE_ROAD, dtype=torch.int32, device="cuda")
    ones = torch.ones((R, V), dtype=torch.int32, device="cuda")
    off = dict(idle_pre=False, idle_now=False, supply=False, cl_orders=False)
    cases = {"z": dict(), "r": dict(roster=True)}
    for k, t in tg.items():
        cases["v" + k] = dict(vehicle_targets=t)
        cases["V" + k] = dict(vehicle_targets=t, vehicle_arrive_min=road, vehicle_counted=ones)
        cases["p" + k] = dict(roster=True, roster_targets=t)
        cases["P" + k] = dict(roster=True, roster_targets=t, roster_arrive_min=road, roster_counted=ones)

    res = {}
    for k, kw in cases.items():
        ms = []
        try:
            for i in range(2 + days):
                env.reset_again()
                env.sync()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                env.run_hooked(T, **off, **kw)
                b.record(stream)
                env.sync()
                torch.cuda.synchronize()
                if i >= 2:
                    ms.append(a.elapsed_time(b))
        except Exception as e:          # a table of the handle is too small for this case's moves (sticky capacity error at sync): said, not timed
            res[k] = dict(error=str(e)[:200])
            continue
        d = sorted(ms)
        cn = env.counters()
        res[k] = dict(slot_us=d[len(d) // 2] / T * 1e3, slot_us_min=d[0] / T * 1e3, slot_us_max=d[-1] / T * 1e3,
                      moves_per_slot=float(cn[:, 4].sum()) / (T * R), dispatch_cost=int(cn[:, 5].sum()))
    for k in tg:          # the timed day is the plain day
        for a, b in (("v", "V"), ("p", "P")):
            if "error" in res[a + k] or "error" in res[b + k]:
                continue
            assert res[a + k]["moves_per_slot"] == res[b + k]["moves_per_slot"] and res[a + k]["dispatch_cost"] == res[b + k]["dispatch_cost"], (a, k)
    out = dict(R=R, C=env.C, V=V, T=T, days=days, dense=env.layout()["dense"], build_id=env._lib.vds_build_id().decode(), cases=res)
    print(json.dumps(out))
    for k, o in res.items():
        if "error" in o:
            print("%-4s not timed: %s" % (k, o["error"]))
            continue
        print("%-4s %7.2f us per slot (%.2f - %.2f), %.1f moves per slot and replica" % (k, o["slot_us"], o["slot_us_min"], o["slot_us_max"], o["moves_per_slot"]))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    env.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1024, int(sys.argv[2]) if len(sys.argv) > 2 else 20, sys.argv[3] if len(sys.argv) > 3 else None)
