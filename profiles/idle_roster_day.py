"""configs[1] hooked day with the idle roster and the dispatch by roster position (vds_run_hooked after vds_run_hooked_roster), next to
the vehicle-form cases of profiles/dispatch_vehicles_day.py re-run in the same process: what DESIGN.md's k_idle_roster /
k_dispatch_roster figures were timed on.

    python profiles/idle_roster_day.py [replicas=1024] [rounds=5] [out.json]

One process, one handle, HIP events around whole run_hooked days (one graph launch each; per-slot time = day / T).  The cases take turns,
`rounds` times over; every timed day follows an untimed day of the same case (which builds / updates the day graph: host work that
would otherwise sit inside the event window):
    z   the hooked day with nothing in it (no planes, no dispatch): what the others are read against
    r   the roster refresh alone (k_idle_roster per slot)
    rb  refresh + roster targets all negative: the dispatch kernel's floor, list walk + contiguous target loads
    rc  ... with ~1 % of the tensor's entries a random valid node: ~1 % of the idle vehicles move per slot
    b   the vehicle form with an all-negative tensor (dispatch_vehicles_day.py's b)
    c   ... with ~1 % of the entries a random valid node (its c)
    e   the per-vehicle planes refresh alone, state | cluster (its e)
Tables: ring_cap = 128 as in dispatch_vehicles_day.py, but idle_cap = 1024 where that script keeps the library's default - rc
overflows the default (see main) - and EVERY case here, b / c / e included, runs on these larger idle tables, so that the arms share them.
The same tensor is applied every slot.  idle / movers per slot are counted on the device in an untimed census day of each case (a
captured policy sums the idle_now plane; the movers are the day's DispatchNum).
Byte models per slot, dense layout (list entries of 4 B; 8 B on the wide layout):
    refresh   R * (64 * C + 4 * (C + 1))  read   (the bucket records, one 64-byte line each; cl_off)
              + R * 4 * idle              read   (the list entries)
              + R * (3 * 4 * V + 4 * (C + 1))  written
    dispatch  k_dispatch_vehicles' model with the 4-byte gather counted as contiguous: R * (8 * idle + 64 * C + 8 * C + 52 * movers)
Kernel time is taken as case - z for r, and (rb | rc) - r for the dispatch; share of peak = model bytes / that time / 8 TB/s."""
import json
import os
import sys

PEAK = 8.0e12


def main(R, rounds, out_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from vehicles_dispatch_simulator_amd import workloads

    w = workloads.didi_day()
    stream = torch.cuda.current_stream()
    # (idle_cap: rc sends whoever stands at a chosen roster position to a random NODE every slot, so a cluster's idle list settles near
    # idle vehicles x its share of the nodes - beyond the default capacity for the largest clusters; every case runs on these tables)
    env = w.make_env(R, stream=stream.cuda_stream, ring_cap=128, idle_cap=1024)
    env.reset(w.vehicle_nodes(R))
    V, C, T = env.V, env.C, env.T
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

    off = dict(idle_pre=False, idle_now=False, supply=False, cl_orders=False)
    cases = {
        "z": dict(),
        "r": dict(roster=True),
        "rb": dict(roster=True, roster_targets=tensor(0.0)),
        "rc": dict(roster=True, roster_targets=tensor(0.01)),
        "b": dict(vehicle_targets=tensor(0.0)),
        "c": dict(vehicle_targets=tensor(0.01)),
        "e": dict(vehicle_planes=dict(state=True, cluster=True)),
    }
    ob = env.obs_torch(inflight=False)
    idle_sum = torch.zeros((), dtype=torch.int64, device="cuda")

    def policy():
        idle_sum.add_(ob[1].sum())

    side = torch.cuda.Stream()
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        for _ in range(2):
            policy()
    stream.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        policy()

    res = {k: dict(day_ms=[]) for k in cases}
    for k, kw in cases.items():          # census: idle vehicles and movers per slot and replica
        env.reset_again(); idle_sum.zero_()
        env.run_hooked(T, policy_graph=graph, **{**off, "idle_now": True}, **kw)
        env.sync()
        res[k]["idle_per_slot"] = int(idle_sum.item()) / (T * R)
        res[k]["moves_per_slot"] = float(env.counters()[:, 4].sum()) / (T * R)
    for _ in range(rounds):
        for k, kw in cases.items():
            for timed in (False, True):
                env.reset_again()
                env.sync()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                env.run_hooked(T, **off, **kw)
                b.record(stream)
                env.sync()
                torch.cuda.synchronize()
                if timed:
                    res[k]["day_ms"].append(a.elapsed_time(b))
    for k, o in res.items():
        d = sorted(o["day_ms"])
        o["slot_us"] = d[len(d) // 2] / T * 1e3
        o["slot_us_min"], o["slot_us_max"] = d[0] / T * 1e3, d[-1] / T * 1e3
        o["minus_z_us"] = o["slot_us"] - res["z"]["slot_us"]
    entry = 4 if env.layout()["dense"] else 8

    def share(model, us):
        return model / (us * 1e-6) / PEAK if us > 0 else None

    o = res["r"]
    o["model_bytes_per_slot"] = R * (64 * C + 4 * (C + 1) + entry * o["idle_per_slot"] + 12 * V + 4 * (C + 1))
    o["kernel_us"] = o["minus_z_us"]
    o["share_of_peak"] = share(o["model_bytes_per_slot"], o["kernel_us"])
    for k in ("rb", "rc"):
        o = res[k]
        o["model_bytes_per_slot"] = R * ((entry + 4) * o["idle_per_slot"] + 72 * C + 52 * o["moves_per_slot"])
        o["kernel_us"] = o["slot_us"] - res["r"]["slot_us"]
        o["share_of_peak"] = share(o["model_bytes_per_slot"], o["kernel_us"])
    for k in ("b", "c"):
        o = res[k]
        o["model_bytes_per_slot"] = R * ((entry + 4) * o["idle_per_slot"] + 64 * C + 52 * o["moves_per_slot"])
        o["kernel_us"] = o["minus_z_us"]
        o["share_of_peak"] = share(o["model_bytes_per_slot"], o["kernel_us"])
    out = dict(R=R, C=C, V=V, T=T, rounds=rounds, dense=env.layout()["dense"], build_id=env._lib.vds_build_id().decode(), cases=res)
    print(json.dumps(out))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    env.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1024, int(sys.argv[2]) if len(sys.argv) > 2 else 5, sys.argv[3] if len(sys.argv) > 3 else None)
