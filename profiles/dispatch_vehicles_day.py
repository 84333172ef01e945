"""configs[1] hooked day with the per-vehicle dispatch (vds_run_hooked after vds_run_hooked_vehicles), what DESIGN.md's
k_dispatch_vehicles figures were timed on.

    python profiles/dispatch_vehicles_day.py [replicas=1024] [rounds=5] [out.json]

One process, one handle, HIP events around whole run_hooked days (one graph launch each; per-slot time = day / T).  The cases take turns,
`rounds` times over; every timed day follows an untimed day of the same case (which builds / updates the day graph: host work that
would otherwise sit inside the event window):
    z  the hooked day with nothing in it (no planes, no dispatch): what the others are read against
    a  the K-form hooked slot, K = 8, an action tensor without actions (k_dispatch_dense reads it and finds none) - the parent's graph
    b  the vehicle form with an all-negative tensor: the kernel's floor, list walk + gather
    c  ... with ~1 % of the tensor's entries a random valid node: ~1 % of the idle vehicles move per slot
    d  ... with ~half of them
    e  the planes refresh alone, state | cluster (fill + k_vehicle_lists + k_vehicle_pull per slot)
The same tensor is applied every slot: whoever is idle and has an entry moves (and moves again once it has arrived).
Byte model of k_dispatch_vehicles per slot: 8 B per idle vehicle (4 B list entry + 4 B gathered target) + 64 B per bucket
(header line) + per mover 32 B (cost sector) + 12 B (arrival entry + minute) + 4 B (atomic on the ring counter) + 4 B (compacted list).
idle / movers per slot are counted on the device in an untimed census day of each case (a captured policy sums the idle_now plane;
the movers are the day's DispatchNum).  Kernel time is taken as case - z (for c / d an approximation: moved vehicles change what the
tick has to do); share of peak = model bytes / that time / 8 TB/s."""
import json
import os
import sys

PEAK = 8.0e12
K_FORM = 8


def main(R, rounds, out_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from vehicles_dispatch_simulator_amd import workloads

    w = workloads.didi_day()
    stream = torch.cuda.current_stream()
    # (ring_cap: half of the idle vehicles of a slot land in 192 clusters within a few arrival slots - the default is sized for the order flow)
    env = w.make_env(R, stream=stream.cuda_stream, ring_cap=128)
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

    acts = torch.full((R, K_FORM, 3), -1, dtype=torch.int32, device="cuda")
    off = dict(idle_pre=False, idle_now=False, supply=False, cl_orders=False)
    cases = {
        "z": dict(),
        "a": dict(actions=acts),
        "b": dict(vehicle_targets=tensor(0.0)),
        "c": dict(vehicle_targets=tensor(0.01)),
        "d": dict(vehicle_targets=tensor(0.5)),
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
    for k in "bcd":
        o = res[k]
        o["model_bytes_per_slot"] = R * (8 * o["idle_per_slot"] + 64 * C + 52 * o["moves_per_slot"])
        o["kernel_us"] = o["slot_us"] - res["z"]["slot_us"]
        o["share_of_peak"] = o["model_bytes_per_slot"] / (o["kernel_us"] * 1e-6) / PEAK if o["kernel_us"] > 0 else None
    out = dict(R=R, C=C, V=V, T=T, rounds=rounds, dense=env.layout()["dense"], build_id=env._lib.vds_build_id().decode(), cases=res)
    print(json.dumps(out))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    env.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1024, int(sys.argv[2]) if len(sys.argv) > 2 else 5, sys.argv[3] if len(sys.argv) > 3 else None)
