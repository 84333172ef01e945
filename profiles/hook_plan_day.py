"""configs[1] hooked day with the observation planes only and with every optional block switched on, and the host side of a
vds_run_hooked call that replays the cached day graph (where the plan is resolved and compared with the one the graph was built with).

    python profiles/hook_plan_day.py [replicas=1024] [rounds=5] [hits=200]

One process, one handle, HIP events around whole run_hooked days (one graph launch; per-slot time = day / T).  The cases take turns,
`rounds` times over; every timed day follows an untimed day of the same case (which builds the day graph).
    o    the four default observation planes, nothing else
    all  observation planes + outcomes, idle heads (L = 4), per-vehicle planes (state | cluster), per-vehicle outcomes, the idle
         roster, the orders block, K = 2 actions and per-vehicle targets (both tensors all negative: the kernels run, nothing moves)
Host time of a hit: `hits` calls of run_hooked(1) at slot 0 with the `all` switches, each behind reset_again + sync (the same first
slot, the same plan: the graph at hand is launched), host clock around the call alone - the five setters, the resolve, the
comparison and hipGraphLaunch of a one-slot graph.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time


def main(R, rounds, hits):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from vehicles_dispatch_simulator_amd import workloads

    w = workloads.didi_day()
    stream = torch.cuda.current_stream()
    env = w.make_env(R, stream=stream.cuda_stream, ring_cap=128, idle_cap=1024)
    init = w.vehicle_nodes(R)
    env.reset(init)
    T = env.T
    acts = torch.full((R, 2, 3), -1, dtype=torch.int32, device="cuda")
    targets = torch.full((R, env.V), -1, dtype=torch.int32, device="cuda")
    cases = {
        "o": dict(),
        "all": dict(outcomes=True, idle_heads=4, vehicle_planes=dict(state=True, cluster=True), vehicle_outcomes=True, roster=True, orders=True,
                    actions=acts, vehicle_targets=targets),
    }
    out = dict(R=R, T=T, build=env._lib.vds_build_id().decode(), main_kernel=env.main_kernel(), us_per_slot={k: [] for k in cases})
    for rnd in range(rounds):
        for name, kw in cases.items():
            for timed in (False, True):     # (the untimed day builds the case's graph: host work that would sit inside the window)
                env.reset_again()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                env.run_hooked(T, **kw)
                b.record(stream)
                env.sync()
                if timed:
                    out["us_per_slot"][name].append(a.elapsed_time(b) * 1e3 / T)
    host = []
    for i in range(hits + 5):
        env.reset_again()
        env.sync()
        t0 = time.perf_counter()
        env.run_hooked(1, **cases["all"])
        t1 = time.perf_counter()
        env.sync()
        if i >= 5:
            host.append((t1 - t0) * 1e6)
    out["hit_host_us"] = dict(median=statistics.median(host), min=min(host), max=max(host), n=len(host))
    out["us_per_slot_median"] = {k: statistics.median(v) for k, v in out["us_per_slot"].items()}
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(a[0] if len(a) > 0 else 1024, a[1] if len(a) > 1 else 5, a[2] if len(a) > 2 else 200)
