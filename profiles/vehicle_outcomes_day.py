"""configs[1] around slot T / 2: the per-vehicle order outcomes of every replica (vds_vehicle_outcomes_device: k_vehicle_outcomes_fill +
k_vehicle_outcomes) next to what a user does without them, env.orders() joined on the vehicle id - what DESIGN.md's figures of the
vehicle outcomes come from.

    python profiles/vehicle_outcomes_day.py [replicas = 1024] [timed repetitions = 20] [sampled replicas = 16] [call | all = all]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/vehicle_outcomes_day.py 1024 20 16 call      # fill and scatter apart

Times: HIP event pairs on the handle's stream around one vehicle_outcomes_device call (the fill and the scatter), median (min - max) of
the repetitions after two warm-ups.  `all` adds: the per-slot difference of a run_hooked day with and without the switch (three days
each, alternating, medians), and the host path - wall time of env.orders() over `sampled` replicas, SCALED to all replicas (and
labelled so).
Byte model, from the slot's own outcome planes:
    fill      16 B per vehicle and replica
    scatter   per processed order of the slot and replica 8 B of result, one 64-byte line stored per match; per order 16 B so_rec +
              4 B so_pnode once (shared by the replicas of a day, L2)
The floor is the model at 8 TB/s."""
import json
import os
import sys
import time

import numpy as np

PEAK = 8.0e12


def byte_model(env):
    R, V = env.R, env.V
    oc = env.outcomes()
    served, rejected = int(oc["served"].sum()), int(oc["rejected"].sum())
    per_replica = (served + rejected) // R
    m = dict(slot=env.clock[0], processed_orders=served + rejected, matches=served, orders_per_replica=per_replica)
    m["fill"] = 16 * R * V
    m["scatter"] = 8 * (served + rejected) + 64 * served + 20 * per_replica
    m["total"] = m["fill"] + m["scatter"]
    m["floor_us"] = m["total"] / PEAK * 1e6
    return m


def main(R, reps, sampled, what):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from vehicles_dispatch_simulator_amd import workloads

    w = workloads.didi_day()
    s = torch.cuda.Stream()
    env = w.make_env(R, stream=s.cuda_stream)
    init = w.vehicle_nodes(R)
    env.reset(init)
    half = env.T // 2
    env.run(half)
    env.step()                                   # the hook's position of slot T / 2

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        env.sync()
        return a.elapsed_time(b)

    out = dict(R=R, V=env.V, T=env.T, slot=half, build=env._lib.vds_build_id().decode(), main_kernel=env.main_kernel())
    model = byte_model(env)
    ms = [events(env.vehicle_outcomes_device_ptr) for _ in range(reps + 2)][2:]
    med = float(np.median(ms))
    out["call"] = dict(ms=(med, float(min(ms)), float(max(ms))), model=model, bytes_per_s=model["total"] / (med * 1e-3),
                       share_of_peak=model["total"] / (med * 1e-3) / PEAK)
    blk = env.vehicle_outcomes_torch()
    env.sync()
    assert int((blk[..., 0] >= 0).sum().item()) == model["matches"]
    if what == "all":
        # the hooked day with and without the switch: whole days, alternating
        days = {False: [], True: []}
        for i in range(8):
            on = bool(i & 1)
            env.reset(init)
            env.sync()
            t = events(lambda: env.run_hooked(env.T, vehicle_outcomes=on, idle_pre=False, idle_now=False, supply=False, cl_orders=False))
            if i >= 2:
                days[on].append(t)
        off_ms, on_ms = float(np.median(days[False])), float(np.median(days[True]))
        out["hooked_day"] = dict(off_ms=days[False], on_ms=days[True], per_slot_off_us=off_ms / env.T * 1e3, per_slot_on_us=on_ms / env.T * 1e3,
                                 per_slot_difference_us=(on_ms - off_ms) / env.T * 1e3)
        # what a user does today: the per-order results of the replicas to the host (then a join on the vehicle id)
        n = min(sampled, R)
        env.orders(0, 1)
        t0 = time.perf_counter()
        env.orders(0, n)
        dt = time.perf_counter() - t0
        out["host_path"] = dict(sampled=n, ms_sampled=dt * 1e3, ms_scaled_to_all_replicas=dt * 1e3 * R / n)
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    what = a.pop() if a and not a[-1].isdigit() else "all"
    a = [int(x) for x in a]
    main(a[0] if a else 1024, a[1] if len(a) > 1 else 20, a[2] if len(a) > 2 else 16, what)
