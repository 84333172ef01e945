"""configs[1]: the per-order block of every replica (vds_orders_device: k_orders_block) next to what a user does without it,
env.orders() over a few replicas - what DESIGN.md's figures of the per-order block come from.

    python profiles/orders_block_day.py [replicas = 1024] [timed repetitions = 20] [sampled replicas = 16] [slot = 74] [hooked = 0]

Times: HIP event pairs on the handle's stream around one orders_device call, median (min - max) of the repetitions after two
warm-ups: (a) the full refresh (0, INT32_MAX) at day end, (b) the refresh (t, t) of one stepped slot.  The host path: wall time of
env.orders(r0, n) over `sampled` replicas, SCALED to all replicas (and labelled so).  With hooked = 1 the script instead runs hooked
days with and without run_hooked(orders=True), for a kernel trace taken from outside (c); it prints the wall time of each.
Byte model: per (order of the range, replica) 8 B of `out` read and 8 B of the block written; per order and day 4 B of ord_q.  The
floor is the model at 8 TB/s."""
import json
import os
import sys
import time

import numpy as np

PEAK = 8.0e12


def model(orders, R, days=1):
    total = orders * R * 16 + orders * days * 4
    return dict(orders=int(orders), bytes=int(total), floor_us=total / PEAK * 1e6)


def main(R, reps, sampled, slot, hooked):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from vehicles_dispatch_simulator_amd import workloads

    w = workloads.didi_day()
    s = torch.cuda.Stream()
    env = w.make_env(R, stream=s.cuda_stream)
    init = w.vehicle_nodes(R)
    env.reset(init)
    out = dict(R=R, O=env.O, T=env.T, build=env._lib.vds_build_id().decode(), main_kernel=env.main_kernel())

    if hooked:
        env.orders_device_ptr()
        for on in (False, True, False, True):
            env.reset(init)
            env.sync()
            t0 = time.perf_counter()
            env.run_hooked(env.T, orders=on)
            env.sync()
            out.setdefault("hooked_day_ms_orders_%s" % ("on" if on else "off"), []).append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(out))
        env.close()
        return

    def timed(fn):
        ms = []
        for i in range(reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            env.sync()
            if i >= 2:
                ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    slot = min(slot, env.T - 2)
    env.run(slot)
    env.step()                                   # the hook's position of `slot`
    blk = env.orders_torch()
    env.sync()
    before = int((blk[0, :, 0] != -2).sum().item())
    env.advance()
    env.step()
    env.orders_device_ptr(slot + 1, slot + 1)
    env.sync()
    n_slot = int((blk[0, :, 0] != -2).sum().item()) - before          # orders processed in slot + 1
    ms = timed(lambda: env.orders_device_ptr(slot + 1, slot + 1))
    m = model(n_slot, R)
    out["one_slot"] = dict(slot=slot + 1, ms=ms, model=m, share_of_peak=m["bytes"] / (ms[0] * 1e-3) / PEAK)
    env.advance()
    env.run(env.T - env.clock[0])
    ms = timed(lambda: env.orders_device_ptr())
    m = model(env.O, R)
    out["full"] = dict(ms=ms, model=m, share_of_peak=m["bytes"] / (ms[0] * 1e-3) / PEAK)
    n = min(sampled, R)
    env.orders(0, 1)
    t0 = time.perf_counter()
    env.orders(0, n)
    dt = time.perf_counter() - t0
    out["host_path"] = dict(sampled=n, ms_sampled=dt * 1e3, ms_scaled_to_all_replicas=dt * 1e3 * R / n)
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(a[0] if a else 1024, a[1] if len(a) > 1 else 20, a[2] if len(a) > 2 else 16, a[3] if len(a) > 3 else 74, a[4] if len(a) > 4 else 0)
