"""Cost of the episode reset with fleets per replica (vds_set_fleet) and of the reset from a device tensor (vds_reset_device) at
configs[1]: what DESIGN.md's section "Fleet size per replica" was timed on.

    python profiles/fleet_reset.py [replicas=1024] [out.json]

One process, one handle, HIP event pairs on the handle's stream, median (min - max) of 20 after 2 warm-ups:
    again_none    vds_reset_again with no map (k_reset_staged with fleet == null: today's reset)
    again_vm1     ... with every fleet at V - 1
    again_spread  ... with fleets spread evenly from 0 to V
    reset_host    vds_reset of the caller's host array (upload + checks + copy + reset kernel; synchronous: wall time between the events)
    reset_torch   vds_reset_device with the same nodes resident on the device (one device-to-device copy in place of the upload)
Byte model of the reset kernel per replica: 4 * fleet read (the start nodes) and one list entry (4 B dense layout, 8 B wide) written
per vehicle, next to the 128 B of headers and counters per (replica, cluster) that do not depend on the fleet."""
import json
import os
import sys


def main(R, out_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from vehicles_dispatch_simulator_amd import workloads

    w = workloads.didi_day()
    stream = torch.cuda.current_stream()
    env = w.make_env(R, stream=stream.cuda_stream)
    nodes = w.vehicle_nodes(R)
    V, C = env.V, env.C
    nodes_dev = torch.from_numpy(nodes).cuda()

    def timed(fn, n=20, warm=2):
        ms = []
        for i in range(warm + n):
            env.sync()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            env.sync()
            torch.cuda.synchronize()
            if i >= warm:
                ms.append(a.elapsed_time(b))
        ms.sort()
        return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])

    res = {}
    maps = dict(again_none=None, again_vm1=np.full(R, V - 1, dtype=np.int32), again_spread=np.linspace(0, V, R).round().astype(np.int32))
    for name, fleet in maps.items():
        env.set_fleet(fleet)
        env.reset(nodes)
        res[name] = timed(env.reset_again)
        vehicles = int(env.fleet.astype(np.int64).sum())
        entry = 4 if env.layout()["dense"] else 8
        res[name]["vehicles"] = vehicles
        res[name]["model_bytes"] = (4 + entry) * vehicles + 128 * R * C
    env.set_fleet(None)
    res["reset_host"] = timed(lambda: env.reset(nodes))
    res["reset_torch"] = timed(lambda: env.reset_torch(nodes_dev))
    out = dict(R=R, C=C, V=V, dense=env.layout()["dense"], build_id=env._lib.vds_build_id().decode(), cases=res)
    print(json.dumps(out))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    env.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1024, sys.argv[2] if len(sys.argv) > 2 else None)
