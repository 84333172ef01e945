"""configs[1] at slot T / 2: the byte model of vds_snapshot / vds_restore and their time next to what a user does without them,
reset_again + run(T / 2) - what DESIGN.md's snapshot figures come from.

    python profiles/snapshot_day.py [replicas = 1024] [timed repetitions = 20] [sampled replicas = 16]

Byte model (read + written, one direction of the copy; a restore moves the same bytes and reads the replica map once per launch),
from the slot's own list lengths and counts:
    records   hdr and cnt, 64 B per bucket each; ring_cnt 4 B per (ring slot, bucket); the static arrival slots 4 B per (order slot, replica) on the dense layout - copied whole
              (modelled as one slot per order of the day: an upper bound)
    rows      every idle list / ring slot / far list up to its length, rounded up to 16-byte pieces, plus the count each row is
              bounded by (the bucket record for idle, fl and both inbox parities; the ring_cnt word for ring and ring_min)
    results   8 B per order processed so far and replica
The idle lengths are exact (the idle_now plane of every replica).  The arrival rows are not visible through the API: they are
modelled from the container views of `sampled` replicas - an entry lies in the ring row of its arrival slot, beyond the ring horizon
in the far list; on the dense layout the order-carrying vehicles sit in the static arrival slots (copied whole, above) and only
dispatched ones in ring rows - and scaled to all replicas.
Times: HIP event pairs on the handle's stream around snapshot, restore (identity), restore through a random permutation and
reset_again + run(T / 2), median of the repetitions after a warm-up."""
import json
import os
import sys

import numpy as np

PEAK = 8.0e12


def rows16(n, es):
    return (np.asarray(n, dtype=np.int64) * es + 15) // 16 * 16


def byte_model(env, sampled, ring_ticks=32):
    R, C, lay = env.R, env.C, env.layout()
    dense = lay["dense"] == 1
    t, now = env.clock
    ob = env.obs()
    es_idle, es_ring = (4, 8) if dense else (8, 16)
    m = dict(dense=dense, slot=t)
    m["records"] = 2 * (64 + 64) * C * R + 2 * 4 * ring_ticks * C * R
    done = int(env.counters()[0, 0])
    m["results"] = 2 * 8 * done * R
    # UPPER bound: one slot per order of the day; the library copies the orders that own a static slot (<= O, not visible through the API),
    # so `total` and every bytes/s derived from it are upper bounds too
    m["arrival_slots"] = 2 * 4 * env.O * R if dense else 0
    m["idle_rows"] = int(2 * rows16(np.minimum(ob["idle_now"], env.idle_cap), es_idle).sum())
    m["row_counts"] = 4 * 64 * C * R + 2 * 4 * ring_ticks * C * R
    ring = far = 0
    tick = 10                                    # (the workloads' slot length: BatchedDispatchEnv's default)
    for r in np.linspace(0, R - 1, min(sampled, R)).astype(int):
        L = env.lists(int(r))
        for c in range(C):
            a, b = L["arr_off"][c], L["arr_off"][c + 1]
            keep = L["arr_order"][a:b] < 0 if dense else np.ones(b - a, dtype=bool)
            ahead = np.maximum(-(-(L["arr_min"][a:b][keep] - now) // tick), 0)
            near = ahead[ahead < ring_ticks]
            if near.size:
                n = np.bincount(near)
                ring += int(rows16(n, es_ring).sum()) + (int(rows16(n, 4).sum()) if dense else 0)
            far += int(rows16((ahead >= ring_ticks).sum(), 16))
    k = R / min(sampled, R)
    m["ring_rows"], m["far_rows"] = int(2 * ring * k), int(2 * far * k)
    m["total"] = sum(v for key, v in m.items() if key not in ("dense", "slot"))
    m["floor_us"] = m["total"] / PEAK * 1e6
    return m


def main(R, reps, sampled):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from vehicles_dispatch_simulator_amd import workloads

    w = workloads.didi_day()
    s = torch.cuda.Stream()
    env = w.make_env(R, stream=s.cuda_stream)
    env.reset(w.vehicle_nodes(R))
    half = env.T // 2

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

    def replay():
        env.reset_again()
        env.run(half)

    out = dict(R=R, T=env.T, slot=half, build=env._lib.vds_build_id().decode(), main_kernel=env.main_kernel())
    out["replay_ms"] = timed(replay)
    env.step()                                   # the hook's position of slot T / 2
    out["model"] = byte_model(env, sampled)
    env.snapshot()
    env.sync()
    out["store_bytes"] = env.snapshot_info()["bytes"]
    out["snapshot_ms"] = timed(env.snapshot)
    out["restore_ms"] = timed(env.restore)
    perm = np.random.default_rng(1).permutation(R).astype(np.int32)
    out["restore_permuted_ms"] = timed(lambda: env.restore(perm))
    dperm = torch.from_numpy(perm).cuda()
    out["restore_device_map_ms"] = timed(lambda: env.restore_torch(dperm))
    for k in ("snapshot_ms", "restore_ms", "restore_permuted_ms"):
        out[k.replace("_ms", "_bytes_per_s")] = out["model"]["total"] / (out[k][0] * 1e-3)
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(a[0] if a else 1024, a[1] if len(a) > 1 else 20, a[2] if len(a) > 2 else 16)
