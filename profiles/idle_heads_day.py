"""configs[1] hooked day with the idle-list heads (vds_run_hooked after vds_run_hooked_idle_heads(L)), what DESIGN.md's k_idle_heads
figures were timed on.  Two modes:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python profiles/idle_heads_day.py run 1024 16
    python profiles/idle_heads_day.py report <dir> <model.json written by the run>

run: two days after a warm-up reset, each a run_hooked day with outcomes=True (k_slot_outcomes in the same trace) and idle_heads=L, whose
captured policy adds up, on the device, the byte model of every k_idle_heads launch from the slot's own list lengths:
    written  2 * R * C * L * 4 B
    read     sum over buckets of 64 B (the bucket record) + ceil(4 * min(len, L) / 64) * 64 B (the list's lines, dense layout)
and prints it as one JSON line (VDS_IDLE_HEADS_MODEL=<file>: also written there).
report: mean / min / max per launch of k_idle_heads next to k_pack_obs, k_slot_outcomes and k_tick_dense of the same trace, the achieved
bytes/s of k_idle_heads under the model and its share of the 8 TB/s peak."""
import csv
import glob
import json
import os
import sys

PEAK = 8.0e12


def run(R, L):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from vehicles_dispatch_simulator_amd import workloads

    w = workloads.didi_day()
    stream = torch.cuda.current_stream()
    env = w.make_env(R, stream=stream.cuda_stream)
    env.reset(w.vehicle_nodes(R))
    ob = env.obs_torch(inflight=False)
    heads = env.idle_heads_torch(L)
    read_bytes = torch.zeros((), dtype=torch.int64, device="cuda")
    filled = torch.zeros((), dtype=torch.int64, device="cuda")
    launches = torch.zeros((), dtype=torch.int64, device="cuda")

    def policy():
        n = ob[1].clamp(max=L).to(torch.int64)                 # min(len(IdleVehicles), L) per bucket
        read_bytes.add_((64 + (4 * n + 63) // 64 * 64).sum())
        filled.add_((heads[0] >= 0).sum())
        launches.add_(1)

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
    read_bytes.zero_(); filled.zero_(); launches.zero_()
    for day in range(2):
        env.reset_again()
        env.run_hooked(env.T, policy_graph=graph, inflight=False, outcomes=True, idle_heads=L)
        env.sync()
    torch.cuda.synchronize()
    n = int(launches.item())
    model = dict(R=R, C=env.C, L=L, T=env.T, launches=n, layout=env.layout()["dense"], written_per_launch=2 * R * env.C * L * 4,
                 read_per_launch=int(read_bytes.item()) / n, filled_share=int(filled.item()) / (n * R * env.C * L))
    model["floor_us"] = (model["written_per_launch"] + model["read_per_launch"]) / PEAK * 1e6
    print(json.dumps(model))
    if os.environ.get("VDS_IDLE_HEADS_MODEL"):
        with open(os.environ["VDS_IDLE_HEADS_MODEL"], "w") as f:
            json.dump(model, f)
    env.close()


def report(d, model_path):
    model = json.load(open(model_path))
    rows = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(p)):
            for k in ("k_idle_heads", "k_pack_obs", "k_slot_outcomes", "k_tick_dense"):
                if k in row["Name"]:
                    c, tot = int(row["Calls"]), float(row["TotalDurationNs"])
                    o = rows.setdefault(k, dict(calls=0, total=0.0, min=1e30, max=0.0))
                    o["calls"] += c; o["total"] += tot; o["min"] = min(o["min"], float(row["MinNs"])); o["max"] = max(o["max"], float(row["MaxNs"]))
    out = dict(model=model)
    for k, o in sorted(rows.items()):
        out[k] = dict(calls=o["calls"], mean_us=o["total"] / o["calls"] / 1e3, min_us=o["min"] / 1e3, max_us=o["max"] / 1e3)
    if "k_idle_heads" in out:
        b = model["written_per_launch"] + model["read_per_launch"]
        bps = b / (out["k_idle_heads"]["mean_us"] * 1e-6)
        out["k_idle_heads"].update(bytes_per_launch=b, bytes_per_s=bps, share_of_peak=bps / PEAK)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]), int(sys.argv[3]))
    else:
        report(sys.argv[2], sys.argv[3])
