"""configs[1] hooked day with the per-cluster outcome planes (vds_run_hooked with VDS_PLANE_OUTCOMES), what DESIGN.md's
k_slot_outcomes figure was timed on:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python profiles/r07/slot_outcomes_day.py 1024

(two days after a warm-up reset: 296 k_slot_outcomes launches of the day graph, plus one from the final read)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
from vehicles_dispatch_simulator_amd import workloads  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
w = workloads.didi_day()
env = w.make_env(R, stream=torch.cuda.current_stream().cuda_stream)
env.reset(w.vehicle_nodes(R))
for day in range(2):
    env.reset_again()
    env.run_hooked(env.T, outcomes=True)
    env.sync()
oc = env.outcomes()
print("T", env.T, "C", env.C, "served", int(oc["served"].sum()), "rejected", int(oc["rejected"].sum()))
env.close()
