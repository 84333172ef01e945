"""Launch-sequence driver of round 8: ONE process issues a fixed list of days on workloads.tiny; run under
`rocprofv3 --kernel-trace` once with the parent build (VDS_LIB) and once with the new one, the two kernel sequences must be
equal line for line (compare_traces.py).

    python profiles/r08_slot_emitter/trace_driver.py MODE NEIGHBOR R

MODE  default   a step / advance day; run(T) at 1, 2 and 3 replica groups; run_hooked with planes 63, a captured policy and K = 2 at
                1 and 2 groups; run_hooked with planes 0, no policy, no actions
      nograph   run(T) with VDS_RUN_GRAPH=0
      alt       run(T) at 1 and 2 groups with VDS_DENSE_TICK_FORMS=alt (wide slots)
      seed      run(T) at 1 and 2 groups with VDS_DENSE_CLUSTER_SEED=1 (mixed slots: needs R >= 64)
      forms     the forms only a stream runs and the wide layout: force_generic 1 (generic k_tick + k_tick_work / the serial pair),
                3 (k_tick_replica2, neighbour search only), 5 resp. VDS_DENSE_DFS=0 (k_tick_rows, plain and in stamp mode) - a
                step / advance day and run(T) at 1 and 2 groups each
Prints what ran (group counts as the library reports them, cells of the form plane in the wide form) so that a trace that
covers less than it claims shows.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
mode, neighbor, R = sys.argv[1], sys.argv[2] == "1", int(sys.argv[3])
if mode == "nograph":
    os.environ["VDS_RUN_GRAPH"] = "0"
if mode == "alt":
    os.environ["VDS_DENSE_TICK_FORMS"] = "alt"
if mode == "seed":
    os.environ["VDS_DENSE_CLUSTER_SEED"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402
from vehicles_dispatch_simulator_amd import workloads  # noqa: E402

w = workloads.tiny(neighbor=neighbor, vehicles=60 if neighbor else 150)
init = w.vehicle_nodes(R)
stream = torch.cuda.current_stream()


def make(**kw):
    env = w.make_env(R, stream=stream.cuda_stream, **kw)
    env.reset(init)
    return env


def step_day(env):
    env.reset_again()
    for _ in range(env.T):
        env.step()
        env.advance()
    env.sync()


def run_day(env, groups):
    env.set_run_groups(groups, -1)
    env.reset_again()
    env.run(env.T)
    env.sync()
    print("run groups asked %d got %d kernel %s wide cells %d" % (groups, env._lib.vds_get_run_groups(env._h), env.main_kernel(), int(env.cluster_forms().sum())), flush=True)


if mode == "default":
    env = make()
    step_day(env)
    for G in (1, 2, 3):
        run_day(env, G)
    K = 2
    n2c = np.asarray(w.city.node2cluster)
    C = int(n2c.max()) + 1
    node_of = torch.tensor([int(np.flatnonzero(n2c == c)[0]) if (n2c == c).any() else 0 for c in range(C)], dtype=torch.int32, device="cuda")

    def policy(ob):     # one idle vehicle from each of the K fullest clusters to the K emptiest
        idle = ob[1]
        src = torch.topk(idle, K, dim=1).indices
        dst = torch.topk(idle + ob[2], K, dim=1, largest=False).indices
        ok = idle.gather(1, src) > 1
        return torch.stack([torch.where(ok, src.int(), torch.full_like(src, -1).int()), torch.zeros_like(src).int(), node_of[dst]], dim=2).contiguous()

    obs = env.obs_torch(inflight=False)
    actions = torch.zeros((R, K, 3), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        for _ in range(2):
            actions.copy_(policy(obs))
    stream.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        actions.copy_(policy(obs))
    for G in (1, 2):
        env.set_run_groups(G, -1)
        env.reset_again()
        env.run_hooked(env.T, actions=actions, policy_graph=graph, inflight=True, outcomes=True)
        env.sync()
        print("hooked planes 63 policy K=%d groups %d" % (K, G), flush=True)
    env.set_run_groups(1, -1)
    env.reset_again()
    env.run_hooked(env.T, idle_pre=False, idle_now=False, supply=False, cl_orders=False, inflight=False, outcomes=False)
    env.sync()
    print("hooked planes 0 no policy", flush=True)
    env.close()
elif mode in ("nograph", "alt", "seed"):
    env = make()
    for G in ((1,) if mode == "nograph" else (1, 2)):
        run_day(env, G)
        run_day(env, G)       # (the form plane of alt / seed is in force from the first episode on; a second day replays)
    env.close()
elif mode == "forms":
    for fg in ((1, 3, 5) if neighbor else (1, 5)):
        if neighbor and fg == 5:
            os.environ["VDS_DENSE_DFS"] = "0"
            env = make()
        else:
            env = make(force_generic=fg)
        print("force_generic %d" % fg, flush=True)
        step_day(env)
        for G in (1, 2):
            run_day(env, G)
        env.close()
else:
    raise SystemExit("unknown mode " + mode)
print("driver done", flush=True)
