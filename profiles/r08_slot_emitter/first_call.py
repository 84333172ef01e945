"""Host time of the FIRST run(T) and the first run_hooked(T) after load_orders (graph build + instantiate; the call returns when the
graph is launched, not when it has run), configs[1] at 1024 replicas, for the build VDS_LIB names.  For information: no threshold.

    VDS_LIB=<libvds.so> python profiles/r08_slot_emitter/first_call.py
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402,F401
from vehicles_dispatch_simulator_amd import _lib, workloads  # noqa: E402

R = 1024
w = workloads.didi_day("cfg2")
nodes = w.vehicle_nodes(R)
out = {"build": _lib.load().vds_build_id().decode(), "replicas": R}
for groups in (1, 2):
    env = w.make_env(R)
    env.set_run_groups(groups, -1)
    env.reset(nodes)
    env.sync()
    T = env.T
    t0 = time.perf_counter()
    env.run(T)
    t1 = time.perf_counter()
    env.sync()
    env.reset_again()
    env.sync()
    t2 = time.perf_counter()
    env.run(T)
    t3 = time.perf_counter()
    env.sync()
    env.reset_again()
    env.sync()
    t4 = time.perf_counter()
    env.run_hooked(T, inflight=False)
    t5 = time.perf_counter()
    env.sync()
    out["groups_%d" % groups] = {"first_run_ms": (t1 - t0) * 1e3, "replayed_run_call_ms": (t3 - t2) * 1e3, "first_run_hooked_ms": (t5 - t4) * 1e3}
    env.close()
print(json.dumps(out))
