"""Branching rollouts from one state: a day runs to a slot, the state is saved there (snapshot), and every replica continues from
replica 0's state (restore through a replica map) with a dispatch decision of its own - branch b moves b idle vehicles from the
cluster with the largest surplus to the one with the largest expected shortage.  The rest of the day runs for all branches at
once and the rejects of each branch are printed.  A second restore rolls all replicas back to their own state at that slot.

    python examples/branch_rollouts.py [branches] [slot]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vehicles_dispatch_simulator_amd import workloads

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
w = workloads.tiny(N=600, C=24, vehicles=400, orders=12000)
env = w.make_env(B)
env.reset_random(np.arange(B, dtype=np.uint64) + np.uint64(w.veh_seed))
slot = int(sys.argv[2]) if len(sys.argv) > 2 else env.T // 3
some_node_of = [int(np.flatnonzero(w.city.node2cluster == c)[0]) for c in range(w.city.C)]

env.run(slot)
env.step()                                  # Update -> Match -> SupplyExpect of the slot: the hook's position, where a policy branches
env.snapshot()
print("snapshot at slot %(step)d (stepped: %(stepped)s), %(bytes)d bytes of device memory" % env.snapshot_info())

env.restore(np.zeros(B, dtype=np.int32))    # every replica continues from replica 0's state
ob = env.obs()
surplus = ob["idle_now"][0] + ob["supply"][0] - ob["cl_orders"][0]
src, dst = int(surplus.argmax()), int(surplus.argmin())
moved = [min(b, int(ob["idle_now"][0][src])) for b in range(B)]
rep = [b for b in range(B) for _ in range(moved[b])]
pos = [p for b in range(B) for p in range(moved[b])]
if rep:
    env.apply_dispatch(rep, [src] * len(rep), pos, [some_node_of[dst]] * len(rep))
env.advance()
env.run(env.T - slot - 1)
cn = env.counters()
print("from slot %d of %d, cluster %d -> cluster %d:" % (slot, env.T, src, dst))
for b in range(B):
    print("  branch %d: %2d vehicles moved, dispatch cost %4d, rejects %d of %d orders" % (b, moved[b], cn[b, 5], cn[b, 1], cn[b, 0]))

env.restore()                               # the plain rollback: every replica back on its own state at the slot
env.advance()
env.run(env.T - slot - 1)
print("rolled back, no dispatch: rejects per replica", env.counters()[:, 1].tolist())
env.close()
