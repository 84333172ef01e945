"""End-of-day statistics PER ORDER, computed on the GPU from the per-order block (``orders_torch``, ``run_hooked(orders=True)``): a hooked
day refreshes, every slot, the rows of the orders the slot processed - ``{vehicle, wait}`` in ``Order.ID`` order, what the reference's
end-of-day report reads off ``Order.ArriveInfo`` / ``Order.PickupWaitTime`` (``simulator.py:1095-1121``) - and at the end the example
prints, next to the counters, per-replica wait-time quantiles and the rejected share per pickup cluster.  Nothing is copied to the host
but the printed figures.

    python examples/order_level_stats.py [replicas]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from vehicles_dispatch_simulator_amd import workloads
from vehicles_dispatch_simulator_amd._lib import COUNTER_NAMES
from vehicles_dispatch_simulator_amd.env import ORDER_PENDING, ORDER_REJECTED

if __name__ == "__main__":
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    w = workloads.tiny()
    env = w.make_env(R, stream=torch.cuda.current_stream().cuda_stream)
    env.reset(w.vehicle_nodes(R))
    blk = env.orders_torch()                                 # [R, O, 2], every row pending: what the day's refreshes accumulate into
    env.run_hooked(env.T, orders=True)                       # every slot t: the rows of the orders processed in t
    env.sync()
    cn = env.counters()
    veh, wait = blk[..., 0], blk[..., 1].to(torch.float32)
    served, rejected = veh >= 0, veh == ORDER_REJECTED
    # per-replica wait-time quantiles over the served orders
    q = torch.tensor([0.5, 0.9, 0.99], device="cuda")
    quant = torch.stack([torch.quantile(wait[r][served[r]], q) if bool(served[r].any()) else torch.zeros(3, device="cuda") for r in range(R)])
    # rejected share per pickup cluster, over all replicas
    cl = torch.from_numpy(np.asarray(w.city.node2cluster)[np.asarray(w.pickup)].astype(np.int64)).cuda()[None, :].expand(R, -1)
    done = served | rejected
    per_cl = torch.zeros(env.C, dtype=torch.int64, device="cuda").scatter_add_(0, cl[done], torch.ones_like(cl[done]))
    rej_cl = torch.zeros(env.C, dtype=torch.int64, device="cuda").scatter_add_(0, cl[rejected], torch.ones_like(cl[rejected]))
    ok = bool((served.sum(dim=1).cpu().numpy() == cn[:, 0] - cn[:, 1]).all()) and bool((rejected.sum(dim=1).cpu().numpy() == cn[:, 1]).all()) and \
        bool(((blk[..., 1].to(torch.int64) * served).sum(dim=1).cpu().numpy() == cn[:, 3]).all()) and int((veh == ORDER_PENDING).sum(dim=1).min().item()) >= 1
    tot = cn.sum(axis=0)
    print("counters      : " + ", ".join("%s %d" % (k, tot[i]) for i, k in enumerate(COUNTER_NAMES) if k != "evals"))
    print("wait quantiles: p50 / p90 / p99 of replica 0: %s; over the replicas p50 spans %.0f .. %.0f" %
          (" / ".join("%.0f" % x for x in quant[0].tolist()), float(quant[:, 0].min()), float(quant[:, 0].max())))
    share = (rej_cl.to(torch.float64) / per_cl.clamp(min=1).to(torch.float64)).cpu().numpy()
    print("rejected share per pickup cluster: " + " ".join("%d:%.2f" % (c, share[c]) for c in range(env.C)))
    print("%d cities x %d slots: the block's served, rejected and wait sums %s the counters" % (R, env.T, "EQUAL" if ok else "DIFFER FROM"))
    env.close()
    sys.exit(0 if ok else 1)
