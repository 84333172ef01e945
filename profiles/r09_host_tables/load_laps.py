"""Ten VDS_LOAD_TIMING=1 reloads of each kind on the library VDS_LIB names: laps go to stderr."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ["VDS_LOAD_TIMING"] = "1"
import numpy as np
import torch
from vehicles_dispatch_simulator_amd import workloads
R = 1024
def say(s):
    sys.stderr.write("## %s\n" % s); sys.stderr.flush()
w = workloads.didi_day("cfg2")
env = w.make_env(R, load=False)
say("warm"); env.load_orders(w.release_min, w.pickup, w.delivery)
env.reset(w.vehicle_nodes(R)); env.run(env.T); env.sync()
for i in range(10):
    say("one"); env.load_orders(w.release_min, w.pickup, w.delivery)
days16 = workloads.distinct_days(w, 16)
m = (np.arange(R) % 16).astype(np.int32)
env3 = w.make_env(R, load=False)
say("warm"); env3.load_order_days(days16, m)
env3.reset(w.vehicle_nodes(R))
for i in range(10):
    say("sixteen"); env3.load_order_days(days16, m)
env3.close(); env.close()
say("done")
