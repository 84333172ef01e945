"""k_tick_dense per slot of the last day, parent build against the per-(slot, cluster) forms, from two rocprofv3 kernel traces:
  (from the repository root; <out>: a directory for the small files the two modes share; VDS_LIB=<parent build> for the parent arm)
  rocprofv3 --kernel-trace --stats --output-format csv -d <trace_<arm>> -- python profiles/r07_cluster_forms/per_slot.py run <wl> <arm> <out>
  python profiles/r07_cluster_forms/per_slot.py read <trace_parent> <trace_new> <wl> <out>
The run: six adaptive days (the choice is made at the start of the third); the last one is the day the table shows."""
import sys
sys.path.insert(0, ".")
if sys.argv[1] == "run":
    import numpy as np, torch
    from vehicles_dispatch_simulator_amd import workloads
    wl, arm, out = sys.argv[2], sys.argv[3], sys.argv[4]
    w = workloads.didi_day("cfg2") if wl == "cfg2" else (workloads.didi_day("cfg4", neighbor=True, service_m=2000.0) if wl == "cfg4" else workloads.stress())
    R = 128 if wl == "cfg5" else 1024
    env = w.make_env(R, stream=torch.cuda.current_stream().cuda_stream)
    env.reset(w.vehicle_nodes(R))
    for _ in range(6):
        env.reset_again(); env.run(env.T); env.sync()
    try:
        plane = env.cluster_forms()
    except AttributeError:          # (the parent build: per-slot forms only)
        plane = np.repeat(env.tick_forms()[:, None], env.C, axis=1)
    np.save("%s/plane_%s_%s.npy" % (out, arm, wl), plane)
else:
    import csv, glob
    import numpy as np
    def last_day(d, T):
        f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
        rows = [r for r in csv.DictReader(open(f)) if "k_tick_dense" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        rows = rows[-T:]
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000 for r in rows], [r["Kernel_Name"] for r in rows]
    da, db, wl, out = sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5]
    pa = np.load("%s/plane_parent_%s.npy" % (out, wl)); pb = np.load("%s/plane_new_%s.npy" % (out, wl))
    T, C = pb.shape
    (a, ka), (b, kb) = last_day(da, T), last_day(db, T)
    print("%s: last day, k_tick_dense %.2f ms (parent) -> %.2f ms (forms per (slot, cluster)); %d slots x %d clusters" % (wl, sum(a) / 1e3, sum(b) / 1e3, T, C))
    print("parent: %d slots in the 16-lane form; this build: %d (slot, cluster) pairs in the 16-lane form, %d slots with both forms (k_tick_dense_mixed)"
          % (int(pa[:, 0].sum()), int(pb.sum()), sum("mixed" in k for k in kb)))
    print("per slot: us parent (form: 8 / 16 lanes) / us this build (16-lane clusters of the slot; M: one launch with both forms)")
    for t0 in range(0, T, 6):
        cells = []
        for t in range(t0, min(t0 + 6, T)):
            fa = "16" if pa[t, 0] else " 8"
            fb = ("M" if "mixed" in kb[t] else " ") + "%3d" % int(pb[t].sum())
            cells.append("%4.0f/%s %4.0f/%s" % (a[t], fa, b[t], fb))
        print("%3d  " % t0 + "  ".join(cells))
