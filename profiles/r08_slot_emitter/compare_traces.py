"""Compares the kernel sequences of two `rocprofv3 --kernel-trace --output-format csv` runs of trace_driver.py: the tuples
(Kernel_Name, Grid_Size, Workgroup_Size, LDS_Block_Size) in start order must be equal line for line.

    python profiles/r08_slot_emitter/compare_traces.py DIR_A DIR_B        # each holds <case>/..._kernel_trace.csv

Prints one line per case (launches, equal or the first differing line) and exits 1 on any difference or a case without a trace.
"""
import csv
import glob
import os
import sys


def sequence(case_dir):
    files = glob.glob(os.path.join(case_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        return None
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    xyz = lambda r, k: "%s x %s x %s" % (r[k + "_X"], r[k + "_Y"], r[k + "_Z"])
    return [(r["Kernel_Name"], xyz(r, "Grid_Size"), xyz(r, "Workgroup_Size"), r["LDS_Block_Size"]) for r in rows]


def main():
    a, b = sys.argv[1], sys.argv[2]
    bad = 0
    for case in sorted(os.listdir(a)):
        sa, sb = sequence(os.path.join(a, case)), sequence(os.path.join(b, case))
        if sa is None or sb is None:
            print("%-24s NO TRACE (%s)" % (case, "first" if sa is None else "second"))
            bad += 1
            continue
        diff = next((i for i, (x, y) in enumerate(zip(sa, sb)) if x != y), None)
        if diff is None and len(sa) != len(sb):
            diff = min(len(sa), len(sb))
        if diff is None:
            print("%-24s %6d launches, %3d distinct kernels: equal" % (case, len(sa), len({x[0] for x in sa})))
        else:
            bad += 1
            print("%-24s DIFFERS at launch %d of %d / %d:\n    %s\n    %s" % (case, diff, len(sa), len(sb), sa[diff] if diff < len(sa) else None, sb[diff] if diff < len(sb) else None))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
