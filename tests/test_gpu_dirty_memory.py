"""The parity suites on device tables that start out DIRTY (``make dirty``, ``-DVDS_DIRTY``, ``VDS_LIB=libvds_dirty.so``).

A fresh process gets device memory that reads as zeros, so no other GPU test can see a kernel or a read path whose result depends on
what a table held before anything wrote it - and the engine leaves a lot unwritten on purpose (``vds_reset`` clears a part of the
state, entries are filtered rather than cleared, padding replicas never run, a reload fills recycled blocks in place).  The dirty
build fills every byte the library obtains for a handle - device tables fresh and recycled, pinned and host staging blocks - with one
byte before first use (``VDS_DIRTY_FILL``, hex, default ``A5``: ``0xA5A5A5A5`` is a negative count, ``0x5A5A5A5A`` a positive one).

* the probe: the fill is live (``vds_debug_dirty_probe``), and absent from the product library;
* the parity legs: existing test files, unchanged, in one pytest subprocess each under the dirty library - what they compare bit for
  bit with the CPU oracle must not move.  Legs run in the order of LEGS.  A leg that ends by a signal, an abort or at its time limit
  sets a flag, and every later test of this module that would start something on the GPU is skipped: nothing follows a fault;
* the transcripts: 12 API scripts (tests/api_script.py, ``record=``) under the product library and under the dirty one with both
  fill bytes - a digest of every array every read entry point returns, after every call.  The three must be identical: the oracle
  has no opinion on much of what is read (planes of a slot not stepped, rows of a replica whose day is over, the tail of a short day),
  a caller sees all of it;
* the host arrays of ``vds_read_lists`` / ``vds_read_vehicles`` / ``vds_read_orders`` handed over poisoned: every element comes back
  defined (include/vds.h says with what).

Seconds per leg under the PRODUCT library on an MI355X (one run each, pytest start-up included), from which the limits follow as
ten times that + 120 s for the build check and start-up - a safety stop, not a measurement:

    a 110   b 53   c 18   d 6   e 15   f 6   g 7   h 9   i 21

The libraries are built on demand into ``build/`` exactly as tests/test_gpu_debug_builds.py does (content hashes, not file times)."""
import json
import os
import signal
import subprocess
import sys

import pytest

from test_gpu_debug_builds import ROOT, build

pytestmark = pytest.mark.gpu
TESTS = os.path.join(ROOT, "tests")

# leg -> (seconds measured under the product library, test files, -k selection or None)
LEGS = {
    "a": (110, ["test_gpu_fuzz_golden.py"], None),
    "b": (53, ["test_gpu_plane_fuzz.py"], None),
    "c": (18, ["test_gpu_api_sequences.py"], None),
    "d": (6, ["test_gpu_snapshot.py"], "rows_at_capacity"),
    "e": (15, ["test_gpu_thresholds.py"], None),
    "f": (6, ["test_gpu_edge_cases.py"], "reset_again_of_a_city or reset_random or reset_checks"),
    # (g: one -k for two files, so each half names its file; in the idle-heads file the tests of order days per replica - regrouped
    # storage, a stream per row - are the three called interleaved_days_* / every_row_its_own_order_stream: "layout" and "replica_days"
    # alone match no test name there)
    "g": (7, ["test_gpu_replica_days.py", "test_gpu_idle_heads.py"],
          "(test_gpu_replica_days and (changes_every_episode or blocks_of_sixteen)) or "
          "(test_gpu_idle_heads and (layout or replica_days or interleaved_days or own_order_stream))"),
    "h": (9, ["test_gpu_device_memory.py"], None),
    # (i: the per-vehicle planes - "every element of a requested plane is written, whatever the tables hold", include/vds.h - and the
    # per-vehicle dispatch: the day walks and the odd sizes of the planes file, the day walks and the chunk boundaries of the dispatch
    # file, the walks of the fuzz file; one -k for three files, each part names its file - test_leg_i_selects_tests_in_each_of_its_files)
    "i": (21, ["test_gpu_vehicle_planes.py", "test_gpu_dispatch_vehicles.py", "test_gpu_vehicle_fuzz.py"],
          "(test_gpu_vehicle_planes and (planes_equal_host_view_and_oracle or odd_vehicle_and_replica_counts)) or "
          "(test_gpu_dispatch_vehicles and (test_day_walk or test_stamp_form_walk or test_chunk_boundaries)) or "
          "(test_gpu_vehicle_fuzz and walk_planes_and_three_dispatch_forms)"),
}
# (leg, fill byte): every leg with the default byte, then the two that reach the most tables with the positive pattern
RUNS = [(k, None) for k in LEGS] + [("a", "5A"), ("c", "5A")]
FAULT_WORDS = ("illegal memory access", "Memory access fault", "core dumped", "Segmentation fault", "HSA_STATUS_ERROR", "Fatal Python error")
_STOPPED = []           # why nothing more is started on the GPU (a leg that faulted, aborted or hung)


def leg_limit(leg):
    return 10 * LEGS[leg][0] + 120


def gpu_allowed():
    if _STOPPED:
        pytest.skip("not started: " + _STOPPED[0])


def run_limited(argv, env, limit, what):
    """One child process (and whatever it starts) under a time limit; (returncode, output).  A child that ends by a signal, by an
    abort or at the limit - or whose output names a GPU fault - stops every later GPU test of this module."""
    p = subprocess.Popen(argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, _ = p.communicate()
        _STOPPED.append("%s was still running at its limit of %d s" % (what, limit))
        pytest.fail("%s: %s\n%s" % (what, _STOPPED[-1], out[-3000:]))
    if p.returncode < 0 or p.returncode in (134, 139) or any(w in out for w in FAULT_WORDS):
        _STOPPED.append("%s ended with status %d (a signal, an abort or a GPU fault)" % (what, p.returncode))
        pytest.fail("%s\n%s" % (_STOPPED[-1], out[-6000:]))
    return p.returncode, out


def dirty_env(fill=None, lib=None):
    env = dict(os.environ)
    env.pop("VDS_DIRTY_FILL", None)
    env.pop("VDS_LIB", None)
    if lib is not None:
        env["VDS_LIB"] = lib
    if fill is not None:
        env["VDS_DIRTY_FILL"] = fill
    return env


PROBE = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from vehicles_dispatch_simulator_amd import workloads, _lib
w = workloads.tiny()
env = w.make_env(3)
out = np.zeros(4, dtype=np.int32)
rc = env._lib.vds_debug_dirty_probe(env._h, out.ctypes.data_as(ctypes.c_void_p))
print("PROBE", _lib.load().vds_build_id().decode(), rc, " ".join("%%08X" %% (int(x) & 0xFFFFFFFF) for x in out))
env.close()
""" % ROOT


def probe(lib, fill):
    rc, out = run_limited([sys.executable, "-c", PROBE], dirty_env(fill, lib), 300, "the probe (%s, fill %s)" % (lib and os.path.basename(lib), fill))
    assert rc == 0, out[-3000:]
    line = [l for l in out.splitlines() if l.startswith("PROBE ")][-1].split()
    return line[1], int(line[2]), line[3:]


def test_the_fill_is_live_in_the_dirty_build_only():
    gpu_allowed()
    lib = build("dirty", "libvds_dirty.so")
    bid, rc, words = probe(lib, None)
    assert bid.endswith("+dirty") and rc == 0 and words == ["A5A5A5A5"] * 4, (bid, rc, words)
    bid, rc, words = probe(lib, "5A")
    assert bid.endswith("+dirty") and rc == 0 and words == ["5A5A5A5A"] * 4, (bid, rc, words)
    bid, rc, words = probe(None, "5A")
    assert bid.count("+") == 1 and rc == -4 and words == ["00000000"] * 4, (bid, rc, words)      # VDS_ESTATE, out untouched


def test_leg_i_selects_tests_in_each_of_its_files():
    """The -k expression of leg i names tests in every one of its three files (collection only: nothing is started on the GPU)."""
    _, files, select = LEGS["i"]
    p = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-m", "gpu", "-k", select] + [os.path.join(TESTS, f) for f in files],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    ids = [l for l in p.stdout.splitlines() if "::" in l]
    per_file = {f: [i for i in ids if f + "::" in i] for f in files}
    assert len(per_file["test_gpu_vehicle_planes.py"]) == 17 + 5, per_file["test_gpu_vehicle_planes.py"]              # the day walks, the odd sizes
    assert len(per_file["test_gpu_dispatch_vehicles.py"]) == 16 + 2 + 14, per_file["test_gpu_dispatch_vehicles.py"]    # day walks, stamp form, chunk cases
    assert len(per_file["test_gpu_vehicle_fuzz.py"]) >= 10 and all("test_walk_planes" in i for i in per_file["test_gpu_vehicle_fuzz.py"]), per_file["test_gpu_vehicle_fuzz.py"]


@pytest.mark.parametrize("leg,fill", RUNS, ids=[k if f is None else "%s-%s" % (k, f) for k, f in RUNS])
def test_parity_on_dirty_tables(leg, fill):
    gpu_allowed()
    lib = build("dirty", "libvds_dirty.so")
    _, files, select = LEGS[leg]
    argv = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu"] + [os.path.join(TESTS, f) for f in files] + (["-k", select] if select else [])
    rc, out = run_limited(argv, dirty_env(fill, lib), leg_limit(leg), "leg %s (fill %s)" % (leg, fill or "A5"))
    print(out[-1500:])
    assert rc == 0 and " passed" in out, out[-6000:]


TRANSCRIPT = r"""
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import api_script
from vehicles_dispatch_simulator_amd import BatchedDispatchEnv, _lib
out = dict(build=_lib.load().vds_build_id().decode(), scripts={})
for seed in api_script.corpus()[0][:12]:
    lines = []
    s = api_script.run_script(BatchedDispatchEnv, seed, record=lines)
    out["scripts"][str(seed)] = dict(lines=lines, log=s.log)
json.dump(out, open(sys.argv[1], "w"))
print("TRANSCRIPTS DONE")
""" % (ROOT, TESTS)


def test_reads_do_not_depend_on_what_the_tables_held(tmp_path):
    """Every byte a read entry point returns is a function of the inputs and the call sequence."""
    gpu_allowed()
    lib = build("dirty", "libvds_dirty.so")
    got = {}
    for name, use, fill in (("product", None, None), ("dirty A5", lib, None), ("dirty 5A", lib, "5A")):
        path = str(tmp_path / (name.replace(" ", "_") + ".json"))
        rc, out = run_limited([sys.executable, "-c", TRANSCRIPT, path], dirty_env(fill, use), 600, "the transcripts (%s)" % name)
        assert rc == 0 and "TRANSCRIPTS DONE" in out, out[-6000:]
        got[name] = json.load(open(path))
        assert got[name]["build"].endswith("+dirty") == (use is not None), got[name]["build"]
    ref = got["product"]["scripts"]
    assert len(ref) == 12 and all(len(v["lines"]) >= 30 * 13 for v in ref.values())
    for name in ("dirty A5", "dirty 5A"):
        for seed, v in got[name]["scripts"].items():
            a, b = ref[seed]["lines"], v["lines"]
            diff = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
            if diff or len(a) != len(b):
                i = diff[0] if diff else min(len(a), len(b))
                where = a[i] if i < len(a) else "<the product transcript ends>"
                names = sorted({a[j].split()[2].split("[")[0] for j in diff})
                call = int(where.split()[0]) if i < len(a) else -1
                pytest.fail("seed %s, %s against the product library: %d of %d digests differ, first at %r (reads that differ anywhere: %s)\nthe script up to that call:\n%s"
                            % (seed, name, len(diff), len(a), where, names, "\n".join(l for l in v["log"] if l.startswith("    --") or int(l.split()[0]) <= call)))


ABI_TAILS = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from vehicles_dispatch_simulator_amd import workloads
P = lambda a: a.ctypes.data_as(C.c_void_p)
w = workloads.tiny(vehicles=90)
R = 3
env = w.make_env(R)
env.reset(w.vehicle_nodes(R))
env.run(7)
env.step()
V, Cn, lib, h = env.V, env.C, env._lib, env._h
for poison in (0x7B, 0xC4):
    for r in range(R):
        io, ao = np.zeros(Cn + 1, np.int32), np.zeros(Cn + 1, np.int32)
        arrs = [np.frombuffer(bytes([poison]) * (4 * V), dtype=np.int32).copy() for _ in range(6)]
        assert lib.vds_read_lists(h, r, P(io), P(arrs[0]), P(arrs[1]), P(ao), P(arrs[2]), P(arrs[3]), P(arrs[4]), P(arrs[5])) == 0
        ni, na = int(io[-1]), int(ao[-1])
        assert 0 < ni < V and 0 < na < V and ni + na == V, (ni, na)
        want = env.lists(r)          # (the binding hands over arrays of -1)
        for a, k, n in zip(arrs, ("idle_veh", "idle_node", "arr_veh", "arr_min", "arr_order", "arr_node"), (ni, ni, na, na, na, na)):
            assert (a[n:] == -1).all(), (k, r, a[n:][:8])
            assert np.array_equal(a, want[k]), (k, r)
        st = np.frombuffer(bytes([poison]) * V, dtype=np.uint8).copy()
        vv = [np.frombuffer(bytes([poison]) * (4 * V), dtype=np.int32).copy() for _ in range(4)]
        assert lib.vds_read_vehicles(h, r, P(st), *[P(a) for a in vv]) == 0
        ref = env.vehicles(r)        # (... and arrays of zeros)
        for a, k in zip([st] + vv, ("state", "node", "cluster", "arrive_min", "order")):
            assert np.array_equal(a, ref[k]), (k, r)
    O = env.O
    st = np.frombuffer(bytes([poison]) * (R * O), dtype=np.uint8).copy()
    ve, wt = [np.frombuffer(bytes([poison]) * (4 * R * O), dtype=np.int32).copy() for _ in range(2)]
    assert lib.vds_read_orders(h, 0, R, P(st), P(ve), P(wt)) == 0
    ref = env.orders()
    assert np.array_equal(st.reshape(R, O), ref["status"]) and (st <= 2).all() and (st == 0).any()
    assert (ve[st == 0] == -1).all() and (wt[st != 1] == -1).all() and (wt[st == 1] >= 0).all()
env.close()
print("TAILS DONE")
""" % ROOT


def test_host_arrays_come_back_defined_in_every_element():
    """The C ABI itself (the Python binding hands over arrays it has filled): ``vds_read_lists`` writes -1 past ``idle_off[C]`` /
    ``arr_off[C]``, ``vds_read_vehicles`` and ``vds_read_orders`` write every element (include/vds.h)."""
    gpu_allowed()
    rc, out = run_limited([sys.executable, "-c", ABI_TAILS], dirty_env(), 300, "the host arrays of the read entry points")
    assert rc == 0 and "TAILS DONE" in out, out[-4000:]
