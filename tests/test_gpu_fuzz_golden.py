"""The HIP tick path on the fuzz corpus (tests/golden/make_fuzz_golden.py): days the unmodified reference ran over the axes the
GPU fuzz tests vary - depth -1..4, ticks of 10 / 5 / 15 / 7 / 3 minutes, raw pickup windows none / 40 / 8 / 0, tie-heavy / long /
negative / fractional costs, 0..139 vehicles, 4..48 clusters, dispatch.  Every day runs as test_gpu_parity.run_day with three
replicas: per tick against the oracle, and replica 0 against the reference's own per-tick record and per-order vectors.
Reads tests/golden only."""
import json
import os
import sys

import pytest

from helpers import fuzz_names, live_window, load_fuzz
from test_gpu_parity import MODES, run_day

pytestmark = pytest.mark.gpu

FUZZ = fuzz_names()
IN_PROCESS_MODES = ("fast", "generic")
SEARCH_MODES = ("dfs_v2", "dfs_wide", "far")
DENSE_MODES = ("dense16", "dense_tiny8", "dense_slow", "dense_ring", "dense_alt", "rows", "far")
WINDOW_MODES = ("generic", "far", "ring64")
NPROC = 4          # (conftest.GPU_WORKERS)


def worker_modes(g):
    """The engine modes beyond IN_PROCESS_MODES a case takes, decided by its data: the neighbour-search kernels where a search can
    leave the pickup's cluster, the dense-tick variants and the row-mapped kernel where the library runs the dense tick (no
    search, default window), the wide-layout paths under a live window; the far tables everywhere."""
    searching = bool(g["neighbor_can_server"]) and int(g["depth_limit"]) > 0
    modes = []
    if searching:
        modes += SEARCH_MODES
    if not searching and not live_window(g):
        modes += DENSE_MODES
    if live_window(g):
        modes += WINDOW_MODES
    return [m for i, m in enumerate(modes) if m not in IN_PROCESS_MODES and m not in modes[:i]]


@pytest.mark.parametrize("mode", IN_PROCESS_MODES)
@pytest.mark.parametrize("name", FUZZ)
def test_fuzz_golden_per_tick(name, mode):
    g = load_fuzz(name)
    run_day(g, R=3, same_init=bool(len(g["dispatch_log"])), **MODES[mode])


def worker_pairs():
    return [(n, m, "tick") for n in FUZZ for m in worker_modes(load_fuzz(n))]


def test_fuzz_golden_modes_in_worker_processes():
    """Every (case, mode) pair of worker_modes as a full per-tick day, dealt to four worker processes (tests/parity_worker.py, as
    test_gpu_parity.test_mode_fixture_product_in_worker_processes: a day's cost is host work)."""
    import conftest
    pairs = worker_pairs()
    assert len(pairs) >= 2 * len(FUZZ) and {m for _, m, _ in pairs} == set(SEARCH_MODES + DENSE_MODES + WINDOW_MODES) - set(IN_PROCESS_MODES)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "parity_worker.py")
    conftest.start_workers("fuzz_golden_modes", [[sys.executable, worker, json.dumps(pairs[i::NPROC])] for i in range(NPROC)])
    done = 0
    for i, (rc, out) in enumerate(conftest.collect_workers("fuzz_golden_modes")):
        assert rc == 0 and "WORKER DONE" in out, "worker %d:\n%s" % (i, out[-3000:])
        done += int(out.split("WORKER DONE")[1].split()[0])
    assert done == len(pairs)


# (a device-resident action tensor carries no arrival time of its own: the days whose hook body booked extra minutes stay with
# vds_apply_dispatch_ex in the tests above)
DEVICE_DISPATCH = [n for n in FUZZ for g in [load_fuzz(n)] if len(g["dispatch_log"]) and "dispatch_extra_minutes" not in g]


@pytest.mark.parametrize("name", DEVICE_DISPATCH)
def test_fuzz_golden_device_resident_dispatch(name):
    """vds_apply_dispatch_device: the reference-side dispatch log replayed as a GPU action tensor."""
    run_day(load_fuzz(name), R=3, same_init=True, device_dispatch=True)


def test_device_dispatch_cases_span_ticks_windows_and_depths():
    gs = [load_fuzz(n) for n in DEVICE_DISPATCH]
    assert any(int(g["tick_minutes"]) != 10 for g in gs) and any(live_window(g) for g in gs)
    assert any(bool(g["neighbor_can_server"]) and int(g["depth_limit"]) >= 2 for g in gs)
