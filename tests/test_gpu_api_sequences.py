"""Random API sequences on one handle against the oracle model (tests/api_script.py; its CPU half, with the coverage conditions of
the corpus and the seeded faults, is tests/test_api_script_model.py): one case per seed on the real ``BatchedDispatchEnv`` - 40 by
default, VDS_APISEQ_N for more - and 8 cases with TWO handles alive at once, each with its own case and model, their calls dealt
alternately on one stream, the second handle closed and opened again half-way.  Bit-exact, no tolerance.  A case that passed has also
given back every device block its handles took (``vds_debug_device_blocks`` before the first handle and after the last close).  A red case names its seed,
the failing call and the script so far; ``api_script.run_script(BatchedDispatchEnv, seed, upto=k)`` replays a prefix."""
import ctypes
import gc
import statistics
import time

import numpy as np

import pytest

import api_script
from api_script import Script, new_stats, run_script
from vehicles_dispatch_simulator_amd import BatchedDispatchEnv, _lib

pytestmark = pytest.mark.gpu

SINGLE, PAIRS = api_script.corpus()


def device_blocks():
    """(live device blocks of the process, their bytes); a handle some earlier test dropped without closing it is collected first"""
    gc.collect()
    out = np.zeros(2, dtype=np.int64)
    assert _lib.load().vds_debug_device_blocks(out.ctypes.data_as(ctypes.c_void_p)) == 0
    return int(out[0]), int(out[1])


class Corpus:
    """Every case runs once per session, whichever test asks first: (seconds, statistics), or the failure it raised."""

    def __init__(self):
        self.done = {}

    def case(self, key):
        if key not in self.done:
            before = device_blocks()
            stats, t0 = new_stats(), time.perf_counter()
            try:
                if isinstance(key, tuple):
                    two_handles(key, stats)
                else:
                    run_script(BatchedDispatchEnv, key, stats=stats)
                self.done[key] = (time.perf_counter() - t0, stats)
                assert device_blocks() == before, "device (blocks, bytes) %s after the case, %s before it" % (device_blocks(), before)
            except BaseException as e:
                self.done[key] = e
        if isinstance(self.done[key], BaseException):
            raise self.done[key]
        return self.done[key]


@pytest.fixture(scope="module")
def corpus():
    return Corpus()


def two_handles(seeds, stats):
    import torch
    stream = torch.cuda.Stream()
    a = Script(BatchedDispatchEnv, seeds[0], stream=stream.cuda_stream, stats=stats)
    b = Script(BatchedDispatchEnv, seeds[1], stream=stream.cuda_stream, stats=stats)
    try:
        more_a = more_b = True
        reopened = False
        while more_a or more_b:
            more_a = more_a and a.next()
            if more_b and not reopened and b.n_calls >= b.length // 2:
                b.reopen()
                reopened = True
            more_b = more_b and b.next()
        assert reopened and a.done and b.done
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("seed", SINGLE)
def test_api_sequence_matches_the_model(corpus, seed):
    corpus.case(seed)


@pytest.mark.parametrize("seeds", PAIRS, ids=["%d+%d" % p for p in PAIRS])
def test_two_handles_alive_at_once(corpus, seeds):
    corpus.case(seeds)


def test_the_corpus_reached_what_it_claims(corpus):
    """Over all cases (run here when this test is selected alone): every restore issued in state VALID was answered as the model
    expects - any other answer fails its case, the count says that there were some -, the tick families, both storage forms of order
    days per replica.  Prints the cost of a case next to that of a fuzz case in the same process."""
    runs = [corpus.case(k) for k in list(SINGLE) + list(PAIRS)]
    kernels, layouts, storage = set(), set(), set()
    for _, st in runs:
        kernels |= st["kernels"]; layouts |= st["layouts"]; storage |= st["storage"]
    valid, ok = sum(st["restores_valid"] for _, st in runs), sum(st["restores_valid_ok"] for _, st in runs)
    assert valid >= 20 and ok == valid, (ok, valid)
    from test_gpu_fuzz import random_case, run_case
    fuzz = []
    for seed in range(16):
        t0 = time.perf_counter()
        run_case(seed, random_case(seed))
        fuzz.append(time.perf_counter() - t0)
    single = [s for s, _ in runs[:len(SINGLE)]]
    print("kernels %s; storage of mixed maps %s; %d restores in state VALID" % (sorted(kernels), sorted(storage), valid))
    print("seconds per case: fuzz median %.3f; single-handle median %.3f, maximum %.3f; two-handle median %.3f"
          % (statistics.median(fuzz), statistics.median(single), max(single), statistics.median([s for s, _ in runs[len(SINGLE):]])))
    assert "k_tick_dense" in kernels, kernels
    assert any(k == "k_tick_rows" and dense == 0 for k, dense, _ in layouts), layouts          # the row tick on the wide layout
    assert "k_tick" in kernels, kernels                                                          # the generic tick
    assert kernels & {"k_dfs_hybrid", "k_tick_replica2", "k_match_dfs"}, kernels                 # a neighbour-search form
    assert {"regrouped", "stream per row"} <= storage, storage
