"""Generator of the slot-length corpus.  Runs ONLY in the build container (needs /root/reference).

    python tests/golden/make_slot_golden.py

The fuzz corpus (make_fuzz_golden.py) draws slot lengths of 10 / 5 / 15 / 7 / 3 minutes and days of at most a few hundred slots.
This corpus is the pin for the rest of the slot-length axis (``TimePeriods`` in the reference, ``tick_minutes`` here): days the
unmodified reference ran with slots of 1, 2, 30, 60, 63, 64, 120 and 1440 minutes, recorded like a fuzz case, and two days whose
release times are stretched over several weeks so that they pass slot 32767 (recorded without per-slot lists and without
dispatch).  Data only.

    1, 2            most trips outlive the 32-slot ring horizon (far list, inbox, migration); static arrival slots cover part
                    of the day only; the division by the slot length is a true division at 1
    30              the multiply-high division (2..63 minutes), days of about 50 slots
    60, 63, 64      the edges of that rule; every trip is due in the next slot or the one after
    120, 1440       days of 15 and 5 slots with hundreds of orders each

DAYS_PER_LENGTH days per slot length, drawn over the fuzz generator's other axes (search on / off with depth 0..3, window
none / 40 / 8, cost styles, dispatch for about 40 %, V 0..139, O 200..1400), the pairing shuffled by SHUFFLE_SEED.  Each of a
length's four days then has a role that overrides the axes the role needs (case_specs), so part of the drawn product never occurs:

    role 0  the dense tick by the library's own rules: no search beyond depth 0, never a window, plain / div7 / frac costs, V >= 40;
            at 60..120 minutes 1400 orders released within a quarter of the day (slots of more than 256 orders), at 1 and 2
            minutes a city of 4 or 6 clusters with plain costs
    role 1  a search that leaves the cluster: search on, depth >= 1, V >= 8
    role 2  a live window (40 or 8), always ``mul`` costs, V >= 40
    role 3  dispatch, V >= 60

Fleets of 0..7 vehicles are therefore not in this corpus (the fuzz corpus has them at its slot lengths).  The coverage conditions
(helpers.slot_coverage_gaps) are computed from the recorded days alone and asserted at the end; the GPU tests take as a length's
searching day the one that served most orders from another cluster (tests/test_gpu_slot_lengths.py asserts at least 10).

Files: tests/golden/slotpack_<k>.npz in the fuzz corpus' form, cases ``slot_<minutes>_<i>`` and ``slot_long_<what>``; the printed
summary is kept as tests/golden/slot_corpus.txt.  fuzzpack_*.npz are not touched.
"""
from __future__ import annotations

import glob
import os
import random
import time
import zipfile

import numpy as np

import make_fuzz_golden as fz          # (puts the repository root and tests/ on sys.path)
from make_fuzz_golden import HERE, MAX_FILE_BYTES, generate, summary_line, synth, rh, helpers      # noqa: F401 (build_city, narrow: inside generate)

LENGTHS = helpers.SLOT_LENGTHS
DAYS_PER_LENGTH = 4
N_CASES = len(LENGTHS) * DAYS_PER_LENGTH
CASES_PER_FILE = 6
SHUFFLE_SEED = 20161102
MAX_CORPUS_BYTES = 3_000_000
SIDES = (1600, 2000, 2400, 3200, 5000, 6400)
STYLES = ("plain", "div7", "mul", "neg", "frac")
DEPTHS = (0, 1, 2, 3)
WINDOWS = (None, 40, 8)


def strata(values, stream):
    out = [values[i % len(values)] for i in range(N_CASES)]
    random.Random(SHUFFLE_SEED + stream).shuffle(out)
    return out


def case_specs():
    side, style, depth = strata(SIDES, 1), strata(STYLES, 2), strata(DEPTHS, 3)
    nbr, window = strata((True, True, False), 4), strata(WINDOWS, 6)
    dispatch = strata((True, True, False, False, False), 7)
    tick = [LENGTHS[i % len(LENGTHS)] for i in range(N_CASES)]        # (every length DAYS_PER_LENGTH times; the other axes are shuffled)
    specs = {}
    for i in range(N_CASES):
        rng = random.Random(SHUFFLE_SEED * 37 + i)
        if i < len(LENGTHS) and tick[i] <= 2:       # (the dense day of 1 and 2 minutes: clusters wide enough that arrivals spread
            side[i], style[i] = max(side[i], 5000), "plain"      # over more than DENSE_PULL_WMAX slots - the dense tick's ring form)
        C = int(np.prod(synth.grid_shape(synth.DEFAULT_BOUND, side[i])))
        s = dict(side_m=side[i], C=C, N=max(rng.randint(30, 220), C + 5), style=style[i], depth=depth[i], neighbor=nbr[i],
                 tick=tick[i], window=window[i], dispatch=dispatch[i], city_seed=7500 + i, order_seed=8500 + i, veh_seed=9500 + i,
                 style_k={"mul": rng.randint(3, 8), "neg": rng.randint(1, 5)}.get(style[i], 0),
                 V=rng.randint(0, 4) if rng.random() < 0.1 else rng.randint(0, 139), O=rng.randint(200, 1400),
                 extra=rng.choice((0, 0, 4, 11)) if dispatch[i] else 0, every=max(3, 60 // tick[i]), empty=[],
                 cluster_mode=rng.choice(("KmeansClustering", "SpectralClustering", "TransportationClustering")), focus=None)
        # the day's role among its slot length's four fixes the axes its coverage condition needs; the rest stays as drawn
        role = i // len(LENGTHS)
        if role == 0:       # the library's own choice of the dense tick: no search, no live window, byte costs, a fleet that serves
            s.update(depth=0 if s["neighbor"] else s["depth"], window=None, V=max(s["V"], 40),
                     style=s["style"] if s["style"] in ("plain", "div7", "frac") else "plain", style_k=0)
            if 60 <= tick[i] < 1440:       # a slot of more than 256 orders: the day's orders released within a quarter of the day
                s.update(O=1400, span=(1, 4))
        elif role == 1:     # a search that leaves the pickup's cluster
            s.update(neighbor=True, depth=max(s["depth"], 1), V=max(s["V"], 8))
        elif role == 2:     # a live window that rejects vehicles that were found
            s.update(window=s["window"] or 8, V=max(s["V"], 40), style="mul", style_k=s["style_k"] or 5)
        else:               # dispatch by the reference-side policy (it moves vehicles out of clusters with three idle ones)
            s.update(dispatch=True, V=max(s["V"], 60))
        specs["slot_%04d_%d" % (tick[i], role)] = s
    # the days of more than 32767 slots: a small city, the day's release times stretched (generate: span) so that orders are served
    # from slot 32768 on and vehicles are under way across it; no lists, no dispatch.  The second has in-cluster costs of at most
    # 4 minutes: every order keeps a static arrival slot (pull_ok, W = 2 <= DENSE_PULL_WMAX)
    base = dict(style_k=0, window=None, dispatch=False, extra=0, empty=[], cluster_mode="KmeansClustering", focus=None, lists=False)
    specs["slot_long_search"] = dict(base, side_m=6400, C=4, N=60, style="plain", depth=1, neighbor=True, tick=1, V=12, O=260,
                                     span=(2452, 100), city_seed=7601, order_seed=8601, veh_seed=9601)
    specs["slot_long_pull"] = dict(base, side_m=5000, C=6, N=90, style="div7", depth=0, neighbor=False, tick=2, V=14, O=300,
                                   span=(5220, 100), city_seed=7602, order_seed=8602, veh_seed=9602)
    return specs


def main():
    if not rh.reference_available():
        raise SystemExit("reference not mounted: golden fixtures can only be generated in the build container")
    for p in glob.glob(os.path.join(HERE, "slotpack_*.npz")):
        os.remove(p)
    specs = case_specs()
    names = sorted(specs)
    t0 = time.time()
    for k in range(0, len(names), CASES_PER_FILE):
        pack = {}
        for name in names[k:k + CASES_PER_FILE]:
            for key, a in generate(name, specs[name]).items():
                pack[name + "/" + key] = a
        np.savez_compressed(os.path.join(HERE, "slotpack_%d.npz" % (k // CASES_PER_FILE)), **pack)
    helpers.forget_slot_index()
    total, lines = 0, []
    for p in sorted(glob.glob(os.path.join(HERE, "slotpack_*.npz"))):
        assert os.path.getsize(p) < MAX_FILE_BYTES, (p, os.path.getsize(p))
        total += os.path.getsize(p)
        sizes = {}
        for zi in zipfile.ZipFile(p).infolist():
            sizes[zi.filename.split("/")[0]] = sizes.get(zi.filename.split("/")[0], 0) + zi.compress_size
        for name in sorted(sizes):
            g = helpers.load_slot(name)
            f = helpers.slot_day_facts(g)
            lines.append(summary_line(name, g, sizes[name], width=16) +
                         " most=%-4d far=%-4d late=%d across=%d" % (f["most"], f["far"], f["served_late"], f["across"]))
    assert total < MAX_CORPUS_BYTES, total
    lines.append("%d cases, %.0f KB in all" % (len(names), total / 1024))
    print("\n".join(lines))
    print("%.0f s" % (time.time() - t0))
    with open(os.path.join(HERE, "slot_corpus.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    missing = helpers.slot_coverage_gaps({n: helpers.load_slot(n) for n in helpers.slot_names()})
    assert not missing, "coverage conditions not met (pick another SHUFFLE_SEED): %s" % missing


if __name__ == "__main__":
    main()
