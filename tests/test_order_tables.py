"""The host tables of a load (csrc/vds_tables.h) on the CPU: what vds_load_static / vds_load_order_days / vds_set_replica_days compute
before anything is uploaded, through the handle-free entries ``vds_debug_order_tables`` and ``vds_debug_replica_plan``.

Expected values are worked out in numpy from every recorded day under tests/golden/ and compared with the reference's own record
where it has one: ``n_ticks``, the cumulative ``t_order_num`` per slot, ``t_cl_orders`` per (slot, cluster), ``o_value``."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import fuzz_names, golden_names, load_golden, slot_names
from vehicles_dispatch_simulator_amd import _lib, synth

EINVAL, ECAPACITY, ESTATE = -1, -3, -4
ALL_DAYS = golden_names("tiny_") + golden_names("real_") + fuzz_names() + slot_names()
WMAX = 3          # DENSE_PULL_WMAX (csrc/vds_device.h)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def order_tables(cost, n2c, Cn, tick, days, ring=32, nbr=None, depth=0, threads=1, every_order=0):
    """days: [(release, pickup, delivery)]; returns (rc, message, dict of arrays)."""
    lib = _lib.load()
    cost = np.ascontiguousarray(cost, np.int32); n2c = np.ascontiguousarray(n2c, np.int32)
    rel = np.ascontiguousarray(np.concatenate([d[0] for d in days]), np.int32)
    pk = np.ascontiguousarray(np.concatenate([d[1] for d in days]), np.int32)
    dl = np.ascontiguousarray(np.concatenate([d[2] for d in days]), np.int32)
    off = np.cumsum([0] + [len(d[0]) for d in days]).astype(np.int64)
    nbr_off, nbr_idx = (None, None) if nbr is None else (np.ascontiguousarray(nbr[0], np.int32), np.ascontiguousarray(nbr[1], np.int32))
    day_out = np.zeros((len(days), 4), np.int32); sizes = np.zeros(8, np.int64)
    err = C.create_string_buffer(512)

    def call(n, nb, nt, m, nf):
        o = dict(so_rec=np.zeros((n, 4), np.int32), ord_q=np.zeros(n, np.int32), so_rank=np.zeros(n, np.int32), so_slot=np.zeros(n, np.int32),
                 bkt_off=np.zeros(nb, np.int32), tick_off=np.zeros(nt, np.int32), d_rec=np.zeros((m, 2), np.int32), d_first=np.zeros(nf, np.int32))
        rc = lib.vds_debug_order_tables(_p(cost), cost.shape[0], _p(n2c), Cn, tick, _p(nbr_off), _p(nbr_idx), depth, ring, len(days), _p(off),
                                        _p(rel), _p(pk), _p(dl), threads, every_order, _p(day_out), _p(sizes), _p(o["so_rec"]), _p(o["ord_q"]),
                                        _p(o["so_rank"]), _p(o["so_slot"]), n, _p(o["bkt_off"]), nb, _p(o["tick_off"]), nt, _p(o["d_rec"]), m,
                                        _p(o["d_first"]), nf, err, len(err))
        return rc, o

    rc, o = call(0, 0, 0, 0, 0)
    if rc == ECAPACITY:                      # the sizes are known now
        rc, o = call(*[int(x) for x in sizes[:5]])
    o.update(day=day_out, W=int(sizes[5]), hmax=int(sizes[6]), pull_ok=int(sizes[7]))
    return rc, err.value.decode(), o


def fixture_day(g):
    return g["o_release_min"], g["o_pickup"], g["o_delivery"]


def city_tables(cost, n2c, Cn):
    """node_local and cl_cmax as csrc/vds_tables.hip defines them: a node's rank among its cluster's nodes, the largest cost inside the block"""
    local = np.full(len(n2c), -1, np.int64); cmax = np.zeros(Cn, np.int64)
    for c in range(Cn):
        nodes = np.flatnonzero(n2c == c)
        local[nodes] = np.arange(nodes.size)
        if nodes.size:
            cmax[c] = max(int(cost[np.ix_(nodes, nodes)].max()), 0)
    return local, cmax


def check_day(cost, n2c, Cn, tick, ring, day, o, d, q_base, first_base, rec_base, bkt, toff, value=None):
    """One day of a result `o` against the formulas of the module docstring; returns the day's sizes."""
    rel, pk, dl = [np.asarray(a, np.int64) for a in day]
    O = rel.size
    T, now0, Oq, qb = [int(x) for x in o["day"][d]]
    assert now0 == rel[0] - tick and T == (rel[-1] + 3 * tick - now0) // tick + 1 and qb == q_base
    run = np.maximum.accumulate(np.maximum((rel - now0) // tick, 0))
    proc = (np.arange(O) < O - 1) & (run < T)
    ids = np.flatnonzero(proc)
    assert Oq == ids.size
    local, cmax = city_tables(cost, n2c, Cn)
    pc, dc = n2c[pk].astype(np.int64), n2c[dl].astype(np.int64)
    val = cost[dl, pk].astype(np.int64) if value is None else np.asarray(value, np.int64)
    # buckets and slots
    b = o["bkt_off"][bkt:bkt + T * Cn + 1].astype(np.int64)
    exp_cl = np.zeros((T, Cn), np.int64)
    np.add.at(exp_cl, (run[ids], pc[ids]), 1)
    assert b[0] == q_base and (np.diff(b).reshape(T, Cn) == exp_cl).all()
    t_off = o["tick_off"][toff:toff + T + 1].astype(np.int64)
    assert t_off[0] == q_base and (np.diff(t_off) == exp_cl.sum(1)).all() and (t_off == b[::Cn]).all()
    # sorted records
    rec = o["so_rec"][q_base:q_base + Oq].astype(np.int64)
    order = ids[np.lexsort((ids, pc[ids], run[ids]))]
    assert (rec[:, 0] == order).all() and (rec[:, 3] == val[order]).all()
    assert (rec[:, 1] == (local[pk[order]] | (local[dl[order]] << 16))).all() and (rec[:, 2] == (dc[order] | (pc[order] << 16))).all()
    # a slot's positions in id order: run is monotone in the id, so the day's ord_q lists the processed ids in order, slot after slot
    oq = o["ord_q"][q_base:q_base + Oq].astype(np.int64)
    assert (o["so_rec"][oq, 0] == ids).all()
    slot_of_pos = np.repeat(np.arange(T), np.diff(t_off))
    assert (run[ids] == slot_of_pos).all() and (oq >= t_off[slot_of_pos]).all() and (oq < t_off[slot_of_pos + 1]).all()
    assert (o["so_rank"][oq] == np.arange(q_base, q_base + Oq) - t_off[slot_of_pos]).all()
    # static arrival slots
    if T + ring >= 65535:
        return T, Oq, 0, 0, 0
    slots = lambda x: np.where(x <= 0, 1, -(-x // tick))
    dmin, dmax = slots(val), slots(val + cmax[np.maximum(pc, 0)])
    pull = ids[dmax[ids] < ring]
    a0 = run + dmin
    by_dest = pull[np.lexsort((pull, a0[pull], dc[pull]))]
    exp_slot = np.full(O, -1, np.int64); exp_slot[by_dest] = np.arange(by_dest.size)
    assert (o["so_slot"][q_base:q_base + Oq] == exp_slot[order]).all()
    TA = T + ring
    cnt = np.zeros((TA + 2, Cn), np.int64)
    np.add.at(cnt, (a0[pull] + 1, dc[pull]), 1)
    # [a, c]: where cluster c's orders with a0 >= a begin in d_rec - behind the orders to the clusters before c and those to c with a0 < a
    to_before = np.concatenate(([0], np.cumsum(np.bincount(dc[pull], minlength=Cn))[:-1]))
    exp_first = rec_base + to_before[None, :] + np.cumsum(cnt, axis=0)[:TA + 1]
    assert (o["d_first"][first_base:first_base + (TA + 1) * Cn].reshape(TA + 1, Cn) == exp_first).all()
    dr = o["d_rec"][rec_base:rec_base + by_dest.size].astype(np.int64) & 0xFFFFFFFF
    assert (dr[:, 0] == (((run[by_dest] & 63) << 26) | by_dest)).all()
    assert (dr[:, 1] == (a0[by_dest] | (local[dl[by_dest]] << 16) | (dmin[by_dest] << 24))).all()
    return T, Oq, by_dest.size, (int((dmax - dmin)[pull].max()) if pull.size else 0), (int(dmin[pull].max()) if pull.size else 0)


@pytest.mark.parametrize("name", ALL_DAYS)
def test_recorded_day(name):
    g = load_golden(name)
    Cn, tick = int(g["C"]), int(g["tick_minutes"]) if "tick_minutes" in g else 10
    ring = (32, 8, 16)[ALL_DAYS.index(name) % 3]
    nbr = (g["nbr_off"], g["nbr_idx"]) if int(g["neighbor_can_server"]) else None
    rc, msg, o = order_tables(g["cost"], g["node2cluster"], Cn, tick, [fixture_day(g)], ring=ring, nbr=nbr, depth=int(g["depth_limit"]), threads=2)
    assert rc == 0, msg
    # the reference's record
    T = int(g["n_ticks"])
    assert o["day"][0].tolist()[:2] == [T, int(g["o_release_min"][0]) - tick]
    assert (np.diff(o["bkt_off"]).reshape(T, Cn) == g["t_cl_orders"]).all()
    assert (o["tick_off"][1:] == np.asarray(g["t_order_num"], np.int64)).all()
    T_, Oq, m, W, hmax = check_day(g["cost"], g["node2cluster"], Cn, tick, ring, fixture_day(g), o, 0, 0, 0, 0, 0, 0, value=g["o_value"])
    assert o["d_rec"].shape[0] == m and (o["W"], o["hmax"]) == (W, hmax) and o["pull_ok"] == (W <= WMAX)


def pull_verdict(g, ring=32):
    """(pull_ok, orders with a static arrival slot, W) of a recorded day at the default ring horizon."""
    rc, msg, o = order_tables(g["cost"], g["node2cluster"], int(g["C"]), int(g["tick_minutes"]), [fixture_day(g)], ring=ring)
    assert rc == 0, msg
    return o["pull_ok"], o["d_rec"].shape[0], o["W"]


def test_slot_corpus_static_arrival_slot_verdicts():
    """What tests/test_gpu_slot_lengths.py relies on: with 1- and 2-minute slots the day meant for the dense tick has orders with a
    static arrival slot and yet the verdict is 0 (in-cluster costs spread arrivals over more than DENSE_PULL_WMAX slots): the
    library picks the dense tick's ring form by itself.  Of the two days beyond slot 32767 the searching one-minute day has the
    same verdict, the two-minute day with costs // 7 keeps its static arrival slots."""
    for name in ("slot_0001_0", "slot_0002_0"):
        ok, m, W = pull_verdict(load_golden(name))
        assert ok == 0 and m > 0 and W > WMAX, (name, ok, m, W)
    for name in ("slot_0060_0", "slot_1440_0"):
        ok, m, W = pull_verdict(load_golden(name))
        assert ok == 1 and m > 0 and W <= WMAX, (name, ok, m, W)
    assert pull_verdict(load_golden("slot_long_search"))[0] == 0
    ok, m, W = pull_verdict(load_golden("slot_long_pull"))
    assert ok == 1 and 0 < W <= WMAX and m == int(load_golden("slot_long_pull")["order_num"])


def _tiny_city():
    g = load_golden("tiny_dispatch")
    return g, g["cost"], g["node2cluster"], int(g["C"])


def _days(g, n, O=700):
    days = [tuple(a[:O] for a in fixture_day(g))]
    for d in range(1, n):
        start, pick, dele = synth.make_orders(9100 + d, int(g["N"]), O - 37 * (d % 5))
        rel = synth.release_minutes(start)
        days.append(((rel - rel[0] + 3 * d).astype(np.int32), pick.astype(np.int32), dele.astype(np.int32)))
    return days


@pytest.mark.parametrize("n_days", [1, 3, 16])
def test_days_back_to_back_and_thread_count(n_days):
    g, cost, n2c, Cn = _tiny_city()
    days = _days(g, n_days)
    rc, msg, a = order_tables(cost, n2c, Cn, 10, days, threads=1)
    assert rc == 0, msg
    rc, msg, b = order_tables(cost, n2c, Cn, 10, days, threads=4)
    assert rc == 0, msg
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    q = fb = rb = bk = tk = 0
    Ws, hs = [0], [0]
    for d, day in enumerate(days):
        T, Oq, m, W, hmax = check_day(cost, n2c, Cn, 10, 32, day, a, d, q, fb, rb, bk, tk)
        q += Oq; fb += (T + 32 + 1) * Cn; rb += m; bk += T * Cn + 1; tk += T + 1
        Ws.append(W); hs.append(hmax)
    assert (q, bk, tk, rb, fb) == (a["so_rec"].shape[0], a["bkt_off"].size, a["tick_off"].size, a["d_rec"].shape[0], a["d_first"].size)
    assert (a["W"], a["hmax"]) == (max(Ws), max(hs))


def _grid(N=6, Cn=2):
    cost = (np.abs(np.arange(N)[:, None] - np.arange(N)[None, :]) * 4 + 3).astype(np.int32)
    return cost, (np.arange(N) * Cn // N).astype(np.int32)


def test_edge_days():
    cost, n2c = _grid()
    i32 = lambda *x: np.array(x, np.int32)
    # one order: the last order is never processed - every table empty, offsets well-formed
    rc, msg, o = order_tables(cost, n2c, 2, 10, [(i32(50), i32(1), i32(4))])
    assert rc == 0 and o["day"].tolist() == [[5, 40, 0, 0]] and o["so_rec"].shape[0] == 0 and o["d_rec"].shape[0] == 0
    assert not o["bkt_off"].any() and o["bkt_off"].size == 11 and not o["tick_off"].any() and o["tick_off"].size == 6 and not o["d_first"].any()
    assert o["pull_ok"] == 1 and (o["W"], o["hmax"]) == (0, 0)
    # every order in one slot and one cluster; a release before the first order's counts for slot 0
    for rel in (i32(50, 50, 51, 52, 59, 59), i32(50, 20, 0, 45, 41, 59)):
        day = (rel, i32(0, 1, 2, 1, 0, 2), i32(3, 4, 5, 0, 3, 1))
        rc, msg, o = order_tables(cost, n2c, 2, 10, [day])
        assert rc == 0, msg
        check_day(cost, n2c, 2, 10, 32, day, o, 0, 0, 0, 0, 0, 0)
        assert o["tick_off"].tolist()[:3] == [0, 0, 5] and o["bkt_off"].tolist()[2:5] == [0, 5, 5] and o["so_rank"].tolist() == [0, 1, 2, 3, 4]
    # a pickup outside [0, N)
    rc, msg, o = order_tables(cost, n2c, 2, 10, [(i32(0, 5, 9), i32(0, 6, 1), i32(1, 2, 3))])
    assert rc == EINVAL and msg == "vds_load_orders: order 1 has a node outside [0,6)"
    # a processed order on a node outside every cluster - but not the never-processed last one
    out = n2c.copy(); out[5] = -1
    rc, msg, o = order_tables(cost, out, 2, 10, [(i32(0, 5, 9), i32(0, 1, 1), i32(1, 5, 3))])
    assert rc == ESTATE and msg == "vds_load_orders: order 1 touches a node outside every cluster (KeyError in the reference, :918/:960)"
    rc, msg, o = order_tables(cost, out, 2, 10, [(i32(0, 5, 9), i32(0, 1, 5), i32(1, 2, 3))])
    assert rc == 0, msg
    # more than 65535 slots
    rc, msg, o = order_tables(cost, n2c, 2, 10, [(i32(0, 700000), i32(0, 1), i32(1, 2))])
    assert rc == EINVAL and msg == "vds_load_orders: 70005 ticks > 65535 unsupported"
    # the stamp form's condition: an order that may outlive the ring horizon owns no slot
    far = cost.copy(); far[4, 0] = 40
    day = (i32(0, 1, 2, 3), i32(0, 1, 2, 0), i32(4, 3, 5, 1))
    assert [order_tables(far, n2c, 2, 10, [day], ring=4, every_order=e)[2]["pull_ok"] for e in (0, 1)] == [1, 0]
    assert order_tables(cost, n2c, 2, 10, [day], ring=4, every_order=1)[2]["pull_ok"] == 1


TICK_MINUTES_MAX = (2**31 - 1) // 5          # VDS_TICK_MINUTES_MAX (include/vds.h)


def test_days_whose_minutes_do_not_fit_int32_are_refused():
    """now0 = first release - tick, t * tick and now0 + t * tick for t <= T are int32 on the device (include/vds.h): the builder refuses
    a day beyond that, and takes the longest slot vds_create accepts on a day that fits."""
    cost, n2c = _grid()
    i32 = lambda *x: np.array(x, np.int32)
    one = (i32(0), i32(1), i32(4))
    rc, msg, o = order_tables(cost, n2c, 2, TICK_MINUTES_MAX, [one])
    assert rc == 0 and o["day"].tolist() == [[5, -TICK_MINUTES_MAX, 0, 0]], (rc, msg)
    for tick, day in ((TICK_MINUTES_MAX + 1, one), (2**30, one),                                 # T * tick
                      (10, (i32(2**31 - 100, 2**31 - 5), i32(0, 1), i32(1, 2))),                # now0 + T * tick
                      (TICK_MINUTES_MAX, (i32(0, TICK_MINUTES_MAX), i32(0, 1), i32(1, 2))),         # (six slots of the longest length)
                      (10, (i32(-2**31 + 5, -2**31 + 9), i32(0, 1), i32(1, 2)))):                 # now0
        rc, msg, o = order_tables(cost, n2c, 2, tick, [day])
        assert rc == EINVAL and msg.startswith("vds_load_orders: the day's minutes ") and "do not fit int32" in msg, (tick, rc, msg)


def replica_plan(rd, n_days, gran_small=0, regroup=1, alloc=0, cap=None):
    lib = _lib.load()
    rd = np.ascontiguousarray(rd, np.int32)
    head = np.zeros(4, np.int32)
    cap = rd.size * 2 + 64 if cap is None else cap
    i2e, rperm, doi = [np.zeros(cap, np.int32) for _ in range(3)]
    e2i = np.zeros(rd.size, np.int32)
    rc = lib.vds_debug_replica_plan(_p(rd), rd.size, n_days, gran_small, regroup, alloc, _p(head), _p(i2e), _p(rperm), _p(doi), cap, _p(e2i))
    R = int(head[0])
    return rc, dict(R=R, row_gran=int(head[1]), chunk_days=int(head[2]), regrouped=int(head[3]), int2ext=i2e[:R], rperm=rperm[:R], day=doi[:R], ext2int=e2i)


def check_regrouped(rd, n_days, p):
    """The properties of a regrouped plan: inverse maps on the real replicas, one day per granule, dummies on the empty day at the
    end of a day's run."""
    rd = np.asarray(rd)
    R, gr = p["R"], p["row_gran"]
    assert p["regrouped"] and p["chunk_days"] == 1 and R % 16 == 0 and R * 4 <= rd.size * 5
    real = p["int2ext"] >= 0
    assert sorted(p["int2ext"][real].tolist()) == list(range(rd.size)) and (p["ext2int"][p["int2ext"][real]] == np.flatnonzero(real)).all()
    assert (p["rperm"] == np.where(real, np.arange(R), -1)).all()
    assert (p["day"][real] == rd[p["int2ext"][real]]).all() and (p["day"][~real] == n_days).all()
    for g0 in range(0, R, gr):
        days = set(p["day"][g0:g0 + gr][real[g0:g0 + gr]].tolist())
        assert len(days) <= 1
        r = real[g0:g0 + gr]
        assert not (r[1:] & ~r[:-1]).any()          # dummies only behind the granule's real replicas
    assert (np.diff(p["day"][real]) >= 0).all()     # the days in order, each in one run


def test_replica_plan():
    rng = np.random.default_rng(5)
    # blocks of 16 on one day each: stored as given
    for R, n_days in ((16, 1), (32, 2), (64, 4), (96, 3)):
        rd = np.repeat(rng.permutation(R // 16) % n_days, 16)
        rc, p = replica_plan(rd, n_days)
        assert rc == 0 and (p["R"], p["row_gran"], p["regrouped"]) == (R, 16, 0) and p["chunk_days"] == (n_days > 1)
        assert (p["day"] == rd).all() and (p["int2ext"] == np.arange(R)).all() and (p["ext2int"] == np.arange(R)).all()
    # blocks of 8 / 4: day groups of that size where they may be used, regrouped otherwise
    rd = np.repeat([0, 1, 1, 0, 2, 2, 0, 1], 8)
    assert replica_plan(rd, 3, gran_small=1)[1]["row_gran"] == 8 and replica_plan(rd, 3, gran_small=1)[1]["regrouped"] == 0
    assert replica_plan(np.repeat([0, 1, 2, 0, 1, 2, 0, 1], 4), 3, gran_small=1)[1]["row_gran"] == 4
    check_regrouped(rd, 3, replica_plan(rd, 3)[1])
    # maps that mix days inside groups of 16, padding under a quarter
    for R, n_days, small in ((64, 2, 0), (96, 3, 0), (96, 4, 1), (80, 2, 1), (72, 2, 0), (90, 3, 1)):
        rd = rng.integers(0, n_days, R)
        rc, p = replica_plan(rd, n_days, gran_small=small)
        assert rc == 0
        if not p["regrouped"]:                      # (the draw needs more than a quarter of padding)
            assert p["chunk_days"] == 0 and p["R"] == R
            continue
        check_regrouped(rd, n_days, p)
        assert p["row_gran"] == 16 or small
    rd = np.array([0] * 40 + [1] * 40)[rng.permutation(80)]
    rc, p = replica_plan(rd, 2)                     # 48 + 48 stored replicas for 80: under a quarter
    check_regrouped(rd, 2, p)
    assert (p["R"], p["row_gran"]) == (96, 16)
    rc, p8 = replica_plan(rd, 2, gran_small=1)
    check_regrouped(rd, 2, p8)
    assert (p8["R"], p8["row_gran"]) == (96, 16)
    # the padding would exceed a quarter: stored as given, every row its own order stream
    rd = np.array([0, 1, 2, 3] * 4)
    rc, p = replica_plan(rd, 4)
    assert rc == 0 and (p["R"], p["chunk_days"], p["regrouped"], p["row_gran"]) == (16, 0, 0, 16) and (p["day"] == rd).all()
    rd = np.array([0] * 17 + [1] * 15)
    assert replica_plan(rd, 2)[1]["regrouped"] == 0 and replica_plan(rd, 2, regroup=0)[1]["chunk_days"] == 0
    rc, p = replica_plan(rd, 2, gran_small=1)       # groups of 4: 20 + 16 = 36 -> 48 stored replicas for 32: too many
    assert p["regrouped"] == 0
    # a replica count that is no multiple of 16
    rd = np.array([0] * 50 + [1] * 40)[rng.permutation(90)]
    rc, p = replica_plan(rd, 2)
    check_regrouped(rd, 2, p)
    assert p["R"] == 112
    assert replica_plan(np.zeros(20, np.int32), 1)[1]["R"] == 20
    # the tables at hand hold more padded replicas: kept while under a quarter
    rd = np.array([0] * 64 + [1] * 32)[rng.permutation(96)]
    assert replica_plan(rd, 2)[1]["R"] == 96
    rc, p = replica_plan(rd, 2, alloc=112)
    check_regrouped(rd, 2, p)
    assert p["R"] == 112 and replica_plan(rd, 2, alloc=128)[1]["R"] == 96
    # a short output array
    rc, p = replica_plan(rd, 2, cap=8)
    assert rc == ECAPACITY and p["R"] == 96
    assert replica_plan(np.array([0, 2]), 2)[0] == EINVAL


def test_hostcheck_builds_and_runs_clean(tmp_path):
    """`make hostcheck`: the builders under the address / undefined-behaviour and the thread sanitizer, as a stand-alone program"""
    out = subprocess.run(["make", "-s", "-j2", "-C", _lib.CSRC, "hostcheck", "CHECKDIR=%s" % tmp_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
