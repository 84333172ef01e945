"""The CPU half of the API-sequence tests (tests/api_script.py): the whole harness - generator, model, runner, comparisons - driven
on ``OracleEnv``, a stand-in for ``BatchedDispatchEnv`` built from CPU oracles alone, for every seed of the GPU corpus
(tests/test_gpu_api_sequences.py).  It proves, without a GPU, that the harness is green on a correct engine, that the corpus reaches
the transitions it claims to reach, and that it goes red when the engine is subtly wrong (eleven seeded faults, one at a time).

``OracleEnv`` keeps its own books - one event log per replica, replayed into a fresh oracle by a restore - and shares none of the
model's bookkeeping code (``api_script.Lineage`` keeps dispatches per slot and is replayed slot by slot)."""
import functools
import random

import numpy as np
import pytest

import api_script
from api_script import MOVERS, KINDS, ScriptFailure, legal_pair, new_stats, run_script
from oracle.oracle import Oracle

FAULTS = ("restore_source", "stale_run", "drop_last_action", "snapshot_survives_map", "stale_cluster_list",
          # the per-vehicle dispatch and the per-vehicle planes:
          "veh_descending",             # the vehicle form applied in descending vehicle order
          "veh_before_kform",           # its entries placed before an earlier K-form call of the same slot
          "veh_stored_replica",         # the target tensor indexed by the stored rather than the caller's replica under a regrouping map
          "veh_refused_applied",        # a refused target applied all the same
          "veh_block_stale_restore",    # the planes block not refreshed after a restore
          "veh_unrequested_written")    # a plane that was not requested overwritten


def _up(x, m):
    return (x + m - 1) // m * m


class _Rep:
    """One replica of the stand-in: an oracle and the log of everything done to it since its reset."""

    def __init__(self, env, init, day):
        self.env, self.init, self.day = env, np.array(init, dtype=np.int32), day
        self.o = env.oracle(day)
        self.o.reset(self.init)
        self.T, self.t, self.log = self.o.num_ticks, 0, []
        self.outc = np.zeros((4, env.C), dtype=np.int64)

    def apply(self, ev):
        self.log.append(ev)
        if ev[0] == "step":
            self.outc = np.zeros((4, self.env.C), dtype=np.int64)
            if self.t < self.T:
                before = self.o.orders()["status"]
                self.o.begin_tick()
                res = self.o.orders()
                cl = self.env.n2c[self.day[1]]
                for o in np.flatnonzero((before == 0) & (res["status"] != 0)):
                    if res["status"][o] == 1:
                        self.outc[0, cl[o]] += 1
                        self.outc[2, cl[o]] += res["wait"][o]
                        self.outc[3, cl[o]] += res["value"][o]
                    else:
                        self.outc[1, cl[o]] += 1
        elif ev[0] == "advance":
            if self.t < self.T:
                self.o.end_tick()
            self.t += 1
        else:
            _, veh, tgt, arr, counted = ev
            if arr is None and counted:
                self.o.dispatch(veh, tgt)
            else:
                self.o.dispatch_at(veh, tgt, arrive_min=arr, counted=counted)

    def idle(self, cl):
        L = self.o.lists()
        return L["idle_veh"][L["idle_off"][cl]:L["idle_off"][cl + 1]]


class OracleEnv:
    """The surface of ``BatchedDispatchEnv`` that the runner uses, on CPU oracles.  ``fault``: one of FAULTS, or None."""
    fault = None

    def __init__(self, cost, node2cluster, nbr_off, nbr_idx, *, replicas, vehicles, depth_limit=0, neighbor_can_server=False, tick_minutes=10,
                 reject_threshold=600_000_000_000, idle_cap=0, **unused):
        self.cost, self.n2c, self.off, self.idx = np.asarray(cost), np.asarray(node2cluster), nbr_off, nbr_idx
        self.R, self.V, self.C, self.N = int(replicas), int(vehicles), len(nbr_off) - 1, self.cost.shape[0]
        self.okw = dict(tick_minutes=tick_minutes, reject_threshold=reject_threshold)
        self.depth, self.nbr = depth_limit, neighbor_can_server
        self.cap_auto, self.cap = idle_cap <= 0, _up(idle_cap, 64) if idle_cap > 0 else 64
        self.days, self.rd, self.reps, self.init = None, None, None, None
        self.prev_days = None
        self.t, self.stepped, self.T = 0, False, 0
        self.snap, self.err = None, False
        self.blocks = {}
        self.cap_changed = False
        self.veh_stale = False

    def oracle(self, day):
        return Oracle(self.cost, self.n2c, self.off, self.idx, self.depth, self.nbr, day[0], day[1], day[2], self.V, **self.okw)

    def to_device(self, a):
        return np.array(a)

    def close(self):
        self.reps = None

    # ---- loads ----------------------------------------------------------------------------------------------------------------
    def _loaded(self, days, rd, keep_snapshot=False):
        if self.days is not None and self.reps is not None:
            self.prev_days = (self.days, self.rd)
        self.days, self.rd, self.reps = days, np.array(rd, dtype=np.int32), None
        self.blocks.pop("veh", None)        # (the planes block lives with the state tables)
        self.T = max(self.oracle(days[d]).num_ticks for d in set(self.rd.tolist()))
        if not keep_snapshot:
            self.snap = None

    def load_orders(self, rel, pick, dele):
        self._loaded([(np.asarray(rel), np.asarray(pick), np.asarray(dele))], np.zeros(self.R, dtype=np.int32))

    def load_order_days(self, days, replica_day=None):
        rd = np.arange(self.R) * len(days) // self.R if replica_day is None else replica_day
        self._loaded([tuple(np.asarray(x) for x in d) for d in days], rd)

    def set_replica_days(self, replica_day):
        self._loaded(self.days, replica_day, keep_snapshot=self.fault == "snapshot_survives_map")

    def replica_ticks(self, r):
        d = self.days[self.rd[r]]
        return self.oracle(d).num_ticks, d[0].size

    def set_idle_cap(self, cap):
        new = min(_up(cap, 64), _up(max(self.V, 1), 64))
        if new != self.cap:
            self.cap, self.snap = new, None
        self.cap_changed = True

    @property
    def idle_cap(self):
        return self.cap

    # ---- episode --------------------------------------------------------------------------------------------------------------
    def _reset(self, init):
        self.init = np.array(init, dtype=np.int32).reshape(self.R, self.V)
        if self.cap_auto and self.V:
            fullest = max(int(np.bincount(self.n2c[row], minlength=self.C).max()) for row in self.init)
            want = min(_up(self.V, 64), _up(2 * fullest + 64, 64))
            if want > self.cap:
                self.cap, self.snap = want, None
        self._start(self.init)

    def _start(self, init):
        self.reps = [_Rep(self, init[r], self.days[self.rd[r]]) for r in range(self.R)]
        self.t, self.stepped, self.err = 0, False, False
        self.stale_run = self.fault == "stale_run" and self.prev_days is not None

    def reset(self, init):
        self._reset(init)
        self.cap_changed = False

    def reset_random(self, seeds):
        init = np.zeros((self.R, self.V), dtype=np.int32)
        for r, s in enumerate(seeds):
            g = random.Random(int(s))
            for v in range(self.V):
                node = g.choice(range(self.N))
                while self.n2c[node] < 0:
                    node = g.choice(range(self.N))
                init[r, v] = node
        self._reset(init)
        self.cap_changed = False

    def reset_again(self):
        init = self.init
        if self.fault == "stale_cluster_list" and self.cap_changed and self.reps is not None and self.V:
            init = init.copy()          # the vehicles that stood idle in cluster 0 stay where they stood
            for r, rep in enumerate(self.reps):
                veh = rep.idle(0)
                init[r, veh] = rep.o.vehicles()["loc"][veh]
        self.cap_changed = False
        self._start(init)

    def _all(self, ev):
        for rep in self.reps:
            rep.apply(ev)

    def step(self):
        assert not self.stepped and self.t < self.T
        self._all(("step",))
        self.stepped, self.veh_stale = True, False

    def advance(self):
        assert self.stepped
        self._all(("advance",))
        self.t, self.stepped, self.veh_stale = self.t + 1, False, False

    def run(self, n):
        if self.stale_run:              # the day graph of before the load: the previous day's orders
            days, rd = self.prev_days
            if len(rd) == self.R:
                for r, rep in enumerate(self.reps):
                    fresh = _Rep(self, rep.init, days[rd[r] % len(days)])
                    for ev in rep.log:
                        fresh.apply(ev)
                    self.reps[r] = fresh
            self.stale_run = False
        for _ in range(n):
            self.step()
            self.advance()

    def apply_dispatch(self, replica, from_cluster, idle_pos, target_node, arrive_min=None, counted=None):
        assert self.stepped
        todo = {}
        for i, (r, cl, pos, tgt) in enumerate(zip(replica, from_cluster, idle_pos, target_node)):
            veh = int(self.reps[r].idle(cl)[pos])
            todo.setdefault(r, []).append((veh, int(tgt), None if arrive_min is None else int(arrive_min[i]), True if counted is None else bool(counted[i])))
        for r, acts in todo.items():      # (one hook body per replica: the oracle takes one counted flag per body)
            assert len({a[3] for a in acts}) == 1
            arr = None if acts[0][2] is None else [a[2] for a in acts]
            self.reps[r].apply(("dispatch", [a[0] for a in acts], [a[1] for a in acts], arr, acts[0][3]))

    def _device_actions(self, r, acts):
        """One hook body of replica r from its [K, 3] actions: the documented refusals raise the sticky error and are skipped."""
        rep = self.reps[r]
        live = [k for k in range(len(acts)) if acts[k][0] >= 0]
        if not live:
            return
        if rep.t >= rep.T:
            self.err = True
            return
        L = rep.o.lists()
        seen, veh, tgt = set(), [], []
        for k in live:
            cl, pos, tg = (int(x) for x in acts[k])
            if cl >= self.C or tg < 0 or tg >= self.N or self.n2c[tg] < 0 or (cl, pos) in seen or pos < 0 or pos >= L["idle_off"][cl + 1] - L["idle_off"][cl]:
                self.err = True
                continue
            seen.add((cl, pos))
            veh.append(int(L["idle_veh"][L["idle_off"][cl] + pos])); tgt.append(tg)
        if veh:
            rep.apply(("dispatch", veh, tgt, None, True))

    def apply_dispatch_torch(self, actions):
        assert self.stepped
        acts = np.array(actions)
        if self.fault == "drop_last_action":
            rows = [r for r in range(self.R) if (acts[r, :, 0] >= 0).any()]
            if rows:
                acts[rows[-1], np.flatnonzero(acts[rows[-1], :, 0] >= 0)[-1], 0] = -1
        for r in range(self.R):
            self._device_actions(r, acts[r])

    def _vehicle_row(self, r, row):
        """One replica's row of a vehicle-form call (include/vds.h): the idle vehicles with a valid target, ascending, as one hook body."""
        rep = self.reps[r]
        L = rep.o.lists()
        idle = np.zeros(self.V, dtype=bool)
        idle[L["idle_veh"][:L["idle_off"][-1]]] = True
        want = np.flatnonzero(idle & (row >= 0))
        if not want.size:
            return
        over = rep.t >= rep.T
        good = [v for v in want if not over and row[v] < self.N and self.n2c[row[v]] >= 0]
        if len(good) < want.size:
            self.err = True
            if self.fault == "veh_refused_applied":     # the day is over, or the node is beyond the city: moved all the same (to node % N)
                good = [v for v in want if self.n2c[row[v] % self.N] >= 0]
        veh, tgt = [int(v) for v in good], [int(row[v] % self.N) for v in good]
        if not veh:
            return
        if self.fault == "veh_descending":
            veh, tgt = veh[::-1], tgt[::-1]
        ev = ("dispatch", veh, tgt, None, True)
        first = max(i for i, e in enumerate(rep.log) if e[0] == "step") + 1      # the slot's earlier dispatch calls: rep.log[first:]
        if self.fault == "veh_before_kform" and len(rep.log) > first:
            fresh = _Rep(self, rep.init, rep.day)
            for e in rep.log[:first] + [ev] + rep.log[first:]:
                fresh.apply(e)
            self.reps[r] = fresh
        else:
            rep.apply(ev)

    def apply_dispatch_vehicles_torch(self, targets):
        assert self.stepped
        tg = np.array(targets)
        assert tg.shape == (self.R, self.V) and tg.dtype == np.int32
        rows = np.arange(self.R)
        if self.fault == "veh_stored_replica" and len(set(self.rd.tolist())) > 1:      # stored by day: replica order[i] reads row i
            order = np.argsort(self.rd, kind="stable")
            rows = np.empty(self.R, dtype=np.int64)
            rows[order] = np.arange(self.R)
        for r in range(self.R):
            self._vehicle_row(r, tg[rows[r]])

    def run_hooked(self, n, actions=None, idle_pre=True, idle_now=True, supply=True, cl_orders=True, inflight=False, outcomes=False, idle_heads=0,
                   vehicle_planes=None, vehicle_targets=None):
        assert not self.stepped and self.t + n <= self.T
        for k in range(n):
            self.step()
            if k == n - 1:
                self.obs_torch(inflight=inflight, idle_pre=idle_pre, idle_now=idle_now, supply=supply, cl_orders=cl_orders)
                if outcomes:
                    self.outcomes_torch()
                if idle_heads:
                    self.idle_heads_torch(idle_heads)
                if vehicle_planes:
                    self.vehicles_torch(**{name: bool(vehicle_planes >> i & 1) for i, name in enumerate(api_script.VEH_PLANES)})
            if actions is not None:
                for r in range(self.R):
                    self._device_actions(r, np.asarray(actions)[r])
            if vehicle_targets is not None:
                self.apply_dispatch_vehicles_torch(vehicle_targets)
            self.advance()

    def set_run_groups(self, groups=0, stagger=-1):
        pass

    def sync(self):
        if self.err:
            self.err = False
            raise Exception("libvds error -4: dispatch of an idle position that does not exist (or listed twice); the action was skipped")

    @property
    def clock(self):
        return self.t, self.reps[0].o.now_min

    # ---- snapshot -------------------------------------------------------------------------------------------------------------
    def snapshot(self):
        self.snap = dict(rows=[(rep.init, rep.day, list(rep.log)) for rep in self.reps], t=self.t, stepped=self.stepped, rd=self.rd.copy())

    def snapshot_info(self):
        return None if self.snap is None else dict(step=self.snap["t"], stepped=self.snap["stepped"], bytes=1)

    def drop_snapshot(self):
        self.snap = None

    def restore(self, src=None):
        if self.snap is None:
            raise Exception("libvds error -4: vds_restore: no snapshot")
        src = list(range(self.R)) if src is None else [int(s) for s in src]
        for r, s in enumerate(src):
            if s < 0 or s >= self.R:
                raise Exception("libvds error -1: vds_restore: replica %d is mapped to replica %d" % (r, s))
            if self.rd[r] != self.rd[s]:
                raise Exception("libvds error -1: vds_restore: order days per replica: replica %d and %d replay different days" % (r, s))
        if self.fault == "restore_source" and self.R > 1 and self.rd[0] == self.rd[1]:
            src[1] = src[0]
        reps = []
        for s in src:
            init, day, log = self.snap["rows"][s]
            rep = _Rep(self, init, day)
            for ev in log:
                rep.apply(ev)
            reps.append(rep)
        self.reps, self.t, self.stepped, self.err = reps, self.snap["t"], self.snap["stepped"], False
        self.veh_stale = self.fault == "veh_block_stale_restore"

    def restore_torch(self, src):
        if self.snap is None:
            raise Exception("libvds error -4: vds_restore_device: no snapshot")
        if len(self.days) > 1:
            raise Exception("libvds error -4: vds_restore_device: order days per replica")
        self.restore(np.asarray(src))

    # ---- reads ----------------------------------------------------------------------------------------------------------------
    def obs(self):
        out = {k: np.zeros((self.R, self.C), dtype=np.int32) for k in api_script.PLANES}
        for r, rep in enumerate(self.reps):
            oo = rep.o.obs()
            for k in out:
                out[k][r] = oo[k]
        return out

    def obs_torch(self, inflight=True, idle_pre=True, idle_now=True, supply=True, cl_orders=True):
        blk = self.blocks.setdefault("obs", np.zeros((5, self.R, self.C), dtype=np.int32))
        ob = self.obs()
        for i, (k, on) in enumerate(zip(api_script.PLANES, (idle_pre, idle_now, supply, cl_orders, inflight))):
            if on:
                blk[i] = ob[k]
        return blk

    def obs_inplace_torch(self):
        if self.reps is None:           # (the views exist from the load on; they are read after a reset)
            return {k: np.zeros((self.R, self.C), dtype=np.int32) for k in ("idle_pre", "idle_now", "cl_orders")}
        ob = self.obs()
        return {k: ob[k] for k in ("idle_pre", "idle_now", "cl_orders")}

    def supply_inplace_torch(self):
        raise Exception("libvds error -4: vds_supply_inplace: SupplyExpect is kept in place on the dense layout only")

    def counters(self):
        return np.array([[rep.o.counters()[k] for k in api_script.COUNTERS] for rep in self.reps], dtype=np.int64)

    def total_counters(self):
        return self.counters().sum(axis=0)

    def orders(self):
        O = max(d[0].size for d in self.days)
        out = dict(status=np.zeros((self.R, O), np.uint8), vehicle=np.zeros((self.R, O), np.int32), wait=np.zeros((self.R, O), np.int32))
        for r, rep in enumerate(self.reps):
            res = rep.o.orders()
            for k in out:
                out[k][r, :res[k].size] = res[k]
        return out

    def lists(self, r):
        o = self.reps[r].o
        L, veh = o.lists(), o.vehicles()
        n, na = L["idle_off"][-1], L["arr_off"][-1]
        out = dict(L, idle_node=np.full(self.V, -1, np.int32), arr_order=np.full(self.V, -1, np.int32), arr_node=np.full(self.V, -1, np.int32))
        out["idle_node"][:n] = veh["loc"][L["idle_veh"][:n]]
        out["arr_order"][:na] = veh["order"][L["arr_veh"][:na]]
        out["arr_node"][:na] = veh["dest"][L["arr_veh"][:na]]
        return out

    def vehicles(self, r):
        o = self.reps[r].o
        L, veh = o.lists(), o.vehicles()
        n, na = L["idle_off"][-1], L["arr_off"][-1]
        fly = L["arr_veh"][:na]
        state = np.zeros(self.V, np.uint8)
        state[fly] = np.where(veh["order"][fly] >= 0, 1, 2)
        node, order, arrive = veh["loc"].copy(), np.full(self.V, -1, np.int32), np.full(self.V, -1, np.int32)
        node[fly], order[fly], arrive[fly] = veh["dest"][fly], veh["order"][fly], L["arr_min"][:na]
        return dict(state=state, node=node, cluster=self.n2c[node], arrive_min=arrive, order=order)

    def vehicles_torch(self, state=True, node=True, cluster=True, arrive_min=True, order=True, source=False):
        """Views of the int32 [6, R, V] block: the wanted planes refreshed, the others keep what the block held."""
        blk = self.blocks.setdefault("veh", np.full((6, self.R, self.V), -1, dtype=np.int32))
        want = (state, node, cluster, arrive_min, order, source)
        stale, self.veh_stale = self.veh_stale, False
        for r in range(self.R):
            W = self.vehicles(r)
            src = np.where(W["state"] == 0, 0, 2)
            for i, name in enumerate(api_script.VEH_PLANES):
                if (want[i] or self.fault == "veh_unrequested_written") and not stale:
                    blk[i, r] = src if name == "source" else W[name]
        return {name: blk[i] for i, name in enumerate(api_script.VEH_PLANES) if want[i]}

    def vehicles_all(self, **planes):
        return {k: v.copy() for k, v in self.vehicles_torch(**planes).items()}

    def idle_heads_torch(self, L):
        blk = self.blocks.setdefault(("heads", L), np.zeros((2, self.R, self.C, L), dtype=np.int32))
        blk[:] = -1
        for r, rep in enumerate(self.reps):
            loc = rep.o.vehicles()["loc"]
            for cl in range(self.C):
                veh = rep.idle(cl)[:L]
                blk[0, r, cl, :veh.size], blk[1, r, cl, :veh.size] = veh, loc[veh]
        return blk

    def idle_heads(self, L):
        blk = self.idle_heads_torch(L)
        return dict(veh=blk[0].copy(), node=blk[1].copy())

    def outcomes_torch(self):
        blk = self.blocks.setdefault("outc", np.zeros((4, self.R, self.C), dtype=np.int64))
        for r, rep in enumerate(self.reps):
            blk[:, r, :] = rep.outc
        return blk

    def outcomes(self):
        blk = self.outcomes_torch()
        return {k: blk[i].copy() for i, k in enumerate(("served", "rejected", "wait_sum", "value_sum"))}

    def main_kernel(self):
        return "oracle"

    def layout(self):
        return dict(dense=-1, dense_st=-1)


def faulty(name):
    return type("OracleEnv_" + name, (OracleEnv,), dict(fault=name))


def corpus_seeds():
    single, pairs = api_script.corpus()
    return list(single) + [s for p in pairs for s in p]


@functools.lru_cache(maxsize=None)
def corpus_stats():
    """Every script of the GPU corpus on the stand-in engine, once: the statistics of what they covered."""
    stats = new_stats()
    for seed in corpus_seeds():
        run_script(OracleEnv, seed, stats=stats)
    return stats


def test_every_script_of_the_corpus_is_green_on_the_stand_in_engine():
    st = corpus_stats()
    assert len(st["calls"]) == len(corpus_seeds())
    assert min(st["calls"]) >= 40, "a script of %d calls" % min(st["calls"])


def test_every_operation_kind_occurs_ten_times():
    st = corpus_stats()
    short = {k: st["kinds"].get(k, 0) for k in KINDS if st["kinds"].get(k, 0) < 10}
    assert not short, short


def test_every_legal_ordered_pair_of_state_moving_calls_occurs_twice():
    """Consecutive state-moving calls, reads ignored (a slot's step / dispatch / advance calls are ONE step-loop).  Of the 169 pairs,
    19 are left out because include/vds.h makes them illegal (api_script.legal_pair): an episode call or a snapshot before the reset
    that a load, another map or another idle capacity requires (16), and reset_again when the start nodes may be gone (3)."""
    st = corpus_stats()
    short = {(a, b): st["pairs"].get((a, b), 0) for a in MOVERS for b in MOVERS if legal_pair(a, b) and st["pairs"].get((a, b), 0) < 2}
    assert not short, short
    assert not [p for p in st["pairs"] if not legal_pair(*p)], "an illegal pair was drawn"


def test_restores_cover_every_validity_state():
    st = corpus_stats()
    assert st["restores"] >= 40
    assert 4 * st["restores_unknown"] <= st["restores"], (st["restores_unknown"], st["restores"])
    assert st["restores_unknown"] >= 1 and st["restores_void"] >= 1 and st["restore_after_dispatch"] >= 1
    assert st["restores_valid_ok"] == st["restores_valid"]


def test_thin_spots_of_the_corpus_have_floors():
    """Both refused forms of a device action, eager runs, the plain rollback, both refused maps, and slot-by-slot progress: dispatch
    calls and advances, on which the dispatch sequence numbers and a restore behind a dispatch depend."""
    st = corpus_stats()
    k = st["kinds"]
    assert st["refused_length"] >= 5 and st["refused_twice"] >= 5, (st["refused_length"], st["refused_twice"])
    assert st["run_eager"] >= 15, st["run_eager"]
    assert st["restore_none_ok"] >= 8, st["restore_none_ok"]
    assert st["refused_map_range"] >= 3 and st["refused_map_day"] >= 3, (st["refused_map_range"], st["refused_map_day"])
    assert st["restore_after_dispatch"] >= 5, st["restore_after_dispatch"]
    dispatches = k["dispatch_host"] + k["dispatch_ex"] + k["dispatch_dev"]
    assert min(k["dispatch_host"], k["dispatch_ex"], k["dispatch_dev"]) >= 30, dispatches       # (each form in most scripts)
    assert k["advance"] >= 2 * len(st["calls"]), k["advance"]                                    # (two closed slots per script on average)
    loads = k["load_orders"] + k["load_order_days"] + k["set_replica_days"]
    assert 2 * dispatches >= loads, (dispatches, loads)
    assert 2 * st["restores_void"] <= st["restores"], (st["restores_void"], st["restores"])


def test_the_vehicle_form_and_the_planes_block_have_floors():
    """The per-vehicle dispatch like the other forms, each of its refusals, a restore right behind it; hooked days with vehicle
    targets applied and refused, called again with the same tensors on the same tables and behind a table change; a device read of
    some planes behind one of all six (what the other planes keep is then known)."""
    st = corpus_stats()
    assert st["kinds"]["dispatch_vehicles"] >= 30, st["kinds"]["dispatch_vehicles"]
    refused = {k: st["refused_veh_" + k] for k in api_script.VEH_REFUSALS}
    assert min(refused.values()) >= 5, refused
    assert st["restore_after_vehicle_dispatch"] >= 3, st["restore_after_vehicle_dispatch"]
    assert st["hook_veh_applied"] >= 10 and st["hook_veh_refused"] >= 10, (st["hook_veh_applied"], st["hook_veh_refused"])
    assert st["hook_veh_same"] >= 3 and st["hook_veh_after_change"] >= 3, (st["hook_veh_same"], st["hook_veh_after_change"])
    assert st["veh_partial_behind_full"] >= 5, st["veh_partial_behind_full"]


def test_hooked_actions_are_applied_and_refused():
    st = corpus_stats()
    assert st["hook_applied"] >= 10 and st["hook_refused"] >= 10, (st["hook_applied"], st["hook_refused"])


def test_day_graphs_come_back_at_the_same_slot_at_another_and_after_a_table_change():
    """``run`` of 8 slots and more with the count of the graph run before: at the same first slot (a replay), at another one, and
    after a load, another map, another idle capacity or other run groups (rebuilt, or updated in place)."""
    st = corpus_stats()
    assert st["run_same"] >= 5 and st["run_moved"] >= 5 and st["run_after_change"] >= 5, (st["run_same"], st["run_moved"], st["run_after_change"])


@pytest.mark.parametrize("fault", FAULTS)
def test_a_seeded_fault_turns_a_script_red(fault):
    env = faulty(fault)
    red = None
    for seed in corpus_seeds():
        try:
            run_script(env, seed)
        except ScriptFailure as e:
            red = (seed, str(e))
            break
    assert red is not None, "no script of the corpus notices the fault %r" % fault
    assert "API script of seed %d failed at call" % red[0] in red[1] and "run_script(env_factory, %d, upto=" % red[0] in red[1]
    print("fault %s: seed %d is red: %s" % (fault, red[0], red[1].splitlines()[0]))


def test_a_prefix_replays_the_same_calls():
    seed = corpus_seeds()[3]
    whole = run_script(OracleEnv, seed)
    part = run_script(OracleEnv, seed, upto=20)
    assert part.n_calls == 20 and [l for l in part.log if not l.startswith("    --")] == [l for l in whole.log if not l.startswith("    --")][:20]


RECORDED_READS = ("clock", "snapshot_info", "obs", "counters", "orders", "outcomes", "idle_heads", "lists[0]", "vehicles[0]", "obs_torch",
                  "obs_inplace_torch", "outcomes_torch", "idle_heads_torch", "vehicles_all", "vehicles_torch")


@pytest.mark.parametrize("seed", corpus_seeds()[:3])
def test_a_recorded_script_is_deterministic_and_draws_the_same_calls(seed):
    """``record=`` on the stand-in engine: two runs give the same transcript, every read entry point is in it after every call that
    leaves an episode to read, and the calls are those of the unrecorded script (recording draws nothing from the generator)."""
    one, two = [], []
    a = run_script(OracleEnv, seed, record=one)
    b = run_script(OracleEnv, seed, record=two)
    plain = run_script(OracleEnv, seed)
    assert one and one == two
    assert a.log == plain.log == b.log and a.n_calls == plain.n_calls
    calls = {}
    for line in one:
        n, kind, name, dig = line.split()
        calls.setdefault(int(n), set()).add(name)
        assert len(dig) == 16
    assert len(calls) >= 30, len(calls)
    R = a.c.R
    for n, names in calls.items():
        assert set(RECORDED_READS) <= names and "lists[%d]" % (R - 1) in names and "vehicles[%d]" % (R - 1) in names, (n, sorted(names))
    # a digest covers every element: one changed value, another digest
    x = np.arange(12, dtype=np.int32).reshape(3, 4)
    y = x.copy()
    y[2, 3] += 1
    assert api_script.digest(dict(a=x)) != api_script.digest(dict(a=y)) and api_script.digest(x) != api_script.digest(x.reshape(4, 3))
