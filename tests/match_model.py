"""TEST INFRASTRUCTURE: a pure-Python model of one city replica whose matches come from outside - the loop of
``vds_apply_match_device`` (include/vds.h) over plain lists and dicts: Update (simulator.py:1006-1024), the commit of a
``MatchFunction`` override that keeps the reference's bookkeeping (:912-973 with the search replaced), SupplyExpect (:880-891) and
the body of a ``DispatchFunction`` (oracle/vds_oracle.c: vds_oracle_dispatch).  Pinned to the unmodified reference by
tests/golden/matchpack_0.npz (tests/golden/make_match_golden.py, tests/test_match_model.py); the GPU tests compare the engine with it.
The getters have the shapes of ``oracle.oracle.Oracle``'s, so the helpers written for the oracle take a model as well."""
from __future__ import annotations

import numpy as np


class MatchModel:
    def __init__(self, cost, node2cluster, C, V, o_release_min, o_pickup, o_delivery, tick_minutes=10, fleet=None):
        self.cost = np.asarray(cost)
        self.n2c = [int(x) for x in node2cluster]
        self.C, self.V, self.tick = int(C), int(V), int(tick_minutes)
        self.fleet = self.V if fleet is None else int(fleet)      # vehicles 0 .. fleet - 1 exist (vds_set_fleet)
        self.rel = [int(x) for x in o_release_min]
        self.pick = [int(x) for x in o_pickup]
        self.dele = [int(x) for x in o_delivery]
        self.O = len(self.rel)
        self.value = [self.road_cost(p, d) for p, d in zip(self.pick, self.dele)]     # :341-342

    def road_cost(self, start, end):            # :263-264
        return int(self.cost[end, start])

    @property
    def num_ticks(self):                        # :1037-1048
        if self.O == 0:
            return 0
        return (self.rel[-1] + 3 * self.tick - (self.rel[0] - self.tick)) // self.tick + 1

    def reset(self, veh_node):
        self.idle = [[] for _ in range(self.C)]
        self.arr = [dict() for _ in range(self.C)]              # vehicle -> arrival minute, insertion ordered
        self.loc = [-1] * self.V
        self.cluster = [-1] * self.V
        self.dest = [-1] * self.V
        self.order = [-1] * self.V
        for v in range(self.fleet):
            n = int(veh_node[v])
            self.loc[v], self.cluster[v] = n, self.n2c[n]
            self.idle[self.n2c[n]].append(v)
        self.o_status = [0] * self.O
        self.o_vehicle = [-1] * self.O
        self.o_wait = [-1] * self.O
        self.order_num = self.reject_num = self.wait_sum = self.dispatch_num = self.dispatch_cost = 0
        self.now = (self.rel[0] if self.O else 0) - self.tick
        self.step = 0
        self.cur = 0
        self.idle_pre = [len(x) for x in self.idle]
        self.cl_orders = [0] * self.C
        self.supply = [0] * self.C
        self.slot_results = {}                  # vehicle -> (order, wait, value, pickup) of the slot matched last

    # ---- one slot: update() -> slot_orders() -> match(row) -> dispatch(...)* -> end_tick()
    def update(self):
        for c in range(self.C):
            self.cl_orders[c] = 0
            for v, t in list(self.arr[c].items()):
                if t <= self.now:
                    self.loc[v], self.dest[v], self.cluster[v], self.order[v] = self.dest[v], -1, c, -1
                    self.idle[c].append(v)
                    del self.arr[c][v]
        self.idle_pre = [len(x) for x in self.idle]

    def slot_orders(self):
        """ids the cursor processes in this slot (quirk Q1: the day's last order is never processed)."""
        ids, k = [], self.cur
        while self.rel[k] < self.now + self.tick and k != self.O - 1:
            ids.append(k)
            k += 1
        return ids

    def match(self, row):
        """row[j]: the vehicle of the slot's j-th order (None: every order rejected).  Returns entries >= V (the sticky error)."""
        named, beyond = set(), 0
        self.slot_results = {}
        for j, o in enumerate(self.slot_orders()):
            self.order_num += 1
            self.cl_orders[self.n2c[self.pick[o]]] += 1
            v = -1 if row is None else int(row[j])
            if v >= self.V:
                beyond += 1
            ok = 0 <= v < self.V and v not in named and self.dest[v] < 0 and self.cluster[v] >= 0 and v in self.idle[self.cluster[v]]
            if 0 <= v < self.V:
                named.add(v)
            if ok:
                wait = self.road_cost(self.loc[v], self.pick[o])
                self.o_wait[o], self.o_vehicle[o], self.o_status[o] = wait, v, 1
                self.wait_sum += wait
                self.order[v], self.dest[v] = o, self.dele[o]
                self.arr[self.n2c[self.dele[o]]][v] = self.now + wait + self.value[o]
                self.idle[self.cluster[v]].remove(v)
                self.slot_results[v] = (o, wait, self.value[o], self.pick[o])
            else:
                self.reject_num += 1
                self.o_status[o] = 2
            self.cur = o + 1
        self.supply = [sum(1 for v, t in self.arr[c].items() if t <= self.now + self.tick and self.order[v] >= 0) for c in range(self.C)]
        return beyond

    def dispatch(self, veh, target_node):
        for v, t in zip(veh, target_node):
            v, t = int(v), int(t)
            assert self.dest[v] < 0 and v in self.idle[self.cluster[v]] and self.n2c[t] >= 0
            c = self.road_cost(self.loc[v], t)
            self.idle[self.cluster[v]].remove(v)
            self.dest[v] = t
            self.arr[self.n2c[t]][v] = self.now + c
            self.dispatch_num += 1
            self.dispatch_cost += c

    def end_tick(self):
        self.step += 1
        self.now += self.tick

    # ---- getters in the oracle's shapes
    def counters(self):
        return dict(order_num=self.order_num, reject_num=self.reject_num, matched=sum(1 for s in self.o_status if s == 1),
                    wait_sum=self.wait_sum, dispatch_num=self.dispatch_num, dispatch_cost=self.dispatch_cost,
                    sum_order_value=sum(v for v, s in zip(self.value, self.o_status) if s != 2), evals=0)

    def obs(self):
        a = lambda x: np.asarray(x, dtype=np.int32)
        return dict(idle_pre=a(self.idle_pre), supply=a(self.supply), cl_orders=a(self.cl_orders),
                    idle_now=a([len(x) for x in self.idle]), inflight=a([len(x) for x in self.arr]))

    def orders(self):
        return dict(status=np.asarray(self.o_status, dtype=np.uint8), vehicle=np.asarray(self.o_vehicle, dtype=np.int32),
                    wait=np.asarray(self.o_wait, dtype=np.int32), value=np.asarray(self.value, dtype=np.int32))

    def vehicles(self):
        a = lambda x: np.asarray(x, dtype=np.int32)
        return dict(loc=a(self.loc), cluster=a(self.cluster), dest=a(self.dest), order=a(self.order))

    def lists(self):
        idle_off, arr_off = np.zeros(self.C + 1, dtype=np.int32), np.zeros(self.C + 1, dtype=np.int32)
        idle_veh, arr_veh, arr_min = (np.full(self.V, -1, dtype=np.int32) for _ in range(3))
        a = b = 0
        for c in range(self.C):
            for v in self.idle[c]:
                idle_veh[a] = v; a += 1
            for v, t in self.arr[c].items():
                arr_veh[b], arr_min[b] = v, t; b += 1
            idle_off[c + 1], arr_off[c + 1] = a, b
        return dict(idle_off=idle_off, idle_veh=idle_veh, arr_off=arr_off, arr_veh=arr_veh, arr_min=arr_min)


def last_or_lowest(model, ids):
    """The matcher of the fixture (tests/golden/make_match_golden.py), on the model's containers: the last vehicle of the pickup
    cluster's idle list, else the first idle vehicle of the lowest-numbered cluster that has one, else nobody - decided order by order,
    with the vehicles the slot's earlier orders took gone."""
    idle = [list(x) for x in model.idle]
    row = []
    for o in ids:
        pc = model.n2c[model.pick[o]]
        src = pc if idle[pc] else next((c for c in range(model.C) if idle[c]), -1)
        if src < 0:
            row.append(-1)
        else:
            row.append(idle[src].pop(-1 if src == pc else 0))
    return row
