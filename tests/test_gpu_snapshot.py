"""vds_snapshot / vds_restore / vds_restore_device: the episode state saved at a slot and copied back through a replica map
(rollback, per-replica forking), against the CPU oracle.  The oracle cannot be cloned, so every replica is a LINEAGE - start nodes plus
the dispatches of every slot - and the oracle of a restored replica is a fresh one replayed on the lineage of the snapshot's source
replica.  Every tick family and both state layouts (test_gpu_parity.MODES), the capacity edges of the row copies, order days per
replica (regrouped storage), the hooked day, the snapshot's lifetime and its errors."""
import numpy as np
import pytest

from helpers import dispatch_by_tick, load_golden, make_oracle
from test_gpu_idle_heads import seeded_init
from test_gpu_parity import MODES, _applies, check_lists, make_env
from test_gpu_replica_days import mk_env, mk_oracle, synth_days

pytestmark = pytest.mark.gpu

BETWEEN, STEPPED, DISPATCHED = 0, 1, 2      # where in a slot a snapshot is taken: before its step, after it, after its dispatch calls


class Line:
    """One replica's lineage and the oracle that stands where the replica stands: start nodes, the order day, the dispatches of
    every slot so far.  ``hist`` (another line's ``history()``): replayed up to there."""

    def __init__(self, g, init, day=None, hist=None):
        self.g, self.init, self.day = g, np.array(init, dtype=np.int32), day
        self.o = make_oracle(g) if day is None else mk_oracle(g, day)
        self.o.reset(self.init)
        self.t, self.stepped, self.acts = 0, False, {}
        if hist is not None:
            t, stepped, acts = hist
            for s in range(t):
                self.step()
                for v, n in acts.get(s, ()):
                    self.dispatch(v, n)
                self.advance()
            if stepped:
                self.step()
                for v, n in acts.get(t, ()):
                    self.dispatch(v, n)

    @property
    def live(self):      # its SimCity loop has not ended (order days per replica: a shorter day stands still afterwards)
        return self.t < self.o.num_ticks

    def step(self):
        if self.live:
            self.o.begin_tick()
        self.stepped = True

    def dispatch(self, veh, tgt):
        self.o.dispatch(veh, tgt)
        self.acts.setdefault(self.t, []).append((np.array(veh), np.array(tgt)))

    def advance(self):
        if self.live:
            self.o.end_tick()
        self.t += 1
        self.stepped = False

    def run(self, n):
        for _ in range(n):
            self.step()
            self.advance()

    def history(self):
        return self.t, self.stepped, {k: list(v) for k, v in self.acts.items()}

    def fork(self, hist):
        return Line(self.g, self.init, self.day, hist)


def open_env(g, R, days=None, replica_day=None, **kw):
    """(env, in-place supply planes or None) for a MODES entry; ``days``: order days per replica."""
    kw = dict(kw)
    want_sup = kw.pop("supply_inplace", False)
    if days is None:
        env = make_env(g, R, **kw)
    else:
        env = mk_env(g, R, **kw)
        env.load_order_days(days, replica_day)
    sup = None
    if want_sup:
        try:
            sup = env.supply_inplace_torch()
        except Exception as e:      # (the library keeps the wide layout for this fixture)
            assert "dense layout only" in str(e), e
    return env, sup


def valid_nodes(g):
    return np.flatnonzero(np.asarray(g["node2cluster"]) >= 0)


def head_moves(g, lines, salt, reps=None):
    """One dispatch per replica, different for each: the head of its fullest idle list to a node of its own."""
    nodes = valid_nodes(g)
    mv = {}
    for r in (range(len(lines)) if reps is None else reps):
        if not lines[r].live:
            continue
        L = lines[r].o.lists()
        n = np.diff(L["idle_off"])
        if n.max() > 0:
            c = int(n.argmax())
            mv[r] = ([int(L["idle_veh"][L["idle_off"][c]])], [int(nodes[(5 * r + 3 * salt + 1) % nodes.size])])
    return mv


def apply_moves(env, lines, mv):
    """{replica: (vehicles, target nodes)} as one hook body per replica: list positions from the oracles' lists as they stand."""
    rep, cl, pos, tgt = [], [], [], []
    for r, (vehs, nodes) in mv.items():
        L = lines[r].o.lists()
        flat = L["idle_veh"][:L["idle_off"][-1]]
        for v, n in zip(vehs, nodes):
            i = int(np.flatnonzero(flat == v)[0])
            c = int(np.searchsorted(L["idle_off"], i, side="right")) - 1
            rep.append(r); cl.append(c); pos.append(i - int(L["idle_off"][c])); tgt.append(int(n))
    if rep:
        env.apply_dispatch(rep, cl, pos, tgt)
    for r, (vehs, nodes) in mv.items():
        lines[r].dispatch(vehs, nodes)


def fixture_moves(rows, R):
    rows = np.array(rows)
    return {r: (rows[:, 1].tolist(), rows[:, 4].tolist()) for r in range(R)}


def drive(env, lines, upto, disp=None, own_moves_from=None):
    """Slot by slot to the start of slot ``upto``: the fixture's dispatches (``disp``, every replica alike) and, from slot
    ``own_moves_from`` on, one dispatch of its own per replica."""
    while lines[0].t < upto:
        t = lines[0].t
        env.step()
        for ln in lines:
            ln.step()
        if disp and t in disp:
            apply_moves(env, lines, fixture_moves(disp[t], len(lines)))
        if own_moves_from is not None and t >= own_moves_from:
            apply_moves(env, lines, head_moves(lines[0].g, lines, t))
        env.advance()
        for ln in lines:
            ln.advance()


def diverge(env, g, n, stepped):
    """n more slots with dispatches no lineage has: every live replica moves the head of its fullest list, read from the engine."""
    nodes = valid_nodes(g)
    for k in range(n):
        if not stepped:
            env.step()
        stepped = False
        idle = env.obs()["idle_now"]
        t = env.clock[0]
        rep = [r for r in range(env.R) if idle[r].max() > 0 and env.replica_ticks(r)[0] > t]
        if rep:
            env.apply_dispatch(rep, [int(idle[r].argmax()) for r in rep], [0] * len(rep), [int(nodes[(11 * r + k + 2) % nodes.size]) for r in rep])
        env.advance()


def reads(env):
    env.sync()
    return dict(clock=env.clock, obs=env.obs(), counters=env.counters(), orders=env.orders(), heads=env.idle_heads(4), outcomes=env.outcomes())


def same_reads(got, seen, src):
    """Every read entry point answers as at the snapshot, replica r showing src[r]'s values."""
    src = np.asarray(src)
    assert got["clock"] == seen["clock"]
    np.testing.assert_array_equal(got["counters"], seen["counters"][src])
    for blk in ("obs", "orders", "heads", "outcomes"):
        for k in seen[blk]:
            np.testing.assert_array_equal(got[blk][k], seen[blk][k][src], err_msg="%s %s" % (blk, k))


def check_state(env, lines, what, sup=None):
    """Clock, observations, counters, container views and per-order results of every replica against its oracle."""
    env.sync()
    assert env.clock[0] == lines[0].t, what
    ob, cn, od = env.obs(), env.counters(), env.orders()
    for r, ln in enumerate(lines):
        oo, oc = ln.o.obs(), ln.o.counters()
        for i, k in enumerate(("order_num", "reject_num", "matched", "wait_sum", "dispatch_num", "dispatch_cost", "sum_order_value", "evals")):
            assert cn[r, i] == oc[k], (what, r, k, cn[r, i], oc[k])
        if ln.stepped and ln.live:
            for k in ("idle_pre", "idle_now", "supply", "cl_orders", "inflight"):
                np.testing.assert_array_equal(ob[k][r], oo[k], err_msg="%s replica %d obs %s" % (what, r, k))
        else:
            np.testing.assert_array_equal(ob["idle_now"][r], oo["idle_now"], err_msg="%s replica %d idle_now" % (what, r))
            np.testing.assert_array_equal(ob["inflight"][r], oo["inflight"], err_msg="%s replica %d inflight" % (what, r))
        check_lists(env, r, ln.o, ln.t)
        res = ln.o.orders()
        n = res["status"].size
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(od[k][r][:n], res[k], err_msg="%s replica %d orders %s" % (what, r, k))
    if sup is not None and lines[0].stepped:
        ring, slot = sup
        np.testing.assert_array_equal(ring[int(slot.item())].cpu().numpy(), ob["supply"], err_msg="%s supply in place" % what)


def coverage(lines):
    """(vehicles in flight, of them dispatched, longest idle list) over the oracles' lists."""
    fly = disp = longest = 0
    for ln in lines:
        L, veh = ln.o.lists(), ln.o.vehicles()
        na = int(L["arr_off"][-1])
        fly = max(fly, na)
        disp = max(disp, int((veh["order"][L["arr_veh"][:na]] < 0).sum()))
        longest = max(longest, int(np.diff(L["idle_off"]).max()))
    return fly, disp, longest


def finish_day(env, lines, disp=None, stepwise=False):
    """From wherever the lines stand to the end of the day: the open slot is closed (with the fixture's dispatches of that slot if
    they were not applied yet), the rest stepwise with the fixture's dispatches or as one ``run`` (the day graph from 8 slots on)."""
    T = env.T
    if lines[0].stepped:
        t = lines[0].t
        if disp and t in disp and t not in lines[0].acts:
            apply_moves(env, lines, fixture_moves(disp[t], len(lines)))
        env.advance()
        for ln in lines:
            ln.advance()
    if disp or stepwise:
        drive(env, lines, T, disp)
    else:
        env.run(T - lines[0].t)
        for ln in lines:
            ln.run(T - ln.t)


def snapshot_at(env, lines, g, pos, disp=None):
    """Brings the open slot to ``pos`` and takes the snapshot; returns (histories, reads at the snapshot)."""
    if pos >= STEPPED:
        env.step()
        for ln in lines:
            ln.step()
    if pos == DISPATCHED:
        t = lines[0].t
        apply_moves(env, lines, fixture_moves(disp[t], len(lines)) if disp and t in disp else head_moves(g, lines, t))
        assert lines[0].acts.get(t), "no dispatch in the snapshot's slot"
    env.snapshot()
    info = env.snapshot_info()
    assert info["step"] == lines[0].t and info["stepped"] == (pos >= STEPPED) and info["bytes"] > 0
    return [ln.history() for ln in lines], reads(env)


# ---- 1. rollback: tiny_dispatch, slot 49, with the fixture's dispatches; the snapshot at each of the three positions
@pytest.mark.parametrize("pos", [BETWEEN, STEPPED, DISPATCHED])
def test_rollback_restores_slot_49_and_the_day_finishes_as_the_oracle(pos):
    g = load_golden("tiny_dispatch")
    R, t0 = 3, 49
    disp = dispatch_by_tick(g)
    if pos == DISPATCHED:       # (behind the fixture's own dispatch calls: the last slot up to 49 that has some - a dispatch the fixture
        t0 = max(t for t in disp if t <= 49)      # does not have would take a vehicle that its later dispatches move)
    init = np.tile(g["veh_node"], (R, 1)).astype(np.int32)
    env, _ = open_env(g, R)
    env.reset(init)
    lines = [Line(g, init[r]) for r in range(R)]
    drive(env, lines, t0, disp)
    hist, seen = snapshot_at(env, lines, g, pos, disp)
    fly, dsp, longest = coverage(lines)
    print("slot %d position %d: %d vehicles in flight, %d of them dispatched, longest idle list %d" % (t0, pos, fly, dsp, longest))
    # (the oracle's lists at slot 49 behind the step: 73 vehicles in flight, 13 of them dispatched, idle lists of up to 18 entries)
    assert (fly, dsp, longest) == (73, 13, 18) if pos == STEPPED else (fly >= 73 and dsp >= 13 and longest >= 17), (fly, dsp, longest)
    diverge(env, g, 10, lines[0].stepped)
    env.restore()
    lines = [ln.fork(h) for ln, h in zip(lines, hist)]
    check_state(env, lines, "after restore")
    same_reads(reads(env), seen, np.arange(R))
    finish_day(env, lines, disp)
    check_state(env, lines, "end of day")
    od, cn = env.orders(), env.counters()
    for k in ("status", "vehicle", "wait"):       # replica 0 also against the reference's own record of the day
        np.testing.assert_array_equal(od[k][0], g["o_" + k])
    assert cn[0, 4] == int(g["dispatch_num"]) and cn[0, 5] == int(g["dispatch_cost"]) and cn[0, 1] == int(g["reject_num"])
    env.close()


def fork_day(g, R, t0, src, kw=None, torch_map=False, days=None, replica_day=None, pos=STEPPED, after_run=False, n_div=3, rollback=True, init=None):
    """A day with per-replica histories to slot t0; snapshot; n_div slots of something else; rollback (checked); restore through
    ``src`` - host map or device map - (checked); every replica a dispatch of its own; the rest of the day as one ``run``."""
    env, sup = open_env(g, R, days, replica_day, **(kw or {}))
    init = seeded_init(g, R) if init is None else init
    env.reset(init)
    lines = [Line(g, init[r], None if days is None else days[replica_day[r]]) for r in range(R)]
    if after_run:           # (stamp form: the snapshot right behind a run, whose last slot leaves the packing to the flush)
        env.run(t0)
        for ln in lines:
            ln.run(t0)
    else:
        own = max(t0 - 2, 0)
        env.run(own)
        for ln in lines:
            ln.run(own)
        drive(env, lines, t0, own_moves_from=own)
    hist, seen = snapshot_at(env, lines, g, pos)
    fly, dsp, longest = coverage(lines)
    assert fly > 0 and longest > 0, "slot %d: nothing in flight or every idle list empty" % t0
    if rollback:
        diverge(env, g, n_div, lines[0].stepped)
        env.restore()
        lines = [ln.fork(h) for ln, h in zip(lines, hist)]
        check_state(env, lines, "rollback", sup)
        same_reads(reads(env), seen, np.arange(R))
    diverge(env, g, n_div, lines[0].stepped)
    if torch_map:
        import torch
        env.restore_torch(torch.tensor(src, dtype=torch.int32, device="cuda"))
    else:
        env.restore(src)
    lines = [lines[s].fork(hist[s]) for s in src]
    check_state(env, lines, "fork", sup)
    same_reads(reads(env), seen, src)
    if not lines[0].stepped:
        env.step()
        for ln in lines:
            ln.step()
    mv = head_moves(g, lines, 1000)
    assert len({tuple(v[1]) for v in mv.values()}) > 1, "the replicas' dispatches do not differ"
    apply_moves(env, lines, mv)
    check_state(env, lines, "fork + dispatch", sup)
    finish_day(env, lines)
    check_state(env, lines, "end of day")
    return env, lines, hist, seen


# ---- 2. fork: replicas 0, 1 and 4 continue from replica 2, replica 2 from replica 0
@pytest.mark.parametrize("torch_map", [False, True], ids=["host_map", "device_map"])
def test_fork_continues_every_replica_from_its_source(torch_map):
    g = load_golden("tiny_kmeans")
    env, _, _, _ = fork_day(g, 5, 60, [2, 2, 0, 4, 2], torch_map=torch_map, rollback=False)
    env.close()


# ---- 3. every tick family and both layouts, rollback + fork in short form
MODE_NAMES = ("fast", "fast_sup", "generic", "far", "far_generic", "dfs_v2", "dfs_wide", "dense16", "dense_tiny", "dense_tiny8", "dense_slow",
              "dense_far", "dense_ring", "dense_ring_far", "dense_alt", "rows", "rows_far", "ring64")
# a slot at which idle lists and in-flight arrivals are both non-empty (asserted from the oracles): the searching fixtures run
# their idle lists empty later in the day
MODE_FIXTURES = {"tiny_kmeans": 40, "tiny_dispatch": 40, "tiny_kmeans_dfs2": 12, "tiny_dispatch_dfs2": 12, "tiny_window4_dfs2": 12}
MODE_PAIRS = [(n, m) for n in MODE_FIXTURES for m in MODE_NAMES if _applies(n, m, every_pair=True)]


@pytest.mark.parametrize("name,mode", MODE_PAIRS)
def test_rollback_and_fork_in_every_tick_family(name, mode):
    g = load_golden(name)
    env, _, _, _ = fork_day(g, 3, MODE_FIXTURES[name], [1, 1, 0], kw=MODES[mode])
    env.close()


@pytest.mark.parametrize("name", ["tiny_kmeans_dfs2", "tiny_dispatch_dfs2", "tiny_window4_dfs2"])
def test_snapshot_right_behind_a_run_in_the_stamp_form(name):
    g = load_golden(name)
    env, _ = open_env(g, 3)
    stamp = env.layout()["dense_st"] == 1
    env.close()
    assert stamp or name == "tiny_window4_dfs2", "the searching fixtures run the stamp form by default"
    env, _, _, _ = fork_day(g, 3, MODE_FIXTURES[name], [2, 0, 0], pos=BETWEEN, after_run=True)
    env.close()


# ---- 4. capacity edges: rows at their capacity; maps across the 16- and 32-replica workgroup boundaries
IDLE_CAP, RING_CAP = 64, 16


def crowded_init(g, R):
    """Start nodes that put exactly IDLE_CAP - r % 5 vehicles of replica r into the largest cluster (64, 63, 62, 61, 60 of the 64
    slots: the full row, and lengths whose last 16-byte piece ends the row in either layout); returns (nodes, that cluster)."""
    n2c = np.asarray(g["node2cluster"])
    big = int(np.bincount(n2c[n2c >= 0]).argmax())
    crowd, rest = np.flatnonzero(n2c == big), np.flatnonzero((n2c >= 0) & (n2c != big))
    init = seeded_init(g, R)
    for r in range(R):
        inside = n2c[init[r]] == big
        want = IDLE_CAP - r % 5
        if inside.sum() < want:
            move = np.flatnonzero(~inside)[:want - inside.sum()]
            init[r, move] = crowd[(move + r) % crowd.size]
        else:
            move = np.flatnonzero(inside)[want:]
            init[r, move] = rest[(move + r) % rest.size]
    return init, big


def arrival_rows(ln, dispatched_only):
    """{(cluster, slots ahead): entries} of the oracle's arrival dicts - the rows of the arrival ring as they stand."""
    L, veh, tick = ln.o.lists(), ln.o.vehicles(), 10
    rows = {}
    for c in range(len(L["arr_off"]) - 1):
        a, b = L["arr_off"][c], L["arr_off"][c + 1]
        keep = veh["order"][L["arr_veh"][a:b]] < 0 if dispatched_only else np.ones(b - a, dtype=bool)
        for sl in np.maximum(-(-(L["arr_min"][a:b][keep] - ln.o.now_min) // tick), 0):
            rows[(c, int(sl))] = rows.get((c, int(sl)), 0) + 1
    return rows


def row_fill(ln, big, k):
    """k idle vehicles of cluster `big` with a target node each, all in ONE other cluster and all due in ONE arrival slot that
    holds nothing yet (the soonest such slot): one row of the arrival ring takes k entries."""
    g = ln.g
    n2c, cost, L, veh = np.asarray(g["node2cluster"]), np.asarray(g["cost"]), ln.o.lists(), ln.o.vehicles()
    idle = L["idle_veh"][L["idle_off"][big]:L["idle_off"][big + 1]]
    taken = arrival_rows(ln, False)
    best = None
    for c2 in range(int(g["C"])):
        nodes2 = np.flatnonzero(n2c == c2)
        if c2 == big or nodes2.size == 0:
            continue
        ahead = -(-cost[np.ix_(nodes2, veh["loc"][idle])].astype(np.int64) // 10)      # RoadCost(vehicle, node) = cost[node, vehicle's node]
        for sl in np.unique(ahead):
            can = np.flatnonzero((ahead == sl).any(axis=0))
            if 1 <= sl < 32 and (c2, int(sl)) not in taken and can.size >= k and (best is None or sl < best[0]):
                best = (int(sl), c2, [int(idle[v]) for v in can[:k]], [int(nodes2[(ahead[:, v] == sl).argmax()]) for v in can[:k]])
    assert best is not None, "no arrival slot takes %d vehicles of cluster %d" % (k, big)
    return best


def plain_slots(env, n, stepped):
    for _ in range(n):
        if not stepped:
            env.step()
        stepped = False
        env.advance()


@pytest.mark.parametrize("R,mode", [(17, "fast"), (33, "fast"), (33, "rows")])
def test_rows_at_capacity_and_maps_across_workgroup_boundaries(R, mode):
    g = load_golden("tiny_kmeans")
    init, big = crowded_init(g, R)
    src = list(range(R - 1, -1, -1))
    env, _ = open_env(g, R, **dict(MODES[mode], idle_cap=IDLE_CAP, ring_cap=RING_CAP))
    assert env.layout()["dense"] == (mode == "fast")
    env.reset(init)
    assert env.idle_cap == IDLE_CAP
    lines = [Line(g, init[r]) for r in range(R)]

    def within_capacity(what):      # (the set-up's own doing, from the oracles: no list or ring row beyond its table)
        for r, ln in enumerate(lines):
            assert np.diff(ln.o.lists()["idle_off"]).max() <= IDLE_CAP, (what, r)
            assert max(arrival_rows(ln, False).values(), default=0) <= RING_CAP, (what, r)

    # (a) idle rows of 60 .. 64 of 64 entries, the snapshot before the first step
    hist, seen = snapshot_at(env, lines, g, BETWEEN)
    longest = [int(np.diff(ln.o.lists()["idle_off"]).max()) for ln in lines]
    print("idle lists of %s of %d entries" % (sorted(set(longest)), IDLE_CAP))
    assert longest == [IDLE_CAP - r % 5 for r in range(R)] and max(longest) == IDLE_CAP and min(longest) >= 56
    plain_slots(env, 2, False)
    env.restore(src)
    lines = [lines[s].fork(hist[s]) for s in src]
    check_state(env, lines, "full idle rows through a reversal")
    same_reads(reads(env), seen, src)
    # (b) one row of the arrival ring per replica with 12 .. 16 of 16 entries: that many vehicles dispatched into one cluster, due in one slot
    env.step()
    for ln in lines:
        ln.step()
    fills = [row_fill(ln, big, RING_CAP - r % 5) for r, ln in enumerate(lines)]
    apply_moves(env, lines, {r: (f[2], f[3]) for r, f in enumerate(fills)})
    rows = [arrival_rows(ln, True)[(f[1], f[0])] for ln, f in zip(lines, fills)]
    print("ring rows of %s of %d entries, due %s slots ahead" % (sorted(set(rows)), RING_CAP, sorted({f[0] for f in fills})))
    assert rows == [RING_CAP - r % 5 for r in range(R)] and max(rows) == RING_CAP and min(rows) >= 12
    within_capacity("behind the dispatch")
    env.snapshot()
    hist, seen = [ln.history() for ln in lines], reads(env)
    plain_slots(env, 2, True)
    env.restore(src)
    lines = [lines[s].fork(hist[s]) for s in src]
    check_state(env, lines, "full ring rows through a reversal")
    same_reads(reads(env), seen, src)
    env.advance()
    for ln in lines:
        ln.advance()
    for k in range(max(f[0] for f in fills) + 1):          # until every filled row has been taken in
        env.step()
        for ln in lines:
            ln.step()
        within_capacity("slot %d" % lines[0].t)
        env.advance()
        for ln in lines:
            ln.advance()
    check_state(env, lines, "behind the filled rows")
    env.close()


# ---- 5. the snapshot outlives a reset; consecutive restores of one snapshot are independent
def test_snapshot_outlives_a_reset_and_restores_do_not_see_each_other():
    g = load_golden("tiny_kmeans")
    R = 3
    init = seeded_init(g, R)
    env, _ = open_env(g, R)
    env.reset(init)
    lines = [Line(g, init[r]) for r in range(R)]
    env.run(30)
    for ln in lines:
        ln.run(30)
    hist, seen = snapshot_at(env, lines, g, BETWEEN)
    env.reset_again()
    env.run(5)
    assert env.clock[0] == 5
    env.restore()
    check_state(env, lines, "restore behind a reset")
    same_reads(reads(env), seen, np.arange(R))
    env.run(env.T - 30)
    for ln in lines:
        ln.run(env.T - 30)
    check_state(env, lines, "end of day")
    for r in range(R):          # the day equals the oracle's uninterrupted day
        o = make_oracle(g)
        o.reset(init[r])
        o.run_day()
        for k in ("status", "vehicle", "wait"):
            np.testing.assert_array_equal(env.orders()[k][r], o.orders()[k])
    env.restore([1, 2, 0])
    env.restore([2, 0, 1])
    lines = [lines[s].fork(hist[s]) for s in (2, 0, 1)]
    check_state(env, lines, "second of two restores")
    same_reads(reads(env), seen, [2, 0, 1])
    env.close()


# ---- 6. the hooked day continues from a restored slot
def test_hooked_day_from_a_restored_slot_equals_the_stepwise_loop():
    import torch
    g = load_golden("tiny_kmeans")
    R, K, t0, src = 4, 2, 40, [3, 0, 0, 1]
    stream = torch.cuda.current_stream().cuda_stream
    init = seeded_init(g, R)
    nodes = valid_nodes(g)
    acts = np.full((R, K, 3), -1, dtype=np.int32)
    for r in range(R):                              # one fixed action per replica: the head of a cluster's list to a node of its own
        acts[r, 0] = (r % int(g["C"]), 0, nodes[(7 * r + 1) % nodes.size])
    actions = torch.from_numpy(acts).cuda()

    def settle(env):            # (an action on an empty list is skipped and reported once: the same in both loops)
        try:
            env.sync()
        except Exception as e:
            assert "dispatch" in str(e), e

    a, _ = open_env(g, R, stream=stream)
    a.reset(init)
    a.run(t0)
    a.snapshot()
    diverge(a, g, 4, False)
    a.restore(src)
    a.run_hooked(a.T - t0, actions=actions)
    settle(a)
    b, _ = open_env(g, R, stream=stream)
    b.reset(init[src])
    b.run(t0)
    for _ in range(t0, b.T):
        b.step()
        b.apply_dispatch_torch(actions)
        b.advance()
    settle(b)
    assert a.clock == b.clock
    np.testing.assert_array_equal(a.counters(), b.counters())
    assert a.counters()[:, 4].sum() > 0, "no action of the fixed tensor was applied"
    oa, ob = a.orders(), b.orders()
    for k in oa:
        np.testing.assert_array_equal(oa[k], ob[k], err_msg=k)
    for r in range(R):
        la, lb = a.lists(r), b.lists(r)
        for k in la:
            np.testing.assert_array_equal(la[k], lb[k], err_msg="replica %d %s" % (r, k))
    a.close(); b.close()


# ---- 7. order days per replica, stored regrouped by day
def test_fork_inside_a_day_with_order_days_per_replica():
    import torch
    g = load_golden("tiny_kmeans")
    R = 7
    days = synth_days(g, 4, seed=911)
    replica_day = np.array([0, 1, 2, 3, 2, 0, 1], dtype=np.int32)      # (days mixed inside a group of 16: regrouped storage)
    src = [5, 6, 4, 3, 2, 0, 1]                                         # every replica from another one of its own day
    assert all(replica_day[s] == replica_day[r] for r, s in enumerate(src))
    env, lines, hist, seen = fork_day(g, R, 20, src, days=days, replica_day=replica_day)
    assert min(ln.o.num_ticks for ln in lines) > 21 and len({ln.o.num_ticks for ln in lines}) > 1
    with pytest.raises(Exception, match=r"libvds error -1: .*order days per replica"):
        env.restore([1, 1, 2, 3, 4, 5, 6])
    with pytest.raises(Exception, match=r"libvds error -4: "):
        env.restore_torch(torch.arange(R, dtype=torch.int32, device="cuda"))
    check_state(env, lines, "after the refused restores")       # (a refused restore changes nothing)
    env.close()


# ---- 8. errors and lifetime
def test_errors_and_lifetime_of_a_snapshot():
    import torch
    g = load_golden("tiny_kmeans")
    R = 4
    init = seeded_init(g, R)
    env, _ = open_env(g, R)
    env.reset(init)
    assert env.snapshot_info() is None
    with pytest.raises(Exception, match=r"libvds error -4: .*no snapshot"):
        env.restore()
    with pytest.raises(Exception, match=r"libvds error -4: .*no snapshot"):
        env.restore_torch(torch.arange(R, dtype=torch.int32, device="cuda"))
    lines = [Line(g, init[r]) for r in range(R)]
    env.run(20)
    for ln in lines:
        ln.run(20)
    hist, seen = snapshot_at(env, lines, g, STEPPED)
    info = env.snapshot_info()
    assert info == dict(step=20, stepped=True, bytes=info["bytes"]) and info["bytes"] > 0
    for bad in (-1, R):
        with pytest.raises(Exception, match=r"libvds error -1: "):
            env.restore([0, bad, 2, 3])
    check_state(env, lines, "after the refused maps")
    # a device map entry of R: that replica stays on its own row, the others are restored, the next sync says so once
    diverge(env, g, 3, True)
    env.restore_torch(torch.tensor([1, R, 0, 0], dtype=torch.int32, device="cuda"))
    with pytest.raises(Exception, match=r"libvds error -4: .*restore"):
        env.sync()
    env.sync()
    lines = [lines[s].fork(hist[s]) for s in (1, 1, 0, 0)]
    check_state(env, lines, "device map with an entry out of range")
    same_reads(reads(env), seen, [1, 1, 0, 0])
    # whatever re-makes the state tables voids the snapshot
    env.set_idle_cap(env.idle_cap + 64)
    assert env.snapshot_info() is None
    with pytest.raises(Exception, match=r"libvds error -4: .*no snapshot"):
        env.restore()
    env.reset(init)
    env.run(5)
    env.snapshot()
    assert env.snapshot_info()["step"] == 5
    env.load_orders(g["o_release_min"], g["o_pickup"], g["o_delivery"])
    assert env.snapshot_info() is None
    with pytest.raises(Exception, match=r"libvds error -4: .*no snapshot"):
        env.restore()
    env.close()
    days = synth_days(g, 2, seed=77)
    env = mk_env(g, R)
    env.load_order_days(days, [0, 0, 1, 1])
    env.reset(init)
    env.run(5)
    env.snapshot()
    assert env.snapshot_info()["step"] == 5
    env.set_replica_days([1, 1, 0, 0])
    assert env.snapshot_info() is None
    with pytest.raises(Exception, match=r"libvds error -4: .*no snapshot"):
        env.restore()
    env.reset(init)
    env.run(3)
    env.snapshot()
    assert env.snapshot_info()["bytes"] > 0
    env.drop_snapshot()
    assert env.snapshot_info() is None
    with pytest.raises(Exception, match=r"libvds error -4: .*no snapshot"):
        env.restore()
    env.close()


# ---- 9. nothing new on the old paths
def test_a_handle_that_never_snapshots_holds_no_snapshot_storage():
    g = load_golden("tiny_kmeans")
    env, _ = open_env(g, 3)
    env.reset(seeded_init(g, 3))
    env.run(env.T)
    env.sync()
    assert env.snapshot_info() is None
    env.close()
