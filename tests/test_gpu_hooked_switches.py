"""One handle, one day, the switches of ``run_hooked`` changed every two slots: what the day graph is rebuilt, updated in place or
replayed for.  Handle A runs the day as ``run_hooked`` segments of two slots, handle B the same slots through ``step``, the
``*_torch`` refreshes of whatever the segment has on, the ``apply_dispatch_*_torch`` calls and ``advance``.  After every segment
every derived block read so far is the same on both handles - the ones the segment refreshed, and the ones it left alone, which
still hold the last refresh - and at the end of the day both agree with the CPU oracle fed the same dispatches.  No policy graph:
the action and target tensors are fixed per segment.  Every expectation is an integer; nothing has a tolerance."""
import numpy as np
import pytest

from helpers import load_golden, oracle_apply
from test_gpu_dispatch_vehicles import CAPS, assert_same_day, day_result, make_oracles, random_targets, seeded_init, to_dev
from test_gpu_idle_roster import oracle_apply_roster, roster_targets
from test_gpu_parity import check_lists, make_env

pytestmark = pytest.mark.gpu
R = 40                  # two groups of 32 and 8 replicas (chunks of 16)
SEG = 2                 # slots per segment
OBS_OFF = dict(idle_pre=False, idle_now=False, supply=False, cl_orders=False)
VEH = dict(state=True, cluster=True)
VEH_B = dict(state=True, node=False, cluster=True, arrive_min=False, order=False)
# the segments' switches; "actions" / "vehicle_targets" / "roster_targets": a fixed tensor made for the segment
SEGMENTS = [
    dict(obs=True),
    dict(outcomes=True, idle_heads=2),
    dict(outcomes=True, idle_heads=3),
    dict(vehicle_planes=VEH, vehicle_targets=True, actions=True),
    dict(vehicle_planes=VEH, vehicle_targets=True, actions=True, vehicle_outcomes=True, orders=True),
    dict(roster=True, roster_targets=True),
    dict(),
    dict(outcomes=True, idle_heads=2),
]


def fullest_actions(g, oracles):
    """K = 2 per replica: the second and the first vehicle of the replica's fullest list to the first clustered node."""
    n0 = int(np.flatnonzero(g["node2cluster"] >= 0)[0])
    acts = np.full((len(oracles), 2, 3), -1, dtype=np.int32)
    for r, o in enumerate(oracles):
        c = int(np.argmax(np.diff(o.lists()["idle_off"])))
        acts[r, 0] = (c, 1, n0); acts[r, 1] = (c, 0, n0)
    return acts


def oracle_kform(o, a):
    """One K-form call of one replica: positions refer to the lists before the call; an action whose list is too short is skipped
    (and reported once by the next sync).  Returns whether one was."""
    L = o.lists()
    vehs, tgts, skipped = [], [], False
    for c, p, tg in a:
        if c < 0:
            continue
        if p < L["idle_off"][c + 1] - L["idle_off"][c]:
            vehs.append(L["idle_veh"][L["idle_off"][c] + p]); tgts.append(tg)
        else:
            skipped = True
    if vehs:
        o.dispatch(np.array(vehs, dtype=np.int32), np.array(tgts, dtype=np.int32))
    return skipped


def settle(env):
    """sync; True where it reports skipped dispatch entries (the sticky error, raised once)."""
    try:
        env.sync()
    except Exception as e:
        assert "skipped" in str(e), e
        return True
    return False


def blocks_of(env):
    """Every derived block but the heads, refreshed once and kept: zero-copy views that later reads do not refresh."""
    b = dict(obs=env.obs_torch(inflight=False)[:4], outcomes=env.outcomes_torch(), vout=env.vehicle_outcomes_torch(), orders=env.orders_torch())
    b.update({"veh_" + k: v for k, v in env.vehicles_torch(**VEH_B).items()})
    b.update({"roster_" + k: v for k, v in env.idle_roster_torch().items()})
    return b


@pytest.mark.parametrize("name,groups,kw", [("tiny_kmeans", 1, {}), ("tiny_kmeans", 2, {}), ("tiny_kmeans_dfs2", 1, {}), ("tiny_kmeans", 1, {"force_generic": 1})],
                         ids=["one-chain", "two-groups", "stamp-form", "eager-generic"])
def test_switches_changed_between_segments_of_one_day(name, groups, kw):
    import torch
    g = load_golden(name)
    init = seeded_init(g, R)
    stream = torch.cuda.current_stream().cuda_stream
    A, B = (make_env(g, R, stream=stream, **CAPS, **kw) for _ in range(2))
    for env in (A, B):
        env.set_run_groups(groups, -1)
        env.reset(init)
    if not kw:
        assert A._lib.vds_get_run_groups(A._h) == groups
    T = A.T
    oracles = make_oracles(g, init)
    rng = np.random.default_rng(11)
    blk = [blocks_of(A), blocks_of(B)]
    heads_L, ran, moved, keep = 0, 0, dict(actions=0, vehicle_targets=0, roster_targets=0), []
    segments = SEGMENTS[:T // SEG]
    for si, seg in enumerate(segments):
        tag = "%s segment %d" % (name, si + 1)
        for o in oracles:
            o.begin_tick()
        # the segment's fixed tensors, from the lists as its first slot's tick leaves them
        fixed = {}
        if seg.get("actions"):
            fixed["actions"] = fullest_actions(g, oracles)
        if seg.get("vehicle_targets"):
            fixed["vehicle_targets"] = random_targets(rng, g, R)
        if seg.get("roster_targets"):
            tg = roster_targets(rng, g, oracles)
            tg[tg >= int(g["N"])] = -1          # (the same tensor meets a longer roster in the second slot: nothing there, not a refusal)
            fixed["roster_targets"] = tg
        dev = {k: to_dev(v) for k, v in fixed.items()}
        keep.append(dev)                        # (alive until the streams have passed the calls)
        L = seg.get("idle_heads", 0)
        if L and L != heads_L:                  # another L re-makes the block: taken (and refreshed) on both handles before the segment
            for b, env in zip(blk, (A, B)):
                b["heads"] = env.idle_heads_torch(L)
            heads_L = L
        on = dict(OBS_OFF) if not seg.get("obs") else {}
        on.update({k: v for k, v in seg.items() if k not in ("obs", "actions", "vehicle_targets", "roster_targets")})
        A.run_hooked(SEG, **on, **dev)
        skipped = False
        for s in range(SEG):
            B.step()
            if seg.get("obs"):
                B.obs_torch(inflight=False)
            if seg.get("outcomes"):
                B.outcomes_torch()
            if L:
                B.idle_heads_torch(L)
            if seg.get("vehicle_planes"):
                B.vehicles_torch(**VEH_B)
            if seg.get("vehicle_outcomes"):
                B.vehicle_outcomes_torch()
            if seg.get("roster"):
                B.idle_roster_torch()
            if seg.get("orders"):
                B.orders_torch(si * SEG + s, si * SEG + s)
            if "actions" in dev:
                B.apply_dispatch_torch(dev["actions"])
            if "vehicle_targets" in dev:
                B.apply_dispatch_vehicles_torch(dev["vehicle_targets"])
            if "roster_targets" in dev:
                B.apply_dispatch_roster_torch(dev["roster_targets"])
            B.advance()
            for r, o in enumerate(oracles):
                if s:
                    o.begin_tick()
                if "actions" in fixed:
                    before = o.counters()["dispatch_num"]
                    skipped |= oracle_kform(o, fixed["actions"][r])
                    moved["actions"] += o.counters()["dispatch_num"] - before
                if "vehicle_targets" in fixed:
                    moved["vehicle_targets"] += oracle_apply(o, fixed["vehicle_targets"][r])[0]
                if "roster_targets" in fixed:
                    m, refused = oracle_apply_roster(o, fixed["roster_targets"][r], g["node2cluster"])
                    assert not any(refused.values()), (tag, refused)
                    moved["roster_targets"] += m
                o.end_tick()
        assert (settle(A), settle(B)) == (skipped, skipped), tag
        assert A.clock == B.clock, tag
        assert set(blk[0]) == set(blk[1])
        for k in blk[0]:        # the blocks the segment had on, and the ones it left alone
            np.testing.assert_array_equal(blk[0][k].cpu().numpy(), blk[1][k].cpu().numpy(), err_msg="%s block %s" % (tag, k))
        ran += 1
    assert ran >= 6
    assert all(moved[k] >= R for k in moved if any(s.get(k) for s in segments)), moved
    # the rest of the day with everything off
    rest = T - ran * SEG
    A.run_hooked(rest, **OBS_OFF)
    for _ in range(rest):
        B.step(); B.advance()
        for o in oracles:
            o.begin_tick(); o.end_tick()
    res = [day_result(A), day_result(B)]
    assert_same_day(res[0], res[1], name + " A against B")
    for k in blk[0]:
        np.testing.assert_array_equal(blk[0][k].cpu().numpy(), blk[1][k].cpu().numpy(), err_msg="%s after the day, block %s" % (name, k))
    for r, o in enumerate(oracles):
        oo, oc = o.orders(), o.counters()
        for env, d in zip((A, B), res):
            check_lists(env, r, o, T)
            for k in ("status", "vehicle", "wait"):
                np.testing.assert_array_equal(d[k][r], oo[k], err_msg="%s replica %d %s" % (name, r, k))
            cn = d["counters"][r]
            assert (cn[0], cn[1], cn[3], cn[4], cn[5]) == (oc["order_num"], oc["reject_num"], oc["wait_sum"], oc["dispatch_num"], oc["dispatch_cost"]), (name, r)
    A.close(); B.close()
