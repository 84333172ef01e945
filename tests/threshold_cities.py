"""Cities placed exactly on the host's layout and kernel thresholds (vds_api.hip load_static / load_orders), one builder per
threshold with a ``side`` parameter: ``0`` at the limit (the faster form must still be chosen), ``1`` one past it.

Every builder returns a dict: ``cost`` (int32 [N, N]), ``n2c``, ``nbr`` (neighbour lists), ``depth``, ``neighbor``, ``V``, ``rel`` /
``pick`` / ``dele`` (one shared order day), ``init`` (int32 [R, V], a different start per replica), ``threshold``, ``idle_cap``,
``far_cap``, and the facts its premise rests on (``facts``: what tests/test_threshold_cities.py checks on the inputs alone).
Block-structured tables: small costs inside each cluster, chosen costs between clusters."""
import numpy as np

from vehicles_dispatch_simulator_amd.env import neighbors_to_csr

R = 3
TICK = 10
SLOTS = 24
BIG_THRESHOLD = 600_000_000_000


def block_city(sizes, seed, in_max=20, cross=(30, 90)):
    """Clusters of the given sizes (nodes numbered cluster by cluster), costs 1..in_max inside a cluster, cross[0]..cross[1]
    between clusters, 0 on the diagonal.  Returns (cost int64 [N, N], node2cluster, first node of each cluster + N)."""
    rng = np.random.default_rng(seed)
    N = int(sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n2c = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    cost = rng.integers(cross[0], cross[1] + 1, size=(N, N)).astype(np.int64)
    for c in range(len(sizes)):
        a, b = off[c], off[c + 1]
        cost[a:b, a:b] = rng.integers(1, in_max + 1, size=(b - a, b - a))
    np.fill_diagonal(cost, 0)
    return cost, n2c, off


def order_day(rng, pick_nodes, dele_nodes, O, slots=SLOTS):
    rel = np.sort(rng.integers(0, slots * TICK, size=O)).astype(np.int32)
    return rel, rng.choice(pick_nodes, size=O).astype(np.int32), rng.choice(dele_nodes, size=O).astype(np.int32)


def starts(rng, V, hot_nodes, all_nodes, shares=(1.0, 0.5, 0.0)):
    """[R, V] start nodes: replica r puts shares[r] of its vehicles on hot_nodes (cycled), the rest anywhere in all_nodes."""
    init = np.empty((R, V), dtype=np.int32)
    hot = np.asarray(hot_nodes)
    for r in range(R):
        k = int(round(V * shares[r % len(shares)]))
        init[r, :k] = hot[np.arange(k) % hot.size]
        init[r, k:] = rng.choice(all_nodes, size=V - k)
        rng.shuffle(init[r])
    return init


def case(cost, n2c, V, day, init, nbr=None, depth=0, neighbor=False, threshold=BIG_THRESHOLD, idle_cap=0, far_cap=0, ring_cap=0, **facts):
    cost = np.asarray(cost, dtype=np.int64)
    assert cost.min() >= -(1 << 31) and cost.max() < (1 << 31)
    C = int(n2c.max()) + 1
    return dict(cost=cost.astype(np.int32), n2c=n2c, nbr=nbr if nbr is not None else [[] for _ in range(C)], depth=depth,
                neighbor=neighbor, V=V, rel=day[0], pick=day[1], dele=day[2], init=init, threshold=threshold, idle_cap=idle_cap,
                far_cap=far_cap or max(64, V), ring_cap=ring_cap, facts=facts)


def cluster_size(side):
    """Row 1: one cluster of 255 / 256 nodes (the dense layout holds clusters of at most 255: load_static, d_ok).  Idle vehicles and
    pickups crowd its local node 254 - with byte blocks the last real column; column 255 is the dead one."""
    n = 255 + side
    cost, n2c, off = block_city([n, 40, 40], seed=11 + side)
    rng = np.random.default_rng(100 + side)
    hot = int(off[0] + 254)
    all_nodes = np.arange(cost.shape[0])
    rel, pick, dele = order_day(rng, all_nodes, all_nodes, 420)
    pick[rng.random(pick.size) < 0.5] = hot
    init = starts(rng, 120, [hot], all_nodes)
    return case(cost, n2c, 120, (rel, pick, dele), init, max_nc=n, hot=hot)


def _far_corner(cost, off, c, value):
    """Every in-cluster cost from / to the last node of cluster c set to value; returns that node."""
    L = int(off[c + 1] - 1)
    cost[L, off[c]:off[c + 1]] = value
    cost[off[c]:off[c + 1], L] = value
    cost[L, L] = 0
    return L


def _corner_day(rng, cost, off, corners, O=360, burst=14):
    """Orders picked up anywhere but at the corners, plus bursts of `burst` orders in one slot in the first cluster: the last orders of
    a burst find one live candidate (the others taken) - a corner vehicle, at the corner's cost - and then none."""
    C = off.size - 1
    N = cost.shape[0]
    plain = np.setdiff1d(np.arange(N), corners)
    rel, pick, dele = order_day(rng, plain, np.arange(N), O)
    b_rel = np.repeat(np.arange(3, SLOTS, 5) * TICK + 1, burst).astype(np.int32)
    b_pick = rng.choice(plain[plain < off[1]], size=b_rel.size).astype(np.int32)
    b_dele = rng.choice(np.arange(off[1], off[C]), size=b_rel.size).astype(np.int32)
    o = np.argsort(np.concatenate([rel, b_rel]), kind="stable")
    return np.concatenate([rel, b_rel])[o], np.concatenate([pick, b_pick])[o], np.concatenate([dele, b_dele])[o]


def byte_max(side):
    """Row 2: largest in-cluster cost 254 / 255 with the whole matrix <= 255 (u8_ok stays on): byte blocks (dead column 0xFF) / int
    blocks (load_static, d8).  Vehicles start on each cluster's corner node, whose every in-cluster cost is that maximum."""
    M = 254 + side
    cost, n2c, off = block_city([40] * 5, seed=21 + side)
    corners = [_far_corner(cost, off, c, M) for c in range(5)]
    rng = np.random.default_rng(200 + side)
    day = _corner_day(rng, cost, off, corners)
    init = starts(rng, 60, corners, np.arange(cost.shape[0]), shares=(1.0, 0.8, 0.5))
    return case(cost, n2c, 60, day, init, in_max=M, cost_max=M)


def cross_max(side, search):
    """Row 3: the in-cluster costs fit a byte; one block of cross-cluster costs (cluster 1 <-> cluster 0) is 255 / 256: u8_ok and the
    byte matrix (cost8) on / off.  With neighbour search (cluster 0 looks into cluster 1, depth 1) cluster 0 starts without vehicles
    and takes many pickups, so its orders are served from cluster 1 at exactly that cost."""
    M = 255 + side
    cost, n2c, off = block_city([40] * 5, seed=31 + side, cross=(30, 200))
    cost[off[1]:off[2], off[0]:off[1]] = M
    cost[off[0]:off[1], off[1]:off[2]] = M
    rng = np.random.default_rng(300 + side)
    N = cost.shape[0]
    rel, pick, dele = order_day(rng, np.arange(N), np.arange(N), 300)
    sel = rng.random(pick.size) < 0.4
    pick[sel] = rng.choice(np.arange(off[0], off[1]), size=int(sel.sum()))
    init = starts(rng, 50, np.arange(off[1], off[2]), np.arange(off[1], N), shares=(0.8, 0.5, 0.3))
    nbr = [[1, 2], [0], [], [4], []]
    return case(cost, n2c, 50, (rel, pick, dele), init, nbr=nbr, depth=1 if search else 0, neighbor=search, cross_max=M)


def lds_int_block(side):
    """Row 4: int blocks (in-cluster costs of 300) of a 127 / 128-node cluster: 127 * 128 * 4 bytes fit the 64 KB of LDS, 128 * 129 * 4
    do not (load_static, `common`)."""
    n = 127 + side
    cost, n2c, off = block_city([n, 30, 30], seed=41 + side)
    corner = _far_corner(cost, off, 0, 300)
    rng = np.random.default_rng(400 + side)
    N = cost.shape[0]
    rel, pick, dele = order_day(rng, np.arange(N), np.arange(N), 360)
    init = starts(rng, 80, [corner] + list(range(int(off[0]), int(off[0]) + 20)), np.arange(N))
    return case(cost, n2c, 80, (rel, pick, dele), init, max_nc=n, cost_max=300)


def fast_cmax(side):
    """Row 5a: largest cost 2^23 - 1 / 2^23 (packed `cost << 7 | pos` keys: fast_ok, load_static).  On the fast side the corner
    vehicles' only candidates cost 2^23 - 1 and must still win over the dead key."""
    M = (1 << 23) - 1 + side
    cost, n2c, off = block_city([40] * 4, seed=51 + side)
    corners = [_far_corner(cost, off, c, M) for c in range(2)]
    rng = np.random.default_rng(500 + side)
    day = _corner_day(rng, cost, off, corners, O=240, burst=8)
    init = starts(rng, 40, corners, np.arange(cost.shape[0]), shares=(1.0, 0.7, 0.4))
    return case(cost, n2c, 40, day, init, cost_max=M, cost_min=0)


def fast_cmin(side):
    """Row 5b: smallest cost 0 / -1 (fast_ok needs cmin >= 0); the -1 entries are in-cluster costs a corner vehicle is matched over:
    RoadCost(corner, pickup) = cost[pickup, corner], the corner's COLUMN."""
    cost, n2c, off = block_city([40] * 4, seed=61 + side)
    corner = _far_corner(cost, off, 0, 3)
    cost[off[0]:corner, corner] = np.where(np.arange(off[0], corner) % 2 == 0, -side, 3)
    rng = np.random.default_rng(600 + side)
    day = _corner_day(rng, cost, off, [corner], O=240, burst=8)
    init = starts(rng, 40, [corner], np.arange(cost.shape[0]), shares=(1.0, 0.7, 0.4))
    return case(cost, n2c, 40, day, init, cost_min=-side)


def reject_window(side):
    """Row 5c: largest cost 200 with reject_threshold 200 / 199: no live pickup window (fast_ok) / a live one (window_live) - the
    corner vehicles' only candidates cost 200, served on one side and rejected on the other."""
    cost, n2c, off = block_city([40] * 4, seed=71)
    corners = [_far_corner(cost, off, c, 200) for c in range(2)]
    rng = np.random.default_rng(700)
    day = _corner_day(rng, cost, off, corners, O=240, burst=8)
    init = starts(rng, 40, corners, np.arange(cost.shape[0]), shares=(1.0, 0.7, 0.4))
    return case(cost, n2c, 40, day, init, threshold=200 - side, cost_max=200)


def bucket_orders(side):
    """Row 6: 64 / 65 orders of one (cluster, slot) - what the fast path of the dense tick takes (vds_tick_dense.hip) - with enough
    idle vehicles in the cluster for all of them; slot 1 holds the burst alone."""
    k = 64 + side
    cost, n2c, off = block_city([60, 60, 60], seed=81)
    rng = np.random.default_rng(800)
    N = cost.shape[0]
    rel, pick, dele = order_day(rng, np.arange(N), np.arange(N), 120)
    keep = rel >= 3 * TICK
    b_rel = np.full(k, TICK + 3, dtype=np.int32)
    b_pick = rng.choice(np.arange(off[0], off[1]), size=k).astype(np.int32)
    b_dele = rng.choice(np.arange(off[1], N), size=k).astype(np.int32)
    day = (np.concatenate([b_rel, rel[keep]]), np.concatenate([b_pick, pick[keep]]), np.concatenate([b_dele, dele[keep]]))
    init = starts(rng, 100, np.arange(off[0], off[0] + 50), np.arange(N), shares=(0.8, 0.75, 0.7))
    return case(cost, n2c, 100, day, init, burst=k)


def bucket_entries(side, tab):
    """Row 6: a list of tab / tab + 1 entries in one bucket that has an order (tab = 128: the tables of the 8-lane form, 256: the
    16-lane form with 256-entry tables and byte costs).  Cluster 0 starts with tab + side vehicles in every replica and never
    receives one (no order delivers there); its orders come from slot 1 on.  The other clusters hold 40 vehicles between them."""
    n0 = tab + side
    cost, n2c, off = block_city([60, 40, 40], seed=83)
    rng = np.random.default_rng(830 + tab)
    N = cost.shape[0]
    rest = np.arange(off[1], N)
    rel, pick, dele = order_day(rng, rest, rest, 200)
    c_rel = np.array([TICK + 2, TICK + 5, 4 * TICK + 1, 9 * TICK + 4], dtype=np.int32)
    c_pick = rng.choice(np.arange(off[0], off[1]), size=c_rel.size).astype(np.int32)
    c_dele = rng.choice(rest, size=c_rel.size).astype(np.int32)
    o = np.argsort(np.concatenate([rel, c_rel]), kind="stable")
    day = tuple(np.concatenate(x)[o] for x in ((rel, c_rel), (pick, c_pick), (dele, c_dele)))
    V = n0 + 40
    init = np.empty((R, V), dtype=np.int32)
    for r in range(R):
        init[r, :n0] = rng.choice(np.arange(off[0], off[1]), size=n0)
        init[r, n0:] = rng.choice(rest, size=40)
        rng.shuffle(init[r])
    return case(cost, n2c, V, day, init, n0=n0, tab=tab)


ARRIVAL_VALUE = 35


def bucket_arrivals(side):
    """Row 6: 64 / 65 vehicles arriving in one cluster in one slot (DN_TH: the arrivals of a bucket the dense tick's fast path takes).
    In slot 1, 32 orders of cluster 0 and 32 / 33 of cluster 2 are picked up on the node their vehicles stand on (wait 0) and delivered
    into cluster 1 at OrderValue 35 each: all of them arrive together.  Every other order is picked up in cluster 1 and delivered into
    cluster 2, later.  ring_cap = V: the wide-layout kernels take these arrivals through the arrival ring, whose
    automatic size (64 entries here) is a capacity the caller raises - an overflow is reported, never silent."""
    cost, n2c, off = block_city([40, 40, 40], seed=85)
    p0, p2 = int(off[0] + 3), int(off[2] + 3)
    cost[off[1]:off[2], p0] = ARRIVAL_VALUE          # OrderValue = RoadCost(pickup, delivery) = cost[delivery, pickup]
    cost[off[1]:off[2], p2] = ARRIVAL_VALUE
    rng = np.random.default_rng(850)
    k0, k2 = 32, 32 + side
    rel, pick, dele = order_day(rng, np.arange(off[1], off[2]), np.arange(off[2], off[3]), 60)
    keep = rel >= 3 * TICK
    b_rel = np.full(k0 + k2, TICK + 3, dtype=np.int32)
    b_pick = np.repeat([p0, p2], [k0, k2]).astype(np.int32)
    b_dele = rng.choice(np.arange(off[1], off[2]), size=k0 + k2).astype(np.int32)
    day = (np.concatenate([b_rel, rel[keep]]), np.concatenate([b_pick, pick[keep]]), np.concatenate([b_dele, dele[keep]]))
    V = 110
    init = np.empty((R, V), dtype=np.int32)
    for r in range(R):
        init[r, :40], init[r, 40:80] = p0, p2
        init[r, 80:] = rng.choice(np.arange(off[1], off[2]), size=30)
        rng.shuffle(init[r])
    return case(cost, n2c, V, day, init, ring_cap=V, arrivals=k0 + k2)


def search_cost(side):
    """Row 7: neighbour search with the largest cost 32 767 / 32 768 (k_tick_replica2 and the hybrid tick need cost_max < 2^15:
    dfs2_ok / hybrid_ok in load_orders), the cross-cluster cost the search pays from cluster 1 into cluster 0."""
    c = cross_max(0, True)
    M = 32767 + side
    cost = c["cost"].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.bincount(c["n2c"]))])
    cost[off[1]:off[2], off[0]:off[1]] = M
    cost[off[0]:off[1], off[1]:off[2]] = M
    return case(cost, c["n2c"], c["V"], (c["rel"], c["pick"], c["dele"]), c["init"], nbr=c["nbr"], depth=1, neighbor=True, cost_max=M)


def dense_search_capacity(side, what):
    """Row 8: neighbour search on the dense layout holds V <= 16 384 vehicles and idle_cap <= 16 384 entries (load_static
    dense_dfs_static_ok, load_orders dense_st).  what = "V": V = 16 384 / 16 385 (idle_cap 16 384); "idle_cap": V = 2 000 and
    idle_cap = 16 384 / 16 385.  Replica 0 starts with all of its vehicles in cluster 1 (side 1 of "V": all but one, so that the list
    fits idle_cap) - one list of 16 384 entries (V = 2 000: 2 000), positions up to 16 383; no order delivers into cluster 1, so it
    never grows.  Cluster 0 starts empty and searches cluster 1, where the vehicles with the highest list positions sit on the node
    nearest to it: the walk takes its vehicles from the end of the full list."""
    cost, n2c, off = block_city([40] * 5, seed=91, cross=(30, 200))
    near = int(off[1] + 7)
    cost[off[0]:off[1], off[1]:off[2]] = 150          # RoadCost(cluster-1 node, cluster-0 pickup) = cost[pickup, node]
    cost[off[0]:off[1], near] = 31
    rng = np.random.default_rng(900 + side)
    N = cost.shape[0]
    V = 16384 + side if what == "V" else 2000
    rel, pick, dele = order_day(rng, np.arange(N), np.setdiff1d(np.arange(N), np.arange(off[1], off[2])), 400, slots=12)
    sel = rng.random(pick.size) < 0.4
    pick[sel] = rng.choice(np.arange(off[0], off[1]), size=int(sel.sum()))
    init = np.stack([rng.choice(np.arange(N), size=V) for r in range(R)]).astype(np.int32)
    others = np.setdiff1d(np.arange(off[1], off[2]), [near])
    init[0] = rng.choice(others, size=V)
    init[0, V - 64:] = near
    init[0, :side * (what == "V")] = off[2]          # (cluster 2)
    nbr = [[1, 2], [0], [3], [4], []]
    return case(cost, n2c, V, (rel, pick, dele), init, nbr=nbr, depth=2, neighbor=True, idle_cap=16384 + (side if what == "idle_cap" else 0),
                near=near)


def visit_sequence(L):
    """Row 9: the longest visit sequence exactly L clusters long past its start cluster (what the library keeps per cluster:
    seq_pad 64 / 128 / 256; the hybrid tick and the dense layout need <= 256): cluster 0 looks into clusters 1 .. L at depth 1, the
    others into their next cluster.  Two nodes per cluster."""
    C = max(L + 1, 66) + 2
    cost, n2c, off = block_city([2] * C, seed=L, cross=(30, 200))
    nbr = [list(range(1, L + 1))] + [[(c + 1) % C] for c in range(1, C)]
    rng = np.random.default_rng(L)
    N = cost.shape[0]
    rel, pick, dele = order_day(rng, np.arange(N), np.arange(N), 360, slots=12)
    sel = rng.random(pick.size) < 0.4
    pick[sel] = rng.integers(0, 2, size=int(sel.sum()))
    init = starts(rng, 60, np.arange(N - 40, N), np.arange(N), shares=(0.9, 0.6, 0.3))
    return case(cost, n2c, 60, (rel, pick, dele), init, nbr=nbr, depth=1, neighbor=True, max_seq=L)


WRAP_COST = 1 << 26
WRAP_K = 32


def _dispatch_city(sizes, seed, V, k, tcost=None):
    """Vehicles crowd cluster 0 (no order is picked up there); the hook moves k of them out of it in slot 0 to one node of cluster 2,
    at RoadCost tcost from every node of cluster 0 where given."""
    cost, n2c, off = block_city(sizes, seed=seed)
    target = int(off[2] + 5)
    if tcost is not None:              # (both directions: RoadCost(LocationNode, target) reads the target's row)
        cost[off[0]:off[1], target] = tcost
        cost[target, off[0]:off[1]] = tcost
    rng = np.random.default_rng(seed + 900)
    N = cost.shape[0]
    rel, pick, dele = order_day(rng, np.arange(off[1], N), np.arange(N), 240)
    init = starts(rng, V, np.arange(off[0], off[1]), np.arange(off[1], N), shares=(0.6, 0.6, 0.6))
    return case(cost, n2c, V, (rel, pick, dele), init, far_cap=V, target=target, k=k, tcost=tcost)


def dispatch_wrap():
    """Row 10c: a generic-layout city (costs of 2^26 >= 2^23); 32 vehicles of cluster 0 dispatched in one call to a node at RoadCost
    2^26 from all of cluster 0: their costs sum to exactly 2^31."""
    return _dispatch_city([40, 40, 40], 101, 80, WRAP_K, WRAP_COST)


def dispatch_dense_control():
    """Row 10, the dense-layout control: 64 dispatches out of cluster 0 in one call at RoadCost 2^23 - 1 each (the largest cost the
    dense layout takes): 64 x (2^23 - 1) < 2^29."""
    return _dispatch_city([80, 40, 40], 102, 120, 64, (1 << 23) - 1)


def dispatch_many():
    """Row 10b: 70 actions of one (replica, cluster) group in one host-list call (two 64-action chunks of k_dispatch)."""
    return _dispatch_city([90, 40, 40], 103, 130, 70)


def oracle_for(c, r):
    from oracle.oracle import Oracle
    off, idx = neighbors_to_csr(c["nbr"])
    o = Oracle(c["cost"], c["n2c"], off, idx, c["depth"], c["neighbor"], c["rel"], c["pick"], c["dele"], c["V"], tick_minutes=TICK,
               reject_threshold=c["threshold"])
    o.reset(c["init"][r])
    return o


def in_cluster_max(c):
    n2c = c["n2c"]
    return int(c["cost"][n2c[:, None] == n2c[None, :]].max())


def cross_cluster_max(c):
    n2c = c["n2c"]
    return int(c["cost"][n2c[:, None] != n2c[None, :]].max())
