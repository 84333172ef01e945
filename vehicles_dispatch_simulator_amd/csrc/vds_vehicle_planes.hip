// Per-vehicle state of every replica (gfx950 / CDNA4, wave64): the fields of `Vehicle` that the tick path changes (the reference's
// objects/objects.py:75-89 - where a vehicle is, whether it carries an order, when it arrives) as six int32 planes [6][R][V] in the
// caller's replica order - vds_read_vehicles (vds_api.hip: read_lists_impl + read_vehicles_impl, the specification) restated on
// the device for all replicas at once and for both layouts:
//   0 state    0 idle, 1 on the way with an order, 2 on the way after a dispatch (-1: in neither container)
//   1 node     idle: LocationNode; on the way: DeliveryPoint - a GLOBAL node id, cl_nodes[cl_off[c] + local]
//   2 cluster  the cluster whose IdleVehicles / VehiclesArrivetime holds the vehicle
//   3 arrive   arrival minute on the day clock, -1 when idle
//   4 order    carried Order.ID, -1 when none
//   5 source   where the engine keeps the vehicle: 0 idle list, 1 static arrival slot, 2 arrival ring, 3 far list, 4 far inbox
// A vehicle sits in exactly one container, so the block is a scatter without conflicts: every container entry is taken by one lane,
// which stores the entry's fields at [ext][veh] of the requested planes - plain loads and stores, no atomics, no LDS.  The caller
// fills the requested planes with -1 ahead of the launches (vds_api.hip), so a plane is written in full whatever the tables hold;
// a vehicle id outside [0, V) or a local node outside its cluster is never used as an index.
// Two kernels, because the containers have two shapes:
// k_vehicle_lists - the per-bucket containers: the idle list, the far list, the far inbox of the parity still to be drained and the
//   H slots of the arrival ring.  The state tables are cluster-major [C][R]: a workgroup takes ONE cluster, ONE container
//   (blockIdx.z: idle list, far list, far inbox, the ring) and 64 consecutive replicas; a group of VP_LPB lanes takes a bucket and
//   strides over its entries (consecutive entries: one 64-byte run of the dense idle list per step) - of the ring, each lane takes
//   whole slots; the 16 groups of a workgroup sit on 16 consecutive replicas, so the header / ring-count loads of a wavefront are
//   neighbouring records.  A group walks VP_RPT buckets (replicas 16 apart) with the
//   loads of each step issued together - the chain count -> entry -> cl_nodes is three dependent round trips, walked once for
//   VP_RPT buckets (IH_RPT of k_idle_heads); entries beyond the first VP_LPB of a bucket take a plain loop.
//   Dense ring entries {veh << 8 | dest_local, key} carry no minute: a dispatched vehicle's is in ring_min, an order-carrying
//   vehicle's is now0 + insert_tick * tick_minutes + PickupWaitTime + OrderValue (:954-960) and needs the order's sorted position
//   q: found by a binary search for the id in ord_q[tick_off[ins] .. tick_off[ins + 1]) - the id-ordered orders of the insert slot
//   (chosen over an id -> q table: no new table, no upload, and these entries are the rare ones - with static arrival slots only
//   the orders whose trip may outlive the ring horizon take the ring).
// k_vehicle_pull - the static arrival slots (Static.pull): the order-carrying vehicles of the dense tick.  Orders-major: the orders
//   that can still be on their way at slot `last` were processed in the slots (last - pull_hmax - pull_W, last], ONE contiguous
//   run of sorted positions [bkt_off[tlo * C], bkt_off[(last + 1) * C]) per replica; thread i takes position qlo + i of VP_RPT
//   consecutive replicas: so_slot / so_rec / out[r] are consecutive across the lanes, the entry D.arr[slot][r] is one 16-byte piece
//   for the four replicas.  In flight: processed (tins <= last, a0 + W > last), not pull_is_reject, pull_slots_ahead(e, last) > 0 -
//   read_lists_impl's test.  Byte model per (order of the window, replica): 8 B result + 4 B entry (a 32-byte sector per four
//   replicas) + per order so_slot 4 B, so_rec 16 B, d_rec 8 B shared by every replica that replays the day (L2).  (Walking the
//   destination buckets through d_first / d_rec like k_pack_obs would read the entries replica-contiguous, but an entry names no
//   order position: the wait and the value would need a slot -> q table.)
// A replica whose order day is over (order days per replica) reports its standing state at its own last slot: last = min(t_last, T_r - 1).
// The lists are compact wherever the entry points run it (HDR_RAW == 0, checked in the WKDEBUG build as k_idle_heads does).
// This file is hashed with the HOST sources (Makefile): it is not one of the tick kernels the profiles/ evidence refers to.
#include "vds_kernels_common.h"
#include "vds_launch.h"
#include <algorithm>
#ifdef WKDEBUG
#include <cstdio>
#endif

namespace vds {

#define VP_THREADS 256
#define VP_LPB 16                // lanes per bucket
#define VP_GROUPS (VP_THREADS / VP_LPB)
#define VP_RPT 4                 // buckets (k_vehicle_lists) / replicas (k_vehicle_pull) per thread: their loads are in flight together
enum { VP_IDLE = 0, VP_FL = 1, VP_INBOX = 2, VP_RING = 3 };      // container of a k_vehicle_lists workgroup; VP_RING + s: ring slot s
enum { SRC_IDLE = 0, SRC_PULL = 1, SRC_RING = 2, SRC_FL = 3, SRC_INBOX = 4 };      // VDS_VEH_SOURCE values (vds.h)

// entries of container z of bucket (c, r)
__device__ __forceinline__ int veh_count(const Static &S, const State &D, int z, int c, int r, int last) {
    const size_t b = (size_t)c * S.R + r;
    const int *h = D.hdr + b * HDR_WORDS;
    int n;
    if (z == VP_IDLE) {
        n = min(h[HDR_IDLE], S.idle_cap);
#ifdef WKDEBUG
        if (h[HDR_RAW] != 0) printf("k_vehicle_lists: raw list (HDR_RAW %d) c %d r %d\n", h[HDR_RAW], c, r);
#endif
    } else if (z == VP_FL) n = min(h[HDR_FL], S.fl_cap);
    else if (z == VP_INBOX) n = last < 0 ? 0 : min(h[HDR_INBOX0 + ((last + 1) & 1)], S.in_cap);      // (none before the first step)
    else n = min(D.ring_cnt[((size_t)(z - VP_RING) * S.C + c) * S.R + r] & 0xFFFF, S.ring_cap);
    return max(n, 0);
}

__device__ __forceinline__ int4 veh_wide(int4 e) { return make_int4(e.x, meta_is_dispatch(e.w) ? -1 : e.y, e.z, meta_dest(e.w)); }

// entry p of container z of bucket (c, r) as {vehicle, order (-1: none), arrival minute (-1: idle), local node in cluster c}
__device__ __forceinline__ int4 veh_entry(const Static &S, const State &D, int z, int c, int r, int last, int p) {
    const size_t b = (size_t)c * S.R + r;
    if (z == VP_IDLE) {
        const uint2 e = idle_ref(S, D, c, r).get(p);
        return make_int4((int)e.x, -1, -1, (int)e.y);
    }
    if (z == VP_FL) return veh_wide(D.fl[b * S.fl_cap + p]);
    if (z == VP_INBOX) return veh_wide(D.inbox[((size_t)((last + 1) & 1) * S.C * S.R + b) * S.in_cap + p]);
    const size_t i = (((size_t)(z - VP_RING) * S.C + c) * S.R + r) * S.ring_cap + p;
    if (!S.dense) return veh_wide(D.ring[i]);
    const uint2 e = ring2(D)[i];
    const int veh = (int)(e.x >> 8), loc = (int)(e.x & 0xFFu), id = dense_key_id(e.y);
    if (dense_key_is_dispatch(e.y)) return make_int4(veh, -1, S.ring_min_on ? D.ring_min[i] : -1, loc);
    // order-carrying: the minute from the order's result; its sorted position by the id among the insert slot's orders
    const DayView dv = day_view(S, r);
    const int ins = dense_key_tick(e.y, max(last, 0));
    int arrive = -1;
    if (ins >= 0 && ins < dv.T) {
        int lo = dv.tick_off[ins];
        const int end = dv.tick_off[ins + 1];
        int hi = end;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (S.so_rec[S.ord_q[mid]].x < id) lo = mid + 1;
            else hi = mid;
        }
        if (lo < end) {
            const int q = S.ord_q[lo];
            const int4 rec = S.so_rec[q];
            if (rec.x == id) arrive = dv.now0 + ins * S.tick_minutes + out_row(S, D, r)[q].y + rec.w;
        }
    }
    return make_int4(veh, id, arrive, loc);
}

struct VehOut { int *p; size_t plane; int V, planes; };
__device__ __forceinline__ void veh_store(const VehOut &o, int ext, int veh, int state, int node, int cluster, int arrive, int order, int source) {
    if ((unsigned)veh >= (unsigned)o.V) return;       // (a corrupt entry: never an index)
    int *p = o.p + (size_t)ext * o.V + veh;
    if (o.planes & 1) p[0] = state;
    if (o.planes & 2) p[o.plane] = node;
    if (o.planes & 4) p[2 * o.plane] = cluster;
    if (o.planes & 8) p[3 * o.plane] = arrive;
    if (o.planes & 16) p[4 * o.plane] = order;
    if (o.planes & 32) p[5 * o.plane] = source;
}

// Container z of cluster c for the VP_RPT buckets of a lane group (replicas rb + u * VP_GROUPS): the lane takes the entries p0, p0 + stride, ...
// of each - the counts of the VP_RPT buckets are loaded together, then their first entries, then the nodes; further entries take a plain loop.
__device__ __forceinline__ void veh_walk(const Static &S, const State &D, const VehOut &o, int z, int c, int rb, const int (&ext)[VP_RPT],
                                         const int (&last)[VP_RPT], int p0, int stride, int col0, int nc) {
    const int source = z == VP_IDLE ? SRC_IDLE : z == VP_FL ? SRC_FL : z == VP_INBOX ? SRC_INBOX : SRC_RING;
    int n[VP_RPT];
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u) n[u] = ext[u] >= 0 ? veh_count(S, D, z, c, rb + u * VP_GROUPS, last[u]) : 0;
    int4 e[VP_RPT];
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u) {
        e[u] = make_int4(-1, -1, -1, 0);
        if (p0 < n[u]) e[u] = veh_entry(S, D, z, c, rb + u * VP_GROUPS, last[u], p0);
    }
    int node[VP_RPT];
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u) {
        node[u] = -1;
        if (p0 < n[u] && (unsigned)e[u].w < (unsigned)nc) node[u] = S.cl_nodes[col0 + e[u].w];
    }
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u)
        if (p0 < n[u]) veh_store(o, ext[u], e[u].x, z == VP_IDLE ? 0 : e[u].y >= 0 ? 1 : 2, node[u], c, e[u].z, e[u].y, source);
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u)
        for (int p = p0 + stride; p < n[u]; p += stride) {
            const int4 f = veh_entry(S, D, z, c, rb + u * VP_GROUPS, last[u], p);
            const int nd = (unsigned)f.w < (unsigned)nc ? S.cl_nodes[col0 + f.w] : -1;
            veh_store(o, ext[u], f.x, z == VP_IDLE ? 0 : f.y >= 0 ? 1 : 2, nd, c, f.z, f.y, source);
        }
}

// t_last: slot stepped last, -1 before the first step.  planes: bit k = plane k is wanted.  out: int32 [6][R_ext][V].
// Grid: x = cluster, y = runs of VP_GROUPS * VP_RPT replicas from S.r_lo on (stored order), up to r_end, z = VP_IDLE / VP_FL / VP_INBOX /
// VP_RING (the whole ring: lane j of a group takes the slots j, j + VP_LPB, ... of its buckets, entry by entry - a slot holds the few
// vehicles that arrive in one cluster in one slot, and most slots none: one workgroup per ring slot was 32 of 35 workgroups per
// (cluster, 64 replicas) that found nothing at configs[1]).
__global__ __launch_bounds__(VP_THREADS) void k_vehicle_lists(Static S, State D, int t_last, int planes, int r_end, int *__restrict__ out) {
    const int c = (int)blockIdx.x, z = (int)blockIdx.z;
    const int g = (int)threadIdx.x / VP_LPB, j = (int)threadIdx.x & (VP_LPB - 1);
    const int rb = S.r_lo + (int)blockIdx.y * (VP_GROUPS * VP_RPT) + g;
    const VehOut o{out, (size_t)S.R_ext * S.V, S.V, planes};
    int ext[VP_RPT], last[VP_RPT];
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u) {
        const int r = rb + u * VP_GROUPS;
        ext[u] = -1; last[u] = -1;
        if (r >= r_end) continue;
        ext[u] = S.int2ext ? S.int2ext[r] : r;                 // block in the caller's replica order (regrouped storage: int2ext; -1: padding)
        if (ext[u] < 0) continue;
        last[u] = min(t_last, day_view(S, r).T - 1);           // a replica whose day is over stopped at its own last slot
    }
    const int col0 = S.cl_off[c], nc = S.cl_off[c + 1] - col0;
    if (z < VP_RING) veh_walk(S, D, o, z, c, rb, ext, last, j, VP_LPB, col0, nc);
    else
        for (int s = j; s < S.H; s += VP_LPB) veh_walk(S, D, o, VP_RING + s, c, rb, ext, last, 0, 1, col0, nc);
}

// Grid: x = runs of VP_THREADS sorted positions of the window, y = runs of VP_RPT replicas from S.r_lo on (stored order), up to r_end.
__global__ __launch_bounds__(VP_THREADS) void k_vehicle_pull(Static S, State D, int t_last, int planes, int r_end, int *__restrict__ out) {
    const int i = (int)blockIdx.x * VP_THREADS + (int)threadIdx.x;
    const int rb = S.r_lo + (int)blockIdx.y * VP_RPT;
    const VehOut o{out, (size_t)S.R_ext * S.V, S.V, planes};
    int ext[VP_RPT], last[VP_RPT], q[VP_RPT], now0[VP_RPT], dbase[VP_RPT];
    const int2 *res[VP_RPT];
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u) {
        const int r = rb + u;
        ext[u] = -1; last[u] = -1; q[u] = -1; now0[u] = 0; dbase[u] = 0; res[u] = D.out;
        if (r >= r_end) continue;
        ext[u] = S.int2ext ? S.int2ext[r] : r;
        if (ext[u] < 0) continue;
        // the replica's day: {bkt_base, now0, T, q_base}
        const int4 rd = S.n_days <= 1 ? make_int4(0, S.now0, S.T, 0) : S.replica_desc[r];
        last[u] = min(t_last, rd.z - 1);
        if (last[u] < 0) continue;
        now0[u] = rd.y;
        dbase[u] = S.n_days <= 1 ? 0 : S.replica_desc2[r].y;
        const int *bkt = S.bkt_off + rd.x;
        const int tlo = max(last[u] - S.pull_hmax - S.pull_W + 1, 0);
        const int qlo = bkt[(size_t)tlo * S.C], qhi = bkt[(size_t)(last[u] + 1) * S.C];
        if (i < qhi - qlo) q[u] = qlo + i;
        res[u] = D.out + (size_t)r * S.Oq - rd.w;              // indexed by absolute sorted position
    }
    int slot[VP_RPT];
    int4 rec[VP_RPT];
    int2 rs[VP_RPT];
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u) {
        slot[u] = -1; rec[u] = make_int4(0, 0, 0, 0); rs[u] = make_int2(-1, 0);
        if (q[u] >= 0) { slot[u] = S.so_slot[q[u]]; rec[u] = S.so_rec[q[u]]; rs[u] = res[u][q[u]]; }
        if (slot[u] >= S.arr_slots) slot[u] = -1;
    }
    int ry[VP_RPT];
    unsigned en[VP_RPT];
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u) {
        ry[u] = 0; en[u] = 0u;
        if (slot[u] >= 0) { ry[u] = S.d_rec[dbase[u] + slot[u]].y; en[u] = D.arr[arr_index(S.R, slot[u], rb + u)]; }
    }
    int node[VP_RPT];
    bool fly[VP_RPT];
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u) {
        const int a0 = ry[u] & 0xFFFF, tins = a0 - (int)((unsigned)ry[u] >> 24);
        // (tins > last: not processed yet; a0 + W <= last: arrived for sure - the entry's slot byte only means something within 127 slots)
        fly[u] = slot[u] >= 0 && tins <= last[u] && a0 + S.pull_W > last[u] && !pull_is_reject(en[u]) && pull_slots_ahead(en[u], last[u]) > 0;
        const int dc = rec[u].z & 0xFFFF, dl = (int)((unsigned)rec[u].y >> 16);
        node[u] = -1;
        if (fly[u] && dc < S.C) {
            const int col0 = S.cl_off[dc];
            if (dl < S.cl_off[dc + 1] - col0) node[u] = S.cl_nodes[col0 + dl];
        }
        ry[u] = tins;
    }
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u)
        if (fly[u]) veh_store(o, ext[u], (int)(en[u] >> 8), 1, node[u], rec[u].z & 0xFFFF, now0[u] + ry[u] * S.tick_minutes + rs[u].y + rec[u].w, rec[u].x, SRC_PULL);
}

// The -1 fill of the requested planes, ahead of the scatter: the rows of the replicas [S.r_lo, r_end) (stored order).  A kernel, so
// that the refresh is one sequence on a stream and inside vds_run_hooked's day graph, which carries kernel nodes only.
// Grid: x = replica, y = runs of VP_THREADS vehicles.
__global__ __launch_bounds__(VP_THREADS) void k_vehicle_fill(Static S, int planes, int r_end, int *__restrict__ out) {
    const int v = (int)blockIdx.y * VP_THREADS + (int)threadIdx.x;
    const int r = S.r_lo + (int)blockIdx.x;
    if (v >= S.V || r >= r_end) return;
    const int ext = S.int2ext ? S.int2ext[r] : r;
    if (ext < 0) return;
    const size_t plane = (size_t)S.R_ext * S.V;
    int *p = out + (size_t)ext * S.V + v;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (planes >> k & 1) p[k * plane] = -1;
}

void emit_vehicle_fill(const Emit &e, const Static &S0, int planes, int *out, int r_lo, int r_n) {
    Static S = S0;
    S.r_lo = r_lo;
    const int n = r_n > 0 ? r_n : S.R - r_lo;
    const dim3 grid(n, (S.V + VP_THREADS - 1) / VP_THREADS), block(VP_THREADS);
    emit_kernel(e, k_vehicle_fill, grid, block, 0, S, planes, r_lo + n, out);
}

void emit_vehicle_lists(const Emit &e, const Static &S0, const State &D, int t_last, int planes, int *out, int r_lo, int r_n) {
    Static S = S0;
    S.r_lo = r_lo;
    const int n = r_n > 0 ? r_n : S.R - r_lo, per = VP_GROUPS * VP_RPT;
    const dim3 grid(S.C, (n + per - 1) / per, VP_RING + 1), block(VP_THREADS);
    emit_kernel(e, k_vehicle_lists, grid, block, 0, S, D, t_last, planes, r_lo + n, out);
}

bool vehicle_pull_needed(const Static &S, int t_last) { return S.pull && t_last >= 0 && S.Oq > 0; }

void emit_vehicle_pull(const Emit &e, const Static &S0, const State &D, int t_last, int planes, int *out, int r_lo, int r_n) {
    Static S = S0;
    S.r_lo = r_lo;
    const int n = r_n > 0 ? r_n : S.R - r_lo;
    // the longest window any replica can have: (hmax + W) slots of at most max_tick_orders orders, never more than a day's orders
    const long long win = std::min<long long>((long long)(S.pull_hmax + S.pull_W) * std::max(S.max_tick_orders, 1), S.Oq);
    const dim3 grid((unsigned)((std::max<long long>(win, 1) + VP_THREADS - 1) / VP_THREADS), (n + VP_RPT - 1) / VP_RPT), block(VP_THREADS);
    emit_kernel(e, k_vehicle_pull, grid, block, 0, S, D, t_last, planes, r_lo + n, out);
}

}  // namespace vds
