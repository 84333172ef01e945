// libvds host unit: what a caller reads of an episode - the observation planes, the counters, the six derived blocks (slot outcomes,
// idle heads, per-vehicle planes, per-vehicle outcomes, idle roster, per-order results) on the device and on the host, and the host
// read-backs vds_read_orders / vds_read_lists / vds_read_vehicles / vds_read_work.  Who refreshes a derived block, with which kernels
// in what order, is said here and nowhere else (ensure_* / refresh_*: the hooked day, vds_api.hip, calls them too).
#include "vds_handle.h"

// A derived block of n elements, made on the first request (it lives with the state tables, MEM_STATE: re-made when they are).  fill:
// the byte every element holds until the first refresh; negative: none - nobody sees the block before a kernel has written all of it.
template <typename T>
static int ensure_block(vds_handle *h, T **p, size_t n, int fill) {
    if (*p) return VDS_OK;
    const int rc = dev_alloc(h, MEM_STATE, p, n);
    if (rc) { *p = nullptr; return rc; }
    if (fill >= 0) HIPCHK(h, hipMemsetAsync(*p, fill, n * sizeof(T), h->stream));
    return VDS_OK;
}

// plane i (n elements each) of the device block `blk` to dst[i], for the k planes whose dst[i] is not null; then vds_sync
template <typename T>
static int read_planes(vds_handle *h, const T *blk, size_t n, void *const *dst, int k) {
    for (int i = 0; i < k; ++i)
        if (dst[i]) HIPCHK(h, hipMemcpyAsync(dst[i], blk + i * n, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    return vds_sync(h);
}

int ensure_outcomes(vds_handle *h) { return ensure_block(h, &h->d_outc, 4 * (size_t)h->R_ext * h->S.C, 0); }
// (-1: "in neither container" until a plane's first refresh)
int ensure_vehicles(vds_handle *h) { return ensure_block(h, &h->d_veh, std::max<size_t>(6 * (size_t)h->R_ext * h->S.V, 1), 0xFF); }
int ensure_vehicle_outcomes(vds_handle *h) { return ensure_block(h, &h->d_vout, std::max<size_t>(4 * (size_t)h->R_ext * h->S.V, 4), -1); }
// (the block is made for one L: it lives with the state tables - re-made when they are, and when another L is asked for)
int ensure_idle_heads(vds_handle *h, int L) {
    if (h->d_heads && h->heads_L == L) return VDS_OK;
    if (h->d_heads) {                                    // another L: the block is made again (work that reads the old one may be in flight)
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->mem[MEM_STATE].release(h->d_heads);
        h->d_heads = nullptr; h->heads_L = 0;
    }
    const int rc = ensure_block(h, &h->d_heads, 2 * (size_t)h->R_ext * h->S.C * L, 0xFF);      // (-1: empty lists until the first refresh)
    if (h->d_heads) h->heads_L = L;
    return rc;
}
// (planes and offsets, roster_off, are ONE block)
int ensure_idle_roster(vds_handle *h) {
    if (h->d_roster) return VDS_OK;
    if (h->S.C > IDLE_ROSTER_C_MAX) return fail(h, VDS_ECAPACITY, "vds_idle_roster_device: %d clusters; k_idle_roster keeps a replica's offsets in LDS, at most %d", h->S.C, (int)IDLE_ROSTER_C_MAX);
    return ensure_block(h, &h->d_roster, 3 * (size_t)h->R_ext * h->S.V + (size_t)h->R_ext * (h->S.C + 1), -1);
}
// (lives with `out`, MEM_RESULTS; not cleared: the first full refresh writes every element)
int ensure_orders(vds_handle *h) {
    if (h->d_orders) return VDS_OK;
    const int rc = dev_alloc(h, MEM_RESULTS, &h->d_orders, 2 * (size_t)h->R_ext * h->O);
    if (rc) h->d_orders = nullptr;
    return rc;
}

// The two derived blocks that take more than one kernel, for the replicas [r_lo, r_lo + r_n) (r_n <= 0: all), on a stream or as
// nodes of a day graph.  Every element of a requested plane / of the block is written, whatever the memory held: -1 first, then the scatter.
// Per-vehicle planes `planes` of d_veh as slot t_last left them (-1: none stepped since the reset)
void refresh_vehicles(Chain &c, vds_handle *h, int t_last, int planes, int r_lo, int r_n) {
    c.add(emit_vehicle_fill, h->S, planes, h->d_veh, r_lo, r_n);
    c.add(emit_vehicle_lists, h->S, h->D, t_last, planes, h->d_veh, r_lo, r_n);
    if (vehicle_pull_needed(h->S, t_last)) c.add(emit_vehicle_pull, h->S, h->D, t_last, planes, h->d_veh, r_lo, r_n);
}
// What each vehicle earned in slot t (stepped == 0: none stepped since the reset, the fill stands), d_vout
void refresh_vehicle_outcomes(Chain &c, vds_handle *h, int t, int stepped, int r_lo, int r_n) {
    c.add(emit_vehicle_outcomes_fill, h->S, h->d_vout, r_lo, r_n);
    if (stepped && h->S.Oq > 0) c.add(emit_vehicle_outcomes, h->S, h->D, t, stepped, h->d_vout, r_lo, r_n);
}

// Rows of d_orders of the orders processed in slots [slot_lo, slot_hi]; last: the slot stepped last (-1: none since the reset - the
// range reads pending).  One kernel; its grid follows the longest id range one replica can have in these slots.
void refresh_orders_block(Chain &c, vds_handle *h, int slot_lo, int slot_hi, int last, int r_lo, int r_n) {
    int tail = 0;                        // a range that reaches a day's last slot runs to the end of the row
    for (const DayHost &H : h->days)
        if (slot_lo < H.T && slot_hi >= H.T - 1) tail = std::max(tail, h->O - H.Oq);
    const long long slots = (long long)std::min(slot_hi, h->S.T - 1) - slot_lo + 1;
    if (slots <= 0) return;              // every day is over before the range
    const int ids = (int)std::min<long long>(h->O, slots * h->S.max_tick_orders + tail);
    c.add(emit_orders_block, h->S, h->D, slot_lo, slot_hi, last, h->O, ids, h->d_orders, r_lo, r_n);
}

// A derived block refreshed on the handle's stream NOW, over all replicas: what the six vds_*_device entry points (`fn`) and the
// vds_read_* behind them do around their own parts - callable at all, `args` (the entry point's own argument check: VDS_OK or the
// refusal), the device, `ensure` (the block made), `refresh` (its kernels added to the chain; VDS_OK or what failed), the launch status.
template <typename A, typename E, typename R>
static int refresh_now(vds_handle *h, const char *fn, A args, E ensure, R refresh) {
    if (!h || !h->have_reset) return fail(h, VDS_EINVAL, "%s: call vds_reset first", fn);
    int rc = args();
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = ensure())) return rc;
    { Chain c(h->stream); if ((rc = refresh(c))) return rc; }
    HIPCHK(h, hipGetLastError());
    return VDS_OK;
}
static int no_args() { return VDS_OK; }

// The counters reduced on the stream now (d_cnt_per per replica, d_cnt_tot their sum): how the counter entry points begin.
// args_ok: the entry point's own arguments are there; refusal: its message otherwise, and before vds_reset
static int reduce_counters_now(vds_handle *h, bool args_ok, const char *refusal) {
    if (!h || !h->have_reset || !args_ok) return fail(h, VDS_EINVAL, "%s", refusal);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    launch_reduce_counters(h->S, h->D, h->d_cnt_per, h->d_cnt_tot, h->stream);
    HIPCHK(h, hipGetLastError());
    return VDS_OK;
}

extern "C" {

int vds_obs_device_planes(vds_handle *h, int32_t planes, void **dev_ptr) { return guarded(h, "vds_obs_device_planes", [&] {
    if (!h || !h->have_reset) return fail(h, VDS_EINVAL, "vds_obs_device: call vds_reset first");
    if (planes <= 0 || planes > 31) return fail(h, VDS_EINVAL, "vds_obs_device_planes: planes is a mask of the five planes (1 .. 31)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    launch_pack_obs(h->S, h->D, h->last_stepped < 0 ? 0 : h->last_stepped, h->last_stepped >= 0 ? 1 : 0, planes, h->d_obs, h->stream);
    HIPCHK(h, hipGetLastError());
    if (dev_ptr) *dev_ptr = h->d_obs;
    return VDS_OK;
}); }
int vds_obs_device(vds_handle *h, void **dev_ptr) { return vds_obs_device_planes(h, 31, dev_ptr); }

int vds_obs_inplace(vds_handle *h, int32_t plane, void **dev_ptr, int64_t *stride_replica, int64_t *stride_cluster) { return guarded(h, "vds_obs_inplace", [&] {
    if (!h || !h->have_orders) return fail(h, VDS_EINVAL, "vds_obs_inplace: load orders first (the state tables are made by the load)");
    if (!dev_ptr || !stride_replica || !stride_cluster) return fail(h, VDS_EINVAL, "vds_obs_inplace: null output pointer");
    const int word = plane == 0 ? HDR_IDLE_PRE : (plane == 1 ? HDR_IDLE : (plane == 3 ? HDR_ORDERS : -1));
    if (word < 0) return fail(h, VDS_EINVAL, "vds_obs_inplace: plane %d is not kept in place (0 idle_pre, 1 idle_now, 3 cl_orders are; supply and inflight: vds_obs_device_planes)", plane);
    if (h->S.int2ext != nullptr || h->S.rperm != nullptr || h->S.R != h->R_ext)
        return fail(h, VDS_ESTATE, "vds_obs_inplace: the replicas are stored regrouped by order day (not in the caller's order): use vds_obs_device_planes");
    *dev_ptr = h->D.hdr + word;
    *stride_replica = HDR_WORDS;
    *stride_cluster = (int64_t)h->S.R * HDR_WORDS;
    return VDS_OK;
}); }

int vds_read_obs(vds_handle *h, int32_t *idle_pre, int32_t *idle_now, int32_t *supply, int32_t *cl_orders, int32_t *inflight) { return guarded(h, "vds_read_obs", [&] {
    int rc = vds_obs_device(h, nullptr);
    if (rc) return rc;
    void *dst[5] = {idle_pre, idle_now, supply, cl_orders, inflight};
    return read_planes(h, h->d_obs, (size_t)h->R_ext * h->S.C, dst, 5);
}); }

// value of the orders of replica r's day that have not been processed (yet): they count in SumOrderValue (:1095-1100)
static long long unprocessed_value(const vds_handle *h, int r) {
    const DayHost &H = h->days[h->replica_day[r]];
    const int tdone = h->last_stepped + 1;   // ticks whose orders have been processed
    const long long processed_value = H.value_upto.empty() ? 0 : H.value_upto[std::min<size_t>(tdone, H.value_upto.size() - 1)];
    return H.value_all - processed_value;
}

static void finish_counters(const vds_handle *h, int r, const long long *raw, int64_t *out) {
    // raw: CNT_* slots; out: VDS_CNT_* slots
    out[VDS_CNT_ORDER_NUM] = raw[CNT_ORDERS];
    out[VDS_CNT_REJECT_NUM] = raw[CNT_REJECTS];
    out[VDS_CNT_MATCHED] = raw[CNT_ORDERS] - raw[CNT_REJECTS];
    out[VDS_CNT_WAIT_SUM] = raw[CNT_WAIT];
    out[VDS_CNT_DISPATCH_NUM] = raw[CNT_DISPATCH];
    out[VDS_CNT_DISPATCH_COST] = raw[CNT_DISPATCH_COST];
    // :1095-1100 sums OrderValue over every order whose ArriveInfo != "Reject": matched + not (yet) processed
    out[VDS_CNT_VALUE_SUM] = raw[CNT_VALUE] + unprocessed_value(h, r);
    out[VDS_CNT_EVALS] = raw[CNT_EVALS];
}

// SupplyExpect (:880-891) where the tick kernels keep it (dense layout, one shared order day): the ring of planes [32][C][R] by arrival
// slot and the device word that says which plane is SupplyExpect of the slot stepped last - both at fixed addresses, so a policy
// captured once as a graph reads ring[*slot] every slot.  No observation pass.
int vds_supply_inplace(vds_handle *h, void **ring, int64_t *stride_plane, int64_t *stride_replica, int64_t *stride_cluster, void **slot_word, int32_t *planes) { return guarded(h, "vds_supply_inplace", [&] {
    if (!h || !h->have_orders) return fail(h, VDS_EINVAL, "vds_supply_inplace: load orders first (the state tables are made by the load)");
    if (!ring || !stride_plane || !stride_replica || !stride_cluster || !slot_word || !planes) return fail(h, VDS_EINVAL, "vds_supply_inplace: null output pointer");
    if (!h->S.dense) return fail(h, VDS_ESTATE, "vds_supply_inplace: SupplyExpect is kept in place on the dense layout only (this handle runs the wide layout: vds_obs_device_planes)");
    if (h->S.n_days > 1 || h->S.int2ext != nullptr || h->S.rperm != nullptr || h->S.R != h->R_ext)
        return fail(h, VDS_ESTATE, "vds_supply_inplace: order days per replica (replicas whose day is over stand still at their own slot; the storage may be regrouped): use vds_obs_device_planes");
    if (!h->D.sup) {
        // the first request switches the planes on: the tick kernels maintain them from the next episode on (a hook-less day does
        // not pay for them: 8 % of the headline, profiles/r06/supply_inplace_ab.txt).  The episode in progress has no planes: reset.
        HIPCHK(h, hipSetDevice(h->cfg.device));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->want_sup = true;
        int rc;
        if ((rc = dev_alloc(h, MEM_STATE, &h->D.sup, (size_t)VDS_SUP_PLANES * h->S.C * h->S.R)) || (rc = dev_alloc(h, MEM_STATE, &h->D.sup_slot, (size_t)1))) { h->D.sup = nullptr; h->D.sup_slot = nullptr; return rc; }
        HIPCHK(h, hipMemsetAsync(h->D.sup, 0, (size_t)VDS_SUP_PLANES * h->S.C * h->S.R * sizeof(int), h->stream));
        HIPCHK(h, hipMemsetAsync(h->D.sup_slot, 0, sizeof(int), h->stream));
        invalidate(h, GRAPH_TABLES | STATE_MEANING);
        h->have_reset = false;                      // vds_reset / vds_reset_again / vds_reset_random must follow
        clock_reset(h);
    }
    *ring = h->D.sup; *slot_word = h->D.sup_slot; *planes = VDS_SUP_PLANES;
    *stride_plane = (int64_t)h->S.C * h->S.R; *stride_cluster = h->S.R; *stride_replica = 1;
    return VDS_OK;
}); }

int vds_counters_device(vds_handle *h, void **dev_ptr) { return guarded(h, "vds_counters_device", [&] {
    const int rc = reduce_counters_now(h, dev_ptr != nullptr, "vds_counters_device: bad argument / call order");
    if (!rc) *dev_ptr = h->d_cnt_per;
    return rc;
}); }

// Per-cluster order outcomes of the slot stepped last (RewardFunction's view of Cluster.Orders, :999-1004): k_slot_outcomes into the
// int64 [4][R_ext][C] block, made on the first request (it lives with the state tables: re-made when they are).
static int outcomes_device_impl(vds_handle *h, void **dev_ptr) {
    const int rc = refresh_now(h, "vds_outcomes_device", no_args, [&] { return ensure_outcomes(h); }, [&](Chain &c) {
        if (h->last_stepped < 0) HIPCHK(h, hipMemsetAsync(h->d_outc, 0, 4 * (size_t)h->R_ext * h->S.C * sizeof(long long), h->stream));
        else c.add(emit_slot_outcomes, h->S, h->D, h->last_stepped, 1, h->d_outc, 0, 0);
        return VDS_OK;
    });
    if (!rc && dev_ptr) *dev_ptr = h->d_outc;
    return rc;
}

int vds_outcomes_device(vds_handle *h, void **dev_ptr) { return guarded(h, "vds_outcomes_device", [&] { return outcomes_device_impl(h, dev_ptr); }); }
int vds_read_outcomes(vds_handle *h, int64_t *served, int64_t *rejected, int64_t *wait_sum, int64_t *value_sum) { return guarded(h, "vds_read_outcomes", [&] {
    const int rc = outcomes_device_impl(h, nullptr);
    if (rc) return rc;
    void *dst[4] = {served, rejected, wait_sum, value_sum};
    return read_planes(h, h->d_outc, (size_t)h->R_ext * h->S.C, dst, 4);
}); }

// The first L entries of every idle list (Cluster.IdleVehicles as DispatchFunction walks it, :893-898; objects.py: Vehicle.ID,
// Vehicle.LocationNode): k_idle_heads into the int32 [2][R_ext][C][L] block, made on the first request for this L (ensure_idle_heads).
static int idle_heads_device_impl(vds_handle *h, int32_t L, void **dev_ptr) {
    const int rc = refresh_now(h, "vds_idle_heads_device", [&] {
        return L < 1 || L > VDS_IDLE_HEADS_MAX ? fail(h, VDS_EINVAL, "vds_idle_heads_device: L = %d is outside 1 .. %d list positions", L, VDS_IDLE_HEADS_MAX) : VDS_OK;
    }, [&] { return ensure_idle_heads(h, L); }, [&](Chain &c) { c.add(emit_idle_heads, h->S, h->D, L, h->d_heads, 0, 0); return VDS_OK; });
    if (!rc && dev_ptr) *dev_ptr = h->d_heads;
    return rc;
}
int vds_idle_heads_device(vds_handle *h, int32_t L, void **dev_ptr) { return guarded(h, "vds_idle_heads_device", [&] { return idle_heads_device_impl(h, L, dev_ptr); }); }
int vds_read_idle_heads(vds_handle *h, int32_t L, int32_t *veh, int32_t *node) { return guarded(h, "vds_read_idle_heads", [&] {
    const int rc = idle_heads_device_impl(h, L, nullptr);
    if (rc) return rc;
    void *dst[2] = {veh, node};
    return read_planes(h, h->d_heads, (size_t)h->R_ext * h->S.C * L, dst, 2);
}); }

// The fields of `Vehicle` that the tick path changes (objects.py:75-89) for every replica at once: k_vehicle_lists / k_vehicle_pull
// (vds_vehicle_planes.hip) into the int32 [6][R_ext][V] block, made on the first request (it lives with the state tables: re-made
// when they are).  read_lists_impl + vds_read_vehicles below are the specification of what the planes hold.
static int vehicles_device_impl(vds_handle *h, int32_t planes, void **dev_ptr) {
    const int rc = refresh_now(h, "vds_vehicles_device", [&] {
        return planes < 1 || planes > 63 ? fail(h, VDS_EINVAL, "vds_vehicles_device: planes = %d is outside 1 .. 63", planes) : VDS_OK;
    }, [&] { return ensure_vehicles(h); }, [&](Chain &c) {
        if ((size_t)h->R_ext * h->S.V > 0) refresh_vehicles(c, h, h->last_stepped, planes, 0, 0);
        return VDS_OK;
    });
    if (!rc && dev_ptr) *dev_ptr = h->d_veh;
    return rc;
}
int vds_vehicles_device(vds_handle *h, int32_t planes, void **dev_ptr) { return guarded(h, "vds_vehicles_device", [&] { return vehicles_device_impl(h, planes, dev_ptr); }); }
int vds_read_vehicles_all(vds_handle *h, int32_t planes, int32_t *out) { return guarded(h, "vds_read_vehicles_all", [&] {
    if (h && h->have_reset && !out) return fail(h, VDS_EINVAL, "vds_read_vehicles_all: out is NULL");
    const int rc = vehicles_device_impl(h, planes, nullptr);
    if (rc) return rc;
    const size_t RV = (size_t)h->R_ext * h->S.V;
    for (int k = 0, n = 0; k < 6 && RV > 0; ++k)
        if (planes >> k & 1) HIPCHK(h, hipMemcpyAsync(out + (size_t)n++ * RV, h->d_veh + k * RV, RV * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return vds_sync(h);
}); }

// What each vehicle earned in the slot stepped last (MatchFunction's matches, :924-975): k_vehicle_outcomes_fill + k_vehicle_outcomes
// (vds_vehicle_outcomes.hip) into the int32 [R_ext][V][4] block, made on the first request (it lives with the state tables: re-made
// when they are).  Derived from `out` on request, like d_outc: nothing of it is kept between calls or saved in a snapshot.
static int vehicle_outcomes_device_impl(vds_handle *h, void **dev_ptr) {
    const int rc = refresh_now(h, "vds_vehicle_outcomes_device", no_args, [&] { return ensure_vehicle_outcomes(h); }, [&](Chain &c) {
        if ((size_t)h->R_ext * h->S.V > 0) refresh_vehicle_outcomes(c, h, std::max(h->last_stepped, 0), h->last_stepped >= 0 ? 1 : 0, 0, 0);
        return VDS_OK;
    });
    if (!rc && dev_ptr) *dev_ptr = h->d_vout;
    return rc;
}
int vds_vehicle_outcomes_device(vds_handle *h, void **dev_ptr) { return guarded(h, "vds_vehicle_outcomes_device", [&] { return vehicle_outcomes_device_impl(h, dev_ptr); }); }
int vds_read_vehicle_outcomes(vds_handle *h, int32_t *order, int32_t *wait, int32_t *value, int32_t *pickup) { return guarded(h, "vds_read_vehicle_outcomes", [&] {
    const int rc = vehicle_outcomes_device_impl(h, nullptr);
    if (rc) return rc;
    const size_t RV = (size_t)h->R_ext * h->S.V;
    if (RV == 0) return vds_sync(h);
    // one copy of the block, de-interleaved on the host
    std::vector<int32_t> blk(4 * RV);
    void *all[1] = {blk.data()};
    const int rcs = read_planes(h, h->d_vout, 4 * RV, all, 1);
    if (rcs) return rcs;
    int32_t *dst[4] = {order, wait, value, pickup};
    for (int k = 0; k < 4; ++k)
        if (dst[k])
            for (size_t i = 0; i < RV; ++i) dst[k][i] = blk[4 * i + k];
    return VDS_OK;
}); }

// Every idle vehicle of every replica in DispatchFunction's order (`for cluster in self.Clusters: for vehicle in cluster.IdleVehicles`,
// :893-898) - the idle group of read_lists_impl for all replicas: k_idle_roster (vds_idle_roster.hip) into the int32 [3][R_ext][V]
// planes and the int32 [R_ext][C + 1] offsets behind them, ONE block made on the first request (it lives with the state tables:
// re-made when they are).  Derived on request: nothing of it is saved in a snapshot.
static int idle_roster_device_impl(vds_handle *h, void **dev_planes, void **dev_off) {
    const int rc = refresh_now(h, "vds_idle_roster_device", no_args, [&] { return ensure_idle_roster(h); },
                               [&](Chain &c) { c.add(emit_idle_roster, h->S, h->D, h->d_roster, roster_off(h), 0, 0); return VDS_OK; });
    if (rc) return rc;
    h->roster_fresh = true;
    if (dev_planes) *dev_planes = h->d_roster;
    if (dev_off) *dev_off = roster_off(h);
    return VDS_OK;
}
int vds_idle_roster_device(vds_handle *h, void **dev_planes, void **dev_off) { return guarded(h, "vds_idle_roster_device", [&] { return idle_roster_device_impl(h, dev_planes, dev_off); }); }
int vds_read_idle_roster(vds_handle *h, int32_t *veh, int32_t *node, int32_t *cluster, int32_t *off) { return guarded(h, "vds_read_idle_roster", [&] {
    const int rc = idle_roster_device_impl(h, nullptr, nullptr);
    if (rc) return rc;
    void *dst[3] = {veh, node, cluster}, *dsto[1] = {off};
    const size_t RV = (size_t)h->R_ext * h->S.V;
    if (RV > 0) { const int rcp = read_planes(h, h->d_roster, RV, dst, 3); if (rcp) return rcp; }
    return read_planes(h, roster_off(h), (size_t)h->R_ext * (h->S.C + 1), dsto, 1);
}); }

// Per-order results in id order (the device form of vds_read_orders): k_orders_block (vds_orders_block.hip) refreshes, in the int32
// [R_ext][O][2] block made on the first request, the rows of the orders processed in slots [slot_lo, slot_hi]; every other row keeps
// what it held.  Derived from `out` on request: nothing of it is saved in a snapshot.
int vds_orders_device(vds_handle *h, int32_t slot_lo, int32_t slot_hi, void **dev_ptr) { return guarded(h, "vds_orders_device", [&] {
    const int rc = refresh_now(h, "vds_orders_device", [&] {
        return slot_lo < 0 || slot_lo > slot_hi ? fail(h, VDS_EINVAL, "vds_orders_device: slots %d .. %d: 0 <= slot_lo <= slot_hi", slot_lo, slot_hi) : VDS_OK;
    }, [&] { return ensure_orders(h); }, [&](Chain &c) { refresh_orders_block(c, h, slot_lo, slot_hi, h->last_stepped, 0, 0); return VDS_OK; });
    if (!rc && dev_ptr) *dev_ptr = h->d_orders;
    return rc;
}); }

int vds_read_counters(vds_handle *h, int64_t *out) { return guarded(h, "vds_read_counters", [&] {
    int rc = reduce_counters_now(h, out != nullptr, "vds_read_counters: bad argument / call order");
    if (rc) return rc;
    std::vector<long long> raw((size_t)h->R_ext * CNT_WORDS);
    HIPCHK(h, hipMemcpyAsync(raw.data(), h->d_cnt_per, raw.size() * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    if ((rc = vds_sync(h))) return rc;
    for (int r = 0; r < h->R_ext; ++r) finish_counters(h, r, raw.data() + (size_t)r * CNT_WORDS, out + (size_t)r * VDS_NUM_COUNTERS);
    return VDS_OK;
}); }

int vds_reduce_counters(vds_handle *h, int64_t *out, void **dev_ptr) { return guarded(h, "vds_reduce_counters", [&] {
    int rc = reduce_counters_now(h, true, "vds_reduce_counters: call vds_reset first");
    if (rc) return rc;
    if (dev_ptr) *dev_ptr = h->d_cnt_tot;
    if (out) {
        long long raw[CNT_WORDS];
        HIPCHK(h, hipMemcpyAsync(raw, h->d_cnt_tot, sizeof(raw), hipMemcpyDeviceToHost, h->stream));
        if ((rc = vds_sync(h))) return rc;
        // value of unprocessed orders counts once per replica
        int64_t tmp[VDS_NUM_COUNTERS];
        finish_counters(h, 0, raw, tmp);
        long long rest = 0;
        for (int r = 0; r < h->R_ext; ++r) rest += unprocessed_value(h, r);
        tmp[VDS_CNT_VALUE_SUM] = raw[CNT_VALUE] + rest;
        memcpy(out, tmp, sizeof(tmp));
    }
    return VDS_OK;
}); }

int vds_reduce_counters_into(vds_handle *h, void *dev_out) { return guarded(h, "vds_reduce_counters_into", [&] {
    const int rc = reduce_counters_now(h, dev_out != nullptr, "vds_reduce_counters_into: bad argument / call order");
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(dev_out, h->d_cnt_tot, CNT_WORDS * sizeof(long long), hipMemcpyDeviceToDevice, h->stream));
    return VDS_OK;
}); }

int vds_read_work(vds_handle *h, int64_t *out) { return guarded(h, "vds_read_work", [&] {
    if (!h || !h->have_reset || !out) return fail(h, VDS_EINVAL, "vds_read_work: bad argument / call order");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    launch_reduce_counters(h->S, h->D, h->d_cnt_per, h->d_cnt_tot, h->stream);
    long long raw[CNT_WORDS];
    HIPCHK(h, hipMemcpyAsync(raw, h->d_cnt_tot, sizeof(raw), hipMemcpyDeviceToHost, h->stream));
    int rc = vds_sync(h);
    if (rc) return rc;
    out[0] = 0;
    for (int r = 0; r < h->R_ext; ++r) out[0] += std::min(h->last_stepped + 1, h->days[h->replica_day[r]].T);
    out[1] = raw[CNT_ORDERS]; out[2] = raw[CNT_ORDERS] - raw[CNT_REJECTS]; out[3] = raw[CNT_EVALS];
    out[4] = raw[CNT_ARRIVALS]; out[5] = raw[CNT_DISPATCH]; out[7] = 0;
    {   // (replica, cluster, tick) buckets the fast kernel handed to a slower path since vds_reset (list beyond the register /
        // LDS tables, far arrivals, oversize arrival slot, cost block beyond LDS)
        int e[4] = {0, 0, 0, 0};
        HIPCHK(h, hipMemcpy(e, h->D.err, sizeof(e), hipMemcpyDeviceToHost));
        out[6] = e[2];
    }
    return VDS_OK;
}); }

int vds_read_orders(vds_handle *h, int32_t r0, int32_t nr, uint8_t *status, int32_t *vehicle, int32_t *wait) { return guarded(h, "vds_read_orders", [&] {
    if (!h || !h->have_reset) return fail(h, VDS_EINVAL, "vds_read_orders: call vds_reset first");
    const Static &S = h->S;
    if (r0 < 0 || nr < 0 || r0 + nr > h->R_ext) return fail(h, VDS_EINVAL, "vds_read_orders: replica range out of bounds");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = vds_sync(h);
    if (rc) return rc;
    const int Oq = S.Oq, O = h->O;     // row strides: the longest day's (a shorter day leaves the tail of its row at 0 / -1)
    std::vector<int2> res((size_t)nr * std::max(Oq, 1));
    if (Oq > 0 && nr > 0 && !h->ext2int.empty()) {
        for (int r = 0; r < nr; ++r)       // regrouped storage: the caller's replica r0 + r lives in row ext2int[r0 + r]
            HIPCHK(h, hipMemcpy(res.data() + (size_t)r * Oq, h->D.out + (size_t)h->ext2int[r0 + r] * Oq, (size_t)Oq * sizeof(int2), hipMemcpyDeviceToHost));
    } else if (Oq > 0 && nr > 0)
        HIPCHK(h, hipMemcpy(res.data(), h->D.out + (size_t)r0 * Oq, (size_t)nr * Oq * sizeof(int2), hipMemcpyDeviceToHost));
    for (int r = 0; r < nr; ++r) {
        const DayHost &H = h->days[h->replica_day[r0 + r]];
        const int last = std::min(h->last_stepped, H.T - 1);
        uint8_t *st = status ? status + (size_t)r * O : nullptr;
        int32_t *vv = vehicle ? vehicle + (size_t)r * O : nullptr;
        int32_t *ww = wait ? wait + (size_t)r * O : nullptr;
        for (int i = 0; i < O; ++i) {
            if (st) st[i] = 0;
            if (vv) vv[i] = -1;
            if (ww) ww[i] = -1;
        }
        for (int q = 0; q < H.Oq; ++q) {
            const int i = H.so_id[q];
            if (H.o_tick[i] > last) continue;                    // cursor has not reached it yet
            const int2 e = res[(size_t)r * Oq + q];
            if (st) st[i] = e.x >= 0 ? 1 : 2;
            if (vv) vv[i] = e.x;
            if (ww) ww[i] = e.x >= 0 ? e.y : -1;
        }
    }
    return VDS_OK;
}); }

static int read_lists_impl(vds_handle *h, int32_t replica, int32_t *idle_off, int32_t *idle_veh, int32_t *idle_node,
                   int32_t *arr_off, int32_t *arr_veh, int32_t *arr_min, int32_t *arr_order, int32_t *arr_node) {
    if (!h || !h->have_reset) return fail(h, VDS_EINVAL, "vds_read_lists: call vds_reset first");
    const Static &S = h->S;
    if (replica < 0 || replica >= h->R_ext) return fail(h, VDS_EINVAL, "vds_read_lists: replica out of range");
    const int replica_ext = replica;
    if (!h->ext2int.empty()) replica = h->ext2int[replica];          // row of the regrouped tables
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = vds_sync(h);
    if (rc) return rc;
    const int C = S.C, R = S.R;
    std::vector<int> hdr((size_t)C * HDR_WORDS);
    HIPCHK(h, hipMemcpy2D(hdr.data(), HDR_WORDS * sizeof(int), h->D.hdr + (size_t)replica * HDR_WORDS, (size_t)R * HDR_WORDS * sizeof(int), HDR_WORDS * sizeof(int), C, hipMemcpyDeviceToHost));
    const bool want_idle = idle_off && idle_veh;
    const bool want_arr = arr_off && arr_veh;
    if (want_idle) {
        std::vector<uint2> idle((size_t)C * S.idle_cap);
        if (S.dense) {      // packed entries {veh << 8 | loc}
            std::vector<unsigned> pk((size_t)C * S.idle_cap);
            HIPCHK(h, hipMemcpy2D(pk.data(), S.idle_cap * sizeof(unsigned), reinterpret_cast<const unsigned *>(h->D.idle) + (size_t)replica * S.idle_cap, (size_t)R * S.idle_cap * sizeof(unsigned), S.idle_cap * sizeof(unsigned), C, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < pk.size(); ++i) idle[i] = make_uint2(pk[i] >> 8, pk[i] & 0xFFu);
        } else
        HIPCHK(h, hipMemcpy2D(idle.data(), S.idle_cap * sizeof(uint2), h->D.idle + (size_t)replica * S.idle_cap, (size_t)R * S.idle_cap * sizeof(uint2), S.idle_cap * sizeof(uint2), C, hipMemcpyDeviceToHost));
        int n = 0;
        idle_off[0] = 0;
        for (int c = 0; c < C; ++c) {
            const int m = hdr[(size_t)c * HDR_WORDS + HDR_IDLE];
            for (int j = 0; j < m; ++j) {
                const uint2 e = idle[(size_t)c * S.idle_cap + j];
                idle_veh[n] = (int)e.x;
                if (idle_node) idle_node[n] = h->cl_nodes[h->cl_off[c] + (int)e.y];
                n++;
            }
            idle_off[c + 1] = n;
        }
        for (int k = n; k < S.V; ++k) {      // past the last list: -1 (vds.h)
            idle_veh[k] = -1;
            if (idle_node) idle_node[k] = -1;
        }
    }
    if (want_arr) {
        // parity holding far posts not yet drained; a replica whose day is over stopped at ITS last tick
        const int last = std::min(h->last_stepped, h->days[h->replica_day[replica_ext]].T - 1);
        const int np = (last + 1) & 1;
        const int H = S.H;
        std::vector<int4> fl((size_t)C * S.fl_cap), inb((size_t)C * S.in_cap), ring((size_t)H * C * S.ring_cap);
        std::vector<int> rcnt((size_t)H * C);
        HIPCHK(h, hipMemcpy2D(fl.data(), S.fl_cap * sizeof(int4), h->D.fl + (size_t)replica * S.fl_cap, (size_t)R * S.fl_cap * sizeof(int4), S.fl_cap * sizeof(int4), C, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy2D(inb.data(), S.in_cap * sizeof(int4), h->D.inbox + ((size_t)np * C * R + replica) * S.in_cap, (size_t)R * S.in_cap * sizeof(int4), S.in_cap * sizeof(int4), C, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy2D(rcnt.data(), sizeof(int), h->D.ring_cnt + replica, (size_t)R * sizeof(int), sizeof(int), (size_t)H * C, hipMemcpyDeviceToHost));
        if (S.dense) {
            // dense entries {veh << 8 | dest_local, key}: widened here.  The arrival minute of an order-carrying entry follows from
            // the order's result (RealExpTime of the slot it was matched in + PickupWaitTime + OrderValue, :954-960); a
            // dispatched vehicle's comes from ring_min
            std::vector<uint2> r2((size_t)H * C * S.ring_cap);
            std::vector<int> rmin((size_t)H * C * S.ring_cap);
            HIPCHK(h, hipMemcpy2D(r2.data(), S.ring_cap * sizeof(uint2), reinterpret_cast<const uint2 *>(h->D.ring) + (size_t)replica * S.ring_cap, (size_t)R * S.ring_cap * sizeof(uint2), S.ring_cap * sizeof(uint2), (size_t)H * C, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy2D(rmin.data(), S.ring_cap * sizeof(int), h->D.ring_min + (size_t)replica * S.ring_cap, (size_t)R * S.ring_cap * sizeof(int), S.ring_cap * sizeof(int), (size_t)H * C, hipMemcpyDeviceToHost));
            DayHost &DH = h->days[h->replica_day[replica_ext]];
            std::vector<int2> res((size_t)std::max(DH.Oq, 1));
            if (DH.Oq > 0) HIPCHK(h, hipMemcpy(res.data(), h->D.out + (size_t)replica * S.Oq, (size_t)DH.Oq * sizeof(int2), hipMemcpyDeviceToHost));
            if (DH.q_of.empty()) { DH.q_of.assign(std::max(DH.O, 1), -1); for (int q = 0; q < DH.Oq; ++q) DH.q_of[DH.so_id[q]] = q; }
            for (int sl = 0; sl < H; ++sl)
                for (int c = 0; c < C; ++c) {
                    const int k = std::min(rcnt[(size_t)sl * C + c] & 0xFFFF, S.ring_cap);
                    for (int j = 0; j < k; ++j) {
                        const size_t i = ((size_t)sl * C + c) * S.ring_cap + j;
                        const uint2 e = r2[i];
                        const int disp = dense_key_is_dispatch(e.y), id = dense_key_id(e.y), ins = dense_key_tick(e.y, std::max(last, 0));
                        int arrive = rmin[i];
                        if (!disp) {
                            const int q = (id >= 0 && id < DH.O) ? DH.q_of[id] : -1;
                            if (q < 0) return fail(h, VDS_ESTATE, "vds_read_lists: corrupt arrival entry (order %d)", id);
                            arrive = DH.now0 + ins * S.tick_minutes + res[q].y + DH.q_value[q];
                        }
                        ring[i] = make_int4((int)(e.x >> 8), id, arrive, meta_pack(ins, disp, (int)(e.x & 0xFFu)));
                    }
                }
        } else
        HIPCHK(h, hipMemcpy2D(ring.data(), S.ring_cap * sizeof(int4), h->D.ring + (size_t)replica * S.ring_cap, (size_t)R * S.ring_cap * sizeof(int4), S.ring_cap * sizeof(int4), (size_t)H * C, hipMemcpyDeviceToHost));
        // static arrival slots (dense tick, S.pull): the order-carrying vehicles on their way sit in D.arr[slot][R]
        std::vector<std::vector<int4>> pulled(S.pull ? C : 0);
        if (S.pull && last >= 0) {
            const int dday = h->replica_day[replica_ext];
            DayHost &DH = h->days[dday];
            const int4 d2 = h->pull_desc[dday];
            const size_t nslot = (size_t)d2.w;
            std::vector<unsigned> col(std::max<size_t>(nslot, 1));
            if (nslot) HIPCHK(h, hipMemcpy2D(col.data(), sizeof(unsigned), h->D.arr + arr_index(S.R, 0, replica), (size_t)R * sizeof(unsigned), sizeof(unsigned), nslot, hipMemcpyDeviceToHost));
            std::vector<int2> res((size_t)std::max(DH.Oq, 1));
            if (DH.Oq > 0) HIPCHK(h, hipMemcpy(res.data(), h->D.out + (size_t)replica * S.Oq, (size_t)DH.Oq * sizeof(int2), hipMemcpyDeviceToHost));
            // destination cluster of a slot: the slots are sorted by it; walk d_first of slot row 0
            std::vector<int> dfirst0((size_t)C + 1);
            {
                std::vector<int> row0((size_t)C);
                HIPCHK(h, hipMemcpy(row0.data(), S.d_first + d2.x, (size_t)C * sizeof(int), hipMemcpyDeviceToHost));
                for (int c = 0; c < C; ++c) dfirst0[c] = row0[c] - d2.y;
                dfirst0[C] = (int)nslot;
            }
            for (int c = 0; c < C; ++c)
                for (int i = dfirst0[c]; i < dfirst0[c + 1]; ++i) {
                    const int2 rec = h->pull_drec[(size_t)d2.y + i];
                    const int a0 = rec.y & 0xFFFF, dmin = (int)((unsigned)rec.y >> 24), tins = a0 - dmin;
                    if (tins > last || a0 + S.pull_W <= last) continue;      // not processed yet / arrived for sure (the entry's slot byte is only meaningful within 127 slots)
                    const unsigned e = col[i];
                    if (pull_is_reject(e) || pull_slots_ahead(e, last) <= 0) continue;      // rejected / arrived
                    const int q = h->pull_slot_q[(size_t)d2.y + i];
                    const int arrive = DH.now0 + tins * S.tick_minutes + res[q].y + DH.q_value[q];      // :954-960
                    pulled[c].push_back(make_int4((int)(e >> 8), dense_key_id((unsigned)rec.x), arrive, meta_pack(tins, 0, (rec.y >> 16) & 0xFF)));
                }
        }
        int n = 0;
        arr_off[0] = 0;
        std::vector<int4> ent;
        for (int c = 0; c < C; ++c) {
            ent.clear();
            if (S.pull) ent.insert(ent.end(), pulled[c].begin(), pulled[c].end());
            const int f = hdr[(size_t)c * HDR_WORDS + HDR_FL];
            const int q = last < 0 ? 0 : hdr[(size_t)c * HDR_WORDS + HDR_INBOX0 + np];
            for (int j = 0; j < f; ++j) ent.push_back(fl[(size_t)c * S.fl_cap + j]);
            for (int j = 0; j < q; ++j) ent.push_back(inb[(size_t)c * S.in_cap + j]);
            for (int sl = 0; sl < H; ++sl) {
                const int k = rcnt[(size_t)sl * C + c] & 0xFFFF;
                for (int j = 0; j < k; ++j) ent.push_back(ring[((size_t)sl * C + c) * S.ring_cap + j]);
            }
            std::sort(ent.begin(), ent.end(), [](const int4 &a, const int4 &b) { return entry_key(a.y, a.w) < entry_key(b.y, b.w); });
            for (const int4 &e : ent) {
                if (n >= S.V) return fail(h, VDS_ESTATE, "vds_read_lists: more in-flight entries than vehicles");
                arr_veh[n] = e.x;
                if (arr_min) arr_min[n] = e.z;
                if (arr_order) arr_order[n] = meta_is_dispatch(e.w) ? -1 : e.y;
                if (arr_node) arr_node[n] = h->cl_nodes[h->cl_off[c] + meta_dest(e.w)];
                n++;
            }
            arr_off[c + 1] = n;
        }
        for (int k = n; k < S.V; ++k) {      // past the last dict: -1 (vds.h)
            arr_veh[k] = -1;
            if (arr_min) arr_min[k] = -1;
            if (arr_order) arr_order[k] = -1;
            if (arr_node) arr_node[k] = -1;
        }
    }
    return VDS_OK;
}
int vds_read_lists(vds_handle *h, int32_t replica, int32_t *idle_off, int32_t *idle_veh, int32_t *idle_node,
                   int32_t *arr_off, int32_t *arr_veh, int32_t *arr_min, int32_t *arr_order, int32_t *arr_node) {
    return guarded(h, "vds_read_lists", [&] { return read_lists_impl(h, replica, idle_off, idle_veh, idle_node, arr_off, arr_veh, arr_min, arr_order, arr_node); });
}

int vds_read_vehicles(vds_handle *h, int32_t replica, uint8_t *state, int32_t *node, int32_t *cluster,
                      int32_t *arrive_min, int32_t *order) { return guarded(h, "vds_read_vehicles", [&] {
    if (!h || !h->have_reset) return fail(h, VDS_EINVAL, "vds_read_vehicles: call vds_reset first");
    const int C = h->S.C, V = h->S.V;
    std::vector<int32_t> io(C + 1), iv(V), in(V), ao(C + 1), av(V), am(V), aor(V), an(V);
    int rc = read_lists_impl(h, replica, io.data(), iv.data(), in.data(), ao.data(), av.data(), am.data(), aor.data(), an.data());
    if (rc) return rc;
    for (int v = 0; v < V; ++v) {       // a vehicle in neither container cannot happen; mark it if it does
        if (state) state[v] = 255;
        if (node) node[v] = -1;
        if (cluster) cluster[v] = -1;
        if (arrive_min) arrive_min[v] = -1;
        if (order) order[v] = -1;
    }
    for (int c = 0; c < C; ++c) {
        for (int k = io[c]; k < io[c + 1]; ++k) {
            const int v = iv[k];
            if (v < 0 || v >= V) return fail(h, VDS_ESTATE, "vds_read_vehicles: corrupt idle list");
            if (state) state[v] = 0;
            if (node) node[v] = in[k];
            if (cluster) cluster[v] = c;
        }
        for (int k = ao[c]; k < ao[c + 1]; ++k) {
            const int v = av[k];
            if (v < 0 || v >= V) return fail(h, VDS_ESTATE, "vds_read_vehicles: corrupt arrival table");
            if (state) state[v] = aor[k] >= 0 ? 1 : 2;
            if (node) node[v] = an[k];
            if (cluster) cluster[v] = c;
            if (arrive_min) arrive_min[v] = am[k];
            if (order) order[v] = aor[k];
        }
    }
    return VDS_OK;
}); }

}  // extern "C"
