// libvds host unit: vds_snapshot / vds_restore / vds_restore_device (the kernels: vds_snapshot.hip).
#include "vds_handle.h"

extern "C" {

// vds_snapshot / vds_restore: the episode state of every replica saved in a store next to the tables and copied back through a
// replica map (vds_snapshot.hip).  What is saved: hdr, cnt, idle, ring, ring_min, ring_cnt, fl, both inbox parities, sup, arr, out and the
// clock (t, last_stepped, the dispatch sequence numbers).  What is not: work / slog / dry (consumed or cleared inside the slot's own
// launches), err / slow_tick / sup_slot (rewritten by every tick launch; the slot word is set to the restored slot's), the derived
// blocks (d_obs, d_outc, d_heads, d_veh, d_vout, d_orders, d_cnt_*: not saved, refreshed on request after a restore - d_vout and d_orders from `out`, which is saved: replica r then shows the rows of src[r] at the snapshot's slot) and stamp (every stamp is 0xFFFF between API calls: the lists are compact there).
static void snap_free(vds_handle *h) {
    vds_handle::Snap &s = h->snap;
    if (!h->mem[MEM_SNAP].empty()) (void)hipStreamSynchronize(h->stream);           // (a copy may still be running)
    h->mem[MEM_SNAP].release_all();
    for (int i = 0; i < 2; ++i) {
        if (s.pin_map[i]) (void)hipHostFree(s.pin_map[i]);
        if (s.pin_ev[i]) (void)hipEventDestroy(s.pin_ev[i]);
        s.pin_map[i] = nullptr; s.pin_ev[i] = nullptr; s.pin_used[i] = false;
    }
    s.D = State{}; s.d_map = nullptr; s.bytes = 0; s.valid = false;
}
// the store fits the tables as they stand
static bool snap_fits(const vds_handle *h) {
    const vds_handle::Snap &s = h->snap;
    const Static &S = h->S;
    return !h->mem[MEM_SNAP].empty() && s.gen == h->state_gen && s.R == S.R && s.C == S.C && s.idle_cap == S.idle_cap && s.ring_cap == S.ring_cap && s.fl_cap == S.fl_cap &&
           s.H == S.H && s.dense == S.dense && s.Oq == S.Oq && s.arr_slots == S.arr_slots && s.sup == (h->D.sup != nullptr) && s.arr == (S.pull && h->D.arr != nullptr);
}
static int snap_alloc(vds_handle *h) {
    snap_free(h);
    vds_handle::Snap &s = h->snap;
    const Static &S = h->S;
    const State &D = h->D;
    const size_t B = (size_t)S.C * S.R, HB = (size_t)S.H * B;
    s.gen = h->state_gen; s.R = S.R; s.C = S.C; s.idle_cap = S.idle_cap; s.ring_cap = S.ring_cap; s.fl_cap = S.fl_cap; s.H = S.H; s.dense = S.dense;
    s.Oq = S.Oq; s.arr_slots = S.arr_slots; s.sup = D.sup != nullptr; s.arr = S.pull && D.arr != nullptr;
    size_t bytes = 0;
    auto get = [&](auto **p, size_t n) { const int rc = dev_alloc(h, MEM_SNAP, p, n); if (!rc) bytes += std::max<size_t>(n, 1) * sizeof(**p); return rc; };
    int rc;
    // (sized like alloc_state / alloc_results size the tables they mirror)
    if ((rc = get(&s.D.hdr, B * HDR_WORDS)) || (rc = get(&s.D.cnt, B * CNT_WORDS)) ||
        (rc = get(&s.D.idle, S.dense ? (B * S.idle_cap + 1) / 2 : B * S.idle_cap)) ||
        (rc = get(&s.D.ring, S.dense ? (HB * S.ring_cap + 1) / 2 : HB * S.ring_cap)) ||
        (D.ring_min && (rc = get(&s.D.ring_min, HB * S.ring_cap))) ||
        (rc = get(&s.D.ring_cnt, HB)) || (rc = get(&s.D.fl, B * S.fl_cap)) || (rc = get(&s.D.inbox, 2 * B * S.in_cap)) ||
        (s.sup && (rc = get(&s.D.sup, (size_t)VDS_SUP_PLANES * B))) ||
        (s.arr && (rc = get(&s.D.arr, (size_t)S.R * S.arr_slots))) ||
        (rc = get(&s.D.out, (size_t)S.R * std::max(S.Oq, 1))) || (rc = get(&s.d_map, (size_t)S.R))) {
        const std::string msg = h->err;
        snap_free(h);
        h->err = msg;
        return rc;
    }
    for (int i = 0; i < 2; ++i)
        if (hipHostMalloc((void **)&s.pin_map[i], (size_t)S.R * sizeof(int), hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&s.pin_ev[i], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            snap_free(h);
            return fail(h, VDS_ENOMEM, "vds_snapshot: no pinned host memory for the restore map");
        }
    for (int i = 0; i < 2; ++i) VDS_DIRTY_HOST(s.pin_map[i], (size_t)S.R * sizeof(int));
    s.bytes = (long long)bytes;
    return VDS_OK;
}
// every table of the snapshot, src -> dst, on the handle's stream
static int snap_copy(vds_handle *h, const State &src, const State &dst, const int *map, int tdone) {
    Chain c(h->stream);
    for (int tb = 0; tb < SNAP_TABLES; ++tb) c.add(emit_snap_table, h->S, src, dst, map, tb, tdone);
    HIPCHK(h, hipGetLastError());
    return VDS_OK;
}

int vds_snapshot(vds_handle *h) { return guarded(h, "vds_snapshot", [&] {
    if (!h || !h->have_reset) return fail(h, VDS_EINVAL, "vds_snapshot: call vds_reset first");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    vds_handle::Snap &s = h->snap;
    s.valid = false;
    if (!snap_fits(h)) { const int rc = snap_alloc(h); if (rc) return rc; }
    const int rc = snap_copy(h, h->D, s.D, nullptr, h->last_stepped + 1);
    if (rc) return rc;
    s.t = h->t; s.last_stepped = h->last_stepped; s.dispatch_seq = h->dispatch_seq; s.seq_tick0 = h->seq_tick0; s.seq_tick = h->seq_tick; s.matched_tick = h->matched_tick;
    s.valid = true;
    return VDS_OK;
}); }

// the copies and the clock of a restore; map: null (identity) or the handle's device map, filled by the caller
static int restore_finish(vds_handle *h, const int *user_dev_map, const int *map) {
    vds_handle::Snap &s = h->snap;
    const Static &S = h->S;
    if (user_dev_map || h->D.sup_slot) {     // (a device map to check, a slot word to set: otherwise the kernel has nothing to do)
        Chain c(h->stream);
        c.add(emit_snap_prep, user_dev_map, s.d_map, S.R, h->D.err, h->D.sup_slot, s.last_stepped < 0 ? 0 : (s.last_stepped + 1) & (VDS_SUP_PLANES - 1));
    }
    const int rc = snap_copy(h, s.D, h->D, map, s.last_stepped + 1);
    if (rc) return rc;
    h->t = s.t; h->last_stepped = s.last_stepped; h->dispatch_seq = s.dispatch_seq; h->seq_tick0 = s.seq_tick0; h->seq_tick = s.seq_tick; h->matched_tick = s.matched_tick;
    h->restored_episode = true;
    h->roster_fresh = false;
    return VDS_OK;
}
static int restore_check(vds_handle *h, const char *who) {
    if (!h) return VDS_EINVAL;
    if (!h->snap.valid || !snap_fits(h)) {
        if (h->snap.valid) { h->snap.valid = false; snap_free(h); }     // (void: the tables were re-made since; the store goes)
        return fail(h, VDS_ESTATE, "%s: no snapshot (none taken, or the state tables were re-made since: vds_load_orders*, vds_set_replica_days, vds_set_idle_cap, a reset that regrew the idle tables, vds_supply_inplace)", who);
    }
    if (!h->have_reset) return fail(h, VDS_EINVAL, "%s: call vds_reset first", who);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return VDS_OK;
}
int vds_restore(vds_handle *h, const int32_t *src_replica) { return guarded(h, "vds_restore", [&] {
    int rc = restore_check(h, "vds_restore");
    if (rc) return rc;
    if (!src_replica) return restore_finish(h, nullptr, nullptr);
    const Static &S = h->S;
    vds_handle::Snap &s = h->snap;
    for (int r = 0; r < h->R_ext; ++r) {
        const int m = src_replica[r];
        if (m < 0 || m >= h->R_ext) return fail(h, VDS_EINVAL, "vds_restore: replica %d is mapped to replica %d of %d", r, m, h->R_ext);
        if (h->replica_day[r] != h->replica_day[m])
            return fail(h, VDS_EINVAL, "vds_restore: order days per replica: replica %d replays day %d, replica %d day %d - a replica can only continue on the day it replays", r, h->replica_day[r], m, h->replica_day[m]);
    }
    // stored replica indices (regrouped storage: through ext2int; a padding replica maps to itself)
    const int pi = s.pin_i;
    s.pin_i ^= 1;
    if (s.pin_used[pi]) HIPCHK(h, hipEventSynchronize(s.pin_ev[pi]));          // (the upload this buffer was the source of, two restores ago)
    int *stage = s.pin_map[pi];
    for (int ri = 0; ri < S.R; ++ri) {
        const int re = h->int2ext.empty() ? ri : h->int2ext[ri];
        stage[ri] = re < 0 ? ri : (h->ext2int.empty() ? src_replica[re] : h->ext2int[src_replica[re]]);
    }
    HIPCHK(h, hipMemcpyAsync(s.d_map, stage, (size_t)S.R * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(s.pin_ev[pi], h->stream));
    s.pin_used[pi] = true;
    return restore_finish(h, nullptr, s.d_map);
}); }
int vds_restore_device(vds_handle *h, const void *dev_src_replica) { return guarded(h, "vds_restore_device", [&] {
    int rc = restore_check(h, "vds_restore_device");
    if (rc) return rc;
    if (!dev_src_replica) return fail(h, VDS_EINVAL, "vds_restore_device: null map (vds_restore(h, NULL) is the plain rollback)");
    if (h->S.n_days > 1 || !h->int2ext.empty() || h->S.R != h->R_ext)
        return fail(h, VDS_ESTATE, "vds_restore_device: order days per replica: the host cannot check that a replica continues on the day it replays - use vds_restore");
    return restore_finish(h, (const int *)dev_src_replica, h->snap.d_map);
}); }

int vds_snapshot_info(const vds_handle *h, int32_t *step, int32_t *stepped, int64_t *bytes) {
    if (!h) return VDS_EINVAL;
    if (!h->snap.valid || !snap_fits(h)) return VDS_ESTATE;
    if (step) *step = h->snap.t;
    if (stepped) *stepped = h->snap.last_stepped == h->snap.t;
    if (bytes) *bytes = h->snap.bytes;
    return VDS_OK;
}
int vds_snapshot_drop(vds_handle *h) { return guarded(h, "vds_snapshot_drop", [&] {
    if (!h) return VDS_EINVAL;
    (void)hipSetDevice(h->cfg.device);
    snap_free(h);
    return VDS_OK;
}); }

}  // extern "C"
