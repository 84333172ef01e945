// libvds host unit: the hooks of include/vds_debug.h - what tests, benchmarks and the instrumented builds ask of a handle
// (vds_debug_*, vds_selftest_dpp); not part of the drop-in surface.
#include "vds_handle.h"

extern "C" {

// per slot 1 where some cluster runs k_tick_dense's 16-lane form; *n_out = T (0: no choice made yet)
int vds_debug_tick_forms(vds_handle *h, uint8_t *out, int32_t cap, int32_t *n_out) {
    if (!h || !out || !n_out || cap < 0) return VDS_EINVAL;
    const int n = (int)std::min<size_t>(h->forms.slot.size(), (size_t)cap);
    for (int i = 0; i < n; ++i) out[i] = h->forms.slot[i].kind != vds_handle::TickForms::BASE;
    *n_out = n;
    return VDS_OK;
}
// [T][C] per (slot, cluster) 1 where k_tick_dense runs the 16-lane form; *n_out = T (0: no choice made yet)
int vds_debug_cluster_forms(vds_handle *h, uint8_t *out, int64_t cap, int32_t *n_out) {
    if (!h || !out || !n_out || cap < 0) return VDS_EINVAL;
    const int T = (int)h->forms.slot.size();
    if ((long long)T * h->S.C > cap) return VDS_EINVAL;
    std::copy(h->forms.plane.begin(), h->forms.plane.end(), out);
    *n_out = T;
    return VDS_OK;
}
// the layout decision as the handle stands (include/vds_debug.h: word order, -1 = does not apply)
int vds_debug_layout(vds_handle *h, int32_t *out, int32_t cap) {
    if (!h || !out || cap < 10) return VDS_EINVAL;
    const Static &S = h->S;
    const bool st = h->have_static, ord = h->have_orders;
    const int32_t w[10] = {
        ord ? S.dense : -1,
        ord ? S.dense_st : -1,
        !st ? -1 : S.blk8s ? 1 : S.blk32s ? 0 : -1,
        st ? S.u8_ok : -1,
        st ? (S.cost8 != nullptr) : -1,
        st ? S.fast_ok : -1,
        st ? S.window_live : -1,
        st && h->dfs_mode ? S.seq_pad : -1,
        ord && S.dense ? S.dense_lpr : -1,
        ord && S.dense ? S.dense_tab : -1,
    };
    std::copy(w, w + 10, out);
    if (cap > 10) out[10] = ord && S.dense ? S.pull : -1;
    for (int i = 11; i < cap; ++i) out[i] = -1;
    return VDS_OK;
}
int vds_debug_graph_pool_size() {      // executable graphs kept alive past their handle's use (tests): none any more
    return 0;
}

// Bench hook (not part of the drop-in surface): timing-only ablation of the fast kernel; any non-zero
// value makes results INVALID.  bit0 no arrival posts, bit1 no idle write-back, bit2 no match loop,
// bit3 no result stores, bit4 no header/counter stores.
int vds_debug_ablate(vds_handle *h, int32_t flags) { return guarded(h, "vds_debug_ablate", [&] {
    if (!h) return VDS_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    set_ablate_tick(flags, h->stream);
    set_ablate_dfs(flags, h->stream);
    set_ablate_dense(flags, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VDS_OK;
}); }

// Test hook (not part of the drop-in surface): overrides for the dense tick, effective from the next vds_load_orders on - lanes
// per replica (16 / 8 / 4; 0 = default), idle entries / arrivals per bucket its fast path takes (0 = 128 / 64), force the slow path.
int vds_debug_dense(vds_handle *h, int32_t lpr, int32_t tab, int32_t keys, int32_t force_slow) { return guarded(h, "vds_debug_dense", [&] {
    if (!h) return VDS_EINVAL;
    h->dbg_dense_lpr = lpr; h->dbg_dense_tab = tab; h->dbg_dense_keys = keys; h->dbg_dense_slow = force_slow;
    return VDS_OK;
}); }

// Guarded build (make canary): number of device tables of this process whose guard zones no longer hold the poison pattern
// (0 in every other build).  Synchronises the handle's stream.
int vds_debug_check_guards(vds_handle *h) { return guarded(h, "vds_debug_check_guards", [&] {
    if (!h) return VDS_EINVAL;
    if (!GUARDED) return 0;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // (returns the number of damaged tables, >= 0, or a negative VDS_E* code: the two cannot be confused)
    int bad = 0;
    std::vector<unsigned char> buf(std::max<size_t>(GUARD_FRONT, GUARD_BACK));
    std::lock_guard<std::mutex> lk(g_guards_mu);
    for (const auto &kv : g_guards) {
        const char *base = (const char *)kv.second.base;
        bool ok = true;
        if (hipMemcpy(buf.data(), base, GUARD_FRONT, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, VDS_EHIP, "vds_debug_check_guards: reading a guard zone failed");
        for (size_t i = 0; i < GUARD_FRONT && ok; ++i) ok = buf[i] == 0xA5;
        if (hipMemcpy(buf.data(), base + GUARD_FRONT + kv.second.bytes, GUARD_BACK, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, VDS_EHIP, "vds_debug_check_guards: reading a guard zone failed");
        for (size_t i = 0; i < GUARD_BACK && ok; ++i) ok = buf[i] == 0xA5;
        if (!ok) { ++bad; fprintf(stderr, "libvds guard: table of %zu bytes at %p was written out of bounds\n", kv.second.bytes, (void *)(base + GUARD_FRONT)); }
    }
    return bad;
}); }

// device blocks of this process that are live (parked ones included) and their bytes, as dev_raw_alloc / dev_free count them
int vds_debug_device_blocks(int64_t out[2]) {
    if (!out) return VDS_EINVAL;
    out[0] = g_dev_blocks.load(); out[1] = g_dev_bytes.load();
    return VDS_OK;
}

// Guarded build only: damages one guard zone on purpose (one byte behind the header table), so that the test of the guard
// check itself has something to find.  Other builds: VDS_EINVAL.
int vds_debug_poke_guard(vds_handle *h) { return guarded(h, "vds_debug_poke_guard", [&] {
    if (!h || !GUARDED || !h->D.hdr) return VDS_EINVAL;
    std::lock_guard<std::mutex> lk(g_guards_mu);
    auto it = g_guards.find((void *)h->D.hdr);
    if (it == g_guards.end()) return VDS_EINVAL;
    HIPCHK(h, hipMemset((char *)it->second.base + GUARD_FRONT + it->second.bytes + 5, 0, 1));
    return VDS_OK;
}); }

// Dirty build only (make dirty): a 4-int table taken through dev_alloc and copied back as it was handed out - the fill byte four
// times over, which is the proof that the fill is live.  Other builds: VDS_ESTATE.
int vds_debug_dirty_probe(vds_handle *h, int32_t out[4]) { return guarded(h, "vds_debug_dirty_probe", [&] {
    if (!h || !out) return VDS_EINVAL;
#ifdef VDS_DIRTY
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int *p = nullptr;
    DevGroup mine;
    const int rc = dev_alloc(h, mine, &p, (size_t)4);
    if (rc) return rc;
    const hipError_t e = hipMemcpy(out, p, 4 * sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, VDS_EHIP, "vds_debug_dirty_probe: copying the table back failed: %s", hipGetErrorString(e));
    return VDS_OK;
#else
    return fail(h, VDS_ESTATE, "vds_debug_dirty_probe: not a dirty build (make dirty)");
#endif
}); }

// instrumented build: launch spans of k_tick_dense ([2 chains][256 slots]{first wavefront in, last out} on the 100 MHz s_memtime
// clock; flag 1048576 of vds_debug_ablate switches the stamps on); out may be null (reset only)
int vds_debug_read_span(vds_handle *h, uint64_t *out1024, int32_t reset) { return guarded(h, "vds_debug_read_span", [&] {
    if (!h) return VDS_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    read_span_dense((unsigned long long *)out1024, reset, h->stream);
    return VDS_OK;
}); }

// the 16 words of the device error block ([4..15]: slow-path reasons of the instrumented build, vds_tick_dense.hip)
int vds_debug_read_err(vds_handle *h, int32_t *out16) { return guarded(h, "vds_debug_read_err", [&] {
    if (!h || !h->have_static || !out16) return VDS_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out16, h->D.err, 16 * sizeof(int), hipMemcpyDeviceToHost));
    return VDS_OK;
}); }

int vds_debug_read_prof(vds_handle *h, uint64_t *out32) { return guarded(h, "vds_debug_read_prof", [&] {
    if (!h || !out32) return VDS_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    for (int i = 0; i < 32; ++i) out32[i] = 0;
    read_prof_tick((unsigned long long *)out32, h->stream);
    read_prof_dfs((unsigned long long *)out32, h->stream);
    read_prof_dense((unsigned long long *)out32, h->stream);
    return VDS_OK;
}); }

// Test hook (not part of the drop-in surface): runs the DPP primitives on `nwaves` x 64 int32
// values: out_wave [nwaves] wave minima; out_rowmin / out_rowsum / out_rowscan [nwaves*64] per-lane
// 16-lane-row min, row sum and row inclusive scan (the latter two of value & 0xFFFF).
int vds_selftest_dpp(vds_handle *h, const int32_t *in, int32_t *out_wave, int32_t *out_rowmin, int32_t *out_rowsum,
                     int32_t *out_rowscan, int32_t nwaves) { return guarded(h, "vds_selftest_dpp", [&] {
    if (!h || !in || !out_wave || !out_rowmin || !out_rowsum || !out_rowscan || nwaves < 1) return VDS_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t n = (size_t)nwaves * 64;
    int *din = nullptr, *d0 = nullptr, *d1 = nullptr, *d2 = nullptr, *d3 = nullptr;
    DevGroup scratch;                                    // (freed on every way out)
    int rc;
    if ((rc = dev_alloc(h, scratch, &din, n)) || (rc = dev_alloc(h, scratch, &d0, (size_t)nwaves)) || (rc = dev_alloc(h, scratch, &d1, n)) ||
        (rc = dev_alloc(h, scratch, &d2, n)) || (rc = dev_alloc(h, scratch, &d3, n))) return rc;
    HIPCHK(h, hipMemcpy(din, in, n * sizeof(int), hipMemcpyHostToDevice));
    launch_selftest_dpp(din, d0, d1, d2, d3, nwaves, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out_wave, d0, (size_t)nwaves * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(out_rowmin, d1, n * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(out_rowsum, d2, n * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(out_rowscan, d3, n * sizeof(int), hipMemcpyDeviceToHost));
    return VDS_OK;
}); }

}  // extern "C"
