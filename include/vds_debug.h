/* vds_debug.h - test / instrumentation hooks exported by libvds.so next to the drop-in boundary of vds.h.
 *
 * NOT part of the boundary: nothing here has a counterpart in the reference.  These entry points exist for the parity
 * tests (tests/), the guarded and instrumented builds (make canary / make prof / make dbg) and the measurement scripts
 * under profiles/.  They are declared so that every symbol libvds.so exports is declared somewhere
 * (tests/test_abi_symbols.py checks include/vds.h + this file against `nm -D`).
 *
 * vds_debug_dense changes which of the library's own (result-identical) kernel variants runs; vds_debug_ablate makes
 * results INVALID (timing only) - neither belongs in a product build's call path.
 */
#ifndef VDS_DEBUG_H
#define VDS_DEBUG_H

#include "vds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dense tick (k_tick_dense) variants, effective from the next vds_load_orders* on: lanes per replica (8 / 16; 0 = default),
 * idle entries / arrivals per bucket its fast path takes (0 = 128 or 256 / 64), force_slow bit 0: every bucket takes the slow
 * path, bit 1: arrival ring instead of static arrival slots.  Results do not depend on any of them (tests/test_gpu_parity.py). */
int vds_debug_dense(vds_handle *h, int32_t lanes_per_replica, int32_t tab, int32_t keys, int32_t force_slow);

/* timing-only ablation switches of the tick kernels (instrumented build; profiles/ablate.py).  Non-zero flags: results INVALID. */
int vds_debug_ablate(vds_handle *h, int32_t flags);

/* instrumented build (make prof): 32 section cycle counters of the tick kernels (profiles/sections*.py) */
int vds_debug_read_prof(vds_handle *h, uint64_t *out32);

/* instrumented build: launch spans of k_tick_dense, [2 chains][256 slots]{first wavefront in, last out} on the 100 MHz
 * s_memrealtime clock; out1024 may be null (reset only) */
int vds_debug_read_span(vds_handle *h, uint64_t *out1024, int32_t reset);

/* the 16 words of the device error block: [0] sticky error bits, [2] buckets off the fast path, [4..15] why (instrumented build) */
int vds_debug_read_err(vds_handle *h, int32_t *out16);

/* guarded build (make canary): device tables of this process whose guard zones were written (0 in every other build);
 * a negative VDS_E* code if the check itself failed */
int vds_debug_check_guards(vds_handle *h);

/* guarded build only: damages one guard zone on purpose (the test of the check); VDS_EINVAL in other builds */
int vds_debug_poke_guard(vds_handle *h);

/* dirty build (make dirty: every byte the library obtains for a handle is filled with the byte VDS_DIRTY_FILL names, hex, default
 * A5, before first use): a 4-int device table taken through the library's allocator and copied back as handed out - four words of the
 * fill byte; VDS_ESTATE in every other build */
int vds_debug_dirty_probe(vds_handle *h, int32_t out[4]);

/* device blocks of this process that the library holds, over all handles: out[0] their number, out[1] their bytes (guard zones not
 * counted; blocks parked for the next load count).  A handle gives back what it took: the pair is the same before vds_create and after
 * vds_destroy (tests/test_gpu_device_memory.py). */
int vds_debug_device_blocks(int64_t out[2]);

/* executable day graphs kept past their handle: always 0 (day graphs are single chains, destroyed with their handle) */
int vds_debug_graph_pool_size(void);

/* k_tick_dense's per-slot form as the handle stands (vds_api.hip adapt_dense): out[t] = 1 where slot t runs 16 lanes per replica with
 * 256-entry tables in some or all of its clusters whatever the base form, 0 where it runs the base form; *n_out = slots written (0: no
 * per-slot choice was made). */
int vds_debug_tick_forms(vds_handle *h, uint8_t *out, int32_t cap, int32_t *n_out);

/* ... per (slot, cluster): out[t * C + c] = 1 where cluster c runs slot t in that form (cap: bytes of out, at least T * C);
 * *n_out = T (0: no choice was made). */
int vds_debug_cluster_forms(vds_handle *h, uint8_t *out, int64_t cap, int32_t *n_out);

/* the layout decision as the handle stands (tests/test_gpu_thresholds.py), cap >= 10 words: out[0] dense layout (k_tick_dense),
 * [1] its stamp form (neighbour search on the dense layout), [2] cost blocks of the dense layout: 1 bytes, 0 ints, [3] u8_ok (every cost
 * of the matrix in 0..255), [4] the byte copy of the whole matrix exists, [5] fast_ok (packed keys), [6] window_live, [7] seq_pad, [8]
 * lanes per replica of k_tick_dense, [9] its fast-path table size (128 / 256), and with cap >= 11 [10] the dense tick's arrival form:
 * 1 static arrival slots, 0 the arrival ring (its own choice when arrivals can lie more than DENSE_PULL_WMAX slots behind their
 * earliest slot, or the debug switch); -1 where a value does not apply (no orders loaded, no dense layout, no neighbour search);
 * words past 11 are -1. */
int vds_debug_layout(vds_handle *h, int32_t *out, int32_t cap);

/* Host tables of a load without a handle or a device (csrc/vds_tables.h; tests/test_order_tables.py): the city of vds_load_static
 * (nbr_off null: no neighbour search) and n_days order days of vds_load_order_days, built with `threads` workers.  Out: day_out
 * [n_days][4] {T, now0, Oq, q_base}; sizes [8] {n processed orders, entries of bkt_off, of tick_off, m arrival slots, entries of d_first,
 * W, hmax, verdict on the static arrival slots (every_order != 0: only if every processed order owns one)}; so_rec [n][4], ord_q,
 * so_rank, so_slot [n] (cap_rec: orders these four hold), bkt_off, tick_off, d_rec [m][2], d_first with their capacities in elements
 * (rows for d_rec).  VDS_ECAPACITY when an array is short (sizes is complete, short arrays are left alone); after any other failure err
 * holds the text vds_last_error would give. */
int vds_debug_order_tables(const int32_t *cost, int32_t N, const int32_t *node2cluster, int32_t C, int32_t tick_minutes,
                           const int32_t *nbr_off, const int32_t *nbr_idx, int32_t depth_limit, int32_t ring_ticks,
                           int32_t n_days, const int64_t *day_off, const int32_t *release_min, const int32_t *pickup,
                           const int32_t *delivery, int32_t threads, int32_t every_order, int32_t *day_out, int64_t *sizes,
                           int32_t *so_rec, int32_t *ord_q, int32_t *so_rank, int32_t *so_slot, int64_t cap_rec,
                           int32_t *bkt_off, int64_t cap_bkt, int32_t *tick_off, int64_t cap_tick, int32_t *d_rec, int64_t cap_drec,
                           int32_t *d_first, int64_t cap_first, char *err, int32_t err_cap);

/* The storage order of the replicas for a replica -> day map (vds_set_replica_days): gran_small_ok - day groups of 8 / 4 replicas may
 * be used, regroup_ok - the replicas may be stored regrouped by day, alloc_replicas - stored replicas of state tables at hand (0: none).
 * head [4] {R, row_gran, chunk_days, regrouped}; int_to_ext, rperm, day_of_internal [R] (cap: entries they hold; -1 / -1 / n_days for a
 * dummy replica, the identity when not regrouped), ext_to_int [R_ext].  VDS_ECAPACITY when R > cap (head is complete). */
int vds_debug_replica_plan(const int32_t *replica_day, int32_t R_ext, int32_t n_days, int32_t gran_small_ok, int32_t regroup_ok,
                           int32_t alloc_replicas, int32_t *head, int32_t *int_to_ext, int32_t *rperm, int32_t *day_of_internal,
                           int32_t cap, int32_t *ext_to_int);

/* DPP primitives of the kernels on nwaves x 64 int32 values (tests/test_gpu_primitives.py): out_wave [nwaves] wavefront
 * minima; out_rowmin / out_rowsum / out_rowscan [nwaves * 64] per-lane 16-lane-row minimum, row sum and inclusive row scan */
int vds_selftest_dpp(vds_handle *h, const int32_t *in, int32_t *out_wave, int32_t *out_rowmin, int32_t *out_rowsum,
                     int32_t *out_rowscan, int32_t nwaves);

#ifdef __cplusplus
}
#endif
#endif
