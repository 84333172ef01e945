// Host-side launchers of the kernel files, as the host units (vds_api*.hip) call them: declarations, and fleet_size (included by
// vds_handle.h and by every file that defines one of them; hashed with the HOST sources: Makefile).
//   launch_*  on a stream (the tick files only: the derived blocks and the tensor dispatch forms have no such twin)
//   emit_*    on a stream or as a kernel node of an explicitly built hipGraph (Emit, vds_device.h), for the replicas
//             [r_lo, r_lo + r_n) - r_lo a multiple of 16; r_n <= 0 (with r_lo 0): all.  One kernel each: which kernels refresh a
//             block, in what order and when, is said once, by vds_api.hip (refresh_*)
#pragma once
#include "vds_device.h"

namespace vds {
// Fleet size per replica (vds_set_fleet; the reference: VehiclesNumber, simulator.py:101, :347): how many vehicles the caller's
// replica `ext` has - vehicles 0 .. n - 1, the rest do not exist.  fleet: int32 [R_ext] by the caller's index, null: V everywhere;
// ext < 0: a padding replica, no vehicles.  The one place the reset kernels and the start-node kernels take their vehicle range from
// (the only definition in this header: both kernel files include it)
__host__ __device__ __forceinline__ int fleet_size(const int *fleet, int ext, int V) { return ext < 0 ? 0 : (fleet ? fleet[ext] : V); }
// ---- vds_tick.hip
// fleet: see fleet_size (a kernel parameter of its own, not a member of Static: the argument block of the tick kernels stays as it is)
void launch_reset(const Static &S, const State &D, const int *veh_node, const int *fleet, hipStream_t st);
bool reset_uses_image(const Static &S);
void launch_reset_capture(const Static &S, const State &D, unsigned *img, int *base, hipStream_t st);
void launch_reset_image(const Static &S, const State &D, const unsigned *img, const int *base, hipStream_t st);
void launch_tick_generic(const Static &S, const State &D, int t, int lds_ints, hipStream_t st);
void launch_tick_work(const Static &S, const State &D, int t, hipStream_t st);
void launch_update_only(const Static &S, const State &D, int t, hipStream_t st);
void emit_tick_rows(const Emit &e, const Static &S, const State &D, int t, int lds_ints, int r_lo, int r_n);
void emit_hybrid_rows(const Emit &e, const Static &S, const State &D, int t, int lds_ints, int r_lo, int r_n);
void launch_dispatch(const Static &S, const State &D, int t, int ngroups, const int *grp_off, const int *a_replica, const int *a_cluster,
                     const int *a_pos, const int *a_target, const int *a_seq, const int *a_arrive, const int *a_counted, hipStream_t st);
void emit_dispatch_dense(const Emit &e, const Static &S, const State &D, int t, int K, const int *actions, int seq_base, int r_lo, int r_n);
void launch_dispatch_dense(const Static &S, const State &D, int t, int K, const int *actions, int seq_base, hipStream_t st);
void emit_pack_obs(const Emit &e, const Static &S, const State &D, int t, int stepped, int planes, int *obs, int r_lo, int r_n);
void launch_pack_obs(const Static &S, const State &D, int t, int stepped, int planes, int *obs, hipStream_t st);
void launch_reduce_counters(const Static &S, const State &D, long long *per, long long *tot, hipStream_t st);
void launch_selftest_dpp(const int *in, int *o0, int *o1, int *o2, int *o3, int nwaves, hipStream_t st);
void set_ablate_tick(int flags, hipStream_t st);
void read_prof_tick(unsigned long long *out, hipStream_t st);
// ---- vds_tick_dense.hip
void emit_tick_dense(const Emit &e, const Static &S, const State &D, int t, int r_lo, int r_n);
void emit_tick_dense_mixed(const Emit &e, const Static &S, const State &D, int t, const int2 *bmap, int nblk);
bool dense_mixed_ok(const Static &S, int slots);
void emit_dense_flush(const Emit &e, const Static &S, const State &D, int r_lo, int r_n);
void set_ablate_dense(int flags, hipStream_t st);
void read_prof_dense(unsigned long long *out, hipStream_t st);
void read_span_dense(unsigned long long *out, int reset, hipStream_t st);
// ---- vds_dfs.hip
void launch_match_dfs(const Static &S, const State &D, int t, hipStream_t st);
void launch_tick_replica2(const Static &S, const State &D, int t, hipStream_t st);
void emit_hybrid_walk(const Emit &e, const Static &S, const State &D, int t, int r_lo, int r_n);
void launch_build_vis(const Static &S, const int *so_bkt0, unsigned *so_vis, unsigned char *so_lb, long long n_orders, hipStream_t st);
size_t dfs_walk_lds(const Static &S);
int dfs_walk_pool(const Static &S);
void set_ablate_dfs(int flags, hipStream_t st);
void read_prof_dfs(unsigned long long *out, hipStream_t st);
// ---- vds_random.hip
// (both by the caller's replica index; fleet: see fleet_size - replica r draws / has checked its first fleet_size vehicles only)
void launch_py_random_nodes(const unsigned long long *seeds, int R, int N, int V, int C, const int *node2cluster, int *veh_node, int *fullest,
                            const int *fleet, hipStream_t st);
void launch_start_nodes_check(const int *veh_node, int R, int N, int V, int C, const int *node2cluster, int *fullest, unsigned long long *bad,
                              const int *fleet, hipStream_t st);
// ---- vds_outcomes.hip
void emit_slot_outcomes(const Emit &e, const Static &S, const State &D, int t, int stepped, long long *oc, int r_lo, int r_n);
// ---- vds_idle_heads.hip
void emit_idle_heads(const Emit &e, const Static &S, const State &D, int L, int *heads, int r_lo, int r_n);
// ---- vds_vehicle_planes.hip
// t_last: slot stepped last (-1: none since the reset); planes: bit k = plane k of the int32 [6][R_ext][V] block `out` is wanted (the
// fill has written -1 there).  Three kernels, one launcher each (a graph node each): the -1 fill, the bucket containers, and - when
// vehicle_pull_needed - the static arrival slots
void emit_vehicle_fill(const Emit &e, const Static &S, int planes, int *out, int r_lo, int r_n);
void emit_vehicle_lists(const Emit &e, const Static &S, const State &D, int t_last, int planes, int *out, int r_lo, int r_n);
bool vehicle_pull_needed(const Static &S, int t_last);
void emit_vehicle_pull(const Emit &e, const Static &S, const State &D, int t_last, int planes, int *out, int r_lo, int r_n);
// ---- vds_vehicle_outcomes.hip
// blk: int32 [R_ext][V][4] {order, wait, value, pickup} per vehicle (16-byte aligned); t: slot stepped last, stepped == 0: none since
// the reset.  Two kernels, one launcher each (a graph node each): the -1 fill of the replicas' rows, then the scatter of the slot's orders
void emit_vehicle_outcomes_fill(const Emit &e, const Static &S, int *blk, int r_lo, int r_n);
void emit_vehicle_outcomes(const Emit &e, const Static &S, const State &D, int t, int stepped, int *blk, int r_lo, int r_n);
// ---- vds_orders_block.hip
// blk: int32 [R_ext][O][2] {vehicle, wait} per order id (8-byte aligned); the rows of the orders processed in slots [slot_lo, slot_hi]
// (clamped per replica to its own day; the day's last slot takes the rest of the row); last: slot stepped last, -1: none since the
// reset; ids: the longest id range of one replica (the grid's size).  One kernel
void emit_orders_block(const Emit &e, const Static &S, const State &D, int slot_lo, int slot_hi, int last, int O, int ids, int *blk, int r_lo, int r_n);
// ---- vds_dispatch_vehicles.hip: one walk, two forms
// targets: int32 [R_ext][V] target node per vehicle (negative: stay); seq_base: sequence numbers the slot's earlier dispatch calls used
// arrive / counted (either may be null; both null: the plain kernels): int32 [R_ext][V] addressed as targets is - the arrival minute
// (VDS_ARRIVE_ROAD: now + RoadCost) and the counted flag of each mover
void emit_dispatch_vehicles(const Emit &e, const Static &S, const State &D, int t, const int *targets, const int *arrive, const int *counted, int seq_base, int r_lo, int r_n);
// targets: int32 [R_ext][V] target node per roster entry (negative: stay), against the offsets `off` of the refresh it was written for
void emit_dispatch_roster(const Emit &e, const Static &S, const State &D, int t, const int *targets, const int *off, const int *arrive, const int *counted, int seq_base, int r_lo, int r_n);
// ---- vds_match_external.hip: the three launches of vds_apply_match_device, over all replicas
// assign: int32 [R_ext][M] vehicle per order of the slot, in Order.ID order (null: every order rejected); claim: int32 [S.R][V], INT_MAX
// everywhere before and after the three; n_orders: orders the slot processes (sizes the claim grid)
enum { MATCH_CLAIM_THREADS = 256 };
// sticky device error bit (err[0], next to the ERR_* of vds_device.h): an assignment entry >= V
enum { ERR_MATCH = 64 };
void emit_match_claim(const Emit &e, const Static &S, const State &D, int t, int n_orders, const int *assign, int M, int *claim);
void emit_match_walk(const Emit &e, const Static &S, const State &D, int t, int *claim);
void emit_match_finish(const Emit &e, const Static &S, const State &D, int t, const int *assign, int M, int *claim);
// ---- vds_idle_roster.hip
// planes: int32 [3][R_ext][V] {veh, node, cluster} by roster position, off: int32 [R_ext][C + 1]; one kernel writes every element of both
// (dynamic LDS: idle_roster_lds, (C + 1) ints - C <= IDLE_ROSTER_C_MAX)
enum { IDLE_ROSTER_C_MAX = 16000 };
void emit_idle_roster(const Emit &e, const Static &S, const State &D, int *planes, int *off, int r_lo, int r_n);
// ---- vds_snapshot.hip
// the tables of a snapshot, one launch each: `src` -> `dst` are State views of the live tables and of the store (either way round),
// map [S.R] stored replica -> stored source replica (null: identity), tdone the slots whose orders have been processed (SNAP_OUT)
enum { SNAP_HDR, SNAP_CNT, SNAP_IDLE, SNAP_RING, SNAP_RING_MIN, SNAP_RING_CNT, SNAP_FL, SNAP_INBOX, SNAP_SUP, SNAP_ARR, SNAP_OUT, SNAP_TABLES };
void emit_snap_table(const Emit &e, const Static &S, const State &src, const State &dst, const int *map, int table, int tdone);
// sticky device error bit (err[0], next to the ERR_* of vds_device.h): a device-resident restore map named a replica outside [0, R)
enum { ERR_RESTORE = 32 };
// the caller's device map `user` (null: none) checked into `map`; the supply planes' slot word (nullable) set to sup_val
void emit_snap_prep(const Emit &e, const int *user, int *map, int R, int *err, int *sup_slot, int sup_val);
}  // namespace vds
