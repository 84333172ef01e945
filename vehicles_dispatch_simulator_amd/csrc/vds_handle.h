// The handle behind the C ABI (include/vds.h) and what more than one host unit (vds_api*.hip) uses of it: private to those units.
// What one unit alone uses is static in that unit.
#pragma once
#include "../../include/vds.h"
#include "../../include/vds_debug.h"
#include "vds_device.h"
#include "vds_launch.h"
#include "vds_hook_plan.h"
#include "vds_mem.h"
#include "vds_tables.h"

#include <algorithm>
#include <unordered_map>
#include <atomic>
#include <chrono>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <vector>

using namespace vds;

extern thread_local std::string g_create_error;      // vds_last_error(NULL): defined in vds_api.hip

// blocks of the process-wide pool of pinned host memory (PinnedPool, vds_api.hip)
void *pinned_get(size_t bytes);
void pinned_put(void *p);
template <typename T>
struct PinnedAlloc {
    using value_type = T;
    PinnedAlloc() = default;
    template <class U> PinnedAlloc(const PinnedAlloc<U> &) {}
    T *allocate(size_t n) { return static_cast<T *>(pinned_get(n * sizeof(T))); }
    void deallocate(T *p, size_t) { pinned_put(p); }
    template <class U, class... A> void construct(U *p, A &&...a) {
        if constexpr (sizeof...(A) == 0) ::new ((void *)p) U; else ::new ((void *)p) U(std::forward<A>(a)...);
    }
    bool operator==(const PinnedAlloc &) const { return true; }
    bool operator!=(const PinnedAlloc &) const { return false; }
};
template <typename T> using pvec = std::vector<T, PinnedAlloc<T>>;


// Device memory of a handle: every block belongs to one of these groups, named where it is allocated (dev_alloc / upload); vds_destroy frees them all
enum Mem {
    MEM_STATIC,                          // static tables, scratch, the device copies of Static / State
    MEM_ORDERS,                          // tables of the loaded day (parked by the next vds_load_orders* for its own tables, DevGroup::recycle)
    MEM_MAP,                             // the replica -> day map's device arrays (replaced by vds_set_replica_days / the next load)
    MEM_RESULTS,                         // per-replica result tables out / arr / slog (sized by S.R), with d_orders (sized by R_ext x O: dropped by every order load)
    MEM_STATE,                           // per-replica state (kept across days while the capacities still fit), with d_outc, d_heads, d_veh, d_vout and d_roster
    MEM_IDLE,                            // the idle table alone (regrown by vds_reset / vds_set_idle_cap)
    MEM_SNAP,                            // the snapshot store
    MEM_GROUPS
};

struct vds_handle {
    vds_config cfg{};
    Static S{};
    State D{};
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string err;
    bool have_static = false, have_orders = false, have_reset = false;
    bool dfs_mode = false;
    bool dfs2_ok = false;   // k_tick_replica2 preconditions hold (load_days_body)
    bool hybrid_ok = false; // hybrid neighbour-search tick (k_tick_rows in stamp mode + k_dfs_walk) preconditions hold
    long long blk_ints = 0; // total size of the per-cluster cost blocks
    // dense layout (k_tick_dense): static preconditions, the layout the state tables were allocated for
    bool dense_static_ok = false;
    bool dense_dfs_static_ok = false;        // ... of the dense layout for the neighbour-search tick (stamp form, Static.dense_st; round 6)
    bool want_sup = false;                   // SupplyExpect kept in place (State.sup): on request (vds_supply_inplace) - the hook-less day pays 8 % for the planes' atomics
    bool nodes_valid = false;                // d_veh_node holds the start nodes of the last vds_reset* (false once the state tables were re-allocated)
    int alloc_dense = -1, alloc_st = -1;
    int seq_tick0 = 0;                       // dispatch_seq at the first dispatch call of the current slot (dense keys carry the sequence number inside the slot)
    int seq_tick = -1;                       // the slot seq_tick0 belongs to
    // device-resident copies of S / D for the slow path of k_tick_dense (Static.self_dev / state_dev), and what they hold
    Static *d_S = nullptr;
    State *d_D = nullptr;
    Static S_up{};
    State D_up{};
    bool have_up = false;
    pvec<int2> pull_drec;                    // host copy of Static.d_rec (the vector it was uploaded from: pinned)
    std::vector<int> pull_slot_q;            // slot (absolute d_rec position) -> q - q_base of its order
    std::vector<int4> pull_desc;             // per day {d_first base, d_rec base, TA, 0} (static arrival slots of the dense tick)
    int pull_Od_max = 0;
    std::vector<int> cl_cmax;                // [C] largest cost inside the cluster's block
    std::vector<int4> cdesc_dense_host;      // host copy of Static.cdesc_dense (empty: no dense blocks)
    int dbg_dense_lpr = 0, dbg_dense_tab = 0, dbg_dense_keys = 0, dbg_dense_slow = 0;      // vds_debug_dense (0: defaults)
    int cost_min = 0, cost_max = 0;
    int max_seq = 0;        // longest visit sequence of FindServerVehicleFunction over the clusters
    std::vector<unsigned char> lbc_host;     // host copy of Static.lbc (empty: none)
    std::vector<int> dfs_off_host, dfs_seq_host;
    int depth_limit = 0;
    int t = 0;              // self.step
    int last_stepped = -1;  // tick of the last vds_step
    int dispatch_seq = 0;
    int O = 0;              // all orders incl. never-processed ones
    int lds_ints = 0;
    // host mirrors
    std::vector<int> node2cluster, node_local, cl_off, cl_nodes, cost_host, corder_host;
    std::vector<DayHost> days;         // the loaded order days
    std::vector<int> replica_day;        // [R_ext] by the caller's replica index
    // Order days per replica with a map that mixes days inside aligned groups of 16: the replicas are stored REGROUPED by day
    // (state index = "internal" replica; every day's last group of 16 padded with dummy replicas that never run), so that
    // every workgroup of the fast kernel and every cache line of the [C][R] tables belongs to one day.  Callers keep their
    // own numbering: every entry point maps.  Empty vectors: identity.
    int R_ext = 0;                       // vds_config.replicas
    std::vector<int> int2ext, ext2int;
    int alloc_R = 0;                     // replica count the state tables were allocated for
    DevGroup mem[MEM_GROUPS];
    vds_handle() { mem[MEM_ORDERS].recycle = true; }
    std::vector<DayDesc> ddesc_host;         // the loaded days (+ the empty day of padding replicas, last)
    size_t res_cap_out = 0, res_cap_arr = 0, res_cap_slog = 0;      // elements the result tables (alloc_results) were allocated for
    int alloc_O = 0;                         // what alloc_state was sized for (orders per day)
    int Oqmax = 0;
    int idle_cap_grown = 0;                  // capacity chosen by a reset histogram or vds_set_idle_cap (0: none)
    // device scratch
    int *d_veh_node = nullptr;
    unsigned long long *d_seeds = nullptr;   // vds_reset_random: the replicas' seeds, the fullest start list per replica
    int *d_fullest = nullptr;
    // the lists of the last reset as a packed image (cities too large for the staged reset kernel: vds_tick.hip, k_reset_image),
    // valid while the start nodes (veh_gen) and the tables (tables_gen) are the ones it was taken from
    unsigned *d_reset_img = nullptr; int *d_reset_base = nullptr;
    size_t reset_img_words = 0, reset_base_words = 0;
    unsigned veh_gen = 0, img_veh_gen = 0, img_tables_gen = 0; bool img_valid = false;
    int *d_veh_stage = nullptr;              // vds_reset: the caller's start nodes land here and are checked on the device before they
    unsigned long long *d_bad = nullptr;     // replace d_veh_node (index of the first node outside every cluster, ~0 if none)
    // vds_set_fleet: vehicles per replica by the caller's index (empty: V everywhere, the kernels get a null pointer); a parameter of
    // the resets, not episode state.  d_fleet [R_ext] lives in MEM_STATIC: it outlives loads, maps and vds_set_idle_cap
    std::vector<int> fleet;
    int *d_fleet = nullptr;
    int *d_obs = nullptr;
    long long *d_outc = nullptr;             // vds_outcomes_device: int64 [4][R_ext][C], made on the first request (in MEM_STATE)
    int *d_heads = nullptr; int heads_L = 0; // vds_idle_heads_device: int32 [2][R_ext][C][heads_L], made on the first request (in MEM_STATE)
    long long *d_cnt_per = nullptr, *d_cnt_tot = nullptr;
    int *d_actions = nullptr;
    size_t actions_cap = 0;
    bool profiling = false;
    // vds_run as one hipGraph: the launches of ticks [run_t0, run_t0 + run_n) captured once, replayed while nothing they
    // depend on (tables, capacities, stream) has changed
    hipGraphExec_t run_exec = nullptr;
    int run_t0 = -1, run_n = 0, run_G = 1;
    int slow_tick_cap = 1, slow_tick_C = 1;  // State.slow_tick is [slow_tick_cap][slow_tick_C]
    // k_tick_dense, one shared order day: where it leaves the base form for the wide one (16 lanes per replica, 256-entry tables), by
    // what the last episode did (adapt_dense)
    struct TickForms {
        std::vector<unsigned char> plane;    // [T][C] 1 = the wide form (empty: nothing left the base form)
        enum Kind : unsigned char { BASE, WIDE, MIXED };
        struct Slot { Kind kind; int off, n; };  // compiled from the plane (compile_forms); MIXED: its block map in d_bmap, workgroups
        std::vector<Slot> slot;
        std::vector<int2> bmap_host;         // the block maps of the day (source of the upload: kept while the handle may run them)
        int2 *d_bmap = nullptr; size_t bmap_cap = 0;
        int adapt = 0;                       // 0 undecided, 1 decided; -1 fixed by the caller / environment
        // as read when the day was loaded: VDS_DENSE_TICK_FORMS=alt (tests), VDS_DENSE_TICK_LIM (buckets per slot of the per-slot rule),
        // VDS_DENSE_CLUSTER_LIM (buckets per (slot, cluster)), VDS_DENSE_CLUSTER_SEED (!= 0: a seeded mixed plane: tests); < 0: defaults
        bool alt = false; int tick_lim = -1, cluster_lim = -1, cluster_seed = 0;
        // the last finished episode's counters, copied into pinned host memory behind the stream (request_counters)
        int *pin_slow = nullptr;             // buckets handed to the slow path
        int *pin_tick = nullptr; size_t pin_tick_cap = 0;   // ... per (slot, cluster) (State.slow_tick), when it ran the whole day
        bool ticks_valid = false;
        long long bucket_ticks = 0;          // bucket-ticks of that episode (0: nothing copied)
        hipEvent_t ev = nullptr;             // recorded behind the copies
    } forms;
    unsigned tables_gen = 0;                 // bumped with run_stale: what a graph was built for (the hooked day graph keeps its own copy)
    bool run_stale = false;                  // tables / capacities changed since the graph was built: same shape -> hipGraphExecUpdate
    hipStream_t run_stream = nullptr;
    int use_graph = -1;                      // -1: ask VDS_RUN_GRAPH (default on)
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    // vds_run / vds_run_hooked: replica GROUPS, launched one after another in the day graph (run_group_count)
    int run_groups = -1;                     // -1: ask VDS_RUN_GROUPS (default: one)
    // vds_run_hooked: the hooked day (tick -> observations -> policy -> dispatch per slot) as one executable graph, the plan it was
    // built with (vds_hook_plan.h), and the sticky switches of the vds_run_hooked_* setters
    hipGraphExec_t hook_exec = nullptr;
    hipGraphExec_t hook_policy_exec = nullptr;   // (eager fallback: the caller's policy graph instantiated by itself)
    void *hook_policy_inst = nullptr;
    HookPlan hook_built;
    HookWant want;
    int *d_veh = nullptr;                    // vds_vehicles_device: int32 [6][R_ext][V], made on the first request (in MEM_STATE)
    int *d_vout = nullptr;                   // vds_vehicle_outcomes_device: int32 [R_ext][V][4], made on the first request (in MEM_STATE)
    int *d_orders = nullptr;                 // vds_orders_device: int32 [R_ext][O][2], made on the first request (in MEM_RESULTS, next to `out`)
    int *d_roster = nullptr;                 // vds_idle_roster_device: int32 [3][R_ext][V] planes, then int32 [R_ext][C + 1] offsets, made on the first request (in MEM_STATE)
    bool roster_fresh = false;               // the block describes the idle lists as they stand: set by a refresh, cleared by whatever can change a list or re-make the tables
    // vds_snapshot / vds_restore: ONE saved episode state per handle - a store sized like the state and result tables it mirrors, made
    // on the first vds_snapshot (a handle that never takes one allocates nothing), and the host's part of the state: the clock
    unsigned state_gen = 0;                  // bumped wherever the state / result tables are re-made or their meaning changes (another day, another
                                             // map, other capacities, the supply planes switched on, the base form of the whole-day rule): a
                                             // snapshot taken before is void.  (Not tables_gen: that one also moves with the run groups and the
                                             // per-slot forms, which leave the tables alone - a snapshot outlives them as it outlives a reset.)
    struct Snap {
        State D{};                           // the store: hdr, cnt, idle, ring, ring_min, ring_cnt, fl, inbox, sup, arr, out (the rest stays null)
        long long bytes = 0;
        bool valid = false;
        unsigned gen = 0;                    // state_gen and the capacities the store was made for / the snapshot taken under
        int R = 0, C = 0, idle_cap = 0, ring_cap = 0, fl_cap = 0, H = 0, dense = 0, Oq = 0, arr_slots = 0;
        bool sup = false, arr = false;
        int t = 0, last_stepped = -1, dispatch_seq = 0, seq_tick0 = 0, seq_tick = -1, matched_tick = -1;
        int *d_map = nullptr;                // [R] the restore map in stored replica indices (host maps are uploaded here, device maps checked into it)
        // host maps are staged in two alternating pinned buffers, each guarded by an event recorded behind its upload: vds_restore waits
        // only for the upload of the restore before the last one, which has long finished - the call stays asynchronous
        int *pin_map[2] = {nullptr, nullptr};
        hipEvent_t pin_ev[2] = {nullptr, nullptr};
        bool pin_used[2] = {false, false};
        int pin_i = 0;
    } snap;
    // vds_set_match_external: the step is Update alone, the slot's matches come from vds_apply_match_device (vds_match_external.hip)
    bool match_external = false;
    int matched_tick = -1;                   // the slot whose vds_apply_match_device has been issued (-1: none since the clock was reset)
    int *d_claim = nullptr;                  // int32 [S.R][V], INT_MAX between calls; made on the first vds_apply_match_device (in MEM_STATE)
    int *d_match_rec = nullptr, *d_match_off = nullptr;      // vds_match_orders_device: int32 [Oq][4] / [T + 1] (in MEM_ORDERS), and their host copies
    std::vector<int> match_rec, match_off;
    bool restored_episode = false;           // the episode continues from a snapshot: its slow-path statistics describe no whole day (adapt_dense)
};

int fail(vds_handle *h, int code, const char *fmt, ...);      // sets vds_last_error (h null: the thread's create error), returns code

#define HIPCHK(h, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return fail(h, VDS_EHIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// n elements (0: one) as a block of group g
template <typename T>
int dev_alloc(vds_handle *h, DevGroup &g, T **p, size_t n) {
    const hipError_t e = g.alloc(p, n);
    if (e != hipSuccess) return fail(h, VDS_ENOMEM, "device allocation of %zu bytes failed: %s", std::max<size_t>(n, 1) * sizeof(T), hipGetErrorString(e));
    return VDS_OK;
}
template <typename T>
int dev_alloc(vds_handle *h, Mem g, T **p, size_t n) { return dev_alloc(h, h->mem[g], p, n); }

// What a change makes stale.  DAY_GRAPHS / GRAPH_TABLES: the day graphs hold other launches / the tables or capacities they read changed
// (run_stale and tables_gen, which the hooked day graph and the reset image compare); STATE_MEANING: the state / result tables were re-made
// or mean something else (state_gen: a snapshot taken before is void).  The first two move the same fields today, on purpose: the call
// site records which of the two happened, nothing tells them apart yet.
enum Changed : unsigned { DAY_GRAPHS = 1, GRAPH_TABLES = 2, STATE_MEANING = 4 };
inline void invalidate(vds_handle *h, unsigned changed) {
    if (changed & (DAY_GRAPHS | GRAPH_TABLES)) { h->run_stale = true; h->tables_gen++; }
    if (changed & STATE_MEANING) h->state_gen++;
    h->roster_fresh = false;
}
// the episode clock back to the start of the day
inline void clock_reset(vds_handle *h) { h->t = 0; h->last_stepped = -1; h->dispatch_seq = 0; h->seq_tick = -1; h->matched_tick = -1; h->roster_fresh = false; }

// No C++ exception may cross the C ABI (vds.h: "never abort"): host allocation failures and the like become a
// status code + vds_last_error.
template <typename F>
int guarded(vds_handle *h, const char *name, F &&body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(h, VDS_ENOMEM, "%s: out of host memory", name);
    } catch (const std::exception &e) {
        return fail(h, VDS_EINVAL, "%s: %s", name, e.what());
    } catch (...) {
        return fail(h, VDS_EINVAL, "%s: unknown C++ exception", name);
    }
}

// One chain of launches: on a stream they are issued in order, in a graph every node depends on the one added before it (day graphs
// are one chain: see the note in vds_api.hip).  add(emit_x, args...) calls emit_x(Emit, args...); after a failure the rest is skipped and err
// says what failed.
struct Chain {
    Emit e;
    hipGraphNode_t tail = nullptr, node = nullptr;
    hipError_t err = hipSuccess;
    explicit Chain(hipStream_t st) { e.st = st; }
    explicit Chain(hipGraph_t g) { e.graph = g; e.node = &node; e.err = &err; }
    Chain(const Chain &) = delete;
    template <typename F, typename... A> void add(F emit, A &&...a) {
        if (err != hipSuccess) return;
        e.deps = tail ? &tail : nullptr; e.ndeps = tail ? 1 : 0;
        emit(e, a...);
        if (e.graph && err == hipSuccess) tail = node;
    }
    // (graphs only) a node without work; a captured graph of the caller's as a child graph
    void add_empty() { add([](const Emit &e) { *e.err = hipGraphAddEmptyNode(e.node, e.graph, e.deps, e.ndeps); }); }
    void add_child(hipGraph_t child) { add([child](const Emit &e) { *e.err = hipGraphAddChildGraphNode(e.node, e.graph, e.deps, e.ndeps, child); }); }
};

// external matching: the reference runs Match before Dispatch (:1079-1083), and the arrival keys order a slot's match entries before its
// dispatch entries - so nothing of slot t but its match may follow its step until vds_apply_match_device has been issued
inline int match_pending(vds_handle *h, const char *fn) {
    if (h->match_external && h->last_stepped == h->t && h->matched_tick != h->t)
        return fail(h, VDS_ESTATE, "%s: external matching: slot %d has been stepped but not matched - call vds_apply_match_device first", fn, h->t);
    return VDS_OK;
}

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ---- defined in one unit, called from others
// vds_api_read.hip: the derived blocks, for the entry points there and for the hooked day (vds_api.hip).  ensure_x makes block x on
// the first request; refresh_x adds the kernels that rewrite it to a chain, for the replicas [r_lo, r_lo + r_n) (r_n <= 0: all) - the
// blocks without a refresh_x take one kernel (emit_slot_outcomes, emit_idle_heads, emit_idle_roster)
int ensure_outcomes(vds_handle *h);
int ensure_idle_heads(vds_handle *h, int L);
int ensure_vehicles(vds_handle *h);
int ensure_vehicle_outcomes(vds_handle *h);
int ensure_idle_roster(vds_handle *h);
int ensure_orders(vds_handle *h);
void refresh_vehicles(Chain &c, vds_handle *h, int t_last, int planes, int r_lo, int r_n);
void refresh_vehicle_outcomes(Chain &c, vds_handle *h, int t, int stepped, int r_lo, int r_n);
void refresh_orders_block(Chain &c, vds_handle *h, int slot_lo, int slot_hi, int last, int r_lo, int r_n);
// the roster block's offsets, int32 [R_ext][C + 1] behind its three planes
inline int *roster_off(vds_handle *h) { return h->d_roster + 3 * (size_t)h->R_ext * h->S.V; }
