// Host tables of libvds: what vds_load_static / vds_load_order_days / vds_set_replica_days compute before anything is uploaded.
// Plain host arithmetic on explicit inputs: no HIP runtime call, no vds_handle (vds_api.hip owns both), so that every builder also
// runs on a machine without a GPU (vds_debug_order_tables / vds_debug_replica_plan, tests/test_order_tables.py, tables_check.cpp).
// A builder that can fail returns a VDS_* code and leaves the text of vds_last_error in `msg`.
#ifndef VDS_TABLES_H
#define VDS_TABLES_H

#include "vds_device.h"

#include <functional>
#include <new>
#include <string>
#include <utility>
#include <vector>

namespace vds {

// host tables that are written completely before they are read (the sorted order records of a load: 50 MB at 16 days): resize()
// default-initialises, so the pages are first touched by the day workers that fill them, not zeroed by the calling thread first
template <typename T>
struct NoInitAlloc {
    using value_type = T;
    NoInitAlloc() = default;
    template <class U> NoInitAlloc(const NoInitAlloc<U> &) {}
    T *allocate(size_t n) { return static_cast<T *>(::operator new(n * sizeof(T))); }
    void deallocate(T *p, size_t) { ::operator delete(p); }
    template <class U, class... A> void construct(U *p, A &&...a) {
        if constexpr (sizeof...(A) == 0) ::new ((void *)p) U; else ::new ((void *)p) U(std::forward<A>(a)...);
    }
    bool operator==(const NoInitAlloc &) const { return true; }
    bool operator!=(const NoInitAlloc &) const { return false; }
};
template <typename T> using hvec = std::vector<T, NoInitAlloc<T>>;

// Where a builder puts one of its LARGE arrays (so_rec, so_slot, d_rec): the caller hands out n uninitialised elements that outlive
// the call - vds_api.hip sizes a vector in a pinned block and uploads from it, so no builder copies such an array
template <typename T> using Place = std::function<T *(size_t n)>;

// the order days of one load are independent until their tables are laid back to back: at most min(threads, 16, n_days) workers
// take days off a counter (one: the calling thread).  fn(d) must not throw.
void for_each_day(int n_days, int threads, const std::function<void(int)> &fn);

// FindServerVehicleFunction (:978-996): clusters in the order the recursion marks them visited, start cluster first
void dfs_visit(int start, int limit, const int32_t *off, const int32_t *idx, std::vector<char> &seen, std::vector<int> &seq);

// ---- city tables (vds_load_static)
struct CityTables {
    int N = 0, C = 0;
    int max_nc = 0;                          // nodes of the largest cluster
    int max_seq = 0, seq_pad = 64;           // longest visit sequence of FindServerVehicleFunction over the clusters, padded row length
    bool any_seq = false;                    // some cluster has a visit sequence beyond itself
    int cmin = 0, cmax = 0;                  // cost range of the whole matrix
    bool u8_blocks = false;                  // every cost inside a cluster block is 0..255: blk8 is filled, cdesc.z / cdesc_ord.w point into it
    bool u8_ok = false;                      // ... and every cost of the matrix: cost8 exists
    bool dense_ok = false, dense_bytes = false;      // the dense blocks exist (max_nc <= 255, < 2^31 bytes); as bytes (every block cost <= 254)
    std::vector<int> cost, costp;            // the matrix as given; with CLUSTER-CONTIGUOUS columns (column cl_off[c] + l holds node cl_nodes[cl_off[c] + l])
    std::vector<int> node2cluster, node_local, cl_off, cl_nodes;
    std::vector<long long> blk_off;          // [C + 1]
    std::vector<int> blk;                    // per-cluster cost blocks: blk[c][p][l] = RoadCost(node_l, node_p) = cost[node_p*N + node_l] (:929)
    std::vector<int4> cdesc;                 // [C] {n_c, block offset, byte block offset, 0}
    std::vector<int> corder;                 // clusters, heaviest first
    std::vector<int4> cdesc_ord;             // cdesc in that order {n_c, block offset, cluster, byte block offset}
    std::vector<unsigned char> blk8;         // byte copy of the blocks (one zero byte when !u8_blocks)
    std::vector<unsigned char> cost8;        // byte copy of costp (+ 16 bytes), empty unless u8_ok
    std::vector<unsigned char> lbc;          // [N][C] cheapest way from any node of the cluster to the pickup node (empty: none)
    std::vector<unsigned char> blk_dense;    // dense blocks: row stride n_c + 1, the extra column holds the dead cost (empty unless dense_ok)
    std::vector<int4> cdesc_dense;           // [C] {n_c, byte offset into blk_dense, cluster, has a visit sequence}, heaviest first
    std::vector<int> cl_cmax;                // [C] largest cost inside the cluster's block
    std::vector<int> dfs_off, dfs_seq;       // visit sequences without the start cluster
    std::vector<unsigned> vis_bits;          // [C][(C + 31) / 32] the visit sets as a bit matrix
};
// nbr_off == nullptr: no neighbour search (vds_config.neighbor_can_server == 0)
int build_city_tables(const int32_t *cost, int N, const int32_t *node2cluster, int C, const int32_t *nbr_off, const int32_t *nbr_idx,
                      int depth_limit, CityTables &out, std::string &msg);

// what the order builders read of a city
struct CityView {
    int N, C, tick_minutes;
    const int *cost, *node2cluster, *node_local, *cl_cmax;
};

// ---- order tables (vds_load_order_days)
// One loaded order day on the host side (the device side is vds::DayDesc)
struct DayHost {
    int O = 0;                           // all orders of the day incl. never-processed ones
    int T = 0, now0 = 0, q_base = 0, Oq = 0;
    std::vector<int> so_id;              // q - q_base -> order id
    std::vector<int> q_value;            // q - q_base -> OrderValue (:341-342)
    std::vector<int> q_of;               // order id -> q - q_base, -1 never processed (built on first use by the dense read side)
    std::vector<int> o_tick;             // order id -> tick (or -1 never processed)
    std::vector<long long> value_upto;   // [T+1] prefix of OrderValue of processed orders by tick
    long long value_all = 0;
};
struct OrderTables {
    int n_days = 0, C = 0;
    int4 *so_rec = nullptr; size_t n_rec = 0;        // sorted by (day, tick, pickup cluster, id): {id, local nodes, clusters, OrderValue}; placed by the caller
    hvec<int> bkt_off, tick_off, ord_q, so_pnode;    // absolute positions; ord_q: a slot's positions in id order
    std::vector<DayDesc> ddesc;                      // the days (+ the empty day of padding replicas, last)
    int Oqmax = 0, Omax = 0, mto = 0;                // most processed orders / orders of a day, most orders of a slot
    long long Ototal = 0;
};
// days: the caller's, re-assigned element by element, so that another load of as many days refills the vectors of the load before
// (50 MB at 16 days stay mapped); after a failure some of its entries are partly filled
int build_order_tables(const CityView &city, int n_days, const int64_t *day_off, const int32_t *release_min, const int32_t *pickup,
                       const int32_t *delivery, int threads, const Place<int4> &place_rec, OrderTables &out, std::vector<DayHost> &days,
                       std::string &msg);
// rank of every sorted position inside its slot; the first bucket (index into bkt_off) of every sorted position's slot
std::vector<int> build_order_ranks(const OrderTables &ot, int threads);
std::vector<int> build_first_buckets(const OrderTables &ot, int threads);

// the order block of vds_match_orders_device for day 0: rec int32 [Oq][4] by Order.ID, slot_off int32 [T + 1]; delivery: the day's array as loaded
void build_match_orders(const OrderTables &ot, const int32_t *delivery, std::vector<int> &rec, std::vector<int> &slot_off);

// ---- static arrival slots of the dense tick ("pull", vds_device.h)
struct PullTables {
    bool ok = false;                         // the verdict: false - the dense tick keeps the arrival ring (nothing below is to be used)
    int *so_slot = nullptr;                  // [n_rec] slot inside the day's d_rec slice, -1: no pull order; placed by the caller
    int2 *d_rec = nullptr; size_t n_drec = 0;        // placed by the caller
    std::vector<int> d_first;
    std::vector<int4> ddesc2;                // per day {d_first base, d_rec base, TA, slots} (+ the empty day)
    int W = 0, hmax = 0, Od_max = 0;
};
// every_order: the stamp form's condition "every processed order owns a slot" is part of the verdict
int build_pull_tables(const OrderTables &ot, const CityView &city, int ring_ticks, bool every_order, int threads, const Place<int> &place_slot,
                      const Place<int2> &place_drec, PullTables &out, std::string &msg);

// slot (absolute d_rec position) -> q - q_base of its order, for tables with pt.ok; slot_q is the caller's and is re-assigned in place
// (a load of as many orders as the one before refills it)
void build_slot_orders(const OrderTables &ot, const PullTables &pt, int threads, std::vector<int> &slot_q);

// per-bucket descriptors of the dense tick with one shared day (Static.tdesc); pull == nullptr: no static arrival slots
std::vector<int4> build_bucket_descs(const OrderTables &ot, const std::vector<int> &corder, const std::vector<int4> &cdesc_dense, const PullTables *pull);

// ---- the storage order of the replicas for a replica -> day map (vds_set_replica_days)
struct ReplicaPlan {
    int R = 0, row_gran = 16, chunk_days = 0;
    std::vector<int> int2ext, ext2int;       // empty: identity
    std::vector<int> rperm;                  // row slot -> internal replica, -1 for a dummy (empty: none)
    std::vector<int> day_of_internal;        // [R]; n_days: the empty day of a dummy
};
// gran8_ok: day groups of 8 / 4 replicas may be used; regroup_ok: the replicas may be stored regrouped by day; alloc_R: stored replicas
// the state tables at hand were allocated for (0: none) - a plan that needs fewer keeps that many while the padding stays under a quarter
ReplicaPlan plan_replicas(const int *replica_day, int R_ext, int n_days, bool gran8_ok, bool regroup_ok, int alloc_R);

}  // namespace vds
#endif
