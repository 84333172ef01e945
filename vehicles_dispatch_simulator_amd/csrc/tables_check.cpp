// Stand-alone check of the host tables' builders (vds_tables.h) for `make hostcheck`: synthetic cities and order days, every table
// built with 1 and with 4 threads, under the address / undefined-behaviour and the thread sanitizer.  Links vds_tables.hip only.
#include "../../include/vds.h"
#include "vds_tables.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace vds;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "tables_check: %s fails (line %d; C=%d days=%d neighbours=%d)\n", #c, __LINE__, C, n_days, (int)with_nbr); exit(1); } } while (0)

static unsigned long long g_lcg = 12345;
static int rnd(int n) { g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull; return (int)((g_lcg >> 33) % (unsigned)n); }

template <typename V> static bool monotone(const V &v) { for (size_t i = 1; i < v.size(); ++i) if (v[i] < v[i - 1]) return false; return true; }
static bool permutation(std::vector<int> v, int base) {      // of base .. base + n - 1
    std::sort(v.begin(), v.end());
    for (size_t i = 0; i < v.size(); ++i) if (v[i] != base + (int)i) return false;
    return true;
}
template <typename T> static void same(const T *a, const T *b, size_t n, const char *what) {
    if (n && memcmp(a, b, n * sizeof(T))) { fprintf(stderr, "tables_check: %s differs between 1 and 4 threads\n", what); exit(1); }
}

struct Built { std::vector<DayHost> days; hvec<int4> rec; hvec<int> slot; hvec<int2> drec; OrderTables ot; PullTables pt; std::vector<int> rank, bkt0, slot_q; std::vector<int4> td; };

int main() {
    for (int C : {1, 4, 48})
        for (int n_days : {1, 3, 16})
            for (bool with_nbr : {false, true}) {
                const int N = 20 + rnd(181), tick = 3 + rnd(10), ring = 8 << rnd(3);
                std::vector<int> cost((size_t)N * N), n2c(N), nbr_off(C + 1, 0), nbr_idx;
                for (int &c : cost) c = rnd(60 * tick / 10 + 5);
                for (int &c : n2c) c = rnd(C + 1) - (rnd(8) == 0);          // some nodes outside every cluster, some clusters may own none
                for (int &c : n2c) if (c >= C) c = C - 1;
                for (int c = 0; c < C; ++c) { for (int k = rnd(4); k > 0; --k) nbr_idx.push_back(rnd(C)); nbr_off[c + 1] = (int)nbr_idx.size(); }
                CityTables ct;
                std::string msg;
                CHECK(build_city_tables(cost.data(), N, n2c.data(), C, with_nbr ? nbr_off.data() : nullptr, nbr_idx.data(), rnd(4) - 1, ct, msg) == VDS_OK);
                CHECK(monotone(ct.cl_off) && monotone(ct.blk_off) && monotone(ct.dfs_off) && permutation(ct.corder, 0));
                CHECK(ct.cl_off[C] <= N && (int)ct.dfs_seq.size() == ct.dfs_off[C] && ct.max_seq <= C);
                std::vector<int> inside;
                for (int n = 0; n < N; ++n) if (n2c[n] >= 0) inside.push_back(n);
                { std::vector<int> nodes(ct.cl_nodes); std::sort(nodes.begin(), nodes.end()); CHECK(nodes == inside); }
                if (inside.empty()) continue;
                std::vector<int64_t> day_off(n_days + 1, 0);
                std::vector<int32_t> rel, pk, dl;
                for (int d = 0; d < n_days; ++d) {
                    const int O = d == 1 ? 1 : 1 + rnd(1500);
                    int t = rnd(100);
                    for (int i = 0; i < O; ++i) {
                        rel.push_back(t + (rnd(16) == 0 ? -rnd(30) : 0)); t += rnd(4);          // mostly sorted, some earlier
                        pk.push_back(inside[rnd((int)inside.size())]); dl.push_back(inside[rnd((int)inside.size())]);
                    }
                    day_off[d + 1] = (int64_t)rel.size();
                }
                const CityView cv{N, C, tick, ct.cost.data(), ct.node2cluster.data(), ct.node_local.data(), ct.cl_cmax.data()};
                Built B[2];
                for (int k = 0; k < 2; ++k) {
                    Built &b = B[k];
                    const int nt = k ? 4 : 1;
                    CHECK(build_order_tables(cv, n_days, day_off.data(), rel.data(), pk.data(), dl.data(), nt, [&](size_t n) { b.rec.resize(n); return b.rec.data(); }, b.ot, b.days, msg) == VDS_OK);
                    b.rank = build_order_ranks(b.ot, nt); b.bkt0 = build_first_buckets(b.ot, nt);
                    CHECK(build_pull_tables(b.ot, cv, ring, false, nt, [&](size_t n) { b.slot.resize(n); return b.slot.data(); },
                                            [&](size_t n) { b.drec.resize(n); return b.drec.data(); }, b.pt, msg) == VDS_OK);
                    if (b.pt.ok) build_slot_orders(b.ot, b.pt, nt, b.slot_q);
                    if (n_days == 1 && !ct.cdesc_dense.empty()) b.td = build_bucket_descs(b.ot, ct.corder, ct.cdesc_dense, b.pt.ok ? &b.pt : nullptr);
                }
                const OrderTables &ot = B[0].ot;
                const PullTables &pt = B[0].pt;
                CHECK(monotone(ot.bkt_off) && monotone(ot.tick_off) && (int)ot.ddesc.size() == n_days + 1);
                CHECK(permutation(std::vector<int>(ot.ord_q.begin(), ot.ord_q.end()), 0));
                for (int d = 0; d < n_days; ++d) {
                    const DayDesc &de = ot.ddesc[d];
                    CHECK(ot.tick_off[de.tick_base] == de.q_base && ot.tick_off[de.tick_base + de.T] == de.q_base + de.Oq);
                    CHECK(ot.bkt_off[de.bkt_base] == de.q_base && ot.bkt_off[de.bkt_base + de.T * C] == de.q_base + de.Oq);
                    std::vector<int> ids(B[0].days[d].so_id), slots;
                    std::sort(ids.begin(), ids.end());
                    CHECK(std::adjacent_find(ids.begin(), ids.end()) == ids.end() && (ids.empty() || (ids[0] >= 0 && ids.back() < B[0].days[d].O - 1)));
                    if (!pt.d_rec) continue;
                    const int4 d2 = pt.ddesc2[d];
                    for (int q = de.q_base; q < de.q_base + de.Oq; ++q) if (pt.so_slot[q] >= 0) slots.push_back(pt.so_slot[q]);
                    CHECK((int)slots.size() == d2.w && permutation(slots, 0) && d2.y + d2.w <= (int)pt.n_drec);
                    for (int c = 0; c < C; ++c) {
                        CHECK(pt.d_first[d2.x + c] >= d2.y && pt.d_first[d2.x + (size_t)d2.z * C + c] <= d2.y + d2.w);
                        for (int a = 0; a < d2.z; ++a) CHECK(pt.d_first[d2.x + (size_t)a * C + c] <= pt.d_first[d2.x + (size_t)(a + 1) * C + c]);
                    }
                }
                const Built &a = B[0], &b = B[1];
                CHECK(a.ot.n_rec == b.ot.n_rec && a.pt.n_drec == b.pt.n_drec && a.pt.ok == b.pt.ok && a.pt.W == b.pt.W && a.pt.hmax == b.pt.hmax && a.pt.Od_max == b.pt.Od_max);
                CHECK(a.ot.bkt_off.size() == b.ot.bkt_off.size() && a.ot.tick_off.size() == b.ot.tick_off.size() && a.pt.d_first == b.pt.d_first && a.slot_q == b.slot_q);
                CHECK(a.rank == b.rank && a.bkt0 == b.bkt0 && a.td.size() == b.td.size());
                same(a.ot.so_rec, b.ot.so_rec, a.ot.n_rec, "so_rec"); same(a.pt.so_slot, b.pt.so_slot, a.ot.n_rec, "so_slot"); same(a.pt.d_rec, b.pt.d_rec, a.pt.n_drec, "d_rec");
                same(a.ot.bkt_off.data(), b.ot.bkt_off.data(), a.ot.bkt_off.size(), "bkt_off"); same(a.ot.tick_off.data(), b.ot.tick_off.data(), a.ot.tick_off.size(), "tick_off");
                same(a.ot.ord_q.data(), b.ot.ord_q.data(), a.ot.n_rec, "ord_q"); same(a.ot.so_pnode.data(), b.ot.so_pnode.data(), a.ot.n_rec, "so_pnode");
                same(a.ot.ddesc.data(), b.ot.ddesc.data(), a.ot.ddesc.size(), "ddesc"); same(a.td.data(), b.td.data(), a.td.size(), "tdesc");
                same(a.pt.ddesc2.data(), b.pt.ddesc2.data(), a.pt.ddesc2.size(), "ddesc2");
                for (int R : {16, 40, 96}) {          // replica plans: every real replica stored once, on its day
                    std::vector<int> rd(R);
                    for (int &x : rd) x = rnd(n_days);
                    const ReplicaPlan P = plan_replicas(rd.data(), R, n_days, rnd(2) != 0, true, 0);
                    CHECK((int)P.day_of_internal.size() == P.R && P.R >= R && (P.int2ext.empty() || P.R % 16 == 0));
                    for (int i = 0; i < P.R && !P.int2ext.empty(); ++i)
                        CHECK(P.int2ext[i] < 0 ? P.day_of_internal[i] == n_days && P.rperm[i] < 0 : P.ext2int[P.int2ext[i]] == i && P.day_of_internal[i] == rd[P.int2ext[i]]);
                }
            }
    puts("tables_check: ok");
    return 0;
}
