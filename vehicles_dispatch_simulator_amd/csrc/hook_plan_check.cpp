// Stand-alone check of the hooked day's plan value (vds_hook_plan.h) for `make hostcheck`.  The oracle is the text the plan replaced:
// the cache fields vds_handle had (`Old`, their names), the store-back that filled them, and the two expressions vds_run_hooked
// compared them with (`same` without its hook_exec term, and `same_shape`), transcribed as they stood.  A call's inputs (`Call`: the
// arguments and the locals run_hooked_impl derived from the sticky switches) are changed one field and two fields at a time; the plan
// of each must compare with the plan of the base exactly as the old expressions compare the two.
#include "vds_hook_plan.h"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

using namespace vds;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "hook_plan_check: %s fails (line %d)\n", #c, __LINE__); exit(1); } } while (0)

// one call of vds_run_hooked as run_hooked_impl saw it
struct Call {
    int t, n_ticks, G, planes, K;
    const void *dev_actions; void *policy_graph; const void *stream; unsigned tables_gen;
    int HL, VP; const int *VT; bool VO, RO; const int *RT; bool OB;
    const long long *d_outc; const int *d_heads, *d_veh, *d_vout, *d_roster, *d_orders;       // the handle's blocks (there or not, on or off)
};
// "what the graph at hand was built with"
struct Old {
    int hook_t0, hook_n, hook_G, hook_planes, hook_K;
    unsigned hook_gen;
    const long long *hook_outc;
    const int *hook_heads; int hook_heads_L;
    int hook_veh_planes; const void *hook_veh_targets; const int *hook_veh;
    const int *hook_vout, *hook_orders, *hook_roster; const void *hook_roster_targets;
    const void *hook_actions; void *hook_policy; const void *hook_stream;
};

// the store-back after install_graph
static Old store_back(const Call &c) {
    Old h{};
    const int HL = c.HL, VP = c.VP; const int *VT = c.VT, *RT = c.RT; const bool VO = c.VO, RO = c.RO, OB = c.OB;
    h.hook_t0 = c.t; h.hook_n = c.n_ticks; h.hook_G = c.G; h.hook_planes = c.planes; h.hook_K = c.K; h.hook_actions = c.dev_actions;
    h.hook_policy = c.policy_graph; h.hook_stream = c.stream; h.hook_gen = c.tables_gen; h.hook_outc = c.d_outc;
    h.hook_heads = HL > 0 ? c.d_heads : nullptr; h.hook_heads_L = HL;
    h.hook_veh_planes = VP; h.hook_veh_targets = VT; h.hook_veh = VP ? c.d_veh : nullptr;
    h.hook_vout = VO ? c.d_vout : nullptr;
    h.hook_roster = RO ? c.d_roster : nullptr; h.hook_roster_targets = RT;
    h.hook_orders = OB ? c.d_orders : nullptr;
    return h;
}
static bool old_same(const Old *h, const Call &c) {
    const int HL = c.HL, VP = c.VP, G = c.G, planes = c.planes, K = c.K, n_ticks = c.n_ticks; const int *VT = c.VT, *RT = c.RT; const bool VO = c.VO, RO = c.RO, OB = c.OB;
    const void *dev_actions = c.dev_actions; void *policy_graph = c.policy_graph;
    const bool same = h->hook_gen == c.tables_gen && h->hook_t0 == c.t && h->hook_n == n_ticks && h->hook_G == G && h->hook_planes == planes && h->hook_K == K &&
                      h->hook_actions == dev_actions && h->hook_policy == policy_graph && h->hook_stream == c.stream && h->hook_outc == c.d_outc &&
                      h->hook_heads == (HL > 0 ? c.d_heads : nullptr) && h->hook_heads_L == HL &&
                      h->hook_veh_planes == VP && h->hook_veh_targets == VT && h->hook_veh == (VP ? c.d_veh : nullptr) &&
                      h->hook_vout == (VO ? c.d_vout : nullptr) &&
                      h->hook_roster == (RO ? c.d_roster : nullptr) && h->hook_roster_targets == RT &&
                      h->hook_orders == (OB ? c.d_orders : nullptr);
    return same;
}
static bool old_same_shape(const Old *h, const Call &c) {
    const int HL = c.HL, VP = c.VP, G = c.G, planes = c.planes, K = c.K, n_ticks = c.n_ticks; const int *VT = c.VT, *RT = c.RT; const bool VO = c.VO, RO = c.RO, OB = c.OB;
    void *policy_graph = c.policy_graph;
    const bool same_shape = h->hook_n == n_ticks && h->hook_G == G && ((h->hook_planes & 31) != 0) == ((planes & 31) != 0) && (h->hook_planes & VDS_PLANE_OUTCOMES) == (planes & VDS_PLANE_OUTCOMES) && (h->hook_heads_L > 0) == (HL > 0) &&
                            (h->hook_K > 0) == (K > 0) && (h->hook_policy != nullptr) == (policy_graph != nullptr) &&
                            (h->hook_veh_planes != 0) == (VP != 0) && (h->hook_veh_targets != nullptr) == (VT != nullptr) &&
                            (h->hook_vout != nullptr) == VO &&
                            (h->hook_roster != nullptr) == RO && (h->hook_roster_targets != nullptr) == (RT != nullptr) &&
                            (h->hook_orders != nullptr) == OB;
    return same_shape;
}

// the plan of a call: the old cache fields, one to one
static HookPlan plan_of(const Call &c) {
    const Old o = store_back(c);
    HookPlan p;
    p.t0 = o.hook_t0; p.n = o.hook_n; p.G = o.hook_G; p.planes = o.hook_planes; p.K = o.hook_K; p.heads_L = o.hook_heads_L; p.veh_planes = o.hook_veh_planes;
    p.gen = o.hook_gen; p.stream = o.hook_stream; p.actions = o.hook_actions; p.policy = o.hook_policy;
    p.outc = o.hook_outc; p.heads = o.hook_heads; p.veh = o.hook_veh; p.vout = o.hook_vout; p.roster = o.hook_roster; p.orders = o.hook_orders;
    p.veh_targets = (const int *)o.hook_veh_targets; p.roster_targets = (const int *)o.hook_roster_targets;
    return p;
}

// addresses that are never read
static long long g_ll[4];
static int g_int[64];
static char g_byte[16];

// One way to change one field of a call.  Every field has three: two values that are on (non-null, non-zero) and differ, and off;
// a change that leaves the field as the base has it is the "and back" case.
typedef std::function<void(Call &)> Change;
static std::vector<std::vector<Change>> changes() {
    std::vector<std::vector<Change>> f;
#define FIELD(name, a, b, off) f.push_back({[](Call &c) { c.name = a; }, [](Call &c) { c.name = b; }, [](Call &c) { c.name = off; }})
    FIELD(t, 4, 6, 0);
    FIELD(n_ticks, 2, 3, 0);
    FIELD(G, 2, 3, 1);
    FIELD(K, 3, 5, 0);
    FIELD(dev_actions, g_byte + 1, g_byte + 2, nullptr);
    FIELD(policy_graph, g_byte + 3, g_byte + 4, nullptr);
    FIELD(stream, g_byte + 5, g_byte + 6, nullptr);
    FIELD(tables_gen, 7u, 9u, 0u);
    FIELD(HL, 2, 3, 0);
    FIELD(VP, 5, 63, 0);
    FIELD(VT, g_int + 1, g_int + 2, nullptr);
    FIELD(VO, true, true, false);
    FIELD(RO, true, true, false);
    FIELD(RT, g_int + 3, g_int + 4, nullptr);
    FIELD(OB, true, true, false);
    FIELD(d_outc, g_ll + 1, g_ll + 2, nullptr);
    FIELD(d_heads, g_int + 5, g_int + 6, nullptr);
    FIELD(d_veh, g_int + 7, g_int + 8, nullptr);
    FIELD(d_vout, g_int + 9, g_int + 10, nullptr);
    FIELD(d_roster, g_int + 11, g_int + 12, nullptr);
    FIELD(d_orders, g_int + 13, g_int + 14, nullptr);
#undef FIELD
    // the mask: the five planes and the outcomes bit are two switches of the shape
    f.push_back({[](Call &c) { c.planes = (c.planes & VDS_PLANE_OUTCOMES) | 5; }, [](Call &c) { c.planes = (c.planes & VDS_PLANE_OUTCOMES) | 31; }, [](Call &c) { c.planes &= VDS_PLANE_OUTCOMES; }});
    f.push_back({[](Call &c) { c.planes |= VDS_PLANE_OUTCOMES; }, [](Call &c) { c.planes |= VDS_PLANE_OUTCOMES; }, [](Call &c) { c.planes &= 31; }});
    return f;
}

// what the ensure_* calls see to before a plan is made: a block that is on is there
static Call ensured(Call c) {
    if ((c.planes & VDS_PLANE_OUTCOMES) && !c.d_outc) c.d_outc = g_ll + 3;
    if (c.HL > 0 && !c.d_heads) c.d_heads = g_int + 20;
    if (c.VP && !c.d_veh) c.d_veh = g_int + 21;
    if (c.VO && !c.d_vout) c.d_vout = g_int + 22;
    if (c.RO && !c.d_roster) c.d_roster = g_int + 23;
    if (c.OB && !c.d_orders) c.d_orders = g_int + 24;
    return c;
}

static long long g_cases = 0, g_equal = 0, g_shape = 0;
static void compare(const Call &a0, const Call &b0) {
    const Call a = ensured(a0), b = ensured(b0);
    const Old built = store_back(a);
    const HookPlan pa = plan_of(a), pb = plan_of(b);
    const bool same = old_same(&built, b), shape = old_same_shape(&built, b);
    CHECK((pa == pb) == same);
    CHECK((pa != pb) == !same);
    CHECK(same_shape(pa, pb) == shape);
    ++g_cases; g_equal += same; g_shape += shape;
}

// The arrival minutes and counted flags of the two target tensors (vds_run_hooked_vehicles_ex / vds_run_hooked_roster_ex), which the
// text the plan replaced never had: the rules are written out.  An address alone makes another plan (no stale graph is served); a
// dispatch node with either tensor is the timed kernel and without both the plain one, so switching them on or off is another shape
// (the graph is built anew) and another address of a tensor that stays on is the same shape (parameters replaced in place).
static long long check_times(const HookPlan &base) {
    CHECK(!base.veh_timed() && !base.roster_timed());
    long long n = 0;
    const int *HookPlan::*fields[4] = {&HookPlan::veh_arrive, &HookPlan::veh_counted, &HookPlan::roster_arrive, &HookPlan::roster_counted};
    for (int i = 0; i < 4; ++i) {
        HookPlan a = base, b = base;
        a.*fields[i] = g_int + 30 + i; b.*fields[i] = g_int + 40 + i;
        CHECK(a != base && base != a && b != base && a != b && a == a);
        CHECK(!same_shape(base, a) && !same_shape(a, base));                 // on / off: another kernel
        CHECK(same_shape(a, b) && same_shape(b, a));                         // another address: in place
        CHECK((i < 2 ? a.veh_timed() : a.roster_timed()) && !(i < 2 ? a.roster_timed() : a.veh_timed()));
        // the second tensor of the same form on top: still the timed kernel; of the other form: that form's node changes
        for (int j = 0; j < 4; ++j) {
            if (j == i) continue;
            HookPlan c = a;
            c.*fields[j] = g_int + 50 + j;
            CHECK(c != a && c != base);
            CHECK(same_shape(a, c) == (i / 2 == j / 2));
            ++n;
        }
        // every other field still decides as it did
        HookPlan d = a;
        d.t0 += 1;
        CHECK(d != a && same_shape(a, d));
        d = a; d.n += 1;
        CHECK(d != a && !same_shape(a, d));
        n += 8;
    }
    return n;
}

int main() {
    // a day with every block on (the blocks there), and one with every block off (no block made yet)
    const Call on = {4, 2, 2, 31 | VDS_PLANE_OUTCOMES, 3, g_byte + 1, g_byte + 3, g_byte + 5, 7u, 2, 5, g_int + 1, true, true, g_int + 3, true,
                     g_ll + 1, g_int + 5, g_int + 7, g_int + 9, g_int + 11, g_int + 13};
    const Call off = {0, 2, 1, 0, 0, nullptr, nullptr, nullptr, 0u, 0, 0, nullptr, false, false, nullptr, false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const std::vector<std::vector<Change>> f = changes();
    for (const Call &base : {on, off}) {
        CHECK(plan_of(base) == plan_of(base) && same_shape(plan_of(base), plan_of(base)));        // equal inputs, equal plans
        { const Call copy = base; compare(base, copy); }
        for (size_t i = 0; i < f.size(); ++i)
            for (const Change &ci : f[i]) {
                Call one = base;
                ci(one);
                compare(base, one); compare(one, base);
                for (size_t j = i + 1; j < f.size(); ++j)
                    for (const Change &cj : f[j]) {
                        Call two = one;
                        cj(two);
                        compare(base, two); compare(two, base); compare(one, two); compare(two, one);
                    }
            }
    }
    // a graph that was dropped matches no call and has no call's shape (n_ticks > 0 wherever a graph is built)
    CHECK(!(HookPlan() == plan_of(on)) && !(HookPlan() == plan_of(off)) && !same_shape(HookPlan(), plan_of(on)) && !same_shape(HookPlan(), plan_of(off)));
    // (the cases are not all on one side of either comparison)
    CHECK(g_equal > 0 && g_equal < g_cases && g_shape > g_equal && g_shape < g_cases);
    const long long nt = check_times(plan_of(ensured(on))) + check_times(plan_of(ensured(off)));
    printf("hook_plan_check: %lld checks of the arrival-minute / counted addresses\n", nt);
    printf("hook_plan_check: %lld comparisons (%lld equal, %lld of one shape)\n", g_cases, g_equal, g_shape);
    puts("hook_plan_check: ok");
    return 0;
}
