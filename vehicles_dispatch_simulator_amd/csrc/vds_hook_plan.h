// What a hooked day (vds_run_hooked, vds_api.hip) is asked to do and what its day graph was built with: host-only values, no HIP
// types (a plain C++17 compiler builds this header: hook_plan_check.cpp), hashed with the host sources.
#pragma once
#include "../../include/vds.h"

#include <tuple>

namespace vds {
// The sticky switches of the vds_run_hooked_* setters, as the caller left them (hook_resolve is their only reader)
struct HookWant {
    int heads_L = 0;                         // vds_run_hooked_idle_heads: > 0 - every slot refreshes the heads block
    int veh_planes = 0;                      // vds_run_hooked_vehicles: every slot refreshes these planes of d_veh (0: none)
    const void *veh_targets = nullptr;       // ... and applies this per-vehicle target tensor behind the policy (null: off)
    const void *veh_arrive = nullptr, *veh_counted = nullptr;          // ... with these minutes / flags per vehicle (vds_run_hooked_vehicles_ex)
    int vout = 0;                            // vds_run_hooked_vehicle_outcomes: every slot refreshes d_vout (0: off)
    int roster = 0;                          // vds_run_hooked_roster: every slot refreshes d_roster (0: off)
    const void *roster_targets = nullptr;    // ... and applies this target tensor by roster position behind the policy (null: off)
    const void *roster_arrive = nullptr, *roster_counted = nullptr;    // ... with these minutes / flags per position (vds_run_hooked_roster_ex)
    int orders = 0;                          // vds_run_hooked_orders: every slot t refreshes range (t, t) of d_orders (0: off)
};

// Everything a hooked-day graph depends on, resolved for one call (hook_resolve): the key of the cached executable graph, and what
// hook_observe / hook_dispatch emit a slot from.  A default-constructed plan matches no call (n == 0).
struct HookPlan {
    int t0 = -1, n = 0, G = 1;               // first slot, slots, replica groups
    int planes = 0, K = 0;                   // the caller's observation mask (bit 5: VDS_PLANE_OUTCOMES) and action count
    int heads_L = 0, veh_planes = 0;
    unsigned gen = 0;                        // tables_gen
    const void *stream = nullptr;
    const void *actions = nullptr;
    void *policy = nullptr;
    // the blocks the nodes write: null where the block is off for this call (outc: the block as it stands, the planes bit says on / off)
    const long long *outc = nullptr;
    const int *heads = nullptr, *veh = nullptr, *vout = nullptr, *roster = nullptr, *orders = nullptr;
    // the target tensors: null where off, and where there are no vehicles
    const int *veh_targets = nullptr, *roster_targets = nullptr;
    // their arrival minutes and counted flags: null where off, and where the targets are
    const int *veh_arrive = nullptr, *veh_counted = nullptr, *roster_arrive = nullptr, *roster_counted = nullptr;

    auto tie() const {
        return std::tie(t0, n, G, planes, K, heads_L, veh_planes, gen, stream, actions, policy, outc, heads, veh, vout, roster, orders,
                        veh_targets, roster_targets, veh_arrive, veh_counted, roster_arrive, roster_counted);
    }
    bool operator==(const HookPlan &o) const { return tie() == o.tie(); }
    bool operator!=(const HookPlan &o) const { return !(*this == o); }

    int obs() const { return planes & 31; }
    bool outcomes() const { return (planes & VDS_PLANE_OUTCOMES) != 0; }
    // the dispatch node is the timed kernel (emit_dispatch_vehicles / emit_dispatch_roster choose by these)
    bool veh_timed() const { return veh_arrive != nullptr || veh_counted != nullptr; }
    bool roster_timed() const { return roster_arrive != nullptr || roster_counted != nullptr; }
    // which nodes a slot has: one bit per optional node family, and which kernel a dispatch node runs
    auto on_off() const {
        return std::make_tuple(obs() != 0, outcomes(), heads_L > 0, K > 0, policy != nullptr, veh_planes != 0, veh_targets != nullptr,
                               vout != nullptr, roster != nullptr, roster_targets != nullptr, orders != nullptr, veh_timed(), roster_timed());
    }
};

// the graph built with `built` has the nodes of `now`, in the same order: its kernel parameters can be replaced in place
inline bool same_shape(const HookPlan &built, const HookPlan &now) {
    return built.n == now.n && built.G == now.G && built.on_off() == now.on_off();
}
}  // namespace vds
