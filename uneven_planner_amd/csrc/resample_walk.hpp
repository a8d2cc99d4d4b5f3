// The comb walk of PlanManager's initial-guess stage (plan_manager.cpp:62-132) and of the test node's variant (alm_traj_opt.cpp:73-144), written once for
// the two places it runs: the host batch routine (resample_host.cpp, uph_resample_batch) and the device kernel that resamples the paths the search left
// in HBM (unevenhip.hip, uph_plan_upload).  Plain C++ with __host__ __device__ under HIP, so that a g++ build of this header alone reproduces the host stage.
//
// Bit-exactness rule: every product and sum stays a separate IEEE operation.  hipcc contracts `a + t * d` and `dx * dx + dy * dy` into v_fma_f64 by
// default, the x86-64 host build has no FMA to contract into: the walk therefore runs with contraction off (the pragma below), and the device's f64
// sqrt and division are the correctly rounded sequences, so host and device produce the same bits.  The boundary velocities sig_vel * cos / sin of the
// end headings (:94-95) are NOT formed here: the device's cos / sin need not round as the host's libm does, so the caller forms them on the host.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/uneven_hip.h"

#if defined(__HIP__)
#define UPH_WALK_HD __host__ __device__
#else
#define UPH_WALK_HD
#endif

namespace uph {

// the per-problem pitches and literals of the two producers (plan_manager.cpp:100, alm_traj_opt.cpp:106-107, 117-118, 137)
struct WalkSetup {
    bool tm;                    // test node's variant: `if` instead of `while`, position nodes also feed the yaw way-points
    double pitch_xy, pitch_yaw, sig_vel;
};
UPH_WALK_HD inline WalkSetup walkSetup(const uph_manager_params& mp) {
    WalkSetup s;
    s.tm = mp.test_mode != 0;
    s.pitch_xy = s.tm ? 0.3 : mp.piece_len;                                         // alm_traj_opt.cpp:117
    s.pitch_yaw = s.tm ? s.pitch_xy / 2.0 : s.pitch_xy / mp.yaw_piece_times;         // plan_manager.cpp:100 / alm_traj_opt.cpp:118
    s.sig_vel = s.tm ? 0.05 : mp.init_sig_vel;                                       // alm_traj_opt.cpp:106-107
    return s;
}

struct WalkEnd {                // what the walk leaves besides the way-points
    double yaw_first, yaw_last; // unwrapped yaw of the first / last pose (:62-78)
    double len;                 // total path length (:103)
};

// path(k, j) = column j (x, y, yaw) of pose k, 0 <= k < m (m >= 2).  Sink: xy(x, y) per position node, yaw(v) per yaw node, in the order the reference
// appends them; unwrapped(k, v) per pose.
template <class Path, class Sink>
UPH_WALK_HD inline WalkEnd resampleWalk(const WalkSetup& s, const Path& path, int64_t m, Sink& sink) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double PI = 3.14159265358979323846;      // M_PI
    double carried_xy = 0.0, carried_yaw = 0.0;
    double len = 0.0;
    // the unwrapped yaw of pose i+1 depends on the unwrapped yaw of pose i (:62-78); carried along the walk instead of a first pass
    double ya = path(0, 2);
    sink.unwrapped(0, ya);
    WalkEnd e;
    e.yaw_first = ya;
    for (int64_t k = 0; k + 1 < m; k++) {
        double yb = path(k + 1, 2);
        while (yb - ya >= PI / 2) yb -= PI * 2;
        while (yb - ya <= -PI / 2) yb += PI * 2;
        sink.unwrapped(k + 1, yb);
        const double ax = path(k, 0), ay = path(k, 1);
        const double dx = path(k + 1, 0) - ax, dy = path(k + 1, 1) - ay, dw = yb - ya;
        const double seg = std::sqrt(dx * dx + dy * dy);                                  // .head(2).norm() (:103)
        len += seg;
        // one arc-length comb per block: a node every `pitch` metres of accumulated path length (plan_manager.cpp:107, :113); the test node emits
        // at most one per segment and keeps the remainder (alm_traj_opt.cpp:122, 128)
        carried_yaw += seg;
        while (carried_yaw > s.pitch_yaw) {                                               // :109-110 / alm_traj_opt.cpp:122-127
            const double t = 1.0 - (carried_yaw - s.pitch_yaw) / seg;
            sink.yaw(ya + t * dw);
            carried_yaw -= s.pitch_yaw;
            if (s.tm) break;
        }
        carried_xy += seg;
        while (carried_xy > s.pitch_xy) {                                                 // :115-116 / alm_traj_opt.cpp:128-134
            const double t = 1.0 - (carried_xy - s.pitch_xy) / seg;
            sink.xy(ax + t * dx, ay + t * dy);
            if (s.tm) sink.yaw(ya + t * dw);                                              // temp_node.z() joins the yaw way-points (:132)
            carried_xy -= s.pitch_xy;
            if (s.tm) break;
        }
        ya = yb;
    }
    e.yaw_last = ya;
    e.len = len;
    return e;
}

// total_time of the stage: alm_traj_opt.cpp:137 / plan_manager.cpp:122
UPH_WALK_HD inline double walkTotalTime(const WalkSetup& s, const uph_manager_params& mp, double len) {
    return s.tm ? len / mp.test_max_vel * 1.2 : len / mp.mean_vel * mp.init_time_times;
}

}  // namespace uph
