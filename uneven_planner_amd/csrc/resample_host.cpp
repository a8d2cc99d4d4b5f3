// libunevenhip.so -- initial-guess producer of the optimiser boundary, batched over paths.
//
// Reference: PlanManager::rcvWpsCallBack after the front-end returns, plan_manager/src/plan_manager.cpp:62-132 -- yaw unwrapping
// (:62-78), boundary states with init_sig_vel along the end headings (:87-95), arc-length insertion of the position / yaw way-points
// by running `while` loops over the path segments (:97-121), total time (:122).  The output arrays are the argument list of
// ALMTrajOpt::optimizeSE2Traj (alm_traj_opt.h:92-98) in the layout uph_problem takes.  Host code: a path has a few hundred poses and
// the walk is sequential; what matters is that a batch of B front-end results becomes the packed arrays of one upload without a
// per-problem round trip through the caller's language.
//
// mp->test_mode: the same stage as the back-end's own test node runs it, ALMTrajOpt::rcvWpsCallBack back_end/src/alm_traj_opt.cpp:73-144 --
// literals instead of the manager parameters (:106-107, 117-118, 137), `if` instead of `while` in both combs (:122, 128: at most one node
// per comb and segment, the remainder carries over), and the position comb also appends its node's interpolated yaw to the yaw way-points
// (:132), after the yaw comb's node of the same segment.
//
// The walk itself is resample_walk.hpp, shared with the device kernel of uph_plan_upload (the same bits on both sides).
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/uneven_hip.h"
#include "resample_walk.hpp"

namespace uph {
void setError(const std::string& s);      // unevenhip.hip
}

namespace {

struct HostPath {         // pose k of one path in the concatenated input
    const double* p;
    double operator()(int64_t k, int j) const { return p[3 * k + j]; }
};
struct HostSink {         // way-points into the caller's arrays (counted beyond the capacity, not written), the unwrapped yaw column
    double *oxy, *oyw, *un;
    int32_t cap_xy, cap_yaw, nxy = 0, nyw = 0;
    void xy(double x, double y) { if (nxy < cap_xy) { oxy[2 * nxy] = x; oxy[2 * nxy + 1] = y; } nxy++; }
    void yaw(double v) { if (nyw < cap_yaw) oyw[nyw] = v; nyw++; }
    void unwrapped(int64_t k, double v) { if (un) un[k] = v; }
};

}  // namespace

extern "C" int uph_resample_batch(const uph_manager_params* mp, int32_t B, const double* paths, const int64_t* offsets, int32_t cap_xy, int32_t cap_yaw,
                                  double* init_xy, double* end_xy, double* init_yaw, double* end_yaw, double* inner_xy, double* inner_yaw,
                                  int32_t* n_inner_xy, int32_t* n_inner_yaw, double* total_time, double* unwrapped) {
    if (!mp || B <= 0 || !paths || !offsets || !init_xy || !end_xy || !init_yaw || !end_yaw || !inner_xy || !inner_yaw || !n_inner_xy || !n_inner_yaw || !total_time ||
        cap_xy < 0 || cap_yaw < 0 || (!mp->test_mode && (!(mp->piece_len > 0.0) || !(mp->yaw_piece_times > 0.0) || !(mp->mean_vel > 0.0))) ||
        (mp->test_mode && !(mp->test_max_vel > 0.0))) {
        uph::setError("uph_resample_batch: bad arguments");
        return UPH_ERR_INVALID;
    }
    const uph::WalkSetup ws = uph::walkSetup(*mp);
    int status = UPH_OK;
    for (int32_t b = 0; b < B; b++) {
        const int64_t o = offsets[b], m = offsets[b + 1] - offsets[b];
        if (m < 2) { uph::setError("uph_resample_batch: a path needs at least two poses"); return UPH_ERR_INVALID; }
        const double* p = paths + 3 * o;
        double* ixy = init_xy + 6 * (size_t)b; double* exy = end_xy + 6 * (size_t)b;
        double* iyw = init_yaw + 3 * (size_t)b; double* eyw = end_yaw + 3 * (size_t)b;
        HostSink sink{inner_xy + 2 * (size_t)cap_xy * b, inner_yaw + (size_t)cap_yaw * b, unwrapped ? unwrapped + o : nullptr, cap_xy, cap_yaw};
        const uph::WalkEnd e = uph::resampleWalk(ws, HostPath{p}, m, sink);
        ixy[0] = p[0]; ixy[1] = p[1]; exy[0] = p[3 * (m - 1)]; exy[1] = p[3 * (m - 1) + 1];      // :87-90, column-major 2x3 {P, V, A}
        iyw[0] = e.yaw_first; iyw[1] = 0.0; iyw[2] = 0.0; eyw[0] = e.yaw_last; eyw[1] = 0.0; eyw[2] = 0.0;    // :91-92
        ixy[2] = ws.sig_vel * std::cos(iyw[0]); ixy[3] = ws.sig_vel * std::sin(iyw[0]);           // :94
        exy[2] = ws.sig_vel * std::cos(eyw[0]); exy[3] = ws.sig_vel * std::sin(eyw[0]);           // :95
        ixy[4] = ixy[5] = exy[4] = exy[5] = 0.0;
        total_time[b] = uph::walkTotalTime(ws, *mp, e.len);
        n_inner_xy[b] = sink.nxy; n_inner_yaw[b] = sink.nyw;
        if (sink.nxy > cap_xy || sink.nyw > cap_yaw) status = UPH_ERR_LIMIT;         // counts are still reported, so the caller can size a second call
    }
    if (status == UPH_ERR_LIMIT) uph::setError("uph_resample_batch: a path produced more way-points than the caller's capacity");
    return status;
}
