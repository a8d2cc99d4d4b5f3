// One sample of a solved trajectory: the evaluation that the post-solve report (Solver::report, solver_program.hpp) reduces and the
// trajectory rollout (uph_rollout_batch, traj_query.hip) writes out row by row.  One definition, so that the two cannot drift apart.
//   getNormSE2Pos / getVel / getAcc of SE2Trajectory (se2traj.hpp:343-361 locatePieceIdx, :106-140 Piece value and derivatives)
//   + the terms of getMaxVxAxAyCurAttSig (alm_traj_opt.h:170-229) and getNonHolError (se2traj.hpp:551-561) at that sample.
#pragma once
#include "terrain_dev.hpp"
#include "uph_common.hpp"

namespace uph {

struct TrajSample {
    double p[2], v[2], a[2];    // position (the trajectory's frame), velocity, acceleration
    double yawn, dyaw;          // normSO2(yaw), yaw rate
    double yaw, ddyaw;          // raw (unwrapped) yaw, yaw acceleration: written only by the YAW2 form (the switch states of uph_replan_upload)
};

// Trajectory of Nxy uniform pieces of Tx (c_xy: 12 coefficients per piece, power k of dim d at 2 k + d) and Nyaw pieces of Ty (c_yaw: 6 per
// piece), sampled at t.  TERMS: out[7] = vx, ax, ay, cur, att (-1 / cos xi), sigma, non-holonomic error, the terrain looked up on `fgrid`
// (the grid descriptor of the trajectory's frame).  YAW2: also the raw yaw and the yaw acceleration (a separate instantiation, so that the report and the
// rollout compile to what they were without it).
template <bool TERMS, bool YAW2 = false>
UPH_HD void trajectorySample(const double* cxy, const double* cyaw, int Nxy, int Nyaw, double Tx, double Ty, double t, const GridDev& fgrid, double gravity,
                             TrajSample& s, double out[7]) {
    // locatePieceIdx (se2traj.hpp:343-361) with uniform durations
    double tl = t; int ix = 0;
    for (; ix < Nxy && tl > Tx; ix++) tl -= Tx;
    if (ix == Nxy) { ix--; tl += Tx; }
    double tw = t; int iw = 0;
    for (; iw < Nyaw && tw > Ty; iw++) tw -= Ty;
    if (iw == Nyaw) { iw--; tw += Ty; }
    double* p = s.p;
    double* v = s.v;
    double* a = s.a;
    for (int dd = 0; dd < 2; dd++) {
        const double* c = cxy + 12 * ix + dd;
        double val = 0, tn = 1.0;
        for (int kk = 0; kk <= 5; kk++) { val += tn * c[kk * 2]; tn *= tl; }
        double dv = 0; tn = 1.0;
        for (int kk = 1; kk <= 5; kk++) { dv += kk * tn * c[kk * 2]; tn *= tl; }
        double da = 0; tn = 1.0;
        for (int kk = 2; kk <= 5; kk++) { da += (kk - 1) * kk * tn * c[kk * 2]; tn *= tl; }
        p[dd] = val; v[dd] = dv; a[dd] = da;
    }
    const double* c = cyaw + 6 * iw;
    double yaw = 0, tn = 1.0;
    for (int kk = 0; kk <= 5; kk++) { yaw += tn * c[kk]; tn *= tw; }
    double dyaw = 0; tn = 1.0;
    for (int kk = 1; kk <= 5; kk++) { dyaw += kk * tn * c[kk]; tn *= tw; }
    const double yawn = normSO2(yaw);
    s.yawn = yawn; s.dyaw = dyaw;
    if (YAW2) {
        double ddyaw = 0; tn = 1.0;
        for (int kk = 2; kk <= 5; kk++) { ddyaw += (kk - 1) * kk * tn * c[kk]; tn *= tw; }
        s.yaw = yaw; s.ddyaw = ddyaw;
    }
    if (!TERMS) return;
    double cy_, sy_;
    sincosFast(yaw, sy_, cy_);
    const double cw = cy_, sw = sy_;
    double tv[7];
    terrainVariables(fgrid, p[0], p[1], yawn, cw, sw, tv, nullptr);
    const double vnorm = sqrt(v[0] * v[0] + v[1] * v[1]);
    const double lon = a[0] * cy_ + a[1] * sy_;
    const double lat = -a[0] * sy_ + a[1] * cy_;
    const double vx = vnorm * tv[0];
    out[0] = vx;
    out[1] = lon * tv[0] + gravity * tv[1];
    out[2] = lat * tv[2] + gravity * tv[3];
    out[3] = (dyaw * tv[5]) / sqrt(vx * vx + delta_sigl);
    out[4] = -1.0 / tv[5];
    out[5] = tv[6];
    out[6] = fabs(v[0] * sy_ + v[1] * (-cy_));
}

// getTotalDuration of that trajectory as Solver::report forms it: running sums of the piece durations, the smaller of the two
UPH_HD double trajTotal(int Nxy, double Tx, int Nyaw, double Ty) {
    double durx = 0.0, dury = 0.0;
    for (int i = 0; i < Nxy; i++) durx += Tx;
    for (int i = 0; i < Nyaw; i++) dury += Ty;
    return durx < dury ? durx : dury;
}

}  // namespace uph
