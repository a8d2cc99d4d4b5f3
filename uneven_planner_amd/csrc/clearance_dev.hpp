// The continuous clearance field of a clearance layer (clearance.hip, polarity UPH_CLEAR_TO_OCCUPIED): c(x, y, yaw) in metres and its gradient (dc/dx, dc/dy).
// One function, clearanceField, shared by the evaluator kernel (uph_clearance_field_kernel, clearance.hip) and the clearance term of the solve kernel
// (Solver<.., CLR = true>::sampleCompute, solver_program.hpp), which runs its three steps apart so that the loads fly during the terrain gather.
//
// The rule (include/uneven_hip.h states it in words):
//   yaw slice   iw = floor((yawn - origin[2]) * yaw_inv) on the NORMALISED yaw: the floor statement of the footprint check (footPointCell) and of the terrain
//               lookup (terrain_dev.hpp).  The field is piecewise constant in yaw; it has no yaw gradient, and neither has the term.
//   cell value  d(cell) = res * sqrt(min(D, rmax^2 + 1)): UPH_CLEAR_FAR becomes the first distance beyond the disc, so the truncated field stays continuous
//               and bounded.
//   xy          bilinear between the four nearest cell centres: u = (x - origin[0]) * xy_inv - 0.5 (the grid's own reciprocal, as every lookup), i0 = floor(u),
//               fx = u - i0; the same in y.  The four corner indices (and iw) are clamped to the grid: the border itself enters through the body layer's
//               UPH_FOOT_OUTSIDE bit.
//   gradient    the exact gradient of the bilinear patch.
//   degenerate  a pose that is not finite, or whose index reaches 2^30 in magnitude: value and gradient 0, and no float-to-int conversion is executed
//               (footPointCell's rule).
// Plain C++ and integer address arithmetic: 32-bit offsets from one uniform base pointer (the layer has fewer than 2^31 entries: uph_clearance_field and
// uph_ctx_set_clearance_term refuse a larger one), four independent 16-bit loads, no LDS, no atomics.  Every product and sum is rounded on its own (no
// contraction), so the device, the CPU emulator and the numpy mirror (uneven_planner_amd/clearance.py clearance_field) perform the same operations.
#pragma once
#include "uph_common.hpp"

namespace uph {

// what the field reads of the grid (GridDev) and of the layer
struct ClearGeom {
    double origin[3], xy_inv, yaw_inv, xy_res;
    int nx, ny, nyaw, rmax;
};
// the term's descriptor: it lies behind OptParams in the buffer BatchDev::params_mem points to, and only CLR code reads it
struct ClearTermDev {
    const unsigned short* D;    // [nx][ny][nyaw], the layer's values
    int rmax, pad;
    double d_safe, weight;
};
struct ClearTaps {
    uint32_t off[4];            // entries (ix0, iy0), (ix1, iy0), (ix0, iy1), (ix1, iy1) of slice iw
    double fx, fy;
    bool ok;                    // false: a degenerate pose (off = 0, fx = fy = 0)
};

UPH_HD ClearGeom clearGeom(const GridDev& g, int rmax) {
    ClearGeom q;
    q.origin[0] = g.origin[0]; q.origin[1] = g.origin[1]; q.origin[2] = g.origin[2];
    q.xy_inv = g.xy_inv; q.yaw_inv = g.yaw_inv; q.xy_res = g.xy_res;
    q.nx = g.nx; q.ny = g.ny; q.nyaw = g.nyaw; q.rmax = rmax;
    return q;
}

// step 1: the four entries and the fractions of a pose (yawn: the normalised yaw)
UPH_HD void clearLocate(const ClearGeom& g, double x, double y, double yawn, ClearTaps& t) {
#pragma clang fp contract(off)
    const double LIM = 1073741824.0;        // 2^30
    const double u = (x - g.origin[0]) * g.xy_inv - 0.5, v = (y - g.origin[1]) * g.xy_inv - 0.5;
    const double fu = floor(u), fv = floor(v), fw = floor((yawn - g.origin[2]) * g.yaw_inv);
    // (a NaN or an infinity fails a comparison here: x - x is 0 for finite x alone)
    const bool ok = (x - x) + (y - y) + (yawn - yawn) == 0.0 && fabs(fu) < LIM && fabs(fv) < LIM && fabs(fw) < LIM;
    const int i0 = (int)(ok ? fu : 0.0), j0 = (int)(ok ? fv : 0.0), w = (int)(ok ? fw : 0.0);
    t.ok = ok;
    t.fx = ok ? u - fu : 0.0; t.fy = ok ? v - fv : 0.0;
    const int hx = g.nx - 1, hy = g.ny - 1, hw = g.nyaw - 1;
    const int xa = i0 < 0 ? 0 : (i0 > hx ? hx : i0), xb = i0 + 1 < 0 ? 0 : (i0 + 1 > hx ? hx : i0 + 1);
    const int ya = j0 < 0 ? 0 : (j0 > hy ? hy : j0), yb = j0 + 1 < 0 ? 0 : (j0 + 1 > hy ? hy : j0 + 1);
    const uint32_t iw = (uint32_t)(w < 0 ? 0 : (w > hw ? hw : w));
    const uint32_t ny = (uint32_t)g.ny, nw = (uint32_t)g.nyaw;
    t.off[0] = ((uint32_t)xa * ny + (uint32_t)ya) * nw + iw;
    t.off[1] = ((uint32_t)xb * ny + (uint32_t)ya) * nw + iw;
    t.off[2] = ((uint32_t)xa * ny + (uint32_t)yb) * nw + iw;
    t.off[3] = ((uint32_t)xb * ny + (uint32_t)yb) * nw + iw;
}
// step 2: the four 16-bit loads, independent of one another
UPH_HD void clearLoad(const unsigned short* D, const ClearTaps& t, int d[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
    // (a pointer fetched from memory has lost its address space: back to global, and the byte offset formed in 32 bits -- entries < 2^31 -- so that the
    // load takes the uniform base as it is and one VGPR of offset)
    typedef const __attribute__((address_space(1))) char* base_t;
    typedef const __attribute__((address_space(1))) unsigned short* val_t;
    const base_t base = (base_t)D;
#pragma unroll
    for (int k = 0; k < 4; k++) d[k] = (int)*(val_t)(base + (t.off[k] << 1));
#else
#pragma unroll
    for (int k = 0; k < 4; k++) d[k] = (int)D[t.off[k]];
#endif
}
// step 3: value (metres) and gradient of the bilinear patch
UPH_HD void clearValue(const ClearGeom& g, const ClearTaps& t, const int d[4], double& c, double& gx, double& gy) {
#pragma clang fp contract(off)
    const int lim = g.rmax * g.rmax + 1;
    double m[4];
#pragma unroll
    for (int k = 0; k < 4; k++) m[k] = g.xy_res * sqrt((double)(d[k] < lim ? d[k] : lim));
    const double fx = t.fx, fy = t.fy;
    const double lo = m[0] * (1.0 - fx) + m[1] * fx, hi = m[2] * (1.0 - fx) + m[3] * fx;
    const double cv = lo * (1.0 - fy) + hi * fy;
    const double dx = ((m[1] - m[0]) * (1.0 - fy) + (m[3] - m[2]) * fy) * g.xy_inv;
    const double dy = (hi - lo) * g.xy_inv;
    c = t.ok ? cv : 0.0; gx = t.ok ? dx : 0.0; gy = t.ok ? dy : 0.0;
}

UPH_HD void clearanceField(const ClearGeom& g, const unsigned short* D, double x, double y, double yawn, double& c, double& gx, double& gy) {
    ClearTaps t;
    int d[4];
    clearLocate(g, x, y, yawn, t);
    clearLoad(D, t, d);
    clearValue(g, t, d, c, gx, gy);
}

}  // namespace uph
