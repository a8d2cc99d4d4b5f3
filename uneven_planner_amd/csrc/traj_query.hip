// libunevenhip.so -- the queries on the resident trajectories of an optimiser context: rollout, check, locate / within, the switch / trajectory states and
// separation / extent / conflicts, the same with oriented rectangles, the start delays on a common clock, the footprint swept over the map's occupancy and the
// clearance layer read along the windows (include/uneven_hip.h uph_rollout_*, uph_check_*, uph_locate_batch, uph_within_batch, uph_traj_states, uph_separation_*,
// uph_extent_batch, uph_conflict*, uph_footprint_*, uph_delay*, uph_footprint_delay*, uph_footprint_check_*, uph_clearance_check_*).  Kernels for gfx950 and their host side; the context, its buffers and the solver live in
// unevenhip.hip (uph_ctx.hpp is what the two share).
//
// One skeleton.  Device: the resident batch as a pointer block (ResidentDev), one view of a trajectory (TrajView), one query record per family -- WinQuery: a
// window of the rollout's time table and the end point; ClockQuery: samples t_from + k dt of a clock several vehicles share, for each of the D delays of the
// launch's table (D = 1 and a null table without one) --, lanes striding over the samples (over the delays, in the delay kernels), their accumulators (Span,
// Box, a (value, sample) selection) reduced by wave_dev.hpp's workgroupReduce, thread 0 writes the row.  The footprint check (FootCheckQuery, a WinQuery with a
// shape) is the one window query whose lanes share a sample: a wave walks its samples and strides over each one's box of map columns.  The queries on a pair of vehicles are one family: one
// record (SepQuery; FootQuery adds the two shapes), one argument block (PairArgs), one body (pairBody) over a metric -- discs or oriented rectangles.  Host:
// trajFrame (the frame of a trajectory, for every record and argument block), checkTrajQueries (the refusals every query passes), formWindowQueries / pairQueries /
// fleetCandidates / extentCall (a call shape's refusals in order, its records, its uploads), clockRun (the clock records in launch order), pairRun (the pair
// records of any metric, chunked by the delay table), fleetConflicts (a fleet's candidates through a pair kernel to the conflict list), fleetDelays (the same through a sweep kernel, level by level, to the schedule), twoWidths (256 lanes for the
// head of a sorted launch, one wave for the rest), runQueryLaunch (events, launch, rows back, the wait).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uneven_hip.h"
#include "trajectory_dev.hpp"
#include "uph_ctx.hpp"
#include "wave_dev.hpp"

// ------------------------------------------------------------------------------------------------ device side
struct ResidentDev {            // the resident batch as the query kernels read it (residentDev)
    const TrajDesc* desc;
    const TrajState* state;
    const double* cxy;
    const double* cyaw;
    const double* tt;           // t_q: q additions of dt to 0.0, shared by the batch
};

// One resident trajectory as a kernel samples it.  Everything here is uniform over a workgroup of the rollout, the check and locate / within (indexed by
// blockIdx only: scalar loads).  sample is trajectorySample itself -- the rollout's statements -- so a state equals the rollout row of the same t bit for
// bit; mapX / mapY add the frame's shift as the rollout does.
struct TrajView {
    const double* cx;
    const double* cy;
    int Nxy, Nyaw;
    double Tx, Ty, sx, sy;
    bool framed;                // the batch solves in local frames
    template <bool TERMS, bool YAW2 = false>
    __device__ __forceinline__ void sample(double t, const GridDev& g, double gravity, TrajSample& s, double* tm) const {
        trajectorySample<TERMS, YAW2>(cx, cy, Nxy, Nyaw, Tx, Ty, t, g, gravity, s, tm);
    }
    __device__ __forceinline__ void state(double t, TrajSample& s) const {      // no terrain; with the raw yaw and the yaw acceleration
        double unused[7];
        GridDev none;
        sample<false, true>(t, none, 0.0, s, unused);
    }
    __device__ __forceinline__ double mapX(double x) const { return framed ? x + sx : x; }
    __device__ __forceinline__ double mapY(double y) const { return framed ? y + sy : y; }
};
__device__ __forceinline__ TrajView trajView(const TrajDesc* desc, const TrajState* state, const double* cxy, const double* cyaw, int b, bool framed, const double* shift) {
    const TrajDesc& td = desc[b];
    TrajView r;
    r.cx = cxy + td.off_cxy; r.cy = cyaw + td.off_cyaw; r.Nxy = td.Nxy; r.Nyaw = td.Nyaw;
    r.Tx = state[b].T_xy; r.Ty = state[b].T_yaw;
    r.framed = framed; r.sx = shift[0]; r.sy = shift[1];
    return r;
}
__device__ __forceinline__ TrajView trajView(const ResidentDev& r, int b, bool framed, const double* shift) {
    return trajView(r.desc, r.state, r.cxy, r.cyaw, b, framed, shift);
}

// ---- trajectory rollout (uph_rollout_batch): every sample of the resident trajectories, one lane per sample, one 64-lane workgroup per
// (trajectory, chunk of 64 samples).  Trajectory-uniform data -- descriptor, state (T_xy, T_yaw), launch record, grid descriptor -- is indexed
// by blockIdx only (scalar loads); the coefficients come from L2.  The rows of a chunk are contiguous in the output: each lane writes its row
// to LDS and the workgroup then streams the chunk out with consecutive lanes on consecutive doubles (a lane-per-row store of a 224-byte row
// would touch a different cache line in every lane of every store).
struct RolloutTraj {            // one trajectory of a rollout launch (formed on the host)
    int64_t row0;               // its first row in the launch's output
    int cnt, rows;              // samples of the t += dt loop; rows = cnt (+ 1 with the end point)
    double total;               // getTotalDuration: t of the end point
    double shift[2];            // map coordinate of the trajectory's frame corner (local frames, TrajFrame); unused in the map's own frame
};
struct RolloutArgs {
    ResidentDev r;
    const GridDev* grid_mem;    // per-trajectory (framed) grid descriptors, or nullptr: the map's own frame (the kernel's grid argument)
    const RolloutTraj* traj;    // [trajectories of the launch]
    double* out;                // [rows of the launch][ncol]
    int b0, channels, ncol;
};
constexpr int ROLL_NT = 64;
constexpr int ROLL_MAXCOL = 9 + 7 + 12;

// the pose of one sample from its (x, y, yaw) in LDS: the statements of uph_pose_kernel (map_build.hip) on inputs the compiler cannot see
// through, so that the two kernels contract the same arithmetic the same way (rows equal uph_terrain_pose_query bit for bit)
__device__ __forceinline__ void rolloutPose(const GridDev& g, const double* in, double* o) {
    const double x = in[0], y = in[1], w = in[2];
    Corners c;
    locate(g, x, y, w, c);
    double tv[4];
    terrainValues(g, c, tv);
    terrainPoseFrom(x, y, w, tv, o);
}

__global__ __launch_bounds__(ROLL_NT) void uph_rollout_kernel(GridDev grid, RolloutArgs a) {
    __shared__ double stage[ROLL_NT * ROLL_MAXCOL];
    const RolloutTraj rt = a.traj[blockIdx.x];
    const int q0 = (int)blockIdx.y * ROLL_NT;
    if (q0 >= rt.rows) return;
    const int nq = rt.rows - q0 < ROLL_NT ? rt.rows - q0 : ROLL_NT;
    const int b = a.b0 + (int)blockIdx.x;
    const int ncol = a.ncol;
    const bool framed = a.grid_mem != nullptr;
    const int pcol = ncol - 12;             // first pose column (when selected)
    if ((int)threadIdx.x < nq) {
        const int q = q0 + (int)threadIdx.x;
        const TrajView tr = trajView(a.r, b, framed, rt.shift);
        const GridDev g = framed ? a.grid_mem[b] : grid;
        const double t = q < rt.cnt ? a.r.tt[q] : rt.total;
        TrajSample s;
        double tm[7];
        if (a.channels & UPH_ROLLOUT_TERRAIN) tr.sample<true>(t, g, grid.gravity, s, tm);
        else tr.sample<false>(t, g, grid.gravity, s, tm);
        double* r = stage + threadIdx.x * ncol;
        if (a.channels & UPH_ROLLOUT_STATE) {
            r[0] = t; r[1] = tr.mapX(s.p[0]); r[2] = tr.mapY(s.p[1]); r[3] = s.yawn;
            r[4] = s.v[0]; r[5] = s.v[1]; r[6] = s.a[0]; r[7] = s.a[1]; r[8] = s.dyaw;
            r += 9;
        }
        if (a.channels & UPH_ROLLOUT_TERRAIN) {
#pragma unroll
            for (int k = 0; k < 7; k++) r[k] = tm[k];
            r += 7;
        }
        if (a.channels & UPH_ROLLOUT_POSE) { r[0] = s.p[0]; r[1] = s.p[1]; r[2] = s.yawn; }       // (the pose's input, in the trajectory's frame)
    }
    __syncthreads();
    if ((a.channels & UPH_ROLLOUT_POSE) && (int)threadIdx.x < nq) {
        double* r = stage + threadIdx.x * ncol + pcol;
        double in[3] = {r[0], r[1], r[2]}, o[12];
        if (framed) {
            rolloutPose(a.grid_mem[b], in, o);
            o[9] += rt.shift[0]; o[10] += rt.shift[1];
        } else {
            rolloutPose(grid, in, o);
        }
#pragma unroll
        for (int k = 0; k < 12; k++) r[k] = o[k];
    }
    __syncthreads();
    double* o = a.out + (size_t)(rt.row0 + q0) * ncol;
    for (int i = (int)threadIdx.x; i < nq * ncol; i += ROLL_NT) o[i] = stage[i];
}

// ---- window queries: (trajectory, time window) pairs of the resident batch, one workgroup per query.  Lane l takes samples l, l + NT, ... of the window, each
// sample the rollout's (same time table, same trajectorySample, same grid descriptor).  Every reduction is a selection under a total order (value, then the
// smaller sample index) or an integer sum, so the order in which lanes and waves are combined cannot change a bit.  Query-uniform data -- query record,
// descriptor, T_xy / T_yaw, grid descriptor, limits -- is indexed by blockIdx only (scalar loads).
struct WinQuery {               // one query of a launch (formed on the host, in launch order: formWindowQueries)
    int32_t b, out;             // resident trajectory; row of the output (the caller's query index)
    int32_t q_lo, n_tab;        // the window's first sample in the time table and the number of samples taken from it
    int32_t end_row, pad;       // != 0: the end point (t = total) closes the window
    double total;               // getTotalDuration: t of the end point
    double shift[2];            // as RolloutTraj
};
__device__ __forceinline__ int winCount(const WinQuery& q) { return q.n_tab + (q.end_row ? 1 : 0); }
__device__ __forceinline__ double winTime(const WinQuery& q, const double* tt, int j) { return j < q.n_tab ? tt[q.q_lo + j] : q.total; }     // t of sample j of the window
constexpr int WIN_NONE = 0x7fffffff;    // no sample

// (value, sample) pairs: the larger (LARGER) or the smaller value wins, equal values go to the smaller sample (no NaN reaches here: the callers make it +inf)
template <bool LARGER>
__device__ __forceinline__ void winTake(double& v, int& i, double ov, int oi) {
    const bool o = (LARGER ? ov > v : ov < v) || (ov == v && oi < i);
    v = o ? ov : v; i = o ? oi : i;
}

// The samples of a window that meet a condition: the first, the last, how many.  A lane takes its samples in ascending order; SpanFold folds another lane's.
struct Span {
    int first = WIN_NONE, last = -1, cnt = 0;
    __device__ __forceinline__ void take(int j) { first = first == WIN_NONE ? j : first; last = j; cnt++; }
};
struct SpanFold {
    __device__ __forceinline__ void operator()(int& lo, int& hi, int& c, int ol, int oh, int oc) const { lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi; c += oc; }
};
// The box of the positions that are not NaN, and the number of those that are.  Min and max are exact: no order of taking or folding can show.
struct Box {
    double x0 = __builtin_huge_val(), x1 = -__builtin_huge_val(), y0 = __builtin_huge_val(), y1 = -__builtin_huge_val();
    int bad = 0;
    __device__ __forceinline__ void take(double X, double Y) {
        if (X == X && Y == Y) {
            x0 = X < x0 ? X : x0; x1 = X > x1 ? X : x1; y0 = Y < y0 ? Y : y0; y1 = Y > y1 ? Y : y1;
        } else {
            bad++;
        }
    }
};
struct BoxFold {
    __device__ __forceinline__ void operator()(double& x0, double& x1, double& y0, double& y1, int& c, double ox0, double ox1, double oy0, double oy1, int oc) const {
        x0 = ox0 < x0 ? ox0 : x0; x1 = ox1 > x1 ? ox1 : x1; y0 = oy0 < y0 ? oy0 : y0; y1 = oy1 > y1 ? oy1 : y1; c += oc;
    }
};

// ---- check (uph_check_batch): the window reduced against limits on the map as it is now.  A 256-lane workgroup; a lane keeps in registers the first sample with a
// violation and its mask, per term the worst value and its sample, two counters (200 VGPRs at two waves per SIMD, no scratch).
struct CheckOut {               // one row per query
    double first_t;             // NaN: no sample violates
    int32_t first_mask, counts[3];      // samples, violating, occupied
    double worst[7], worst_t[7];
};
struct CheckArgs {
    ResidentDev r;
    const GridDev* grid_mem;    // as RolloutArgs
    const WinQuery* qs;
    const char* occ;            // the map's occupancy layer [nx_hold][ny][nyaw] (uph_frontend_query's)
    CheckOut* out;
    double lim[7];
};
constexpr int CHECK_NT = 256, CHECK_NW = CHECK_NT / 64;
constexpr unsigned long long CHECK_NONE = ~0ull;
// its waves' slots in LDS, in doubles: per term a (double, int), then the first violation, then the two counters
constexpr int CHECK_RED_TERM = wavesBytes<double, int>(CHECK_NW) / 8, CHECK_RED_FIRST = 7 * CHECK_RED_TERM;
constexpr int CHECK_RED_SUMS = CHECK_RED_FIRST + wavesBytes<unsigned long long>(CHECK_NW) / 8, CHECK_RED_END = CHECK_RED_SUMS + wavesBytes<int, int>(CHECK_NW) / 8;

__global__ __launch_bounds__(CHECK_NT, 2) void uph_check_kernel(GridDev grid, CheckArgs a) {
    __shared__ double s_red[CHECK_RED_END];
    const WinQuery cq = a.qs[blockIdx.x];
    const int b = cq.b;
    const TrajView tr = trajView(a.r, b, a.grid_mem != nullptr, cq.shift);
    const GridDev g = tr.framed ? a.grid_mem[b] : grid;
    const int n = winCount(cq);
    // first: (sample << 8) | mask of the first violating sample, so that one unsigned minimum carries both
    unsigned long long first = CHECK_NONE;
    double wv[7];
    int wi[7];
#pragma unroll
    for (int k = 0; k < 7; k++) { wv[k] = -__builtin_huge_val(); wi[k] = WIN_NONE; }
    int nviol = 0, nocc = 0;
    for (int j = (int)threadIdx.x; j < n; j += CHECK_NT) {
        const double t = winTime(cq, a.r.tt, j);
        TrajSample s;
        double tm[7];
        tr.sample<true>(t, g, grid.gravity, s, tm);
        // the sample's values leave trajectorySample as they leave it in the rollout (stored, there): nothing below may be contracted into its arithmetic
        double px = s.p[0], py = s.p[1], w = s.yawn;
        asm volatile("" : "+v"(px), "+v"(py), "+v"(w));
#pragma unroll
        for (int k = 0; k < 7; k++) asm volatile("" : "+v"(tm[k]));
        // isOccupancy at the STATE row's (x, y, yaw), map coordinates, on the map's own grid: the statements of uph_frontend_kernel (map_build.hip)
        const double x = tr.mapX(px), y = tr.mapY(py);
        const int ix = (int)floor((x - grid.origin[0]) * grid.xy_inv), iy = (int)floor((y - grid.origin[1]) * grid.xy_inv), iw = (int)floor((w - grid.origin[2]) * grid.yaw_inv);
        const int ixh = ix - grid.x_off;
        const bool in = ix >= 0 && iy >= 0 && iw >= 0 && ix <= grid.nx - 1 && iy <= grid.ny - 1 && iw <= grid.nyaw - 1 && ixh >= 0 && ixh <= grid.nx_hold - 1;
        const int occ = in ? (int)a.occ[((size_t)ixh * grid.ny + iy) * grid.nyaw + iw] : -1;
        int mask = occ != 0 ? 1 << UPH_CHECK_OCC_BIT : 0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const double v = tm[k], m = k < 4 ? fabs(v) : v;
            if (!(m <= a.lim[k])) mask |= 1 << k;
            const double key = fabs(v) < __builtin_huge_val() ? m : __builtin_huge_val();      // non-finite (NaN included): +inf
            if (key > wv[k]) { wv[k] = key; wi[k] = j; }
        }
        if (mask != 0) {
            nviol++;
            if (first == CHECK_NONE) first = ((unsigned long long)(unsigned)j << 8) | (unsigned)mask;
        }
        nocc += occ != 0 ? 1 : 0;
    }
    const auto worst = [](double& v, int& i, double ov, int oi) { winTake<true>(v, i, ov, oi); };
    const auto least = [](unsigned long long& k, unsigned long long o) { k = o < k ? o : k; };
    const auto sum2 = [](int& x, int& y, int ox, int oy) { x += ox; y += oy; };
#pragma unroll
    for (int k = 0; k < 7; k++) rowReduce(worst, wv[k], wi[k]);
    rowReduce(least, first);
    rowReduce(sum2, nviol, nocc);
#pragma unroll
    for (int k = 0; k < 7; k++) rowLeaders(worst, wv[k], wi[k]);
    rowLeaders(least, first);
    rowLeaders(sum2, nviol, nocc);
    // the waves' slots are disjoint: one barrier for all of them
#pragma unroll
    for (int k = 0; k < 7; k++) wavesPut<CHECK_NW>(s_red + CHECK_RED_TERM * k, wv[k], wi[k]);
    wavesPut<CHECK_NW>(s_red + CHECK_RED_FIRST, first);
    wavesPut<CHECK_NW>(s_red + CHECK_RED_SUMS, nviol, nocc);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 7; k++) wavesFold<CHECK_NW>(worst, s_red + CHECK_RED_TERM * k, wv[k], wi[k]);
    wavesFold<CHECK_NW>(least, s_red + CHECK_RED_FIRST, first);
    if (!wavesFold<CHECK_NW>(sum2, s_red + CHECK_RED_SUMS, nviol, nocc)) return;
    const double nan = __builtin_nan("");
    CheckOut o;
    o.first_t = first == CHECK_NONE ? nan : winTime(cq, a.r.tt, (int)(first >> 8));
    o.first_mask = first == CHECK_NONE ? 0 : (int)(first & 0xff);
    o.counts[0] = n; o.counts[1] = nviol; o.counts[2] = nocc;
    for (int k = 0; k < 7; k++) {
        o.worst[k] = wv[k];
        o.worst_t[k] = wi[k] == WIN_NONE ? nan : winTime(cq, a.r.tt, wi[k]);
    }
    a.out[cq.out] = o;
}

// ---- switch states (uph_replan_upload, uph_traj_states, uph_refine_upload): trajectory b of the resident batch at its clamped time, one lane per query.  The
// sample is the rollout's, so at a rollout row's t the state equals that row bit for bit; the duration is the rollout's too (trajTotal).  Row q: x, y (map
// coordinates), dx, dy, ddx, ddy, normSO2(yaw), dyaw, ddyaw; COLS = TRAJ_STATE_COLS adds the raw yaw as column 9.  The 9-column instantiation is uph_replan_upload's.
template <int COLS>
__global__ __launch_bounds__(64) void uph_switch_state_kernel(const TrajDesc* __restrict__ desc, const TrajState* __restrict__ state, const double* __restrict__ cxy,
                                                              const double* __restrict__ cyaw, const SwitchQuery* __restrict__ qs, int nq, double* __restrict__ out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const SwitchQuery sq = qs[q];
    const TrajView tr = trajView(desc, state, cxy, cyaw, sq.b, sq.framed != 0, sq.shift);
    const double total = trajTotal(tr.Nxy, tr.Tx, tr.Nyaw, tr.Ty);
    const double t = sq.t <= 0.0 ? 0.0 : (sq.t >= total ? total : sq.t);
    TrajSample s;
    tr.state(t, s);
    double* o = out + (size_t)q * COLS;
    o[0] = tr.mapX(s.p[0]); o[1] = tr.mapY(s.p[1]);
    o[2] = s.v[0]; o[3] = s.v[1]; o[4] = s.a[0]; o[5] = s.a[1];
    o[6] = s.yawn; o[7] = s.dyaw; o[8] = s.ddyaw;
    if (COLS > SWITCH_COLS) o[9] = s.yaw;
}

// ---- locate / within (uph_locate_batch, uph_within_batch): geometric reductions over the STATE samples of a window.  No terrain: a sample is two quintics,
// about a tenth of the check's, so a query of the tracking workload (101 samples) gets one wave (NT = 64, no LDS, no barrier) and only windows longer than
// LOC_SHORT samples get the check's 256 lanes; the host splits the sorted launch at that length.  The selection makes the answer the same for either width.
//   locate: the sample nearest to a pose (d2 = ex ex + ey ey with both products rounded, the smaller sample among equals, NaN as +inf), then, uniform
//           work of thread 0, a safeguarded Newton iteration on g(t) = e . v inside the bracket of the neighbouring samples; state and tracking error there.
//   within: first and last sample inside a closed rect, the number of samples inside.
struct LocQuery : WinQuery {
    double p[4];                // locate: pose x, y, yaw (map coordinates);  within: rect x0, x1, y0, y1
};
struct LocateOut {              // one row per query
    double near_t, near_d2;     // coarse stage
    double t, d2;
    double state[TRAJ_STATE_COLS];
    double err[3];              // e_lon, e_lat, e_yaw
    int32_t count, refined;
};
struct WithinOut {
    double enter_t, leave_t;    // NaN: no sample inside
    int32_t counts[2];          // samples, inside
};
struct LocArgs {
    ResidentDev r;
    const LocQuery* qs;
    void* out;                  // LocateOut / WithinOut rows
    int framed, q0;             // the batch solves in local frames (add shift, as the rollout does); first query of this launch
};
constexpr int LOC_SHORT = 192;  // windows of at most this many samples run on one wave
constexpr int LOC_NEWTON = 8;

// the STATE row at t: position in map coordinates as the rollout and uph_switch_state_kernel form it.  The values leave trajectorySample as they leave it
// there (stored): nothing after this may be contracted into its arithmetic.
__device__ __forceinline__ void locSample(const TrajView& tr, double t, TrajSample& s, double& X, double& Y) {
    tr.state(t, s);
    X = tr.mapX(s.p[0]); Y = tr.mapY(s.p[1]);
    asm volatile("" : "+v"(X), "+v"(Y));
}
// squared distance with both products rounded before the add
__device__ __forceinline__ double locD2(double ex, double ey) {
    double xx = ex * ex, yy = ey * ey;
    asm volatile("" : "+v"(xx), "+v"(yy));
    return xx + yy;
}

template <int NT>
__global__ __launch_bounds__(NT) void uph_locate_kernel(LocArgs a) {
    const LocQuery lq = a.qs[a.q0 + blockIdx.x];
    const TrajView tr = trajView(a.r, lq.b, a.framed != 0, lq.shift);
    const int n = winCount(lq);
    const double x = lq.p[0], y = lq.p[1];
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    double v = inf;
    int i = WIN_NONE;
    for (int j = (int)threadIdx.x; j < n; j += NT) {
        TrajSample s;
        double X, Y;
        locSample(tr, winTime(lq, a.r.tt, j), s, X, Y);
        const double d2 = locD2(X - x, Y - y);
        winTake<false>(v, i, d2 < inf ? d2 : inf, j);       // NaN: +inf
    }
    const auto nearest = [](double& v, int& i, double ov, int oi) { winTake<false>(v, i, ov, oi); };
    if (!workgroupReduce<NT>(nearest, v, i)) return;
    // sample k of the window (NaN outside it: an empty window answers NaN by this path, not by a special one)
    auto tau = [&](int k) { return k < 0 || k >= n ? nan : winTime(lq, a.r.tt, k); };
    LocateOut o;
    o.count = n; o.near_t = tau(i); o.near_d2 = v;
    const double lo = tau(i - 1 > 0 ? i - 1 : 0), hi = tau((i < n - 2 ? i : n - 2) + 1);
    double t = o.near_t, ta = lo, tb = hi;
    TrajSample s, s0;
    double X, Y, X0 = nan, Y0 = nan, d2 = nan;
    for (int it = 0;; it++) {
        locSample(tr, t, s, X, Y);
        const double ex = X - x, ey = Y - y;
        d2 = locD2(ex, ey);
        if (it == 0) { s0 = s; X0 = X; Y0 = Y; }
        if (it == LOC_NEWTON) break;                        // the candidate left by the last iteration
        const double g = ex * s.v[0] + ey * s.v[1];
        const double h = s.v[0] * s.v[0] + s.v[1] * s.v[1] + ex * s.a[0] + ey * s.a[1];
        if (g > 0.0) tb = t;
        else if (g < 0.0) ta = t;
        else if (g == 0.0) break;
        double tn = t - g / h;
        if (!(h > 0.0 && ta <= tn && tn <= tb)) tn = 0.5 * (ta + tb);
        if (tn == t) break;
        t = tn;
    }
    const bool refined = d2 <= v;
    if (!refined) { s = s0; X = X0; Y = Y0; t = o.near_t; d2 = v; }
    o.t = t; o.d2 = d2; o.refined = refined ? 1 : 0;
    o.state[0] = X; o.state[1] = Y; o.state[2] = s.v[0]; o.state[3] = s.v[1]; o.state[4] = s.a[0]; o.state[5] = s.a[1];
    o.state[6] = s.yawn; o.state[7] = s.dyaw; o.state[8] = s.ddyaw; o.state[9] = s.yaw;
    const double rx = x - X, ry = y - Y;
    double sw, cw;
    sincos(s.yaw, &sw, &cw);
    o.err[0] = rx * cw + ry * sw;
    o.err[1] = ry * cw - rx * sw;
    o.err[2] = normSO2(lq.p[2] - s.yaw);
    ((LocateOut*)a.out)[lq.out] = o;
}

template <int NT>
__global__ __launch_bounds__(NT) void uph_within_kernel(LocArgs a) {
    const LocQuery lq = a.qs[a.q0 + blockIdx.x];
    const TrajView tr = trajView(a.r, lq.b, a.framed != 0, lq.shift);
    const int n = winCount(lq);
    const double x0 = lq.p[0], x1 = lq.p[1], y0 = lq.p[2], y1 = lq.p[3];
    Span in;
    for (int j = (int)threadIdx.x; j < n; j += NT) {
        TrajSample s;
        double X, Y;
        locSample(tr, winTime(lq, a.r.tt, j), s, X, Y);
        if (x0 <= X && X <= x1 && y0 <= Y && Y <= y1) in.take(j);       // (a NaN position is not inside)
    }
    if (!workgroupReduce<NT>(SpanFold(), in.first, in.last, in.cnt)) return;
    const double nan = __builtin_nan("");
    WithinOut o;
    o.enter_t = in.cnt == 0 ? nan : winTime(lq, a.r.tt, in.first);
    o.leave_t = in.cnt == 0 ? nan : winTime(lq, a.r.tt, in.last);
    o.counts[0] = n; o.counts[1] = in.cnt;
    ((WithinOut*)a.out)[lq.out] = o;
}

// ---- separation / extent (uph_separation_batch, uph_extent_batch, uph_conflicts_batch; the pair kernels themselves follow the footprint rule below): reductions
// over the positions of resident trajectories on a clock
// that several vehicles share.  Sample k of a query sits at tau_k = t_from + k dt (the product rounded, then the sum: no time table, the clock may stand at
// 1000 s); a vehicle is a trajectory and its start time t0 on that clock, and stands at uph_switch_state_kernel's state of u = tau - t0: at its start before
// it leaves, at its goal after it arrives.  As locate / within: no terrain, no scratch, one wave for K <= LOC_SHORT samples and 256 lanes beyond.
struct ClockTraj {              // one vehicle of a query
    int32_t b, pad;             // resident trajectory (of its side's context)
    double t0;                  // its start on the common clock
    double shift[2];            // as RolloutTraj
};
struct ClockQuery {             // one query of a launch (formed on the host by clockQuery, in launch order: clockRun)
    int32_t out, K;             // row of the launch's output (with a delay table: rows out * D .. out * D + D - 1); samples
    int32_t D, pad;             // delays of the launch's table; 1 without one.  (Ahead of the times: behind them the compiler loads t_from, dt and SepQuery's
                                // R2 a wait later than the rest of the record, and uph_separation_kernel<64> at 101 samples runs 1.7 % longer.)
    double t_from, dt;
};
struct SepQuery : ClockQuery {  // the record of a pair of vehicles
    double R2;                  // a sample is below when its squared distance (d2; footprints: c2) < R2
    ClockTraj a, b;             // with a delay table, b is the one delayed
};
struct ExtQuery : ClockQuery {
    ClockTraj a;
};
struct SepOut {                 // one row per query
    double min_d2, min_t;       // +inf, NaN: no sample
    double first_t, last_t;     // first / last sample below (NaN: none)
    int32_t counts[2];          // samples, below
    static constexpr int NC = 2;        // counts of a row
};
struct ExtOut {
    double box[4];              // xmin, xmax, ymin, ymax over the samples whose position is not NaN
    int32_t counts[2];          // samples, NaN samples
};
struct SweepOut {               // one row per (query, delay)
    double min_d2, min_t;       // as SepOut
    int32_t below, k;           // samples below; the sample of the minimum (WIN_NONE: none)
};
template <class Q, class Out>   // SepQuery -> SepOut, or SweepOut with a delay table; FootQuery -> FootOut, or FootSweepOut with a delay table
struct PairArgs {
    ResidentDev ra, rb;         // the two sides' resident batches (one context: the same)
    const Q* qs;
    Out* out;
    int framed_a, framed_b, q0; // as LocArgs, per side
    const double* delta;        // [D] the launch's delay table; nullptr without one
};
struct ExtArgs {
    ResidentDev r;
    const ExtQuery* qs;
    ExtOut* out;
    int framed, q0;
    const double* delta;        // as PairArgs
};

// tau_k with the product rounded before the add
__device__ __forceinline__ double clockTau(const ClockQuery& q, int k) {
    double p = (double)k * q.dt;
    asm volatile("" : "+v"(p));
    return q.t_from + p;
}
struct ClockView {              // one vehicle as a kernel samples it (query-uniform)
    TrajView tr;
    double t0, total;
};
__device__ __forceinline__ ClockView clockView(const ResidentDev& r, const ClockTraj& c, bool framed) {
    ClockView v;
    v.tr = trajView(r, c.b, framed, c.shift);
    v.t0 = c.t0;
    v.total = trajTotal(v.tr.Nxy, v.tr.Tx, v.tr.Nyaw, v.tr.Ty);
    return v;
}
// the vehicle's position at tau: uph_switch_state_kernel's clamp of its own time, then the STATE row's x, y there; YAW: its pose, with the raw yaw of the same state
// (uph_traj_states' column 9) in *psi
template <bool YAW = false>
__device__ __forceinline__ void clockSample(const ClockView& v, double tau, double& X, double& Y, double* psi = nullptr) {
    const double u = tau - v.t0;
    const double t = u <= 0.0 ? 0.0 : (u >= v.total ? v.total : u);
    TrajSample s;
    locSample(v.tr, t, s, X, Y);
    if constexpr (YAW) {
        *psi = s.yaw;
        asm volatile("" : "+v"(*psi));
    }
}

// the workgroup's box from its lanes', and the query's row (both extent kernels end here)
template <int NT>
__device__ __forceinline__ void extentRow(const ExtArgs& a, const ExtQuery& eq, Box& box) {
    if (!workgroupReduce<NT>(BoxFold(), box.x0, box.x1, box.y0, box.y1, box.bad)) return;
    ExtOut o;
    o.box[0] = box.x0; o.box[1] = box.x1; o.box[2] = box.y0; o.box[3] = box.y1;
    o.counts[0] = eq.K; o.counts[1] = box.bad;
    a.out[eq.out] = o;
}

template <int NT>
__global__ __launch_bounds__(NT) void uph_extent_kernel(ExtArgs a) {
    const ExtQuery eq = a.qs[a.q0 + blockIdx.x];
    const ClockView va = clockView(a.r, eq.a, a.framed != 0);
    Box box;
    for (int j = (int)threadIdx.x; j < eq.K; j += NT) {
        double X, Y;
        clockSample(va, clockTau(eq, j), X, Y);
        box.take(X, Y);
    }
    extentRow<NT>(a, eq, box);
}

// ---- footprints (uph_footprint_separation_batch, uph_footprint_conflicts_batch): the separation query with the vehicles as oriented rectangles.  A sample also
// takes the raw yaw of the two states it evaluates anyway, and the pair metric is the rule of include/uneven_hip.h: four separating axes, then the eight corner
// distances.  Every product and sum of the rule is rounded on its own (fp contract off in footClearance), so the two widths and any split of the samples over lanes
// compute the same bits.  No terrain, no scratch.
struct FootShape {              // query-uniform, formed on the host (footShape)
    double hl, o, w;            // half length (front + rear) / 2, the centre's offset along the heading (front - rear) / 2, half width
};
struct FootQuery : SepQuery {   // R2 = M2: a sample is below when it overlaps or c2 < M2
    FootShape sa, sb;
};
struct FootOut : SepOut {       // min_d2 is min_c2; counts: samples, below, and behind them
    int32_t over, pad;          // overlapping
    static constexpr int NC = 3;
};
static_assert(sizeof(SepOut) == 40 && sizeof(FootOut) == 48, "4 doubles, then counts[3] contiguous");

// one corner of a rectangle (centre Cx, Cy; hx, hy = hl u; wx, wy = w v) against the other rectangle (centre Ox, Oy; heading co, so; half sizes hlo, wo)
__device__ __forceinline__ double footCorner(double px, double py, double Ox, double Oy, double co, double so, double hlo, double wo) {
#pragma clang fp contract(off)
    const double e0 = px - Ox, e1 = py - Oy;
    const double lx = fabs(e0 * co + e1 * so) - hlo, ly = fabs(e0 * (-so) + e1 * co) - wo;
    const double ex = lx > 0.0 ? lx : 0.0, ey = ly > 0.0 ? ly : 0.0;
    return ex * ex + ey * ey;
}
__device__ __forceinline__ double footCorners(double Cx, double Cy, double c, double s, const FootShape& R, double Ox, double Oy, double co, double so, const FootShape& O) {
#pragma clang fp contract(off)
    const double hx = R.hl * c, hy = R.hl * s, wx = R.w * (-s), wy = R.w * c;
    double m = __builtin_huge_val();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double sx = (k & 2) ? -1.0 : 1.0, sy = (k & 1) ? -1.0 : 1.0;
        const double d2 = footCorner((Cx + sx * hx) + sy * wx, (Cy + sx * hy) + sy * wy, Ox, Oy, co, so, O.hl, O.w);
        m = d2 < m ? d2 : m;
    }
    return m;
}
// The rule in two parts, so that a kernel that meets one vehicle's pose many times (uph_footprint_sweep_kernel) takes its sine and cosine once.  The front, per
// vehicle: whether its pose is finite (footFinite) and c, s of its heading (sincosFast); footPose is the two for one vehicle.  The core: c2 and whether the
// rectangles overlap, from the two points, the two headings' c, s and `finite` (both fronts'); a pose that is not finite: NaN, not overlapping.  footClearance
// is the front of both vehicles and the core.
__device__ __forceinline__ bool footFinite(double X, double Y, double psi, bool so_far = true) {     // (one chain of && over both vehicles, in footClearance)
    const double inf = __builtin_huge_val();
    return so_far && fabs(X) < inf && fabs(Y) < inf && fabs(psi) < inf;
}
__device__ __forceinline__ bool footPose(double X, double Y, double psi, double& c, double& s) {
    const bool finite = footFinite(X, Y, psi);
    sincosFast(psi, s, c);
    return finite;
}
__device__ __forceinline__ void footCore(const FootShape& A, const FootShape& B, double Xa, double Ya, double ca, double sa, double Xb, double Yb, double cb, double sb,
                                         bool finite, double& c2, bool& over) {
#pragma clang fp contract(off)
    const double Cax = A.o * ca, Cay = A.o * sa;
    const double Cbx = (Xb - Xa) + B.o * cb, Cby = (Yb - Ya) + B.o * sb;
    const double dx = Cbx - Cax, dy = Cby - Cay;
    // the axes' products: n . u and n . v of the axis' own rectangle are c c + s s and exactly 0; across the two, u_a . u_b = v_a . v_b and |u_a . v_b| = |v_a . u_b|
    const double naa = ca * ca + sa * sa, nbb = cb * cb + sb * sb;
    const double uu = fabs(ca * cb + sa * sb), uv = fabs(ca * (-sb) + sa * cb);
    const double g0 = fabs(dx * ca + dy * sa) - (A.hl * naa + (B.hl * uu + B.w * uv));
    const double g1 = fabs(dx * (-sa) + dy * ca) - (A.w * naa + (B.hl * uv + B.w * uu));
    const double g2 = fabs(dx * cb + dy * sb) - ((A.hl * uu + A.w * uv) + B.hl * nbb);
    const double g3 = fabs(dx * (-sb) + dy * cb) - ((A.hl * uv + A.w * uu) + B.w * nbb);
    const double g01 = g0 > g1 ? g0 : g1, g23 = g2 > g3 ? g2 : g3;
    const double g = g01 > g23 ? g01 : g23;
    const double ma = footCorners(Cax, Cay, ca, sa, A, Cbx, Cby, cb, sb, B), mb = footCorners(Cbx, Cby, cb, sb, B, Cax, Cay, ca, sa, A);
    over = finite && g <= 0.0;
    c2 = !finite ? __builtin_nan("") : (over ? 0.0 : (ma < mb ? ma : mb));
}
__device__ __forceinline__ void footClearance(const FootShape& A, const FootShape& B, double Xa, double Ya, double psia, double Xb, double Yb, double psib, double& c2,
                                              bool& over) {
    const bool finite = footFinite(Xb, Yb, psib, footFinite(Xa, Ya, psia));
    double sa, ca, sb, cb;
    sincosFast(psia, sa, ca);
    sincosFast(psib, sb, cb);
    footCore(A, B, Xa, Ya, ca, sa, Xb, Yb, cb, sb, finite, c2, over);
}

// ---- the pair queries (uph_separation_kernel, uph_footprint_kernel): one body over a metric.  A metric names its record and row, says whether it counts
// overlaps, and evaluates one sample: the squared distance m2 of the two vehicles at tau and whether they overlap.  A sample is below when it overlaps or m2 < R2
// (a NaN m2 is not below).
struct DiscMetric {             // points: d2 of the two positions
    typedef SepQuery Query;
    typedef SepOut Out;
    static constexpr bool OVERLAPS = false;
    static __device__ __forceinline__ void sample(const Query&, const ClockView& va, const ClockView& vb, double tau, double& m2, bool& over) {
        double Xa, Ya, Xb, Yb;
        clockSample(va, tau, Xa, Ya);
        clockSample(vb, tau, Xb, Yb);
        m2 = locD2(Xa - Xb, Ya - Yb);
        over = false;
    }
};
struct RectMetric {             // oriented rectangles: footClearance of the two poses
    typedef FootQuery Query;
    typedef FootOut Out;
    static constexpr bool OVERLAPS = true;
    static __device__ __forceinline__ void sample(const Query& q, const ClockView& va, const ClockView& vb, double tau, double& m2, bool& over) {
        double Xa, Ya, Pa, Xb, Yb, Pb;
        clockSample<true>(va, tau, Xa, Ya, &Pa);
        clockSample<true>(vb, tau, Xb, Yb, &Pb);
        footClearance(q.sa, q.sb, Xa, Ya, Pa, Xb, Yb, Pb, m2, over);
    }
};
struct PairFold {               // the (value, sample) selection and the span; with a sixth value, the sum of the overlaps
    __device__ __forceinline__ void operator()(double& v, int& i, int& lo, int& hi, int& c, double ov, int oi, int ol, int oh, int oc) const {
        winTake<false>(v, i, ov, oi);
        SpanFold()(lo, hi, c, ol, oh, oc);
    }
    __device__ __forceinline__ void operator()(double& v, int& i, int& lo, int& hi, int& c, int& no, double ov, int oi, int ol, int oh, int oc, int ono) const {
        (*this)(v, i, lo, hi, c, ov, oi, ol, oh, oc);
        no += ono;
    }
};
template <int NT, class M>
__device__ __forceinline__ void pairBody(const PairArgs<typename M::Query, typename M::Out>& a) {
    const typename M::Query pq = a.qs[a.q0 + blockIdx.x];
    const ClockView va = clockView(a.ra, pq.a, a.framed_a != 0), vb = clockView(a.rb, pq.b, a.framed_b != 0);
    const int n = pq.K;
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    double v = inf;
    int i = WIN_NONE, nover = 0;
    Span below;
    for (int j = (int)threadIdx.x; j < n; j += NT) {
        double m2;
        bool over;
        M::sample(pq, va, vb, clockTau(pq, j), m2, over);
        winTake<false>(v, i, m2 < inf ? m2 : inf, j);       // NaN: +inf
        if (over || m2 < pq.R2) below.take(j);
        nover += over ? 1 : 0;
    }
    bool mine;
    if constexpr (M::OVERLAPS) mine = workgroupReduce<NT>(PairFold(), v, i, below.first, below.last, below.cnt, nover);
    else mine = workgroupReduce<NT>(PairFold(), v, i, below.first, below.last, below.cnt);
    if (!mine) return;
    typename M::Out o;
    o.min_d2 = v;
    o.min_t = i == WIN_NONE ? nan : clockTau(pq, i);
    o.first_t = below.cnt == 0 ? nan : clockTau(pq, below.first);
    o.last_t = below.cnt == 0 ? nan : clockTau(pq, below.last);
    o.counts[0] = n; o.counts[1] = below.cnt;
    if constexpr (M::OVERLAPS) { o.over = nover; o.pad = 0; }
    a.out[pq.out] = o;
}
template <int NT>
__global__ __launch_bounds__(NT) void uph_separation_kernel(PairArgs<SepQuery, SepOut> a) { pairBody<NT, DiscMetric>(a); }
template <int NT>
__global__ __launch_bounds__(NT) void uph_footprint_kernel(PairArgs<FootQuery, FootOut> a) { pairBody<NT, RectMetric>(a); }

// ---- start delays (uph_delay_sweep_batch, uph_delay_extent_batch, uph_delays_batch): the separation / the extent of a query (the same records) for every start
// t0 + delta_j of a table of D delays that all queries of a launch share (formed on the host: the device only adds).  One workgroup per query, lanes own DELAYS, not samples:
// the samples are walked in tiles of DELAY_TILE, ascending inside a lane, so a lane's (d2, k) selection meets the tie rule without a cross-lane step.
//   few delays (D * G <= NT, G the largest such power of two): the G lanes tid = dl * G + g of delay dl take the samples g, g + G, ... of each tile and are
//       folded once, after the last tile, through LDS -- a selection under a total order and integer sums: the split cannot show in the result;
//   many delays (D > NT): P = ceil(D / NT) passes per tile; a lane's rows carry its state from tile to tile (its own loads after its own stores).
constexpr int DELAY_TILE = 128;             // samples of a tile (UPH_DELAY_TILE)
static_assert(DELAY_TILE == UPH_DELAY_TILE, "the tile length the header documents");

struct DelaySplit {
    int G, DL, P;               // lanes per delay, delays per pass, passes
};
template <int NT>
__device__ __forceinline__ DelaySplit delaySplit(int D) {
    DelaySplit s;
    s.G = 1;
    while (2 * s.G * D <= NT) s.G *= 2;
    s.DL = NT / s.G;
    s.P = (D + s.DL - 1) / s.DL;
    return s;
}
// The double loop both kernels run.  A body provides
//   park(k0, m)   the workgroup prepares samples k0 .. k0 + m - 1 of the tile (uniform; may hold barriers),
//   open(j)       this lane begins delay j for the tile,
//   sample(s, k)  sample k = k0 + s of the query under the delay that is open,
//   close(j)      the delay's samples of the tile are done,
//   release()     the tile is done (uniform).
template <class Body>
__device__ __forceinline__ void delayLoop(const ClockQuery& q, const DelaySplit& sp, Body& body) {
    const int dl = (int)threadIdx.x / sp.G, g = (int)threadIdx.x % sp.G;
    for (int k0 = 0; k0 < q.K; k0 += DELAY_TILE) {
        const int m = q.K - k0 < DELAY_TILE ? q.K - k0 : DELAY_TILE;
        body.park(k0, m);
        for (int p = 0; p < sp.P; p++) {
            const int j = p * sp.DL + dl;
            if (j >= q.D) continue;
            body.open(j);
            for (int s = g; s < m; s += sp.G) body.sample(s, k0 + s);
            body.close(j);
        }
        body.release();
    }
}

template <int NT>
struct SweepBody {
    const SepQuery& sq;
    const PairArgs<SepQuery, SweepOut>& a;
    ClockView va, vb;
    double t0_b;
    double* ax;                 // [DELAY_TILE] a's positions of the tile, in LDS
    double* ay;
    bool spill;                 // more than one pass: the state lives in the lane's row between tiles
    double v;
    int i, cnt;
    __device__ __forceinline__ SweepOut* row(int j) const { return a.out + (size_t)sq.out * sq.D + j; }
    __device__ __forceinline__ void put(int j) const {
        SweepOut o;
        o.min_d2 = v; o.min_t = i == WIN_NONE ? __builtin_nan("") : clockTau(sq, i);
        o.below = cnt; o.k = i;
        *row(j) = o;
    }
    __device__ __forceinline__ void park(int k0, int m) {
        for (int s = (int)threadIdx.x; s < m; s += NT) {
            double X, Y;
            clockSample(va, clockTau(sq, k0 + s), X, Y);
            ax[s] = X; ay[s] = Y;
        }
        __syncthreads();
    }
    __device__ __forceinline__ void open(int j) {
        vb.t0 = t0_b + a.delta[j];
        if (spill) { const SweepOut o = *row(j); v = o.min_d2; i = o.k; cnt = o.below; }
    }
    __device__ __forceinline__ void sample(int s, int k) {
        double Xb, Yb;
        clockSample(vb, clockTau(sq, k), Xb, Yb);
        const double d2 = locD2(ax[s] - Xb, ay[s] - Yb);
        winTake<false>(v, i, d2 < __builtin_huge_val() ? d2 : __builtin_huge_val(), k);      // NaN: +inf
        cnt += d2 < sq.R2 ? 1 : 0;                                                                // (a NaN d2 is not below)
    }
    __device__ __forceinline__ void close(int j) { if (spill) put(j); }
    __device__ __forceinline__ void release() { __syncthreads(); }
};

template <int NT>
__global__ __launch_bounds__(NT) void uph_delay_sweep_kernel(PairArgs<SepQuery, SweepOut> a) {
    __shared__ double s_xy[2 * DELAY_TILE];
    __shared__ double s_v[NT];
    __shared__ int s_i[2 * NT];
    const SepQuery sq = a.qs[a.q0 + blockIdx.x];
    const DelaySplit sp = delaySplit<NT>(sq.D);
    SweepBody<NT> body{sq, a, clockView(a.ra, sq.a, a.framed_a != 0), clockView(a.rb, sq.b, a.framed_b != 0), sq.b.t0, s_xy, s_xy + DELAY_TILE, sp.P > 1,
                       __builtin_huge_val(), WIN_NONE, 0};
    const int dl = (int)threadIdx.x / sp.G, g = (int)threadIdx.x % sp.G;
    if (body.spill) for (int j = (int)threadIdx.x; j < sq.D; j += NT) body.put(j);      // (G = 1: lane dl owns rows dl, dl + NT, ...)
    delayLoop(sq, sp, body);
    if (body.spill) return;
    if (sp.G > 1) {             // the lanes of a delay, folded by its first lane
        s_v[threadIdx.x] = body.v; s_i[2 * threadIdx.x] = body.i; s_i[2 * threadIdx.x + 1] = body.cnt;
        __syncthreads();
        if (g == 0)
            for (int o = (int)threadIdx.x + 1; o < (int)threadIdx.x + sp.G; o++) { winTake<false>(body.v, body.i, s_v[o], s_i[2 * o]); body.cnt += s_i[2 * o + 1]; }
    }
    if (g == 0 && dl < sq.D) body.put(dl);
}

// ---- the delay sweep with oriented rectangles (uph_footprint_delay_sweep_batch, uph_footprint_delays_batch): SweepBody with the footprint rule.  Vehicle a does
// not move with the delay, so its pose AND the sine and cosine of its heading are taken once per tile (footPose) and parked: a (delay, sample) pays one pose and
// one sincosFast, b's, where uph_footprint_kernel pays two of each.  The row carries the overlap count next to SweepOut's fields.
struct FootSweepOut {           // one row per (query, delay)
    double min_c2, min_t;       // as FootOut
    int32_t below, k;           // as SweepOut
    int32_t over, pad;          // samples that overlap
};
static_assert(sizeof(SweepOut) == 24 && sizeof(FootSweepOut) == 32, "the rows DELAY_ROWS counts");

template <int NT>
struct FootSweepBody {
    const FootQuery& fq;
    const PairArgs<FootQuery, FootSweepOut>& a;
    ClockView va, vb;
    double t0_b;
    double* pa;                 // [4][DELAY_TILE] a's X, Y, cos, sin of the tile, in LDS; X is NaN where a's pose is not finite
    bool spill;                 // as SweepBody
    double v;
    int i, cnt, nover;
    __device__ __forceinline__ FootSweepOut* row(int j) const { return a.out + (size_t)fq.out * fq.D + j; }
    __device__ __forceinline__ void put(int j) const {
        FootSweepOut o;
        o.min_c2 = v; o.min_t = i == WIN_NONE ? __builtin_nan("") : clockTau(fq, i);
        o.below = cnt; o.k = i; o.over = nover; o.pad = 0;
        *row(j) = o;
    }
    __device__ __forceinline__ void park(int k0, int m) {
        for (int s = (int)threadIdx.x; s < m; s += NT) {
            double X, Y, P, c, sn;
            clockSample<true>(va, clockTau(fq, k0 + s), X, Y, &P);
            const bool finite = footPose(X, Y, P, c, sn);
            pa[s] = finite ? X : __builtin_nan(""); pa[DELAY_TILE + s] = Y; pa[2 * DELAY_TILE + s] = c; pa[3 * DELAY_TILE + s] = sn;
        }
        __syncthreads();
    }
    __device__ __forceinline__ void open(int j) {
        vb.t0 = t0_b + a.delta[j];
        if (spill) { const FootSweepOut o = *row(j); v = o.min_c2; i = o.k; cnt = o.below; nover = o.over; }
    }
    __device__ __forceinline__ void sample(int s, int k) {
        const double inf = __builtin_huge_val();
        double Xb, Yb, Pb, cb, sb, c2;
        bool over;
        clockSample<true>(vb, clockTau(fq, k), Xb, Yb, &Pb);
        const bool fb = footPose(Xb, Yb, Pb, cb, sb);
        const double Xa = pa[s];
        footCore(fq.sa, fq.sb, Xa, pa[DELAY_TILE + s], pa[2 * DELAY_TILE + s], pa[3 * DELAY_TILE + s], Xb, Yb, cb, sb, fabs(Xa) < inf && fb, c2, over);
        winTake<false>(v, i, c2 < inf ? c2 : inf, k);               // NaN: +inf
        cnt += over || c2 < fq.R2 ? 1 : 0;                          // (a NaN c2 is not below)
        nover += over ? 1 : 0;
    }
    __device__ __forceinline__ void close(int j) { if (spill) put(j); }
    __device__ __forceinline__ void release() { __syncthreads(); }
};

template <int NT>
__global__ __launch_bounds__(NT) void uph_footprint_sweep_kernel(PairArgs<FootQuery, FootSweepOut> a) {
    __shared__ double s_pa[4 * DELAY_TILE];
    __shared__ double s_v[NT];
    __shared__ int s_i[3 * NT];
    const FootQuery fq = a.qs[a.q0 + blockIdx.x];
    const DelaySplit sp = delaySplit<NT>(fq.D);
    FootSweepBody<NT> body{fq, a, clockView(a.ra, fq.a, a.framed_a != 0), clockView(a.rb, fq.b, a.framed_b != 0), fq.b.t0, s_pa, sp.P > 1,
                           __builtin_huge_val(), WIN_NONE, 0, 0};
    const int dl = (int)threadIdx.x / sp.G, g = (int)threadIdx.x % sp.G;
    if (body.spill) for (int j = (int)threadIdx.x; j < fq.D; j += NT) body.put(j);      // (G = 1: lane dl owns rows dl, dl + NT, ...)
    delayLoop(fq, sp, body);
    if (body.spill) return;
    if (sp.G > 1) {             // the lanes of a delay, folded by its first lane
        s_v[threadIdx.x] = body.v; s_i[3 * threadIdx.x] = body.i; s_i[3 * threadIdx.x + 1] = body.cnt; s_i[3 * threadIdx.x + 2] = body.nover;
        __syncthreads();
        if (g == 0)
            for (int o = (int)threadIdx.x + 1; o < (int)threadIdx.x + sp.G; o++) {
                winTake<false>(body.v, body.i, s_v[o], s_i[3 * o]);
                body.cnt += s_i[3 * o + 1]; body.nover += s_i[3 * o + 2];
            }
    }
    if (g == 0 && dl < fq.D) body.put(dl);
}

struct DextBody {
    const ExtQuery& eq;
    const ExtArgs& a;
    ClockView va;
    double t0;
    Box box;
    __device__ __forceinline__ void park(int, int) {}
    __device__ __forceinline__ void open(int j) { va.t0 = t0 + a.delta[j]; }
    __device__ __forceinline__ void sample(int, int k) {
        double X, Y;
        clockSample(va, clockTau(eq, k), X, Y);
        box.take(X, Y);
    }
    __device__ __forceinline__ void close(int) {}
    __device__ __forceinline__ void release() {}
};

// the hull over the delays of uph_extent_kernel's boxes: min and max are exact, so neither the split nor the fold can show
template <int NT>
__global__ __launch_bounds__(NT) void uph_delay_extent_kernel(ExtArgs a) {
    const ExtQuery eq = a.qs[a.q0 + blockIdx.x];
    DextBody body{eq, a, clockView(a.r, eq.a, a.framed != 0), eq.a.t0, Box()};
    delayLoop(eq, delaySplit<NT>(eq.D), body);
    extentRow<NT>(a, eq, body.box);
}

// ---- footprint check (uph_footprint_check_batch): the window query of the check with the vehicle as an oriented rectangle swept over the map's occupancy layers.
// The rule is include/uneven_hip.h's: a sample's pose covers the column of its point and every column whose centre lies in the rectangle inflated by the margin;
// a covered column has kinds (XY, YAW, OUTSIDE), a sample is a hit when a kind of a covered column is in `layers`.  One workgroup per query, two stages per chunk of
// NT samples: lane l evaluates the pose of its sample (one trajectory evaluation, one sincosFast, the enumeration box), then each wave walks its up to 64 samples one
// after another -- the sample's values are read from the owning lane (readlane: wave-uniform by construction), the 64 lanes stride over the box's columns along iy,
// so that the byte loads of occ_r2 are consecutive, three ballots give the sample's kinds, and only the first hit sample of a wave pays a wave reduction for its
// smallest hit cell.  What a sample contributes lands in the owning lane's accumulators; the column sums stay in the lanes that counted them.  Everything is an integer
// sum, an OR decided by a ballot or a selection under a total order: neither the launch width nor the lane split can show.  Reads occ / occ_r2 on the map's own grid
// and no terrain cell: local frames enter through mapX / mapY only.
struct FootCheckQuery : WinQuery {
    double hl, o, w;            // footShape's, hl and w inflated by the margin on the host (one rounded add each)
    int32_t layers, pad2;       // UPH_FOOT_* kinds that make a column a hit
};
struct FootCheckOut {           // one row per query
    double first_t, last_t;     // NaN: no hit sample
    unsigned long long cells[2];        // covered columns, hit columns, summed over the window
    int32_t first_mask, first_cell[2], counts[5];       // counts: samples, hit samples, samples with a covered column of kind XY / YAW / OUTSIDE
};
struct FootCheckGrid {          // what the kernel reads of the map's own grid descriptor
    int nx, ny, nyaw, x_off, nx_hold;
    double origin[3], xy_res, xy_inv, yaw_inv;
};
struct FootCheckArgs {
    ResidentDev r;
    const FootCheckQuery* qs;
    FootCheckOut* out;
    const char* occ;            // [nx_hold][ny][nyaw]
    const char* occ_r2;         // [nx_hold][ny]
    FootCheckGrid g;
    int framed, q0;             // as LocArgs
};
constexpr double FOOT_INDEX_MAX = 1073741824.0;         // 2^30: a point's column index at or beyond it does not "fit 31 bits" with the box's pad and extent
constexpr unsigned long long FOOT_NO_CELL = ~0ull;
// (ix, iy) as one key whose unsigned order is the lexicographic order of the signed pair
__device__ __forceinline__ unsigned long long footCellKey(int ix, int iy) {
    return ((unsigned long long)((unsigned)ix ^ 0x80000000u) << 32) | ((unsigned)iy ^ 0x80000000u);
}
// the rectangle's centre and the half extents of its axis-aligned hull, every product and sum rounded on its own
__device__ __forceinline__ void footHull(double X, double Y, double c, double s, double hl, double o, double w, double& Cx, double& Cy, double& ex, double& ey) {
#pragma clang fp contract(off)
    Cx = X + o * c; Cy = Y + o * s;
    ex = hl * fabs(c) + w * fabs(s);
    ey = hl * fabs(s) + w * fabs(c);
}
// floor((C -+ e - origin) * inv) -+ 1, as doubles (no conversion here: the caller converts what it has found to fit)
__device__ __forceinline__ void footBoxAxis(double C, double e, double origin, double inv, double& lo, double& hi) {
#pragma clang fp contract(off)
    lo = floor(((C - e) - origin) * inv) - 1.0;
    hi = floor(((C + e) - origin) * inv) + 1.0;
}
// whether the centre of column (ix, iy) lies in the rectangle: the membership test of the rule, every product and sum rounded on its own
__device__ __forceinline__ bool footCentreIn(const FootCheckGrid& g, int ix, int iy, double Cx, double Cy, double c, double s, double hl, double w) {
#pragma clang fp contract(off)
    const double Px = g.origin[0] + ((double)ix + 0.5) * g.xy_res, Py = g.origin[1] + ((double)iy + 0.5) * g.xy_res;
    const double dx = Px - Cx, dy = Py - Cy;
    return fabs(dx * c + dy * s) <= hl && fabs(dx * (-s) + dy * c) <= w;
}
// the cell (px, py, iw) of a pose's point: check's own floor statements on X, Y and the normalised yaw, kept in double until they are known to fit.  Returns
// whether the pose fits (finite, every index below 2^30 in magnitude; a NaN yawn: false); one that does not converts constants: (0, 0, -1)
__device__ __forceinline__ bool footPointCell(const FootCheckGrid& g, double X, double Y, double psi, double yawn, int& px, int& py, int& iw) {
    const double fpx = floor((X - g.origin[0]) * g.xy_inv), fpy = floor((Y - g.origin[1]) * g.xy_inv), fpw = floor((yawn - g.origin[2]) * g.yaw_inv);
    const bool fits = footFinite(X, Y, psi) && fabs(fpx) < FOOT_INDEX_MAX && fabs(fpy) < FOOT_INDEX_MAX && fabs(fpw) < FOOT_INDEX_MAX;
    px = (int)(fits ? fpx : 0.0); py = (int)(fits ? fpy : 0.0); iw = (int)(fits ? fpw : -1.0);
    return fits;
}

template <int NT>
__global__ __launch_bounds__(NT) void uph_footprint_check_kernel(FootCheckArgs a) {
    const FootCheckQuery fq = a.qs[a.q0 + blockIdx.x];
    const TrajView tr = trajView(a.r, fq.b, a.framed != 0, fq.shift);
    const FootCheckGrid& g = a.g;
    const int n = winCount(fq);
    const int lane = (int)threadIdx.x & 63, wave0 = uni((int)threadIdx.x & ~63);
    const int layers = fq.layers;
    Span hit;
    unsigned long long first = CHECK_NONE, cell = FOOT_NO_CELL, ncov = 0, nhit = 0;
    int nxy = 0, nyw = 0, nout = 0;
    bool had = false;           // this wave has met a hit sample (wave-uniform): a later one cannot be the window's first
    for (int c0 = 0; c0 < n; c0 += NT) {
        // stage 1: the pose of this lane's sample and what the walk needs of it
        const int j = c0 + (int)threadIdx.x;
        double Cx = 0.0, Cy = 0.0, cs = 1.0, sn = 0.0;
        int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1, px = 0, py = 0, iw = -1, ok = 0;
        if (j < n) {
            TrajSample s;
            double X, Y;
            locSample(tr, winTime(fq, a.r.tt, j), s, X, Y);
            double psi = s.yaw, yawn = s.yawn;
            asm volatile("" : "+v"(psi), "+v"(yawn));
            sincosFast(psi, sn, cs);
            double ex, ey, fx0, fx1, fy0, fy1;
            footHull(X, Y, cs, sn, fq.hl, fq.o, fq.w, Cx, Cy, ex, ey);
            footBoxAxis(Cx, ex, g.origin[0], g.xy_inv, fx0, fx1);
            footBoxAxis(Cy, ey, g.origin[1], g.xy_inv, fy0, fy1);
            const bool fits = footPointCell(g, X, Y, psi, yawn, px, py, iw);
            ok = fits ? 1 : 0;
            // a pose that does not fit converts zeros: its box is empty.  One that fits has its box within 2^14 columns of its point (the host's limit): the corners fit too
            bx0 = (int)(fits ? fx0 : 0.0); bx1 = (int)(fits ? fx1 : -1.0); by0 = (int)(fits ? fy0 : 0.0); by1 = (int)(fits ? fy1 : -1.0);
        }
        // stage 2: the wave walks its samples c0 + wave0 + k
        const int left = n - (c0 + wave0), mine = left < 0 ? 0 : (left < 64 ? left : 64);
        for (int k = 0; k < mine; k++) {
            const double uCx = readLane(Cx, k), uCy = readLane(Cy, k), uc = readLane(cs, k), us = readLane(sn, k);
            const int ux0 = readLane(bx0, k), ux1 = readLane(bx1, k), uy0 = readLane(by0, k), uy1 = readLane(by1, k);
            const int upx = readLane(px, k), upy = readLane(py, k), uiw = readLane(iw, k), uok = readLane(ok, k);
            const int nby = uy1 - uy0 + 1, total = (ux1 - ux0 + 1) * nby;      // (an empty box: ux1 - ux0 + 1 = 0)
            const bool w_in = uiw >= 0 && uiw <= g.nyaw - 1;
            int kinds = 0, cov = 0, hits = 0;
            unsigned long long low = FOOT_NO_CELL;
            // column i of the box: (ux0 + i / nby, uy0 + i % nby), stepped by 64 without a division per column
            int rx = nby > 0 ? lane / nby : 0, ry = nby > 0 ? lane - rx * nby : 0;
            const int sx = nby > 0 ? 64 / nby : 0, sy = nby > 0 ? 64 - sx * nby : 0;
            for (int i = lane; i < total; i += 64) {
                const int ix = ux0 + rx, iy = uy0 + ry;
                if ((ix == upx && iy == upy) || footCentreIn(g, ix, iy, uCx, uCy, uc, us, fq.hl, fq.w)) {
                    const int ixh = ix - g.x_off;
                    const bool in = ix >= 0 && iy >= 0 && w_in && ix <= g.nx - 1 && iy <= g.ny - 1 && ixh >= 0 && ixh <= g.nx_hold - 1;       // check's `in`
                    int kind = UPH_FOOT_OUTSIDE;
                    if (in) {
                        const size_t col = (size_t)ixh * g.ny + iy;
                        kind = (a.occ_r2[col] != 0 ? UPH_FOOT_OCC_XY : 0) | (a.occ[col * g.nyaw + uiw] != 0 ? UPH_FOOT_OCC_YAW : 0);
                    }
                    kinds |= kind; cov++;
                    if (kind & layers) {
                        hits++;
                        const unsigned long long key = footCellKey(ix, iy);
                        low = key < low ? key : low;
                    }
                }
                rx += sx; ry += sy;
                if (ry >= nby) { ry -= nby; rx++; }
            }
            ncov += (unsigned long long)cov; nhit += (unsigned long long)hits;
            // the sample's kinds: an OR over the wave, bit by bit (a pose that does not fit covers nothing and is of kind OUTSIDE)
            const int m = (__ballot(kinds & UPH_FOOT_OCC_XY) ? UPH_FOOT_OCC_XY : 0) | (__ballot(kinds & UPH_FOOT_OCC_YAW) ? UPH_FOOT_OCC_YAW : 0) |
                          (__ballot(kinds & UPH_FOOT_OUTSIDE) || !uok ? UPH_FOOT_OUTSIDE : 0);
            const int mask = m & layers;
            unsigned long long lowest = FOOT_NO_CELL;
            if (mask != 0 && !had) {        // (wave-uniform)
                const auto least = [](unsigned long long& x, unsigned long long o) { x = o < x ? o : x; };
                rowReduce(least, low);
                rowLeaders(least, low);
                lowest = low;
                had = true;
            }
            if (lane == k) {
                const int jk = c0 + wave0 + k;
                nxy += m & UPH_FOOT_OCC_XY ? 1 : 0; nyw += m & UPH_FOOT_OCC_YAW ? 1 : 0; nout += m & UPH_FOOT_OUTSIDE ? 1 : 0;
                if (mask != 0) {
                    hit.take(jk);
                    if (first == CHECK_NONE) { first = ((unsigned long long)(unsigned)jk << 8) | (unsigned)mask; cell = lowest; }
                }
            }
        }
    }
    // the first hit sample's key carries its cell along; the rest are sums and the span
    const auto fold = [](unsigned long long& f, unsigned long long& ce, unsigned long long& nc, unsigned long long& nh, int& lo, int& hi, int& c, int& x, int& y, int& o,
                         unsigned long long of, unsigned long long oce, unsigned long long onc, unsigned long long onh, int olo, int ohi, int oc, int ox, int oy, int oo) {
        ce = of < f ? oce : ce; f = of < f ? of : f;
        nc += onc; nh += onh;
        SpanFold()(lo, hi, c, olo, ohi, oc);
        x += ox; y += oy; o += oo;
    };
    if (!workgroupReduce<NT>(fold, first, cell, ncov, nhit, hit.first, hit.last, hit.cnt, nxy, nyw, nout)) return;
    const double nan = __builtin_nan("");
    FootCheckOut o;
    o.first_t = hit.cnt == 0 ? nan : winTime(fq, a.r.tt, hit.first);
    o.last_t = hit.cnt == 0 ? nan : winTime(fq, a.r.tt, hit.last);
    o.cells[0] = ncov; o.cells[1] = nhit;
    o.first_mask = first == CHECK_NONE ? 0 : (int)(first & 0xff);
    o.first_cell[0] = cell == FOOT_NO_CELL ? -1 : (int)((unsigned)(cell >> 32) ^ 0x80000000u);
    o.first_cell[1] = cell == FOOT_NO_CELL ? -1 : (int)((unsigned)cell ^ 0x80000000u);
    o.counts[0] = n; o.counts[1] = hit.cnt; o.counts[2] = nxy; o.counts[3] = nyw; o.counts[4] = nout;
    a.out[fq.out] = o;
}

// ---- clearance check (uph_clearance_check_batch): the window query of the check against a clearance layer (clearance.hip), the squared distance transform of a
// body layer.  One lane per sample: the cell of the sample's point by the footprint check's own statements (footPointCell), one 16-bit load of D there -- 0 for a
// sample outside the grid --, then the fold of (value, sample) for the min, a Span for the samples below the query's threshold and two counts.  The leader forms the
// cell of the min's sample once more, by the same statements.  Reads no terrain cell and no occupancy byte.
struct ClearQuery : WinQuery {
    int32_t below2, pad2;       // a sample is below when its value is smaller
};
struct ClearOut {               // one row per query
    double min_t, first_t, last_t;      // NaN: an empty window / no sample below
    int32_t min_d2, min_cell[3], counts[4];     // -1 and (-1, -1, -1): an empty window; counts: samples, below, outside, far
};
struct ClearCheckArgs {
    ResidentDev r;
    const ClearQuery* qs;
    ClearOut* out;
    const unsigned short* D;    // [nx][ny][nyaw]
    FootCheckGrid g;
    int framed, q0;             // as LocArgs
};
// the value of the sample at t and its cell: D there, or 0 and `in` = false for a sample outside the grid (a degenerate pose included)
__device__ __forceinline__ int clearSample(const ClearCheckArgs& a, const TrajView& tr, double t, int& px, int& py, int& iw, bool& in) {
    TrajSample s;
    double X, Y;
    locSample(tr, t, s, X, Y);
    double psi = s.yaw, yawn = s.yawn;
    asm volatile("" : "+v"(psi), "+v"(yawn));
    const FootCheckGrid& g = a.g;
    const bool fits = footPointCell(g, X, Y, psi, yawn, px, py, iw);
    in = fits && px >= 0 && py >= 0 && iw >= 0 && px <= g.nx - 1 && py <= g.ny - 1 && iw <= g.nyaw - 1;
    return in ? (int)a.D[((size_t)px * g.ny + py) * g.nyaw + iw] : 0;
}

template <int NT>
__global__ __launch_bounds__(NT) void uph_clearance_check_kernel(ClearCheckArgs a) {
    const ClearQuery cq = a.qs[a.q0 + blockIdx.x];
    const TrajView tr = trajView(a.r, cq.b, a.framed != 0, cq.shift);
    const int n = winCount(cq);
    int v = WIN_NONE, i = WIN_NONE, nout = 0, nfar = 0;
    Span below;
    for (int j = (int)threadIdx.x; j < n; j += NT) {
        int px, py, iw;
        bool in;
        const int d = clearSample(a, tr, winTime(cq, a.r.tt, j), px, py, iw, in);
        nout += in ? 0 : 1; nfar += d == UPH_CLEAR_FAR ? 1 : 0;
        if (d < cq.below2) below.take(j);
        if (d < v) { v = d; i = j; }        // (ascending j: the earliest of equal values stays)
    }
    const auto fold = [](int& v, int& i, int& lo, int& hi, int& c, int& no, int& nf, int ov, int oi, int olo, int ohi, int oc, int ono, int onf) {
        const bool o = ov < v || (ov == v && oi < i);
        v = o ? ov : v; i = o ? oi : i;
        SpanFold()(lo, hi, c, olo, ohi, oc);
        no += ono; nf += onf;
    };
    if (!workgroupReduce<NT>(fold, v, i, below.first, below.last, below.cnt, nout, nfar)) return;
    const double nan = __builtin_nan("");
    ClearOut o;
    o.min_d2 = -1; o.min_t = nan;
    o.min_cell[0] = o.min_cell[1] = o.min_cell[2] = -1;
    if (i != WIN_NONE) {
        int px, py, iw;
        bool in;
        o.min_t = winTime(cq, a.r.tt, i);
        o.min_d2 = clearSample(a, tr, o.min_t, px, py, iw, in);
        if (in) { o.min_cell[0] = px; o.min_cell[1] = py; o.min_cell[2] = iw; }
    }
    o.first_t = below.cnt == 0 ? nan : winTime(cq, a.r.tt, below.first);
    o.last_t = below.cnt == 0 ? nan : winTime(cq, a.r.tt, below.last);
    o.counts[0] = n; o.counts[1] = below.cnt; o.counts[2] = nout; o.counts[3] = nfar;
    a.out[cq.out] = o;
}

// ------------------------------------------------------------------------------------------------ host side
static ResidentDev residentDev(uph_ctx* c) {
    ResidentDev r;
    r.desc = c->d_desc.as<TrajDesc>(); r.state = c->d_state.as<TrajState>();
    r.cxy = c->d_cxy.as<double>(); r.cyaw = c->d_cyaw.as<double>();
    r.tt = c->d_roll_tt.as<double>();
    return r;
}
// Trajectory b of c as every record and argument block names its frame: whether the batch solves in local frames (the result), and, where asked for, the map
// coordinate of b's frame corner (0 in the map's own frame).  The one reader of c->frames in this file.
static int trajFrame(const uph_ctx* c, int32_t b = 0, double* shift = nullptr) {
    const bool framed = !c->frames.empty();
    if (shift) for (int d = 0; d < 2; d++) shift[d] = framed ? c->frames[(size_t)b].shift[d] : 0.0;
    return framed ? 1 : 0;
}

// The check every query on resident trajectories passes (uph_traj_states / uph_replan_upload / uph_refine_upload, the window queries, the common-clock queries): no
// asynchronous solve is in flight on c, c holds resident trajectories and every query names one of them at a finite time
int checkTrajQueries(const uph_ctx* c, int32_t n, const int32_t* traj, const double* t, const char* who) {
    if (c->pending) { setError(std::string(who) + ": an asynchronous solve is in flight (uph_batch_wait first)"); return UPH_ERR_INVALID; }
    if (c->B <= 0 || !c->traj_resident) {
        setError(std::string(who) + ": no trajectory is resident (uph_batch_solve / uph_eval_batch after the upload first)"); return UPH_ERR_INVALID;
    }
    for (int32_t q = 0; q < n; q++) {
        const int32_t b = traj[q];
        if (b < 0 || b >= c->B) { setError(std::string(who) + ": query " + std::to_string(q) + " names no trajectory of the resident batch"); return UPH_ERR_INVALID; }
        if (!c->rejected.empty() && c->rejected[(size_t)b]) {
            if (c->is_fleet) { setError(std::string(who) + ": query " + std::to_string(q) + " names an empty slot of the fleet (no trajectory)"); return UPH_ERR_INVALID; }
            setError(std::string(who) + ": query " + std::to_string(q) + " names an UPH_RET_UNSUPPORTED slot (no trajectory)"); return UPH_ERR_INVALID;
        }
        if (!std::isfinite(t[q])) { setError(std::string(who) + ": query " + std::to_string(q) + " has a non-finite time"); return UPH_ERR_INVALID; }
    }
    return UPH_OK;
}

// the states of queries sq on c's resident trajectories into c->d_sw_out [n][cols] (enqueued on c's stream, not waited for)
int launchTrajStates(uph_ctx* c, const std::vector<SwitchQuery>& sq, int cols) {
    const size_t n = sq.size();
    if (c->d_sw_q.ensure(sizeof(SwitchQuery) * n) || c->d_sw_out.ensure(sizeof(double) * cols * n)) return UPH_ERR_HIP;
    HIPCHK(hipMemcpyAsync(c->d_sw_q.p, sq.data(), sizeof(SwitchQuery) * n, hipMemcpyHostToDevice, c->stream));
    const auto kernel = cols == SWITCH_COLS ? uph_switch_state_kernel<SWITCH_COLS> : uph_switch_state_kernel<TRAJ_STATE_COLS>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, c->d_desc.as<TrajDesc>(), c->d_state.as<TrajState>(), c->d_cxy.as<double>(),
                       c->d_cyaw.as<double>(), c->d_sw_q.as<SwitchQuery>(), (int)n, c->d_sw_out.as<double>());
    HIPCHK(hipGetLastError());
    return UPH_OK;
}

SwitchQuery trajQuery(const uph_ctx* c, int32_t b, double t) {
    SwitchQuery r;
    r.b = b; r.t = t;
    r.framed = trajFrame(c, b, r.shift);
    return r;
}

// ---- trajectory rollout (include/uneven_hip.h uph_rollout_*) -------------------------------------------------------------------------------
// Sample times: t_q = the value after q additions of dt to 0.0 -- the running sum of the reference's `for (t = 0; t < total; t += dt)` loops
// (alm_traj_opt.h:182, alm_traj_opt.cpp:1109) and of Solver::report -- built ONCE per call, serially in fp64, up to the longest trajectory and
// shared by the batch; a trajectory's count is the first q with t_q >= total (binary search).  A NaN duration has no samples, as in the loop.
static int rolloutTimes(double dt, double tmax, std::vector<double>& tab) {
    tab.assign(1, 0.0);
    double t = 0.0;
    while (t < tmax && (int64_t)tab.size() <= UPH_ROLLOUT_MAX_SAMPLES) {
        const double tn = t + dt;
        if (!(tn > t)) { setError("uph_rollout: the running sum t += dt stops growing before it reaches the trajectory's duration"); return UPH_ERR_LIMIT; }
        t = tn;
        tab.push_back(t);
    }
    return UPH_OK;
}

struct RolloutSizes {
    std::vector<double> tab;        // t_q
    std::vector<int32_t> cnt;       // samples of the loop per trajectory
    std::vector<double> total;      // durations
    std::vector<int64_t> offs;      // [B + 1] row offsets
};

// durations as Solver::report forms them (trajTotal); skip[b] != 0: no rows
static int rolloutSizes(int B, const int32_t* n_xy, const double* T_xy, const int32_t* n_yaw, const double* T_yaw, const int* skip, double dt, int with_end,
                        RolloutSizes& rs) {
    if (!(dt > 0.0) || !std::isfinite(dt)) { setError("uph_rollout: dt must be positive and finite"); return UPH_ERR_INVALID; }
    rs.cnt.assign(B, 0); rs.total.assign(B, 0.0); rs.offs.assign((size_t)B + 1, 0);
    double tmax = 0.0;
    for (int b = 0; b < B; b++) {
        if (n_xy[b] < 0 || n_yaw[b] < 0) { setError("uph_rollout_sizes: negative piece count"); return UPH_ERR_INVALID; }
        if (skip && skip[b]) continue;
        rs.total[b] = trajTotal(n_xy[b], T_xy[b], n_yaw[b], T_yaw[b]);
        if (rs.total[b] > tmax) tmax = rs.total[b];
    }
    const int r = rolloutTimes(dt, tmax, rs.tab);
    if (r != UPH_OK) return r;
    for (int b = 0; b < B; b++) {
        int64_t rows = 0;
        if (!(skip && skip[b])) {
            const int64_t q = std::lower_bound(rs.tab.begin(), rs.tab.end(), rs.total[b]) - rs.tab.begin();
            if (q >= (int64_t)rs.tab.size()) {
                setError("uph_rollout: trajectory " + std::to_string(b) + " needs more than UPH_ROLLOUT_MAX_SAMPLES samples at this dt");
                return UPH_ERR_LIMIT;
            }
            rs.cnt[b] = (int32_t)q;
            rows = q + (with_end ? 1 : 0);
        }
        rs.offs[b + 1] = rs.offs[b] + rows;
    }
    return UPH_OK;
}

static int rolloutColumns(int channels) {
    return (channels & UPH_ROLLOUT_STATE ? 9 : 0) + (channels & UPH_ROLLOUT_TERRAIN ? 7 : 0) + (channels & UPH_ROLLOUT_POSE ? 12 : 0);
}

// the resident batch of c: checks + sizes
static int rolloutPlanCtx(uph_ctx* c, double dt, int with_end, RolloutSizes& rs, const char* who) {
    if (!c || c->B <= 0) { setError(std::string(who) + ": no batch uploaded"); return UPH_ERR_INVALID; }
    if (c->pending) { setError(std::string(who) + ": an asynchronous solve is in flight (uph_batch_wait first)"); return UPH_ERR_INVALID; }
    if (!c->traj_resident) {
        setError(std::string(who) + ": no trajectory is resident -- the batch was uploaded but not solved or evaluated since (uph_batch_solve / uph_eval_batch first)");
        return UPH_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(uphMapDevice(c->map)));
    const int r = refreshStates(c);
    if (r != UPH_OK) return r;
    const int B = c->B;
    std::vector<int32_t> nx(B), ny(B);
    std::vector<double> tx(B), ty(B);
    for (int b = 0; b < B; b++) { nx[b] = c->desc[b].Nxy; ny[b] = c->desc[b].Nyaw; tx[b] = c->state_host[b].T_xy; ty[b] = c->state_host[b].T_yaw; }
    return rolloutSizes(B, nx.data(), tx.data(), ny.data(), ty.data(), c->rejected.data(), dt, with_end, rs);
}

// enqueue the kernel for trajectories [b0, b1) writing rows offs[b0] .. offs[b1] to out_dev (row offs[b0] first); the time table is resident
static int rolloutLaunch(uph_ctx* c, const GridDev& grid, const RolloutSizes& rs, int channels, int b0, int b1, double* out_dev, std::vector<RolloutTraj>& rec) {
    const int n = b1 - b0;
    if (n <= 0 || rs.offs[b1] == rs.offs[b0]) return UPH_OK;
    rec.assign(n, RolloutTraj());
    int ychunks = 0;
    for (int k = 0; k < n; k++) {
        const int b = b0 + k;
        RolloutTraj& t = rec[k];
        t.row0 = rs.offs[b] - rs.offs[b0];
        t.cnt = rs.cnt[b];
        t.rows = (int)(rs.offs[b + 1] - rs.offs[b]);
        t.total = rs.total[b];
        trajFrame(c, b, t.shift);
        ychunks = std::max(ychunks, (t.rows + ROLL_NT - 1) / ROLL_NT);
    }
    if (c->d_roll_traj.ensure(sizeof(RolloutTraj) * n)) return UPH_ERR_HIP;
    HIPCHK(hipMemcpyAsync(c->d_roll_traj.p, rec.data(), sizeof(RolloutTraj) * n, hipMemcpyHostToDevice, c->stream));
    RolloutArgs a;
    a.r = residentDev(c);
    a.grid_mem = trajFrame(c) ? c->d_gridmem.as<GridDev>() : nullptr;
    a.traj = c->d_roll_traj.as<RolloutTraj>(); a.out = out_dev;
    a.b0 = b0; a.channels = channels; a.ncol = rolloutColumns(channels);
    hipLaunchKernelGGL(uph_rollout_kernel, dim3(n, ychunks), dim3(ROLL_NT), 0, c->stream, grid, a);
    HIPCHK(hipGetLastError());
    return UPH_OK;
}

// common part of the two variants: arguments, sizes, grid descriptors, time table
static int rolloutBegin(uph_ctx* c, double dt, int with_end, int channels, int b0, int b1, const void* out, RolloutSizes& rs, GridDev& grid, const char* who) {
    if (!c || !out || (channels & ~UPH_ROLLOUT_ALL) || !(channels & UPH_ROLLOUT_ALL)) { setError(std::string(who) + ": bad arguments (null pointer or channel mask)"); return UPH_ERR_INVALID; }
    if (b0 < 0 || b1 < b0 || b1 > c->B) { setError(std::string(who) + ": trajectory range [b0, b1) outside the batch"); return UPH_ERR_INVALID; }
    int r = rolloutPlanCtx(c, dt, with_end, rs, who);
    if (r != UPH_OK) return r;
    r = syncGridMem(c, grid);
    if (r != UPH_OK) return r;
    if (c->d_roll_tt.ensure(8 * rs.tab.size())) return UPH_ERR_HIP;
    HIPCHK(hipMemcpyAsync(c->d_roll_tt.p, rs.tab.data(), 8 * rs.tab.size(), hipMemcpyHostToDevice, c->stream));
    return UPH_OK;
}

// the host variant stages chunks of whole trajectories through a device buffer of at most this size (one trajectory at the sample cap: 59 MB)
static const size_t ROLL_STAGE_BYTES = (size_t)256 << 20;

// ---- check (include/uneven_hip.h uph_check_*) ------------------------------------------------------------------------------------------------
// the window [t_from, t_to] in the first cnt entries of the time table (strictly increasing): samples [q_lo, q_hi) have t_from <= t_q and t_q <= t_to
static void checkWindow(const std::vector<double>& tab, int64_t cnt, int with_end, double total, double t_from, double t_to, int32_t& q_lo, int32_t& q_hi,
                        int32_t& end_row) {
    const auto b = tab.begin(), e = tab.begin() + cnt;
    const int64_t lo = std::lower_bound(b, e, t_from) - b;            // the first q with t_from <= t_q
    const int64_t hi = std::upper_bound(b, e, t_to) - b;              // the first q with t_to < t_q
    q_lo = (int32_t)lo; q_hi = (int32_t)(hi < lo ? lo : hi);
    end_row = (with_end && t_from <= total && total <= t_to) ? 1 : 0;
}

// what the window queries share: every refusal (outputs untouched), the caller's own check of each query's row, which also stores it in the record (own(q, record)),
// the windows in the rollout's time table, the query records in launch order -- the longest windows first (as the uploads order the solves by predicted cost: the
// tail of the launch is made of short workgroups), stable -- and the time table and the records on the device (d_roll_tt, d_win_q)
template <class Q, class Own>
static int formWindowQueries(uph_ctx* c, int32_t n, const int32_t* traj, const double* t_from, const double* t_to, double dt, int32_t with_end, const char* who,
                             std::vector<Q>& qs, Own own) {
    if (!(dt > 0.0) || !std::isfinite(dt)) { setError(std::string(who) + ": dt must be positive and finite"); return UPH_ERR_INVALID; }
    int r = checkTrajQueries(c, n, traj, t_from, who);
    if (r != UPH_OK) return r;
    if (t_to) for (int32_t q = 0; q < n; q++) if (std::isnan(t_to[q])) { setError(std::string(who) + ": query " + std::to_string(q) + " has a NaN t_to"); return UPH_ERR_INVALID; }
    qs.assign((size_t)n, Q());
    for (int32_t q = 0; q < n; q++) if ((r = own(q, qs[(size_t)q])) != UPH_OK) return r;
    RolloutSizes rs;
    r = rolloutPlanCtx(c, dt, with_end, rs, who);
    if (r != UPH_OK) return r;
    for (int32_t q = 0; q < n; q++) {
        const int32_t b = traj[q];
        Q& k = qs[(size_t)q];
        int32_t q_hi = 0;
        k.b = b; k.out = q; k.pad = 0;
        checkWindow(rs.tab, rs.cnt[(size_t)b], with_end, rs.total[(size_t)b], t_from[q], t_to ? t_to[q] : __builtin_huge_val(), k.q_lo, q_hi, k.end_row);
        k.n_tab = q_hi - k.q_lo;
        k.total = rs.total[(size_t)b];
        trajFrame(c, b, k.shift);
    }
    std::stable_sort(qs.begin(), qs.end(), [](const Q& x, const Q& y) { return x.n_tab + x.end_row > y.n_tab + y.end_row; });
    if (c->d_roll_tt.ensure(8 * rs.tab.size()) || c->d_win_q.ensure(sizeof(Q) * (size_t)n)) return UPH_ERR_HIP;
    HIPCHK(hipMemcpyAsync(c->d_roll_tt.p, rs.tab.data(), 8 * rs.tab.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_win_q.p, qs.data(), sizeof(Q) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    return UPH_OK;
}

// the launch(es) of a window query between the context's events -- launch() enqueues on the context's stream and returns hipGetLastError() --, the rows of
// d_win_out to the host, the wait (also after a failed launch: nothing of this call stays queued, and the host copies outlive it), the time between the events
template <class Out, class Launch>
static int runQueryLaunch(uph_ctx* c, Launch launch, std::vector<Out>& out, double& ms_out) {
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    const hipError_t le = launch();
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    const hipError_t ce = hipMemcpyAsync(out.data(), c->d_win_out.p, sizeof(Out) * out.size(), hipMemcpyDeviceToHost, c->stream);
    const hipError_t se = hipStreamSynchronize(c->stream);
    HIPCHK(le); HIPCHK(ce); HIPCHK(se);
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_out = ms;
    return UPH_OK;
}

// The launch of records sorted by work (the most first; work(q) of record q) at two widths: 256 lanes for the head of more than LOC_SHORT samples, one wave for
// the rest, the second launch told where it starts (a.q0).  The split is found here; the result is runQueryLaunch's launch().
template <class Work, class Args, class K256, class K64>
static auto twoWidths(uph_ctx* c, size_t n, Work work, Args a, K256 k256, K64 k64) {
    size_t n_long = 0;
    while (n_long < n && work(n_long) > LOC_SHORT) n_long++;
    return [=]() mutable {
        hipError_t le = hipSuccess;
        a.q0 = 0;
        if (n_long > 0) { hipLaunchKernelGGL(k256, dim3((unsigned)n_long), dim3(256), 0, c->stream, a); le = hipGetLastError(); }
        if (n > n_long && le == hipSuccess) { a.q0 = (int)n_long; hipLaunchKernelGGL(k64, dim3((unsigned)(n - n_long)), dim3(64), 0, c->stream, a); le = hipGetLastError(); }
        return le;
    };
}

// locate / within: the records in launch order with the caller's `extra` doubles per query (pose / rect) in each, launched at two widths
template <class Out, class K256, class K64>
static int locRun(uph_ctx* c, int32_t n, const int32_t* traj, const double* t_from, const double* t_to, double dt, int32_t with_end, const double* rows, int extra,
                  const char* who, K256 k256, K64 k64, std::vector<Out>& out) {
    std::vector<LocQuery> qs;
    int r = formWindowQueries(c, n, traj, t_from, t_to, dt, with_end, who, qs, [&](int32_t q, LocQuery& k) {
        for (int d = 0; d < 4; d++) k.p[d] = d < extra ? rows[(size_t)extra * q + d] : 0.0;
        for (int d = 0; d < extra; d++) if (extra == 3 ? !std::isfinite(k.p[d]) : std::isnan(k.p[d])) {
            setError(std::string(who) + ": query " + std::to_string(q) + (extra == 3 ? " has a non-finite pose component" : " has a NaN rect bound")); return (int)UPH_ERR_INVALID;
        }
        return (int)UPH_OK;
    });
    if (r != UPH_OK) return r;
    if (c->d_win_out.ensure(sizeof(Out) * (size_t)n)) return UPH_ERR_HIP;
    LocArgs a;
    a.r = residentDev(c); a.qs = c->d_win_q.as<LocQuery>(); a.out = c->d_win_out.p; a.framed = trajFrame(c); a.q0 = 0;
    out.resize((size_t)n);
    const auto work = [&](size_t q) { return qs[q].n_tab + qs[q].end_row; };
    return runQueryLaunch(c, twoWidths(c, (size_t)n, work, a, k256, k64), out, c->last_locate_ms);
}

// ---- separation / extent / conflicts (include/uneven_hip.h uph_separation_*, uph_extent_batch, uph_conflict*) -----------------------------------------
constexpr int64_t CLOCK_MAX_SAMPLES = (int64_t)1 << 22;     // samples of one query
constexpr size_t CLOCK_CHUNK = (size_t)1 << 16;             // queries of one launch pair: bounds the records and rows on the device (a dense fleet's candidates)

static double clockTauHost(double t_from, int64_t k, double dt) {
#pragma clang fp contract(off)
    const double p = (double)k * dt;
    return t_from + p;
}
// how a refusal names query q of a call (q < 0: the call has one window): formed only when something is refused
static std::string whoQuery(const std::string& who, int32_t q) { return q < 0 ? who : who + ": query " + std::to_string(q); }
// K = the number of k >= 0 with tau_k <= t_to (tau_k does not decrease with k: rounding is monotone); the bounds and dt are finite, dt > 0
static int clockCount(double t_from, double t_to, double dt, int64_t& K, const std::string& who, int32_t q) {
    K = 0;
    if (!(t_from <= t_to)) return UPH_OK;
    if (clockTauHost(t_from, CLOCK_MAX_SAMPLES, dt) <= t_to) { setError(whoQuery(who, q) + ": the window holds more than 2^22 samples at this dt"); return UPH_ERR_LIMIT; }
    int64_t lo = 0, hi = CLOCK_MAX_SAMPLES;                 // tau_lo <= t_to < tau_hi
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (clockTauHost(t_from, mid, dt) <= t_to) lo = mid;
        else hi = mid;
    }
    K = lo + 1;
    return UPH_OK;
}
static int clockWindow(double t_from, double t_to, double dt, int64_t& K, const std::string& who, int32_t q = -1) {
    if (!(dt > 0.0) || !std::isfinite(dt)) { setError(whoQuery(who, q) + ": dt must be positive and finite"); return UPH_ERR_INVALID; }
    if (!std::isfinite(t_from) || !std::isfinite(t_to)) { setError(whoQuery(who, q) + ": a window bound is not finite"); return UPH_ERR_INVALID; }
    return clockCount(t_from, t_to, dt, K, who, q);
}
static ClockTraj clockTraj(const uph_ctx* c, int32_t b, double t0) {
    ClockTraj r;
    r.b = b; r.pad = 0; r.t0 = t0;
    trajFrame(c, b, r.shift);
    return r;
}
// The start delays of a call: delta_j = delay0 + j * step.  The calls without delays pass no table: their records say D = 1 and their kernels get a null pointer.
struct DelayTable {
    double delay0, step;
    int32_t D;
    std::vector<double> delta;
};
static int32_t delayCount(const DelayTable* dl) { return dl ? dl->D : 1; }
// The one former of a clock record's head: everything else zero, D from the call's delay table -- clockWork, and with it the launch width, goes by it
template <class Q>
static Q clockQuery(int64_t K, double t_from, double dt, const DelayTable* dl) {
    Q q{};
    q.K = (int32_t)K; q.t_from = t_from; q.dt = dt; q.D = delayCount(dl);
    return q;
}
// the record of a pair of vehicles, SepQuery or one that extends it: the head and the pair fields (R: the radius, or the margin), the rest zero
template <class Q = SepQuery>
static Q pairQuery(int64_t K, double t_from, double dt, const DelayTable* dl, double R, const ClockTraj& a, const ClockTraj& b) {
    Q q = clockQuery<Q>(K, t_from, dt, dl);
    q.R2 = R * R; q.a = a; q.b = b;
    return q;
}
// the samples a query's workgroup evaluates: what the launch order and the launch width go by
static int64_t clockWork(const ClockQuery& q) { return (int64_t)q.K * q.D; }

// n <= CLOCK_CHUNK queries in the caller's order -> their rows (`per` of them each) in that order: the records in launch order (the most samples first, stable) on
// the device, launched at two widths, the kernels' time added to ms
template <class Q, class Out, class Args>
static int clockRun(uph_ctx* c, Q* qs, size_t n, Args a, void (*k256)(Args), void (*k64)(Args), Out* rows, double& ms, size_t per = 1) {
    for (size_t q = 0; q < n; q++) qs[q].out = (int32_t)q;
    std::stable_sort(qs, qs + n, [](const Q& x, const Q& y) { return clockWork(x) > clockWork(y); });
    if (c->d_win_q.ensure(sizeof(Q) * n) || c->d_win_out.ensure(sizeof(Out) * n * per)) return UPH_ERR_HIP;
    HIPCHK(hipMemcpyAsync(c->d_win_q.p, qs, sizeof(Q) * n, hipMemcpyHostToDevice, c->stream));
    a.qs = c->d_win_q.as<Q>(); a.out = c->d_win_out.as<Out>();
    std::vector<Out> out(n * per);
    double one = 0.0;
    const int r = runQueryLaunch(c, twoWidths(c, n, [&](size_t q) { return clockWork(qs[q]); }, a, k256, k64), out, one);
    if (r != UPH_OK) return r;
    ms += one;
    std::copy(out.begin(), out.end(), rows);
    return UPH_OK;
}

// the pairs (i < j) of n boxes the rule does not drop, sorted by (i, j): a sort by xmin and a sweep.  With the boxes in that order, the pairs of box p end at the
// first q with xmin_q - xmax_p > r_p + r_max: rounding is monotone, so every later q has xmin_q - xmax_p > r_p + r_q too and is dropped by the rule itself.
typedef std::pair<int32_t, int32_t> IdxPair;
static int candidatePairs(int32_t n, const double* box, const double* radius, const char* who, std::vector<IdxPair>& pairs) {
    double rmax = 0.0;
    for (int32_t i = 0; i < n; i++) {
        if (!std::isfinite(radius[i]) || radius[i] < 0.0) { setError(std::string(who) + ": radius " + std::to_string(i) + " is negative or not finite"); return UPH_ERR_INVALID; }
        for (int k = 0; k < 4; k++) if (std::isnan(box[4 * (size_t)i + k])) { setError(std::string(who) + ": box " + std::to_string(i) + " has a NaN bound"); return UPH_ERR_INVALID; }
        rmax = std::max(rmax, radius[i]);
    }
    std::vector<int32_t> ord((size_t)n);
    for (int32_t i = 0; i < n; i++) ord[(size_t)i] = i;
    std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return box[4 * (size_t)x] < box[4 * (size_t)y] || (box[4 * (size_t)x] == box[4 * (size_t)y] && x < y); });
    pairs.clear();
    for (int32_t p = 0; p < n; p++) {
        const int32_t i = ord[(size_t)p];
        const double* bi = box + 4 * (size_t)i;
        const double far = radius[i] + rmax;
        for (int32_t q = p + 1; q < n; q++) {
            const int32_t j = ord[(size_t)q];
            const double* bj = box + 4 * (size_t)j;
            if (bj[0] - bi[1] > far) break;
            const double R = radius[i] + radius[j];
            if (bi[0] - bj[1] > R || bj[0] - bi[1] > R || bi[2] - bj[3] > R || bj[2] - bi[3] > R) continue;
            pairs.push_back(i < j ? IdxPair(i, j) : IdxPair(j, i));
        }
    }
    std::sort(pairs.begin(), pairs.end());
    return UPH_OK;
}

// ---- start delays (include/uneven_hip.h uph_delay_*) -------------------------------------------------------------------------------------------------
constexpr int32_t DELAY_MAX = 4096;                         // delays of one table
constexpr int64_t DELAY_MAX_WORK = (int64_t)1 << 26;        // K * D of one query: a workgroup's serial work is at most that of 16 separation queries of CLOCK_MAX_SAMPLES
constexpr size_t DELAY_ROWS = (size_t)1 << 20;              // sweep rows of one launch pair (24 MB on the device; 32 MB of footprint rows)

static const double* delayDev(uph_ctx* c, const DelayTable* dl) { return dl ? c->d_delay.as<double>() : nullptr; }
// delta by clockTau's rule
static int delayTable(double delay0, double delay_step, int32_t D, std::vector<double>& delta, const std::string& who) {
    if (!(delay_step > 0.0) || !std::isfinite(delay_step)) { setError(who + ": delay_step must be positive and finite"); return UPH_ERR_INVALID; }
    if (!std::isfinite(delay0)) { setError(who + ": delay0 is not finite"); return UPH_ERR_INVALID; }
    if (D < 1) { setError(who + ": D must be at least 1"); return UPH_ERR_INVALID; }
    if (D > DELAY_MAX) { setError(who + ": more than 4096 delays"); return UPH_ERR_LIMIT; }
    delta.resize((size_t)D);
    for (int32_t j = 0; j < D; j++) delta[(size_t)j] = clockTauHost(delay0, j, delay_step);
    return UPH_OK;
}
// the table formed, and every start t0[q] + delta_j finite (delta_j does not decrease with j and rounding is monotone: the two ends decide)
static int delayAdmit(DelayTable* dl, int32_t n, const double* t0, const std::string& who) {
    if (!dl) return UPH_OK;
    const int r = delayTable(dl->delay0, dl->step, dl->D, dl->delta, who);
    if (r != UPH_OK) return r;
    for (int32_t q = 0; q < n; q++)
        if (!std::isfinite(t0[q] + dl->delta.front()) || !std::isfinite(t0[q] + dl->delta.back())) {
            setError(who + ": query " + std::to_string(q) + " has a delayed start that is not finite"); return UPH_ERR_INVALID;
        }
    return UPH_OK;
}
// the number of delays each vehicle may use (nullptr: D for all)
static int delayLimits(const std::string& who, int32_t n, const int32_t* n_delays, int32_t D) {
    if (n_delays) for (int32_t i = 0; i < n; i++)
        if (n_delays[i] < 1 || n_delays[i] > D) { setError(who + ": vehicle " + std::to_string(i) + " has an n_delays outside [1, D]"); return UPH_ERR_INVALID; }
    return UPH_OK;
}
static int delayWork(int64_t K, const DelayTable* dl, const std::string& who, int32_t q = -1) {
    if (K * (int64_t)delayCount(dl) > DELAY_MAX_WORK) { setError(whoQuery(who, q) + ": more than 2^26 samples times delays"); return UPH_ERR_LIMIT; }
    return UPH_OK;
}
static int delayUpload(uph_ctx* c, const DelayTable* dl) {
    if (!dl) return UPH_OK;
    if (c->d_delay.ensure(8 * dl->delta.size())) return UPH_ERR_HIP;
    HIPCHK(hipMemcpyAsync(c->d_delay.p, dl->delta.data(), 8 * dl->delta.size(), hipMemcpyHostToDevice, c->stream));
    return UPH_OK;
}
// the queries of one launch pair: the rows stay below DELAY_ROWS and the records below CLOCK_CHUNK
static size_t delayChunk(int32_t D) { return std::max<size_t>(1, std::min(CLOCK_CHUNK, DELAY_ROWS / (size_t)D)); }

// the pair queries qs (formed by pairQuery; the table, if any, is on ca's device) -> a row per query, or per (query, delay), in the caller's order; qs is left in
// launch order
template <class Q, class Out>
static int pairRun(uph_ctx* ca, uph_ctx* cb, std::vector<Q>& qs, const DelayTable* dl, void (*k256)(PairArgs<Q, Out>), void (*k64)(PairArgs<Q, Out>),
                   std::vector<Out>& rows, double& ms) {
    const size_t D = (size_t)delayCount(dl), chunk = delayChunk((int32_t)D);
    for (const Q& q : qs)               // the rows a workgroup writes and the rows allocated here both go by the table
        if (q.D != (int32_t)D) { setError("pairRun: a record was not formed from this call's delay table"); return UPH_ERR_INVALID; }
    rows.resize(qs.size() * D);
    PairArgs<Q, Out> a{};
    a.ra = residentDev(ca); a.rb = residentDev(cb);
    a.framed_a = trajFrame(ca); a.framed_b = trajFrame(cb);
    a.delta = delayDev(ca, dl);
    for (size_t s = 0; s < qs.size(); s += chunk) {
        const int r = clockRun(ca, qs.data() + s, std::min(chunk, qs.size() - s), a, k256, k64, rows.data() + s * D, ms, D);
        if (r != UPH_OK) return r;
    }
    return UPH_OK;
}
// the extents of n vehicles of c (already checked: checkTrajQueries, the windows' K; c's device is current), over every delay of the table if there is one (already
// uploaded), in launches of at most CLOCK_CHUNK
static int extentRun(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* t_from, const int64_t* K, double dt, const DelayTable* dl,
                     std::vector<ExtOut>& out, double& ms) {
    ExtArgs a{};
    a.r = residentDev(c); a.framed = trajFrame(c); a.delta = delayDev(c, dl);
    const auto k256 = dl ? uph_delay_extent_kernel<256> : uph_extent_kernel<256>, k64 = dl ? uph_delay_extent_kernel<64> : uph_extent_kernel<64>;
    out.resize((size_t)n);
    std::vector<ExtQuery> qs;
    for (size_t s = 0; s < (size_t)n; s += CLOCK_CHUNK) {
        const size_t m = std::min(CLOCK_CHUNK, (size_t)n - s);
        qs.resize(m);
        for (size_t k = 0; k < m; k++) {
            qs[k] = clockQuery<ExtQuery>(K[s + k], t_from[s + k], dt, dl);
            qs[k].a = clockTraj(c, traj[s + k], t0[s + k]);
        }
        const int r = clockRun(c, qs.data(), m, a, k256, k64, out.data() + s, ms);
        if (r != UPH_OK) return r;
    }
    return UPH_OK;
}

// What uph_extent_batch and uph_delay_extent_batch are: the refusals, a window per query, the (swept) extents, the rows to the caller's arrays, the kernels' time
// to the context's `last_ms`
static int extentCall(const std::string& who, uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* t_from, const double* t_to, double dt,
                      DelayTable* dl, double* box, int32_t* counts, double uph_ctx::*last_ms) {
    if (!c || n <= 0 || !traj || !t0 || !t_from || !t_to) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    int r = checkTrajQueries(c, n, traj, t0, who.c_str());
    if (r != UPH_OK || (r = delayAdmit(dl, n, t0, who)) != UPH_OK) return r;
    std::vector<int64_t> K((size_t)n);
    for (int32_t q = 0; q < n; q++)
        if ((r = clockWindow(t_from[q], t_to[q], dt, K[(size_t)q], who, q)) != UPH_OK || (r = delayWork(K[(size_t)q], dl, who, q)) != UPH_OK) return r;
    HIPCHK(hipSetDevice(uphMapDevice(c->map)));
    if ((r = delayUpload(c, dl)) != UPH_OK) return r;
    std::vector<ExtOut> out;
    double ms = 0.0;
    if ((r = extentRun(c, n, traj, t0, t_from, K.data(), dt, dl, out, ms)) != UPH_OK) return r;
    c->*last_ms = ms;
    for (int32_t q = 0; q < n; q++) {
        const ExtOut& o = out[(size_t)q];
        if (box) for (int k = 0; k < 4; k++) box[4 * (size_t)q + k] = o.box[k];
        if (counts) for (int k = 0; k < 2; k++) counts[2 * (size_t)q + k] = o.counts[k];
    }
    return UPH_OK;
}

// What the pair calls (uph_separation_batch, uph_footprint_separation_batch, uph_delay_sweep_batch, uph_footprint_delay_sweep_batch) share: every refusal in their one order, cb defaulting to ca,
// the pair fields of their records (radius: the margin, for footprints), ca's device current with cb's stream drained, the table on it
template <class Q>
static int pairQueries(const std::string& who, uph_ctx* ca, uph_ctx*& cb, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, const double* t0_b,
                       const double* t_from, const double* t_to, double dt, const double* radius, DelayTable* dl, std::vector<Q>& qs) {
    if (!ca || n <= 0 || !traj_a || !traj_b || !t0_a || !t0_b || !t_from || !t_to || !radius) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    if (!cb) cb = ca;
    if (uphMapDevice(ca->map) != uphMapDevice(cb->map)) { setError(who + ": the two contexts are on different devices"); return UPH_ERR_INVALID; }
    int r = checkTrajQueries(ca, n, traj_a, t0_a, who.c_str());
    if (r == UPH_OK) r = checkTrajQueries(cb, n, traj_b, t0_b, who.c_str());
    if (r != UPH_OK || (r = delayAdmit(dl, n, t0_b, who)) != UPH_OK) return r;
    qs.resize((size_t)n);
    for (int32_t q = 0; q < n; q++) {
        if (!std::isfinite(radius[q]) || radius[q] < 0.0) { setError(whoQuery(who, q) + " has a negative or non-finite radius"); return UPH_ERR_INVALID; }
        int64_t K = 0;
        if ((r = clockWindow(t_from[q], t_to[q], dt, K, who, q)) != UPH_OK || (r = delayWork(K, dl, who, q)) != UPH_OK) return r;
        qs[(size_t)q] = pairQuery<Q>(K, t_from[q], dt, dl, radius[q], clockTraj(ca, traj_a[q], t0_a[q]), clockTraj(cb, traj_b[q], t0_b[q]));
    }
    HIPCHK(hipSetDevice(uphMapDevice(ca->map)));
    if (cb != ca) HIPCHK(hipStreamSynchronize(cb->stream));     // what cb's stream still writes of its trajectories is there before the launch on ca's
    return delayUpload(ca, dl);
}

// the rows of a pair call to the caller's arrays, each of which may be null (min: min_d2 / min_c2)
template <class Out>
static void pairRowsOut(const std::vector<Out>& out, double* min, double* min_t, double* first_t, double* last_t, int32_t* counts) {
    for (size_t q = 0; q < out.size(); q++) {
        const Out& o = out[q];
        if (min) min[q] = o.min_d2;
        if (min_t) min_t[q] = o.min_t;
        if (first_t) first_t[q] = o.first_t;
        if (last_t) last_t[q] = o.last_t;
        if (counts) for (int k = 0; k < 2; k++) counts[Out::NC * q + k] = o.counts[k];
        if constexpr (Out::NC == 3) if (counts) counts[3 * q + 2] = o.over;
    }
}

// What the fleet calls (uph_conflicts_batch, uph_footprint_conflicts_batch, uph_delays_batch, uph_footprint_delays_batch) share up to their candidates: every refusal in their one order, the one window's K, the (swept)
// extents on the device, the pairs of vehicles whose boxes the rule does not drop
static int fleetCandidates(const std::string& who, uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* radius, const int32_t* n_delays,
                           double t_from, double t_to, double dt, DelayTable* dl, int64_t& K, std::vector<IdxPair>& cand, double& ms) {
    int r = checkTrajQueries(c, n, traj, t0, who.c_str());
    if (r != UPH_OK) return r;
    for (int32_t i = 0; i < n; i++)
        if (!std::isfinite(radius[i]) || radius[i] < 0.0) { setError(who + ": vehicle " + std::to_string(i) + " has a negative or non-finite radius"); return UPH_ERR_INVALID; }
    if ((r = delayAdmit(dl, n, t0, who)) != UPH_OK) return r;
    if (dl && (r = delayLimits(who, n, n_delays, dl->D)) != UPH_OK) return r;
    if ((r = clockWindow(t_from, t_to, dt, K, who)) != UPH_OK || (r = delayWork(K, dl, who)) != UPH_OK) return r;
    HIPCHK(hipSetDevice(uphMapDevice(c->map)));
    if ((r = delayUpload(c, dl)) != UPH_OK) return r;
    const std::vector<double> tf((size_t)n, t_from);
    const std::vector<int64_t> Ks((size_t)n, K);
    std::vector<ExtOut> ext;
    if ((r = extentRun(c, n, traj, t0, tf.data(), Ks.data(), dt, dl, ext, ms)) != UPH_OK) return r;
    std::vector<double> box(4 * (size_t)n);
    for (int32_t i = 0; i < n; i++) for (int k = 0; k < 4; k++) box[4 * (size_t)i + k] = ext[(size_t)i].box[k];
    return candidatePairs(n, box.data(), radius, who.c_str(), cand);
}

// What the fleet conflict calls are behind their own refusals: fleetCandidates with the broad-phase radii, the pair query of every candidate -- form(K, i, j), its
// record -- a launch pair per CLOCK_CHUNK of them, the conflicts in the candidates' (i, j) order, the first cap of them to the caller's arrays (each may be null), the
// kernels' time to the context's `last_ms`
template <class Q, class Out, class Form>
static int fleetConflicts(const std::string& who, uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* radius, double t_from, double t_to, double dt,
                          Form form, void (*k256)(PairArgs<Q, Out>), void (*k64)(PairArgs<Q, Out>), double uph_ctx::*last_ms, int64_t cap, int32_t* pairs, double* rows,
                          int32_t* below, int64_t* n_conflicts, int64_t* n_candidates) {
    int64_t K = 0;
    std::vector<IdxPair> cand;
    double ms = 0.0;
    int r = fleetCandidates(who, c, n, traj, t0, radius, nullptr, t_from, t_to, dt, nullptr, K, cand, ms);
    if (r != UPH_OK) return r;
    std::vector<IdxPair> hit;
    std::vector<Out> hit_rows, out;
    std::vector<Q> qs;
    for (size_t s = 0; s < cand.size(); s += CLOCK_CHUNK) {
        const size_t m = std::min(CLOCK_CHUNK, cand.size() - s);
        qs.resize(m);
        for (size_t k = 0; k < m; k++) qs[k] = form(K, cand[s + k].first, cand[s + k].second);
        if ((r = pairRun(c, c, qs, nullptr, k256, k64, out, ms)) != UPH_OK) return r;
        for (size_t k = 0; k < m; k++) if (out[k].counts[1] > 0) { hit.push_back(cand[s + k]); hit_rows.push_back(out[k]); }
    }
    c->*last_ms = ms;
    for (size_t k = 0; k < hit.size() && (int64_t)k < cap; k++) {
        const Out& o = hit_rows[k];
        if (pairs) { pairs[2 * k] = hit[k].first; pairs[2 * k + 1] = hit[k].second; }
        if (rows) { rows[4 * k] = o.min_d2; rows[4 * k + 1] = o.min_t; rows[4 * k + 2] = o.first_t; rows[4 * k + 3] = o.last_t; }
        if (below) below[k] = o.counts[1];
    }
    if (n_conflicts) *n_conflicts = (int64_t)hit.size();
    if (n_candidates) *n_candidates = (int64_t)cand.size();
    return UPH_OK;
}
// the getter of a call family's kernel time (`who`: the call's own name)
static int kernelMs(const char* who, const uph_ctx* c, double uph_ctx::*last_ms, double* kernel_ms) {
    if (!c || !kernel_ms) { setError(std::string(who) + ": bad arguments"); return UPH_ERR_INVALID; }
    *kernel_ms = c->*last_ms;
    return UPH_OK;
}

// level of vehicle j among pairs (i < j, already checked): 0 without a smaller partner, else 1 + the largest level of its smaller partners
static void delayLevels(int32_t n, const std::vector<IdxPair>& pairs, std::vector<int32_t>& level) {
    std::vector<IdxPair> by_j(pairs.size());
    for (size_t k = 0; k < pairs.size(); k++) by_j[k] = IdxPair(pairs[k].second, pairs[k].first);
    std::sort(by_j.begin(), by_j.end());
    level.assign((size_t)n, 0);
    for (const IdxPair& p : by_j) level[(size_t)p.first] = std::max(level[(size_t)p.first], level[(size_t)p.second] + 1);     // (the levels of i < j are final)
}

// ---- footprints (include/uneven_hip.h uph_footprint_*): what the calls add to the pair family -- the shapes' refusals, the record's shapes, the broad-phase radii
// the refusals of n shapes [n][3] and (margin != nullptr) n margins, named `what` in the message ("shape", "shape_a", ...)
static int footAdmit(const std::string& who, int32_t n, const double* shape, const char* what, const double* margin) {
    for (int32_t q = 0; q < n; q++) {
        for (int k = 0; k < 3; k++) {
            const double s = shape[3 * (size_t)q + k];
            if (!std::isfinite(s) || s < 0.0) { setError(whoQuery(who, q) + " has a negative or non-finite " + what + " component"); return UPH_ERR_INVALID; }
        }
        if (margin && (!std::isfinite(margin[q]) || margin[q] < 0.0)) { setError(whoQuery(who, q) + " has a negative or non-finite margin"); return UPH_ERR_INVALID; }
    }
    return UPH_OK;
}
static FootShape footShape(const double* s3) {
    FootShape s;
    s.hl = 0.5 * (s3[0] + s3[1]); s.o = 0.5 * (s3[0] - s3[1]); s.w = s3[2];
    return s;
}
// r = (hypot(max(front, rear), half_width) + margin) (1 + 2^-40), each operation rounded (shapes and margins already admitted)
static double footRadius(const double* s3, double margin) {
#pragma clang fp contract(off)
    const double reach = std::hypot(std::max(s3[0], s3[1]), s3[2]) + margin;
    return reach * (1.0 + 0x1p-40);
}
static int footRadii(const std::string& who, int32_t n, const double* shape, const double* margin, std::vector<double>& r) {
    r.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        r[(size_t)i] = footRadius(shape + 3 * (size_t)i, margin[i]);
        if (!std::isfinite(r[(size_t)i])) { setError(whoQuery(who, i) + " has a shape and margin whose radius is not finite"); return UPH_ERR_INVALID; }
    }
    return UPH_OK;
}
// ---- footprint check (include/uneven_hip.h uph_footprint_check_*): the rectangle inflated by the margin, and the bound on the columns of a sample's box
constexpr int64_t FOOT_CHECK_MAX_COLUMNS = (int64_t)1 << 14;
struct FootCheckShape {
    double hl, o, w;            // footShape's hl and w, each + margin (one rounded add)
};
static FootCheckShape footCheckShape(const double* s3, double margin) {
#pragma clang fp contract(off)
    const FootShape f = footShape(s3);
    FootCheckShape s;
    s.hl = f.hl + margin; s.o = f.o; s.w = f.w + margin;
    return s;
}
// cols = side * side, side = floor(2 hypot(hl', w') (1 + 2^-40) / res) + 4: the hull's half extents hl'|c| + w'|s| and hl'|s| + w'|c| are at most hypot(hl', w') to
// the roundings 2^-40 pays for, two floors that far apart differ by at most floor(2 e / res) + 1, and the pad adds a column on either side.  Saturates at 2^62.
static int footCheckColumns(const std::string& who, int32_t q, const FootCheckShape& s, double res, int64_t& cols) {
#pragma clang fp contract(off)
    const double reach = std::hypot(s.hl, s.w) * (1.0 + 0x1p-40);
    if (!std::isfinite(reach)) { setError(whoQuery(who, q) + " has a shape and margin whose reach is not finite"); return UPH_ERR_INVALID; }
    const double side = std::floor(2.0 * reach / res) + 4.0;
    cols = side < 0x1p31 ? (int64_t)side * (int64_t)side : (int64_t)1 << 62;
    return UPH_OK;
}
// What the schedule calls (uph_delays_batch, uph_footprint_delays_batch) are behind their own refusals: fleetCandidates on swept boxes with the broad-phase radii,
// the candidates' levels, a round per level -- the sweep record of every candidate of the level, form(K, dl, h, start_h, i) with h at its effective start, through
// a sweep kernel whose rows carry `below` --, the sequential greedy's choice per vehicle, the kernels' time to the context's last_delay_ms
template <class Q, class Row, class Form>
static int fleetDelays(const std::string& who, uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* radius, const int32_t* n_delays, double t_from,
                       double t_to, double dt, double delay0, double delay_step, int32_t D, Form form, void (*k256)(PairArgs<Q, Row>), void (*k64)(PairArgs<Q, Row>),
                       int32_t* choice, double* start, int32_t* blocker, int64_t* n_candidates, int32_t* n_rounds, int32_t* n_unresolved) {
    DelayTable dl{delay0, delay_step, D};
    const std::vector<double>& delta = dl.delta;
    int64_t K = 0;
    std::vector<IdxPair> cand;
    double ms = 0.0;
    int r = fleetCandidates(who, c, n, traj, t0, radius, n_delays, t_from, t_to, dt, &dl, K, cand, ms);
    if (r != UPH_OK) return r;
    // the candidates' levels on the host
    std::vector<int32_t> level;
    delayLevels(n, cand, level);
    const int32_t rounds = *std::max_element(level.begin(), level.end());
    // a round per level: the vehicles of the level swept against their partners ahead, which are all placed by then
    std::vector<std::vector<size_t>> cand_of((size_t)rounds + 1);       // the candidates of each level (that of the later vehicle), in (h, i) order
    std::vector<std::vector<int32_t>> veh_of((size_t)rounds + 1);
    for (size_t p = 0; p < cand.size(); p++) cand_of[(size_t)level[(size_t)cand[p].second]].push_back(p);
    for (int32_t i = 0; i < n; i++) veh_of[(size_t)level[(size_t)i]].push_back(i);
    std::vector<int32_t> ch((size_t)n, 0), blk((size_t)n, -1);
    std::vector<char> taken((size_t)n * D, 0);      // [i][j]: vehicle i is below a partner ahead at delay j
    std::vector<Q> qs;
    std::vector<Row> rows;
    for (int32_t lv = 1; lv <= rounds; lv++) {
        const std::vector<size_t>& of = cand_of[(size_t)lv];
        qs.resize(of.size());
        for (size_t k = 0; k < of.size(); k++) {
            const int32_t h = cand[of[k]].first, i = cand[of[k]].second;
            qs[k] = form(K, &dl, h, t0[h] + delta[(size_t)std::max(ch[(size_t)h], 0)], i);
        }
        if ((r = pairRun(c, c, qs, &dl, k256, k64, rows, ms)) != UPH_OK) return r;
        for (size_t k = 0; k < of.size(); k++) {        // (h ascending for each vehicle: the first h below at delay 0 is the smallest)
            const int32_t h = cand[of[k]].first, i = cand[of[k]].second;
            for (int32_t j = 0; j < D; j++) if (rows[k * (size_t)D + j].below > 0) taken[(size_t)i * D + j] = 1;
            if (blk[(size_t)i] < 0 && rows[k * (size_t)D].below > 0) blk[(size_t)i] = h;
        }
        for (const int32_t i : veh_of[(size_t)lv]) {
            const int32_t nd = n_delays ? n_delays[i] : D;
            int32_t j = 0;
            while (j < nd && taken[(size_t)i * D + j]) j++;
            ch[(size_t)i] = j < nd ? j : -1;
            if (j < nd) blk[(size_t)i] = -1;
        }
    }
    c->last_delay_ms = ms;
    int32_t unresolved = 0;
    for (int32_t i = 0; i < n; i++) {
        if (choice) choice[i] = ch[(size_t)i];
        if (start) start[i] = t0[i] + delta[(size_t)std::max(ch[(size_t)i], 0)];
        if (blocker) blocker[i] = blk[(size_t)i];
        unresolved += ch[(size_t)i] < 0 ? 1 : 0;
    }
    if (n_candidates) *n_candidates = (int64_t)cand.size();
    if (n_rounds) *n_rounds = rounds;
    if (n_unresolved) *n_unresolved = unresolved;
    return UPH_OK;
}
extern "C" {

int uph_traj_states(uph_ctx* c, int32_t n, const int32_t* traj, const double* t, double* out10) {
    if (!c || n <= 0 || !traj || !t || !out10) { setError("uph_traj_states: bad arguments"); return UPH_ERR_INVALID; }
    int r = checkTrajQueries(c, n, traj, t, "uph_traj_states");
    if (r != UPH_OK) return r;
    HIPCHK(hipSetDevice(uphMapDevice(c->map)));
    std::vector<SwitchQuery> sq((size_t)n);
    for (int32_t q = 0; q < n; q++) sq[(size_t)q] = trajQuery(c, traj[q], t[q]);
    r = launchTrajStates(c, sq);
    if (r != UPH_OK) { hipStreamSynchronize(c->stream); return r; }
    HIPCHK(hipMemcpyAsync(out10, c->d_sw_out.p, sizeof(double) * TRAJ_STATE_COLS * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return UPH_OK;
}

int uph_rollout_sizes(int32_t B, const int32_t* n_xy, const double* T_xy, const int32_t* n_yaw, const double* T_yaw, double dt, int32_t with_end,
                      int64_t* offsets) {
    if (B < 0 || !offsets || (B > 0 && (!n_xy || !T_xy || !n_yaw || !T_yaw))) { setError("uph_rollout_sizes: bad arguments"); return UPH_ERR_INVALID; }
    RolloutSizes rs;
    const int r = rolloutSizes(B, n_xy, T_xy, n_yaw, T_yaw, nullptr, dt, with_end, rs);
    if (r != UPH_OK) return r;
    std::memcpy(offsets, rs.offs.data(), 8 * ((size_t)B + 1));
    return UPH_OK;
}

int uph_rollout_plan(uph_ctx* c, double dt, int32_t with_end, int64_t* offsets) {
    if (!offsets) { setError("uph_rollout_plan: bad arguments"); return UPH_ERR_INVALID; }
    RolloutSizes rs;
    const int r = rolloutPlanCtx(c, dt, with_end, rs, "uph_rollout_plan");
    if (r != UPH_OK) return r;
    std::memcpy(offsets, rs.offs.data(), 8 * ((size_t)c->B + 1));
    return UPH_OK;
}

int uph_rollout_batch(uph_ctx* c, double dt, int32_t with_end, int32_t channels, int32_t b0, int32_t b1, double* out) {
    RolloutSizes rs;
    GridDev grid;
    int r = rolloutBegin(c, dt, with_end, channels, b0, b1, out, rs, grid, "uph_rollout_batch");
    if (r != UPH_OK) return r;
    const size_t row_bytes = 8 * (size_t)rolloutColumns(channels);
    const size_t need = row_bytes * (size_t)(rs.offs[b1] - rs.offs[b0]);
    if (need > 0 && c->d_roll_stage.ensure(std::min(need, ROLL_STAGE_BYTES))) return UPH_ERR_HIP;
    std::vector<RolloutTraj> rec;
    for (int k0 = b0; k0 < b1;) {
        int k1 = k0 + 1;           // whole trajectories while they fit the staging buffer (one always does)
        while (k1 < b1 && row_bytes * (size_t)(rs.offs[k1 + 1] - rs.offs[k0]) <= ROLL_STAGE_BYTES) k1++;
        const size_t bytes = row_bytes * (size_t)(rs.offs[k1] - rs.offs[k0]);
        if (bytes > 0) {
            r = rolloutLaunch(c, grid, rs, channels, k0, k1, c->d_roll_stage.as<double>(), rec);
            if (r != UPH_OK) { hipStreamSynchronize(c->stream); return r; }
            HIPCHK(hipMemcpyAsync((char*)out + row_bytes * (size_t)(rs.offs[k0] - rs.offs[b0]), c->d_roll_stage.p, bytes, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        k0 = k1;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return UPH_OK;
}

int uph_rollout_batch_dev(uph_ctx* c, double dt, int32_t with_end, int32_t channels, int32_t b0, int32_t b1, void* out_dev) {
    RolloutSizes rs;
    GridDev grid;
    int r = rolloutBegin(c, dt, with_end, channels, b0, b1, out_dev, rs, grid, "uph_rollout_batch_dev");
    if (r != UPH_OK) return r;
    std::vector<RolloutTraj> rec;
    r = rolloutLaunch(c, grid, rs, channels, b0, b1, (double*)out_dev, rec);
    const hipError_t e = hipStreamSynchronize(c->stream);      // (also after a failed launch: nothing of this call stays queued)
    if (r != UPH_OK) return r;
    if (e != hipSuccess) { setError(std::string("uph_rollout_batch_dev: ") + hipGetErrorString(e)); return UPH_ERR_HIP; }
    return UPH_OK;
}

int uph_check_limits(const uph_ctx* c, double* lim7) {
    if (!c || !lim7) { setError("uph_check_limits: bad arguments"); return UPH_ERR_INVALID; }
    const OptParams& P = c->P;
    const double l[7] = {P.max_vel, P.max_acc_lon, P.max_acc_lat, P.max_kap, -P.min_cxi, P.max_sig, __builtin_huge_val()};
    std::memcpy(lim7, l, sizeof(l));
    return UPH_OK;
}

int uph_check_window(double dt, int32_t with_end, double total, double t_from, double t_to, int32_t* q_lo, int32_t* q_hi, int32_t* end_row) {
    if (!q_lo || !q_hi || !end_row) { setError("uph_check_window: bad arguments"); return UPH_ERR_INVALID; }
    if (!(dt > 0.0) || !std::isfinite(dt)) { setError("uph_check_window: dt must be positive and finite"); return UPH_ERR_INVALID; }
    if (std::isnan(t_from) || std::isnan(t_to)) { setError("uph_check_window: a window bound is NaN"); return UPH_ERR_INVALID; }
    std::vector<double> tab;
    const int r = rolloutTimes(dt, total, tab);
    if (r != UPH_OK) return r;
    const int64_t cnt = std::lower_bound(tab.begin(), tab.end(), total) - tab.begin();       // (a NaN total: no samples, as in the loop)
    if (cnt >= (int64_t)tab.size()) { setError("uph_check_window: the trajectory needs more than UPH_ROLLOUT_MAX_SAMPLES samples at this dt"); return UPH_ERR_LIMIT; }
    checkWindow(tab, cnt, with_end, total, t_from, t_to, *q_lo, *q_hi, *end_row);
    return UPH_OK;
}

int uph_check_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t_from, const double* t_to, double dt, int32_t with_end, const double* lim7,
                    double* first_t, int32_t* first_mask, int32_t* counts, double* worst, double* worst_t) {
    if (!c || n <= 0 || !traj || !t_from) { setError("uph_check_batch: bad arguments"); return UPH_ERR_INVALID; }
    std::vector<WinQuery> qs;
    int r = formWindowQueries(c, n, traj, t_from, t_to, dt, with_end, "uph_check_batch", qs, [](int32_t, WinQuery&) { return (int)UPH_OK; });
    if (r != UPH_OK) return r;
    GridDev grid;
    r = syncGridMem(c, grid);
    if (r != UPH_OK) return r;
    if (c->d_win_out.ensure(sizeof(CheckOut) * (size_t)n)) return UPH_ERR_HIP;
    CheckArgs a;
    a.r = residentDev(c); a.grid_mem = trajFrame(c) ? c->d_gridmem.as<GridDev>() : nullptr; a.qs = c->d_win_q.as<WinQuery>(); a.out = c->d_win_out.as<CheckOut>();
    const char* occ_r2 = nullptr;
    uphMapOcc(c->map, &a.occ, &occ_r2);
    if (lim7) std::memcpy(a.lim, lim7, sizeof(a.lim));
    else uph_check_limits(c, a.lim);
    std::vector<CheckOut> out((size_t)n);
    r = runQueryLaunch(c, [&]() { hipLaunchKernelGGL(uph_check_kernel, dim3((unsigned)n), dim3(CHECK_NT), 0, c->stream, grid, a); return hipGetLastError(); }, out, c->last_check_ms);
    if (r != UPH_OK) return r;
    for (int32_t q = 0; q < n; q++) {
        const CheckOut& o = out[(size_t)q];
        if (first_t) first_t[q] = o.first_t;
        if (first_mask) first_mask[q] = o.first_mask;
        if (counts) for (int k = 0; k < 3; k++) counts[3 * (size_t)q + k] = o.counts[k];
        if (worst) for (int k = 0; k < 7; k++) worst[7 * (size_t)q + k] = o.worst[k];
        if (worst_t) for (int k = 0; k < 7; k++) worst_t[7 * (size_t)q + k] = o.worst_t[k];
    }
    return UPH_OK;
}

int uph_check_kernel_ms(const uph_ctx* c, double* kernel_ms) { return kernelMs("uph_check_kernel_ms", c, &uph_ctx::last_check_ms, kernel_ms); }


// ---- locate / within (include/uneven_hip.h uph_locate_*, uph_within_batch) ---------------------------------------------------------------------------
int uph_locate_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* poses, const double* t_from, const double* t_to, double dt, int32_t with_end,
                     double* near_t, double* near_d2, int32_t* count, double* t, int32_t* refined, double* state, double* d2, double* err) {
    if (!c || n <= 0 || !traj || !poses || !t_from) { setError("uph_locate_batch: bad arguments"); return UPH_ERR_INVALID; }
    std::vector<LocateOut> out;
    const int r = locRun(c, n, traj, t_from, t_to, dt, with_end, poses, 3, "uph_locate_batch", uph_locate_kernel<256>, uph_locate_kernel<64>, out);
    if (r != UPH_OK) return r;
    for (int32_t q = 0; q < n; q++) {
        const LocateOut& o = out[(size_t)q];
        if (near_t) near_t[q] = o.near_t;
        if (near_d2) near_d2[q] = o.near_d2;
        if (count) count[q] = o.count;
        if (t) t[q] = o.t;
        if (refined) refined[q] = o.refined;
        if (state) for (int k = 0; k < TRAJ_STATE_COLS; k++) state[(size_t)TRAJ_STATE_COLS * q + k] = o.state[k];
        if (d2) d2[q] = o.d2;
        if (err) for (int k = 0; k < 3; k++) err[3 * (size_t)q + k] = o.err[k];
    }
    return UPH_OK;
}

int uph_within_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* rects, const double* t_from, const double* t_to, double dt, int32_t with_end,
                     double* enter_t, double* leave_t, int32_t* counts) {
    if (!c || n <= 0 || !traj || !rects || !t_from) { setError("uph_within_batch: bad arguments"); return UPH_ERR_INVALID; }
    std::vector<WithinOut> out;
    const int r = locRun(c, n, traj, t_from, t_to, dt, with_end, rects, 4, "uph_within_batch", uph_within_kernel<256>, uph_within_kernel<64>, out);
    if (r != UPH_OK) return r;
    for (int32_t q = 0; q < n; q++) {
        const WithinOut& o = out[(size_t)q];
        if (enter_t) enter_t[q] = o.enter_t;
        if (leave_t) leave_t[q] = o.leave_t;
        if (counts) for (int k = 0; k < 2; k++) counts[2 * (size_t)q + k] = o.counts[k];
    }
    return UPH_OK;
}

int uph_locate_kernel_ms(const uph_ctx* c, double* kernel_ms) { return kernelMs("uph_locate_kernel_ms", c, &uph_ctx::last_locate_ms, kernel_ms); }


// ---- separation / extent / conflicts on a common clock (include/uneven_hip.h) -----------------------------------------------------------------------
int uph_separation_times(double t_from, double t_to, double dt, int64_t* K) {
    if (!K) { setError("uph_separation_times: bad arguments"); return UPH_ERR_INVALID; }
    int64_t k = 0;
    const int r = clockWindow(t_from, t_to, dt, k, "uph_separation_times");
    if (r != UPH_OK) return r;
    *K = k;
    return UPH_OK;
}

int uph_extent_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* t_from, const double* t_to, double dt, double* box, int32_t* counts) {
    return extentCall("uph_extent_batch", c, n, traj, t0, t_from, t_to, dt, nullptr, box, counts, &uph_ctx::last_sep_ms);
}

int uph_separation_batch(uph_ctx* ca, uph_ctx* cb, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, const double* t0_b, const double* t_from,
                         const double* t_to, double dt, const double* radius, double* min_d2, double* min_t, double* first_t, double* last_t, int32_t* counts) {
    std::vector<SepQuery> qs;
    int r = pairQueries("uph_separation_batch", ca, cb, n, traj_a, traj_b, t0_a, t0_b, t_from, t_to, dt, radius, nullptr, qs);
    if (r != UPH_OK) return r;
    std::vector<SepOut> out;
    double ms = 0.0;
    if ((r = pairRun(ca, cb, qs, nullptr, uph_separation_kernel<256>, uph_separation_kernel<64>, out, ms)) != UPH_OK) return r;
    ca->last_sep_ms = ms;
    pairRowsOut(out, min_d2, min_t, first_t, last_t, counts);
    return UPH_OK;
}

int uph_conflict_candidates(int32_t n, const double* box, const double* radius, int64_t cap, int32_t* pairs, int64_t* n_pairs) {
    if (n < 0 || cap < 0 || (n > 0 && (!box || !radius)) || (cap > 0 && !pairs)) { setError("uph_conflict_candidates: bad arguments"); return UPH_ERR_INVALID; }
    std::vector<IdxPair> found;
    const int r = candidatePairs(n, box, radius, "uph_conflict_candidates", found);
    if (r != UPH_OK) return r;
    for (size_t k = 0; k < found.size() && (int64_t)k < cap; k++) { pairs[2 * k] = found[k].first; pairs[2 * k + 1] = found[k].second; }
    if (n_pairs) *n_pairs = (int64_t)found.size();
    return UPH_OK;
}

int uph_conflicts_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* radius, double t_from, double t_to, double dt, int64_t cap,
                        int32_t* pairs, double* rows, int32_t* below, int64_t* n_conflicts, int64_t* n_candidates) {
    if (!c || n <= 0 || !traj || !t0 || !radius || cap < 0) { setError("uph_conflicts_batch: bad arguments"); return UPH_ERR_INVALID; }
    const auto form = [&](int64_t K, int32_t i, int32_t j) {
        return pairQuery(K, t_from, dt, nullptr, radius[i] + radius[j], clockTraj(c, traj[i], t0[i]), clockTraj(c, traj[j], t0[j]));
    };
    return fleetConflicts("uph_conflicts_batch", c, n, traj, t0, radius, t_from, t_to, dt, form, uph_separation_kernel<256>, uph_separation_kernel<64>,
                          &uph_ctx::last_sep_ms, cap, pairs, rows, below, n_conflicts, n_candidates);
}

int uph_separation_kernel_ms(const uph_ctx* c, double* kernel_ms) { return kernelMs("uph_separation_kernel_ms", c, &uph_ctx::last_sep_ms, kernel_ms); }

// ---- footprints (include/uneven_hip.h) -------------------------------------------------------------------------------------------------------------------
int uph_footprint_radii(int32_t n, const double* shape, const double* margin, double* r) {
    const std::string who = "uph_footprint_radii";
    if (n < 0 || (n > 0 && (!shape || !margin || !r))) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    std::vector<double> out;
    int rc = footAdmit(who, n, shape, "shape", margin);
    if (rc != UPH_OK || (rc = footRadii(who, n, shape, margin, out)) != UPH_OK) return rc;
    std::copy(out.begin(), out.end(), r);
    return UPH_OK;
}

int uph_footprint_separation_batch(uph_ctx* ca, uph_ctx* cb, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, const double* t0_b,
                                   const double* t_from, const double* t_to, double dt, const double* shape_a, const double* shape_b, const double* margin, double* min_c2,
                                   double* min_t, double* first_t, double* last_t, int32_t* counts) {
    const std::string who = "uph_footprint_separation_batch";
    if (!ca || n <= 0 || !shape_a || !shape_b || !margin) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    int r = footAdmit(who, n, shape_a, "shape_a", margin);
    if (r != UPH_OK || (r = footAdmit(who, n, shape_b, "shape_b", nullptr)) != UPH_OK) return r;
    std::vector<FootQuery> qs;      // the pair call's refusals, windows and vehicles, the margin in the radius' place
    if ((r = pairQueries(who, ca, cb, n, traj_a, traj_b, t0_a, t0_b, t_from, t_to, dt, margin, nullptr, qs)) != UPH_OK) return r;
    for (int32_t q = 0; q < n; q++) { qs[(size_t)q].sa = footShape(shape_a + 3 * (size_t)q); qs[(size_t)q].sb = footShape(shape_b + 3 * (size_t)q); }
    std::vector<FootOut> out;
    double ms = 0.0;
    if ((r = pairRun(ca, cb, qs, nullptr, uph_footprint_kernel<256>, uph_footprint_kernel<64>, out, ms)) != UPH_OK) return r;
    ca->last_foot_ms = ms;
    pairRowsOut(out, min_c2, min_t, first_t, last_t, counts);
    return UPH_OK;
}

int uph_footprint_conflicts_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* shape, const double* margin, double t_from, double t_to,
                                  double dt, int64_t cap, int32_t* pairs, double* rows, int32_t* below, int64_t* n_conflicts, int64_t* n_candidates) {
    const std::string who = "uph_footprint_conflicts_batch";
    if (!c || n <= 0 || !traj || !t0 || !shape || !margin || cap < 0) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    std::vector<double> radius;
    int r = footAdmit(who, n, shape, "shape", margin);
    if (r != UPH_OK || (r = footRadii(who, n, shape, margin, radius)) != UPH_OK) return r;
    const auto form = [&](int64_t K, int32_t i, int32_t j) {
        FootQuery q = pairQuery<FootQuery>(K, t_from, dt, nullptr, margin[i] + margin[j], clockTraj(c, traj[i], t0[i]), clockTraj(c, traj[j], t0[j]));
        q.sa = footShape(shape + 3 * (size_t)i); q.sb = footShape(shape + 3 * (size_t)j);
        return q;
    };
    return fleetConflicts(who, c, n, traj, t0, radius.data(), t_from, t_to, dt, form, uph_footprint_kernel<256>, uph_footprint_kernel<64>, &uph_ctx::last_foot_ms, cap,
                          pairs, rows, below, n_conflicts, n_candidates);
}

int uph_footprint_kernel_ms(const uph_ctx* c, double* kernel_ms) { return kernelMs("uph_footprint_kernel_ms", c, &uph_ctx::last_foot_ms, kernel_ms); }

// ---- footprint check (include/uneven_hip.h) ------------------------------------------------------------------------------------------------------------
int uph_footprint_check_columns(const uph_map_params* mp, int32_t n, const double* shape, const double* margin, int64_t* cols) {
    const std::string who = "uph_footprint_check_columns";
    if (!mp || n < 0 || (n > 0 && (!shape || !cols))) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    if (!(mp->xy_resolution > 0.0) || !std::isfinite(mp->xy_resolution)) { setError(who + ": the map's xy_resolution must be positive and finite"); return UPH_ERR_INVALID; }
    int r = footAdmit(who, n, shape, "shape", margin);
    if (r != UPH_OK) return r;
    std::vector<int64_t> out((size_t)n);
    for (int32_t q = 0; q < n; q++) {
        const FootCheckShape s = footCheckShape(shape + 3 * (size_t)q, margin ? margin[q] : 0.0);
        if ((r = footCheckColumns(who, q, s, mp->xy_resolution, out[(size_t)q])) != UPH_OK) return r;
    }
    std::copy(out.begin(), out.end(), cols);
    return UPH_OK;
}

int uph_footprint_check_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t_from, const double* t_to, double dt, int32_t with_end, const double* shape,
                              const double* margin, int32_t layers, double* first_t, double* last_t, int32_t* first_mask, int32_t* first_cell, int32_t* counts,
                              int64_t* cells) {
    const std::string who = "uph_footprint_check_batch";
    if (!c || n <= 0 || !traj || !t_from || !shape) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    if (layers < 1 || layers > UPH_FOOT_ALL) { setError(who + ": layers must be a non-empty subset of UPH_FOOT_ALL (1 .. 7)"); return UPH_ERR_INVALID; }
    int r = footAdmit(who, n, shape, "shape", margin);
    if (r != UPH_OK) return r;
    const double res = uphMapGrid(c->map).xy_res;
    std::vector<FootCheckQuery> qs;
    r = formWindowQueries(c, n, traj, t_from, t_to, dt, with_end, who.c_str(), qs, [&](int32_t q, FootCheckQuery& k) {
        const FootCheckShape s = footCheckShape(shape + 3 * (size_t)q, margin ? margin[q] : 0.0);
        int64_t cols = 0;
        const int rc = footCheckColumns(who, q, s, res, cols);
        if (rc != UPH_OK) return rc;
        if (cols > FOOT_CHECK_MAX_COLUMNS) { setError(whoQuery(who, q) + " has a shape and margin whose box can exceed 2^14 columns of the map"); return (int)UPH_ERR_LIMIT; }
        k.hl = s.hl; k.o = s.o; k.w = s.w; k.layers = layers; k.pad2 = 0;
        return (int)UPH_OK;
    });
    if (r != UPH_OK) return r;
    GridDev grid;
    r = syncGridMem(c, grid);
    if (r != UPH_OK) return r;
    if (c->d_win_out.ensure(sizeof(FootCheckOut) * (size_t)n)) return UPH_ERR_HIP;
    FootCheckArgs a;
    a.r = residentDev(c); a.qs = c->d_win_q.as<FootCheckQuery>(); a.out = c->d_win_out.as<FootCheckOut>(); a.framed = trajFrame(c); a.q0 = 0;
    uphMapOcc(c->map, &a.occ, &a.occ_r2);
    a.g.nx = grid.nx; a.g.ny = grid.ny; a.g.nyaw = grid.nyaw; a.g.x_off = grid.x_off; a.g.nx_hold = grid.nx_hold;
    for (int d = 0; d < 3; d++) a.g.origin[d] = grid.origin[d];
    a.g.xy_res = grid.xy_res; a.g.xy_inv = grid.xy_inv; a.g.yaw_inv = grid.yaw_inv;
    std::vector<FootCheckOut> out((size_t)n);
    const auto work = [&](size_t q) { return qs[q].n_tab + qs[q].end_row; };
    r = runQueryLaunch(c, twoWidths(c, (size_t)n, work, a, uph_footprint_check_kernel<256>, uph_footprint_check_kernel<64>), out, c->last_foot_check_ms);
    if (r != UPH_OK) return r;
    for (int32_t q = 0; q < n; q++) {
        const FootCheckOut& o = out[(size_t)q];
        if (first_t) first_t[q] = o.first_t;
        if (last_t) last_t[q] = o.last_t;
        if (first_mask) first_mask[q] = o.first_mask;
        if (first_cell) for (int k = 0; k < 2; k++) first_cell[2 * (size_t)q + k] = o.first_cell[k];
        if (counts) for (int k = 0; k < 5; k++) counts[5 * (size_t)q + k] = o.counts[k];
        if (cells) for (int k = 0; k < 2; k++) cells[2 * (size_t)q + k] = (int64_t)o.cells[k];
    }
    return UPH_OK;
}

int uph_footprint_check_kernel_ms(const uph_ctx* c, double* kernel_ms) {
    return kernelMs("uph_footprint_check_kernel_ms", c, &uph_ctx::last_foot_check_ms, kernel_ms);
}

// ---- clearance check (include/uneven_hip.h uph_clearance_check_*) ------------------------------------------------------------------------------------------
int uph_clearance_check_batch(uph_ctx* c, uph_clearance* layer, int32_t n, const int32_t* traj, const double* t_from, const double* t_to, double dt, int32_t with_end,
                              const int32_t* below2, int32_t* min_d2, double* min_t, int32_t* min_cell, double* first_t, double* last_t, int32_t* counts) {
    const std::string who = "uph_clearance_check_batch";
    if (!c || !layer || n <= 0 || !traj || !t_from || !below2) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    const uph_body_layer* body = uphClearanceBody(layer);
    if (uphBodyLayerMap(body) != c->map) { setError(who + ": the clearance layer belongs to another map than the context's"); return UPH_ERR_INVALID; }
    if (!uphClearanceFresh(layer)) { setError(who + ": the clearance layer is behind its body layer (uph_clearance_update with the rewritten rect, or uph_clearance_build)"); return UPH_ERR_INVALID; }
    if (!uphBodyLayerFresh(body)) { setError(who + ": the body layer is behind the map's occupancy (uph_body_layer_update / uph_body_layer_build, then the clearance layer's)"); return UPH_ERR_INVALID; }
    std::vector<ClearQuery> qs;
    int r = formWindowQueries(c, n, traj, t_from, t_to, dt, with_end, who.c_str(), qs, [&](int32_t q, ClearQuery& k) {
        if (below2[q] < 0) { setError(whoQuery(who, q) + " has a negative below2"); return (int)UPH_ERR_INVALID; }
        k.below2 = below2[q]; k.pad2 = 0;
        return (int)UPH_OK;
    });
    if (r != UPH_OK) return r;
    GridDev grid;
    r = syncGridMem(c, grid);
    if (r != UPH_OK) return r;
    if (c->d_win_out.ensure(sizeof(ClearOut) * (size_t)n)) return UPH_ERR_HIP;
    ClearCheckArgs a;
    a.r = residentDev(c); a.qs = c->d_win_q.as<ClearQuery>(); a.out = c->d_win_out.as<ClearOut>(); a.framed = trajFrame(c); a.q0 = 0;
    a.D = uphClearanceValues(layer);
    // a body layer is made of a whole-grid map (no tile): the layer's dimensions are the grid's
    a.g.nx = grid.nx; a.g.ny = grid.ny; a.g.nyaw = grid.nyaw; a.g.x_off = 0; a.g.nx_hold = grid.nx;
    for (int d = 0; d < 3; d++) a.g.origin[d] = grid.origin[d];
    a.g.xy_res = grid.xy_res; a.g.xy_inv = grid.xy_inv; a.g.yaw_inv = grid.yaw_inv;
    std::vector<ClearOut> out((size_t)n);
    const auto work = [&](size_t q) { return qs[q].n_tab + qs[q].end_row; };
    r = runQueryLaunch(c, twoWidths(c, (size_t)n, work, a, uph_clearance_check_kernel<256>, uph_clearance_check_kernel<64>), out, c->last_clear_check_ms);
    if (r != UPH_OK) return r;
    for (int32_t q = 0; q < n; q++) {
        const ClearOut& o = out[(size_t)q];
        if (min_d2) min_d2[q] = o.min_d2;
        if (min_t) min_t[q] = o.min_t;
        if (min_cell) for (int k = 0; k < 3; k++) min_cell[3 * (size_t)q + k] = o.min_cell[k];
        if (first_t) first_t[q] = o.first_t;
        if (last_t) last_t[q] = o.last_t;
        if (counts) for (int k = 0; k < 4; k++) counts[4 * (size_t)q + k] = o.counts[k];
    }
    return UPH_OK;
}

int uph_clearance_check_kernel_ms(const uph_ctx* c, double* kernel_ms) {
    return kernelMs("uph_clearance_check_kernel_ms", c, &uph_ctx::last_clear_check_ms, kernel_ms);
}

// ---- start delays (include/uneven_hip.h) -----------------------------------------------------------------------------------------------------------------
int uph_delay_times(double delay0, double delay_step, int32_t D, double* delta) {
    if (!delta) { setError("uph_delay_times: bad arguments"); return UPH_ERR_INVALID; }
    std::vector<double> tab;
    const int r = delayTable(delay0, delay_step, D, tab, "uph_delay_times");
    if (r != UPH_OK) return r;
    std::copy(tab.begin(), tab.end(), delta);
    return UPH_OK;
}

int uph_delay_levels(int32_t n, int64_t n_pairs, const int32_t* pairs, int32_t* level) {
    if (n < 0 || n_pairs < 0 || (n_pairs > 0 && !pairs) || (n > 0 && !level)) { setError("uph_delay_levels: bad arguments"); return UPH_ERR_INVALID; }
    std::vector<IdxPair> ps((size_t)n_pairs);
    for (int64_t k = 0; k < n_pairs; k++) {
        const int32_t i = pairs[2 * k], j = pairs[2 * k + 1];
        if (!(0 <= i && i < j && j < n)) { setError("uph_delay_levels: pair " + std::to_string(k) + " does not have 0 <= i < j < n"); return UPH_ERR_INVALID; }
        ps[(size_t)k] = IdxPair(i, j);
    }
    std::vector<int32_t> lv;
    delayLevels(n, ps, lv);
    std::copy(lv.begin(), lv.end(), level);
    return UPH_OK;
}

int uph_delay_sweep_batch(uph_ctx* ca, uph_ctx* cb, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, const double* t0_b, const double* t_from,
                          const double* t_to, double dt, const double* radius, double delay0, double delay_step, int32_t D, double* min_d2, double* min_t, int32_t* below,
                          int32_t* first_clear, int32_t* counts) {
    DelayTable dl{delay0, delay_step, D};
    std::vector<SepQuery> qs;
    int r = pairQueries("uph_delay_sweep_batch", ca, cb, n, traj_a, traj_b, t0_a, t0_b, t_from, t_to, dt, radius, &dl, qs);
    if (r != UPH_OK) return r;
    std::vector<int32_t> Ks((size_t)n);
    for (int32_t q = 0; q < n; q++) Ks[(size_t)q] = qs[(size_t)q].K;       // (pairRun leaves qs in launch order)
    std::vector<SweepOut> rows;
    double ms = 0.0;
    if ((r = pairRun(ca, cb, qs, &dl, uph_delay_sweep_kernel<256>, uph_delay_sweep_kernel<64>, rows, ms)) != UPH_OK) return r;
    ca->last_delay_ms = ms;
    for (int32_t q = 0; q < n; q++) {
        int32_t clear = -1;
        for (int32_t j = 0; j < D; j++) {
            const size_t at = (size_t)q * D + j;
            const SweepOut& o = rows[at];
            if (min_d2) min_d2[at] = o.min_d2;
            if (min_t) min_t[at] = o.min_t;
            if (below) below[at] = o.below;
            if (clear < 0 && o.below == 0) clear = j;
        }
        if (first_clear) first_clear[q] = clear;
        if (counts) counts[q] = Ks[(size_t)q];
    }
    return UPH_OK;
}

int uph_delay_extent_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* t_from, const double* t_to, double dt, double delay0, double delay_step,
                           int32_t D, double* box, int32_t* counts) {
    DelayTable dl{delay0, delay_step, D};
    return extentCall("uph_delay_extent_batch", c, n, traj, t0, t_from, t_to, dt, &dl, box, counts, &uph_ctx::last_delay_ms);
}

int uph_delays_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* radius, const int32_t* n_delays, double t_from, double t_to, double dt,
                     double delay0, double delay_step, int32_t D, int32_t* choice, double* start, int32_t* blocker, int64_t* n_candidates, int32_t* n_rounds,
                     int32_t* n_unresolved) {
    const std::string who = "uph_delays_batch";
    if (!c || n <= 0 || !traj || !t0 || !radius) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    const auto form = [&](int64_t K, const DelayTable* dl, int32_t h, double start_h, int32_t i) {
        return pairQuery(K, t_from, dt, dl, radius[h] + radius[i], clockTraj(c, traj[h], start_h), clockTraj(c, traj[i], t0[i]));
    };
    return fleetDelays<SepQuery, SweepOut>(who, c, n, traj, t0, radius, n_delays, t_from, t_to, dt, delay0, delay_step, D, form, uph_delay_sweep_kernel<256>,
                                           uph_delay_sweep_kernel<64>, choice, start, blocker, n_candidates, n_rounds, n_unresolved);
}

// ---- start delays with oriented rectangles (include/uneven_hip.h) -----------------------------------------------------------------------------------------
int uph_footprint_delay_sweep_batch(uph_ctx* ca, uph_ctx* cb, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, const double* t0_b,
                                    const double* t_from, const double* t_to, double dt, const double* shape_a, const double* shape_b, const double* margin, double delay0,
                                    double delay_step, int32_t D, double* min_c2, double* min_t, int32_t* below, int32_t* overlapping, int32_t* first_clear,
                                    int32_t* counts) {
    const std::string who = "uph_footprint_delay_sweep_batch";
    if (!ca || n <= 0 || !shape_a || !shape_b || !margin) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    int r = footAdmit(who, n, shape_a, "shape_a", margin);
    if (r != UPH_OK || (r = footAdmit(who, n, shape_b, "shape_b", nullptr)) != UPH_OK) return r;
    DelayTable dl{delay0, delay_step, D};
    if ((r = delayTable(delay0, delay_step, D, dl.delta, who)) != UPH_OK) return r;         // with the shapes: what needs no context is refused before one is read
    std::vector<FootQuery> qs;      // the pair call's refusals, windows and vehicles, the margin in the radius' place
    if ((r = pairQueries(who, ca, cb, n, traj_a, traj_b, t0_a, t0_b, t_from, t_to, dt, margin, &dl, qs)) != UPH_OK) return r;
    std::vector<int32_t> Ks((size_t)n);
    for (int32_t q = 0; q < n; q++) {                                       // (pairRun leaves qs in launch order)
        qs[(size_t)q].sa = footShape(shape_a + 3 * (size_t)q); qs[(size_t)q].sb = footShape(shape_b + 3 * (size_t)q);
        Ks[(size_t)q] = qs[(size_t)q].K;
    }
    std::vector<FootSweepOut> rows;
    double ms = 0.0;
    if ((r = pairRun(ca, cb, qs, &dl, uph_footprint_sweep_kernel<256>, uph_footprint_sweep_kernel<64>, rows, ms)) != UPH_OK) return r;
    ca->last_delay_ms = ms;
    for (int32_t q = 0; q < n; q++) {
        int32_t clear = -1;
        for (int32_t j = 0; j < D; j++) {
            const size_t at = (size_t)q * D + j;
            const FootSweepOut& o = rows[at];
            if (min_c2) min_c2[at] = o.min_c2;
            if (min_t) min_t[at] = o.min_t;
            if (below) below[at] = o.below;
            if (overlapping) overlapping[at] = o.over;
            if (clear < 0 && o.below == 0) clear = j;
        }
        if (first_clear) first_clear[q] = clear;
        if (counts) counts[q] = Ks[(size_t)q];
    }
    return UPH_OK;
}

int uph_footprint_delays_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* shape, const double* margin, const int32_t* n_delays,
                               double t_from, double t_to, double dt, double delay0, double delay_step, int32_t D, int32_t* choice, double* start, int32_t* blocker,
                               int64_t* n_candidates, int32_t* n_rounds, int32_t* n_unresolved) {
    const std::string who = "uph_footprint_delays_batch";
    if (!c || n <= 0 || !traj || !t0 || !shape || !margin) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    std::vector<double> radius;
    int r = footAdmit(who, n, shape, "shape", margin);
    if (r != UPH_OK || (r = footRadii(who, n, shape, margin, radius)) != UPH_OK) return r;
    std::vector<double> table;      // with the shapes: what needs no context is refused before one is read
    if ((r = delayTable(delay0, delay_step, D, table, who)) != UPH_OK || (r = delayLimits(who, n, n_delays, D)) != UPH_OK) return r;
    const auto form = [&](int64_t K, const DelayTable* dl, int32_t h, double start_h, int32_t i) {
        FootQuery q = pairQuery<FootQuery>(K, t_from, dt, dl, margin[h] + margin[i], clockTraj(c, traj[h], start_h), clockTraj(c, traj[i], t0[i]));
        q.sa = footShape(shape + 3 * (size_t)h); q.sb = footShape(shape + 3 * (size_t)i);
        return q;
    };
    return fleetDelays<FootQuery, FootSweepOut>(who, c, n, traj, t0, radius.data(), n_delays, t_from, t_to, dt, delay0, delay_step, D, form,
                                                uph_footprint_sweep_kernel<256>, uph_footprint_sweep_kernel<64>, choice, start, blocker, n_candidates, n_rounds,
                                                n_unresolved);
}

int uph_delay_kernel_ms(const uph_ctx* c, double* kernel_ms) { return kernelMs("uph_delay_kernel_ms", c, &uph_ctx::last_delay_ms, kernel_ms); }

}  // extern "C"
