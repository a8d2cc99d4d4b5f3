"""Host-side mirror of the reference's ALMTrajOpt (back_end/include/back_end/alm_traj_opt.h:21-120) over the batched
MI355X back-end.  Same public parameter names, same `optimizeSE2Traj` argument list and return codes; `getTraj()`
returns the piece durations and coefficient matrices the reference's SE2Trajectory holds.  `optimize_batch` is the
batched form (B independent goals solved by one kernel launch, one workgroup per trajectory)."""
import ctypes as C

import numpy as np

from . import _lib

# plan_manager/params/run_hill.yaml:32-55
HILL_OPT_PARAMS = dict(rho_T=100000.0, rho_ter=10.0, max_vel=0.5, max_acc_lon=5.0, max_acc_lat=10.0, max_kap=2.1,
                       min_cxi=0.8, max_sig=0.05, use_scaling=True, rho=1.0, beta=1000.0, gamma=1.0,
                       epsilon_con=0.001, max_iter=10.0, g_epsilon=1.0e-3, min_step=1.0e-32, inner_max_iter=10000.0,
                       delta=1.0e-4, mem_size=256, past=3, int_K=16)
_INT_FIELDS = ("use_scaling", "mem_size", "past", "int_K")


def pack_problems(probs, int_K=16, with_sizes=False):
    """problem dicts -> a ctypes array of uph_problem (column-major matrices, as Eigen::MatrixXd holds them) + the numpy arrays its pointers
    refer to (keep them alive while the array is in use) [+ the per-problem sizes]; no device, no context needed"""
    arr = (_lib.Problem * len(probs))()
    keep, sizes = [], []
    for i, pr in enumerate(probs):
        ixy = np.ascontiguousarray(np.asarray(pr["inner_xy"], dtype=np.float64).T)       # column-major 2 x (Nxy-1)
        iyw = np.ascontiguousarray(pr["inner_yaw"], dtype=np.float64)
        keep += [ixy, iyw]
        a = arr[i]
        a.n_inner_xy, a.n_inner_yaw = ixy.shape[0], iyw.shape[0]
        a.init_xy[:] = np.asarray(pr["init_xy"], dtype=np.float64).T.ravel().tolist()
        a.end_xy[:] = np.asarray(pr["end_xy"], dtype=np.float64).T.ravel().tolist()
        a.init_yaw[:] = np.asarray(pr["init_yaw"], dtype=np.float64).ravel().tolist()
        a.end_yaw[:] = np.asarray(pr["end_yaw"], dtype=np.float64).ravel().tolist()
        a.inner_xy, a.inner_yaw = _dp(ixy), _dp(iyw)
        a.total_time = float(pr["total_time"])
        nxy, nyaw = a.n_inner_xy + 1, a.n_inner_yaw + 1
        sizes.append(dict(Nxy=nxy, Nyaw=nyaw, n=2 * (nxy - 1) + (nyaw - 1) + 1, S=nxy * (int(int_K) + 1)))
    return (arr, keep, sizes) if with_sizes else (arr, keep)


def _dp(a):
    return a.ctypes.data_as(_lib.DP)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def norm_so2(yaw):
    """UnevenMap::normSO2 (uneven_map.cpp:63-70) as the device forms it (csrc/uph_common.hpp): whole turns added / removed one at a time"""
    y = float(yaw)
    for _ in range(4096):
        if not y < -np.pi:
            break
        y += 2 * np.pi
    for _ in range(4096):
        if not y > np.pi:
            break
        y -= 2 * np.pi
    return y


class SE2Traj:
    """What MINCO_SE2::getTraj() yields (se2traj.hpp:682-695, 844-850): per piece a duration and a D x 6 coefficient
    matrix, highest order first."""

    def __init__(self, c_xy, c_yaw, T_xy, T_yaw):
        self.c_xy, self.c_yaw, self.T_xy, self.T_yaw = c_xy, c_yaw, T_xy, T_yaw
        nxy, nyaw = c_xy.shape[0] // 6, c_yaw.shape[0] // 6
        self.pos_durations = np.full(nxy, T_xy)
        self.yaw_durations = np.full(nyaw, T_yaw)
        self.pos_coeffs = c_xy.reshape(nxy, 6, 2).transpose(0, 2, 1)[:, :, ::-1].copy()      # (piece, dim, 6) descending powers
        self.yaw_coeffs = c_yaw.reshape(nyaw, 6, 1).transpose(0, 2, 1)[:, :, ::-1].copy()

    def getTotalDuration(self):
        return min(self.pos_durations.sum(), self.yaw_durations.sum())

    @staticmethod
    def _locate(durs, t):
        """PolyTrajectory::locatePieceIdx (se2traj.hpp:343-361)"""
        idx = 0
        while idx < len(durs) and t > durs[idx]:
            t -= durs[idx]
            idx += 1
        if idx == len(durs):
            idx -= 1
            t += durs[idx]
        return idx, t

    @staticmethod
    def _value(c_desc, t):
        """Piece::getValue (se2traj.hpp:106-116): coefficients highest order first, value += tn * coeff, tn *= t"""
        v, tn = 0.0, 1.0
        for i in range(5, -1, -1):
            v += tn * c_desc[i]
            tn *= t
        return v

    def getValue(self, t, yaw=False):
        durs = self.yaw_durations if yaw else self.pos_durations
        co = self.yaw_coeffs if yaw else self.pos_coeffs
        total = 0.0
        for d_ in durs:                                  # getTotalDuration's running sum (se2traj.hpp:290-299)
            total += d_
        idx, tl = self._locate(list(durs), total if t is None else t)
        return np.array([self._value(co[idx, d], tl) for d in range(co.shape[1])])

    @staticmethod
    def _derivs(c_desc, t):
        """value, first and second derivative of one piece polynomial at t, in the device's order (trajectory_dev.hpp): ascending powers, tn *= t"""
        v = dv = dd = 0.0
        tn = 1.0
        for k in range(6):
            v += tn * c_desc[5 - k]
            tn *= t
        tn = 1.0
        for k in range(1, 6):
            dv += k * tn * c_desc[5 - k]
            tn *= t
        tn = 1.0
        for k in range(2, 6):
            dd += (k - 1) * k * tn * c_desc[5 - k]
            tn *= t
        return v, dv, dd

    def getState(self, t):
        """host mirror of the switch state uph_replan_upload evaluates on the device: at t clamped to [0, getTotalDuration()] (the running sums of
        the piece durations, the smaller one, as the rollout forms the duration), x, y, dx, dy, ddx, ddy, normSO2(yaw), dyaw, ddyaw -- the pieces
        located by locatePieceIdx (se2traj.hpp:343-361).  Coordinates of the coefficients' frame (a batch solved in local frames: add the shift)."""
        tx = ty = 0.0
        for d_ in self.pos_durations:
            tx += d_
        for d_ in self.yaw_durations:
            ty += d_
        total = tx if tx < ty else ty
        t = float(t)
        t = 0.0 if t <= 0.0 else (total if t >= total else t)
        ix, tl = self._locate(list(self.pos_durations), t)
        iw, tw = self._locate(list(self.yaw_durations), t)
        px, vx, ax = self._derivs(self.pos_coeffs[ix, 0], tl)
        py, vy, ay = self._derivs(self.pos_coeffs[ix, 1], tl)
        w, dw, ddw = self._derivs(self.yaw_coeffs[iw, 0], tw)
        return np.array([px, py, vx, vy, ax, ay, norm_so2(w), dw, ddw])

    def to_msg(self):
        """the mpc_controller/SE2Traj message PlanManager publishes (mpc_controller/msg/SE2Traj.msg:1-9, filled as at
        plan_manager.cpp:150-182): pos_pts / angle_pts = piece start points + the end point (geometry_msgs/Point: x, y, z),
        posT_pts / angleT_pts = piece durations, init_v = init_a = 0.  start_time is the caller's (ros::Time::now())."""
        nxy, nyaw = self.pos_durations.size, self.yaw_durations.size
        pos = np.zeros((nxy + 1, 3))
        for i in range(nxy):
            pos[i, 0], pos[i, 1] = self._value(self.pos_coeffs[i, 0], 0.0), self._value(self.pos_coeffs[i, 1], 0.0)
        pos[nxy, :2] = self.getValue(None)
        ang = np.zeros((nyaw + 1, 3))
        for i in range(nyaw):
            ang[i, 0] = self._value(self.yaw_coeffs[i, 0], 0.0)
        ang[nyaw, 0] = self.getValue(None, yaw=True)[0]
        return dict(pos_pts=pos, angle_pts=ang, init_v=np.zeros(3), init_a=np.zeros(3), posT_pts=self.pos_durations.copy(),
                    angleT_pts=self.yaw_durations.copy())

    def waypoints(self):
        """pos_pts (x, y) / angle_pts of the message"""
        m = self.to_msg()
        return m["pos_pts"][:, :2], m["angle_pts"][:, 0]


# uph_rollout_* channel groups (include/uneven_hip.h): columns of a rollout row, in this order when selected
ROLLOUT_STATE, ROLLOUT_TERRAIN, ROLLOUT_POSE = 1, 2, 4
ROLLOUT_ALL = 7
ROLLOUT_MAX_SAMPLES = 262144
ROLLOUT_COLUMNS = {ROLLOUT_STATE: ("t", "x", "y", "yaw", "dx", "dy", "ddx", "ddy", "dyaw"),
                   ROLLOUT_TERRAIN: ("vx", "ax", "ay", "cur", "att", "sigma", "nonhol"),
                   ROLLOUT_POSE: ("R00", "R10", "R20", "R01", "R11", "R21", "R02", "R12", "R22", "px", "py", "pz")}


def rollout_columns(channels=ROLLOUT_ALL):
    """names of the columns of a rollout row for a channel mask"""
    return [n for g in (ROLLOUT_STATE, ROLLOUT_TERRAIN, ROLLOUT_POSE) if channels & g for n in ROLLOUT_COLUMNS[g]]


def rollout_sizes(n_xy, T_xy, n_yaw, T_yaw, dt=0.01, with_end=False):
    """uph_rollout_sizes (host only): offsets[B + 1] of the rows of trajectories of n_xy pieces of T_xy and n_yaw pieces of T_yaw"""
    n_xy, n_yaw = np.ascontiguousarray(n_xy, dtype=np.int32), np.ascontiguousarray(n_yaw, dtype=np.int32)
    T_xy, T_yaw = np.ascontiguousarray(T_xy, dtype=np.float64), np.ascontiguousarray(T_yaw, dtype=np.float64)
    B = n_xy.shape[0]
    offs = np.zeros(B + 1, dtype=np.int64)
    _lib.check(_lib.load().uph_rollout_sizes(B, _ip(n_xy), _dp(T_xy), _ip(n_yaw), _dp(T_yaw), float(dt), int(bool(with_end)),
                                             offs.ctypes.data_as(C.POINTER(C.c_int64))), "uph_rollout_sizes")
    return offs


def split_rollout(offsets, rows):
    """(offsets, rows) of a rollout -> one view of rows per trajectory (offsets relative to the first trajectory of the range)"""
    o = np.asarray(offsets) - int(offsets[0])
    return [rows[int(o[i]):int(o[i + 1])] for i in range(len(o) - 1)]


# uph_check_batch (include/uneven_hip.h): the seven terms of a mask are the ROLLOUT_TERRAIN columns, bit CHECK_OCC_BIT is the occupancy
CHECK_OCC_BIT = _lib.UPH_CHECK_OCC_BIT
CHECK_TERMS = ROLLOUT_COLUMNS[ROLLOUT_TERRAIN]


def check_window(dt, with_end, total, t_from, t_to):
    """uph_check_window (host only): (q_lo, q_hi, end_row) -- the samples q_lo <= q < q_hi of the running sum t += dt, and whether the end row at
    t = total, that the window [t_from, t_to] holds of a trajectory of duration total"""
    v = [C.c_int32(0) for _ in range(3)]
    _lib.check(_lib.load().uph_check_window(float(dt), int(bool(with_end)), float(total), float(t_from), float(t_to), *[C.byref(x) for x in v]),
               "uph_check_window")
    return v[0].value, v[1].value, bool(v[2].value)


def check_rows(t, terms, occ, lim, t_from=-np.inf, t_to=np.inf):
    """Host mirror of one uph_check_batch query, written from the rule and not from the kernel: reduces one trajectory's rollout rows -- t (n,), terms
    (n, 7) the ROLLOUT_TERRAIN columns, occ (n,) uph_frontend_query's occ at the rows' (x, y, yaw) -- whose t lies in [t_from, t_to].
    Term k violates when not (|v| <= lim[k]) for k < 4 and when not (v <= lim[k]) for k >= 4 (a NaN violates); occ != 0 sets bit CHECK_OCC_BIT.
    Returns the dict of ALMTrajOpt.check for that query: first_t, first_mask, counts (3,), worst (7,), worst_t (7,)."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    terms = np.asarray(terms, dtype=np.float64).reshape(-1, 7)
    occ = np.asarray(occ).reshape(-1)
    lim = np.asarray(lim, dtype=np.float64).reshape(7)
    with np.errstate(invalid="ignore"):
        sel = (t_from <= t) & (t <= t_to)
    t, v, occ = t[sel], terms[sel], occ[sel]
    m = np.concatenate([np.abs(v[:, :4]), v[:, 4:]], axis=1)
    with np.errstate(invalid="ignore"):
        viol = ~(m <= lim[None, :])                                 # a NaN compares false: it violates
    occupied = occ != 0
    mask = (viol.astype(np.int64) << np.arange(7)[None, :]).sum(axis=1) + (occupied.astype(np.int64) << CHECK_OCC_BIT)
    counts = np.array([t.shape[0], np.count_nonzero(mask), np.count_nonzero(occupied)], dtype=np.int32)
    bad = np.nonzero(mask)[0]
    first_t, first_mask = (t[bad[0]], int(mask[bad[0]])) if bad.size else (np.nan, 0)
    worst, worst_t = np.full(7, -np.inf), np.full(7, np.nan)
    if t.shape[0]:
        key = np.where(np.isfinite(v), m, np.inf)
        at = np.argmax(key, axis=0)                                 # the first occurrence of the maximum: a tie stays with the earlier sample
        worst, worst_t = key[at, np.arange(7)], t[at]
    return dict(first_t=first_t, first_mask=first_mask, counts=counts, worst=worst, worst_t=worst_t)


# uph_locate_batch / uph_within_batch (include/uneven_hip.h): numpy mirrors written from the rule, not from the kernel
LOCATE_NEWTON = 8


def _window(t, t_from, t_to):
    with np.errstate(invalid="ignore"):
        return (t_from <= t) & (t <= t_to)


def locate_rows(t, xy, pose, t_from=-np.inf, t_to=np.inf):
    """Host mirror of the coarse stage of one uph_locate_batch query: among one trajectory's rollout rows -- t (n,), xy (n, 2) the STATE columns x, y --
    whose t lies in [t_from, t_to], the one nearest to pose (x, y[, yaw]) by d2 = ex ex + ey ey (each product rounded, then the add).  A NaN d2 reads
    +inf, a tie stays with the earlier row.  Returns near_t, near_d2, count, and for locate_refine j (the winner's index in the window, -1: empty
    window) and times (the window's t)."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    pose = np.asarray(pose, dtype=np.float64).reshape(-1)
    sel = _window(t, t_from, t_to)
    t, xy = t[sel], xy[sel]
    if t.shape[0] == 0:
        return dict(near_t=np.nan, near_d2=np.inf, count=0, j=-1, times=t)
    with np.errstate(over="ignore", invalid="ignore"):
        ex, ey = xy[:, 0] - pose[0], xy[:, 1] - pose[1]
        d2 = ex * ex + ey * ey
    key = np.where(np.isnan(d2), np.inf, d2)
    j = int(np.argmin(key))                                         # the first occurrence of the minimum
    return dict(near_t=t[j], near_d2=key[j], count=t.shape[0], j=j, times=t)


def within_rows(t, xy, rect, t_from=-np.inf, t_to=np.inf):
    """Host mirror of one uph_within_batch query: the rows of the window [t_from, t_to] inside the closed rect (x0, x1, y0, y1); a NaN position is
    outside, a reversed rect is empty.  Returns enter_t / leave_t (t of the first / last row inside, NaN: none) and counts (2,): rows, rows inside."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    x0, x1, y0, y1 = (float(v) for v in np.asarray(rect, dtype=np.float64).reshape(4))
    sel = _window(t, t_from, t_to)
    t, xy = t[sel], xy[sel]
    with np.errstate(invalid="ignore"):
        inside = np.nonzero((x0 <= xy[:, 0]) & (xy[:, 0] <= x1) & (y0 <= xy[:, 1]) & (xy[:, 1] <= y1))[0]
    return dict(enter_t=t[inside[0]] if inside.size else np.nan, leave_t=t[inside[-1]] if inside.size else np.nan,
                counts=np.array([t.shape[0], inside.size], dtype=np.int32))


def _state10(traj, shift, t):
    """uph_traj_states' row of an SE2Traj at t (not clamped: the refinement stays inside the samples), the frame shift added to the position"""
    ix, tl = traj._locate(list(traj.pos_durations), t)
    iw, tw = traj._locate(list(traj.yaw_durations), t)
    px, vx, ax = traj._derivs(traj.pos_coeffs[ix, 0], tl)
    py, vy, ay = traj._derivs(traj.pos_coeffs[ix, 1], tl)
    w, dw, ddw = traj._derivs(traj.yaw_coeffs[iw, 0], tw)
    return np.array([px + shift[0], py + shift[1], vx, vy, ax, ay, norm_so2(w), dw, ddw, w])


def locate_errors(state, pose):
    """e_lon, e_lat, e_yaw of a pose (x, y, yaw) against a traj_states row: r = (x, y) - (X, Y) along and across the raw yaw psi (column 9), and
    normSO2(yaw - psi)"""
    psi = state[9]
    rx, ry = pose[0] - state[0], pose[1] - state[1]
    return np.array([rx * np.cos(psi) + ry * np.sin(psi), ry * np.cos(psi) - rx * np.sin(psi), norm_so2(pose[2] - psi)])


def locate_refine(se2traj, shift, pose, times, j):
    """Host mirror of the refinement of one uph_locate_batch query on a downloaded SE2Traj (`shift`: its frame's corner in map coordinates, (0, 0) for a
    batch in the map's frame): `times` are the window's samples and j the coarse winner (locate_rows).  A safeguarded Newton iteration on
    g(t) = e . v inside [times[max(j - 1, 0)], times[min(j + 1, n - 1)]], at most LOCATE_NEWTON iterations; the candidate is kept when its d2 is not
    larger than the coarse one.  Returns t, refined, state (10,), d2, err (3,), lo, hi and iters (evaluations of g)."""
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    pose = np.asarray(pose, dtype=np.float64).reshape(3)
    n = times.shape[0]
    nan = np.nan
    if n == 0 or j < 0:
        return dict(t=nan, refined=0, state=np.full(10, nan), d2=np.inf, err=np.full(3, nan), lo=nan, hi=nan, iters=0)
    lo, hi = times[max(j - 1, 0)], times[min(j + 1, n - 1)]

    def at(t):
        s = _state10(se2traj, shift, t)
        ex, ey = s[0] - pose[0], s[1] - pose[1]
        with np.errstate(over="ignore", invalid="ignore"):
            return s, ex, ey, ex * ex + ey * ey

    s0, _, _, d0 = at(times[j])
    d0 = np.inf if np.isnan(d0) else d0
    t, a, b, iters = times[j], lo, hi, 0
    with np.errstate(all="ignore"):
        for _ in range(LOCATE_NEWTON):
            s, ex, ey, _ = at(t)
            iters += 1
            g = ex * s[2] + ey * s[3]
            h = s[2] * s[2] + s[3] * s[3] + ex * s[4] + ey * s[5]
            if g > 0:
                b = t
            elif g < 0:
                a = t
            elif g == 0:
                break
            tn = t - g / h if h > 0 else nan
            if not (h > 0 and a <= tn <= b):
                tn = 0.5 * (a + b)
            if tn == t:
                break
            t = tn
    s, _, _, d2 = at(t)
    refined = bool(d2 <= d0)
    if not refined:
        t, s, d2 = times[j], s0, d0
    return dict(t=t, refined=int(refined), state=s, d2=d2, err=locate_errors(s, pose), lo=lo, hi=hi, iters=iters)


# uph_separation_batch / uph_extent_batch / uph_conflict_candidates (include/uneven_hip.h): numpy mirrors written from the rule, not from the kernels
def separation_times(t_from, t_to, dt):
    """Host mirror of the sample times of a window on the common clock: tau_k = t_from + k * dt (the product rounded, then the sum) for every k >= 0
    with tau_k <= t_to, as an array (empty when t_to < t_from).  Raises for bounds or a dt the library refuses and for more than 2^22 samples."""
    t_from, t_to, dt = float(t_from), float(t_to), float(dt)
    if not (np.isfinite(t_from) and np.isfinite(t_to) and np.isfinite(dt) and dt > 0.0):
        raise _lib.UnevenHipError("separation_times: the bounds must be finite and dt positive and finite")
    if t_to < t_from:
        return np.zeros(0)
    cap = _lib.SEPARATION_MAX_SAMPLES + 1
    n = int(min((t_to - t_from) / dt, float(cap))) + 2
    while True:                                                     # tau does not decrease with k: grow until the last one is beyond t_to
        n = min(n, cap)
        with np.errstate(over="ignore"):
            p = np.arange(n, dtype=np.float64) * dt
            tau = t_from + p
        if tau[-1] > t_to or n == cap:
            break
        n *= 2
    K = int(np.count_nonzero(tau <= t_to))
    if K > _lib.SEPARATION_MAX_SAMPLES:
        raise _lib.UnevenHipError("separation_times: the window holds more than 2^22 samples at this dt")
    return tau[:K]


def separation_rows(tau, xy_a, xy_b, radius):
    """Host mirror of one uph_separation_batch query: tau (K,) the sample times, xy_a / xy_b (K, 2) the two vehicles' positions at them, radius = R.
    d2 = ex ex + ey ey (each product rounded, then the add); a sample is below when d2 < R * R, strictly (a NaN d2 never is); for the minimum a NaN d2
    reads +inf and a tie stays with the earlier sample.  Returns min_d2, min_t, first_t, last_t (NaN: no such sample) and counts (2,): samples, below."""
    tau = np.asarray(tau, dtype=np.float64).reshape(-1)
    a = np.asarray(xy_a, dtype=np.float64).reshape(-1, 2)
    b = np.asarray(xy_b, dtype=np.float64).reshape(-1, 2)
    R = np.float64(radius)
    if tau.shape[0] == 0:
        return dict(min_d2=np.inf, min_t=np.nan, first_t=np.nan, last_t=np.nan, counts=np.zeros(2, dtype=np.int32))
    with np.errstate(over="ignore", invalid="ignore"):
        ex, ey = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
        d2 = ex * ex + ey * ey
        below = np.nonzero(d2 < R * R)[0]
    key = np.where(np.isnan(d2), np.inf, d2)
    j = int(np.argmin(key))                                         # the first occurrence of the minimum
    return dict(min_d2=key[j], min_t=tau[j], first_t=tau[below[0]] if below.size else np.nan, last_t=tau[below[-1]] if below.size else np.nan,
                counts=np.array([tau.shape[0], below.size], dtype=np.int32))


def extent_rows(xy):
    """Host mirror of one uph_extent_batch query on the vehicle's positions xy (K, 2) at the window's samples: box (4,) = xmin, xmax, ymin, ymax over
    the rows without a NaN ((+inf, -inf, +inf, -inf): none) and counts (2,): samples, NaN samples."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    ok = ~np.isnan(xy).any(axis=1)
    v = xy[ok]
    box = np.array([v[:, 0].min(), v[:, 0].max(), v[:, 1].min(), v[:, 1].max()]) if v.shape[0] else np.array([np.inf, -np.inf, np.inf, -np.inf])
    return dict(box=box, counts=np.array([xy.shape[0], xy.shape[0] - v.shape[0]], dtype=np.int32))


def conflict_candidates(box, radius):
    """Host mirror of uph_conflict_candidates: the pairs (i < j) of boxes box (n, 4) = xmin, xmax, ymin, ymax with radii radius (n,) that the rule does
    not drop -- dropped iff xmin_i - xmax_j > R, xmin_j - xmax_i > R or either of the same in y, R = r_i + r_j -- as an (m, 2) int32 array in (i, j) order"""
    box = np.asarray(box, dtype=np.float64).reshape(-1, 4)
    r = np.asarray(radius, dtype=np.float64).reshape(-1)
    n = box.shape[0]
    R = r[:, None] + r[None, :]
    with np.errstate(invalid="ignore"):
        gx = box[:, None, 0] - box[None, :, 1]                      # [i, j] = xmin_i - xmax_j
        gy = box[:, None, 2] - box[None, :, 3]
        drop = (gx > R) | (gx.T > R) | (gy > R) | (gy.T > R)
    keep = ~drop & (np.arange(n)[:, None] < np.arange(n)[None, :])
    return np.argwhere(keep).astype(np.int32).reshape(-1, 2)


# uph_footprint_radii / uph_footprint_separation_batch / uph_footprint_conflicts_batch (include/uneven_hip.h): numpy mirrors written from the rule.  Every product
# and every sum below is rounded on its own, in the order the header gives; against the device only the sine and the cosine differ (numpy's, not sincosFast).
def _shapes(shape, n, who):
    s = np.asarray(shape, dtype=np.float64)
    if s.shape[-1:] != (3,):
        raise _lib.UnevenHipError(who + ": a shape is (front, rear, half_width)")
    s = np.ascontiguousarray(np.broadcast_to(s, (n, 3)))
    if not (np.isfinite(s).all() and (s >= 0.0).all()):
        raise _lib.UnevenHipError(who + ": a shape component is negative or not finite")
    return s


def footprint_radii(shape, margin):
    """Host mirror of uph_footprint_radii: shape (n, 3) = front, rear, half_width and margin (n,) (a scalar is broadcast) give the broad-phase radius
    r_i = (hypot(max(front, rear), half_width) + margin_i) * (1 + 2^-40) for conflict_candidates on extent()'s boxes.  Raises for what the library refuses."""
    s = np.asarray(shape, dtype=np.float64).reshape(-1, 3)
    s = _shapes(s, s.shape[0], "footprint_radii")
    m = np.ascontiguousarray(np.broadcast_to(np.asarray(margin, dtype=np.float64), (s.shape[0],)))
    if not (np.isfinite(m).all() and (m >= 0.0).all()):
        raise _lib.UnevenHipError("footprint_radii: a margin is negative or not finite")
    return (np.hypot(np.maximum(s[:, 0], s[:, 1]), s[:, 2]) + m) * (1.0 + 2.0 ** -40)


def footprint_clearance2(xy_a, yaw_a, shape_a, xy_b, yaw_b, shape_b, gap=False):
    """Host mirror of the footprint rule at K samples: xy (K, 2) and yaw (K,) the two vehicles' poses (traj_states' columns 0, 1 and 9), shape = (front,
    rear, half_width) each.  Returns c2 (K,) -- the squared distance between the two rectangles, 0 where they overlap or touch, NaN where a pose is not
    finite -- and the overlap flags (K,); gap = True adds g (K,), the largest of the four separating-axis gaps (overlap is g <= 0)."""
    a, b = np.asarray(xy_a, dtype=np.float64).reshape(-1, 2), np.asarray(xy_b, dtype=np.float64).reshape(-1, 2)
    K = a.shape[0]
    wa, wb = (np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.float64), (K,))) for w in (yaw_a, yaw_b))
    (fa, ra, ha), (fb, rb, hb) = (_shapes(s, 1, "footprint_clearance2")[0] for s in (shape_a, shape_b))
    hla, oa, hlb, ob = 0.5 * (fa + ra), 0.5 * (fa - ra), 0.5 * (fb + rb), 0.5 * (fb - rb)
    with np.errstate(over="ignore", invalid="ignore"):
        bad = ~(np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(wa) & np.isfinite(wb))
        ca, sa, cb, sb = np.cos(wa), np.sin(wa), np.cos(wb), np.sin(wb)
        ua, va, ub, vb = (ca, sa), (-sa, ca), (cb, sb), (-sb, cb)
        dot = lambda p, q: p[0] * q[0] + p[1] * q[1]
        # coordinates relative to vehicle a's point
        Ca = (oa * ca, oa * sa)
        Cb = ((b[:, 0] - a[:, 0]) + ob * cb, (b[:, 1] - a[:, 1]) + ob * sb)
        d = (Cb[0] - Ca[0], Cb[1] - Ca[1])
        g = np.full(K, -np.inf)
        for n in (ua, va, ub, vb):
            reach = (hla * np.abs(dot(n, ua)) + ha * np.abs(dot(n, va))) + (hlb * np.abs(dot(n, ub)) + hb * np.abs(dot(n, vb)))
            g = np.maximum(g, np.abs(dot(d, n)) - reach)
        c2 = np.full(K, np.inf)
        for (C, u, v, hl, w), (Co, uo, vo, hlo, wo) in (((Ca, ua, va, hla, ha), (Cb, ub, vb, hlb, hb)), ((Cb, ub, vb, hlb, hb), (Ca, ua, va, hla, ha))):
            for sx in (1.0, -1.0):
                for sy in (1.0, -1.0):
                    e = ((C[0] + sx * (hl * u[0])) + sy * (w * v[0]) - Co[0], (C[1] + sx * (hl * u[1])) + sy * (w * v[1]) - Co[1])
                    ex, ey = np.maximum(np.abs(dot(e, uo)) - hlo, 0.0), np.maximum(np.abs(dot(e, vo)) - wo, 0.0)
                    c2 = np.minimum(c2, ex * ex + ey * ey)
        over = ~bad & (g <= 0.0)
        c2 = np.where(bad, np.nan, np.where(over, 0.0, c2))
        g = np.where(bad, np.nan, g)
    return (c2, over, g) if gap else (c2, over)


def footprint_rows(tau, xy_a, yaw_a, shape_a, xy_b, yaw_b, shape_b, margin):
    """Host mirror of one uph_footprint_separation_batch query: tau (K,) the sample times, the poses at them, the two shapes and margin = M.  A sample is
    below when the rectangles overlap or c2 < M * M, strictly (a NaN c2 never is); for the minimum a NaN c2 reads +inf and a tie stays with the earlier
    sample.  Returns min_c2, min_t, first_t, last_t (NaN: no such sample) and counts (3,): samples, below, overlapping."""
    tau = np.asarray(tau, dtype=np.float64).reshape(-1)
    M = np.float64(margin)
    if not (np.isfinite(M) and M >= 0.0):
        raise _lib.UnevenHipError("footprint_rows: the margin is negative or not finite")
    if tau.shape[0] == 0:
        return dict(min_c2=np.inf, min_t=np.nan, first_t=np.nan, last_t=np.nan, counts=np.zeros(3, dtype=np.int32))
    c2, over = footprint_clearance2(xy_a, yaw_a, shape_a, xy_b, yaw_b, shape_b)
    with np.errstate(invalid="ignore"):
        below = np.nonzero(over | (c2 < M * M))[0]
    key = np.where(np.isnan(c2), np.inf, c2)
    j = int(np.argmin(key))                                         # the first occurrence of the minimum
    return dict(min_c2=key[j], min_t=tau[j], first_t=tau[below[0]] if below.size else np.nan, last_t=tau[below[-1]] if below.size else np.nan,
                counts=np.array([tau.shape[0], below.size, np.count_nonzero(over)], dtype=np.int32))


# uph_footprint_check_columns / uph_footprint_check_batch (include/uneven_hip.h): numpy mirrors written from the rule.  Every product and every sum is rounded on
# its own, in the order the header gives; against the device only the sine and the cosine differ.
FOOT_OCC_XY, FOOT_OCC_YAW, FOOT_OUTSIDE, FOOT_ALL = _lib.UPH_FOOT_OCC_XY, _lib.UPH_FOOT_OCC_YAW, _lib.UPH_FOOT_OUTSIDE, _lib.UPH_FOOT_ALL
FOOT_INDEX_MAX = 2.0 ** 30


def footprint_grid(uneven_map):
    """the geometry footprint_cover / footprint_check_rows need of an UnevenMap: origin (3,), res, yaw_res, nx, ny, nyaw, and the rows held (x_off, nx_hold)"""
    nx, ny, nyaw = (int(v) for v in uneven_map.voxel_num)
    x_off = 0 if uneven_map.tile is None else uneven_map.tile[0]
    return dict(origin=np.asarray(uneven_map.map_origin, dtype=np.float64).copy(), res=float(uneven_map.xy_resolution), yaw_res=float(uneven_map.yaw_resolution),
                nx=nx, ny=ny, nyaw=nyaw, x_off=x_off, nx_hold=int(uneven_map.rows_held))


def _inflated(shape, margin, who):
    f, r, h = _shapes(shape, 1, who)[0]
    m = np.float64(margin)
    if not (np.isfinite(m) and m >= 0.0):
        raise _lib.UnevenHipError(who + ": the margin is negative or not finite")
    return 0.5 * (f + r) + m, 0.5 * (f - r), h + m


def footprint_check_columns(shape, margin, res):
    """Host mirror of uph_footprint_check_columns for one shape: the bound on the columns of one sample's enumeration box, side * side with
    side = floor(2 hypot(hl', w') (1 + 2^-40) / res) + 4 (saturating at 2^62)."""
    hl, _, w = _inflated(shape, margin, "footprint_check_columns")
    reach = np.hypot(hl, w) * (1.0 + 2.0 ** -40)
    if not np.isfinite(reach):
        raise _lib.UnevenHipError("footprint_check_columns: the reach is not finite")
    side = np.floor(2.0 * reach / np.float64(res)) + 4.0
    return int(side) ** 2 if side < 2.0 ** 31 else 1 << 62


def footprint_cover(pose, yawn, shape, margin, grid, pad=1):
    """Host mirror of the footprint check's cover rule at n poses: pose (n, 3) = X, Y, psi (traj_states' columns 0, 1 and 9), yawn (n,) the normalised yaw
    (column 6), shape = (front, rear, half_width) inflated by margin, grid = footprint_grid(map).  For every pose the S columns of one common box around the
    rectangle's hull with `pad` columns of pad (at least the kernel's one): ix, iy (n, S), their gap g = max(|(P - C) . u| - hl', |(P - C) . v| - w') (n, S)
    -- a column is covered iff g <= 0 or it is the point's --, point (n, 2) the point's own column, iw (n,) the yaw bin and ok (n,): False for a degenerate
    pose (a value not finite or an index at or above 2^30), which covers nothing; its rows hold zeros and g = +inf."""
    p = np.asarray(pose, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    wn = np.ascontiguousarray(np.broadcast_to(np.asarray(yawn, dtype=np.float64), (n,)))
    hl, o, w = _inflated(shape, margin, "footprint_cover")
    org, res = np.asarray(grid["origin"], dtype=np.float64), np.float64(grid["res"])
    inv, yinv = 1.0 / res, 1.0 / np.float64(grid["yaw_res"])
    with np.errstate(over="ignore", invalid="ignore"):
        X, Y, psi = p[:, 0], p[:, 1], p[:, 2]
        fp = np.stack([np.floor((X - org[0]) * inv), np.floor((Y - org[1]) * inv), np.floor((wn - org[2]) * yinv)], axis=1)
        ok = np.isfinite(p).all(axis=1) & np.isfinite(wn) & (np.abs(fp) < FOOT_INDEX_MAX).all(axis=1)       # (a NaN index compares false)
        X, Y, psi, fp = np.where(ok, X, 0.0), np.where(ok, Y, 0.0), np.where(ok, psi, 0.0), np.where(ok[:, None], fp, 0.0)
        c, s = np.cos(psi), np.sin(psi)
        Cx, Cy = X + o * c, Y + o * s
        ex, ey = hl * np.abs(c) + w * np.abs(s), hl * np.abs(s) + w * np.abs(c)
        x0, x1 = np.floor(((Cx - ex) - org[0]) * inv) - pad, np.floor(((Cx + ex) - org[0]) * inv) + pad
        y0, y1 = np.floor(((Cy - ey) - org[1]) * inv) - pad, np.floor(((Cy + ey) - org[1]) * inv) + pad
    point, iw = fp[:, :2].astype(np.int64), fp[:, 2].astype(np.int64)
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    sx, sy = (int((x1.astype(np.int64) - x0).max()) + 1, int((y1.astype(np.int64) - y0).max()) + 1) if n else (0, 0)
    ix = np.repeat(x0[:, None] + np.arange(sx)[None, :], sy, axis=1)                  # (n, sx * sy), iy fastest
    iy = np.tile(y0[:, None] + np.arange(sy)[None, :], (1, sx))
    Px, Py = org[0] + (ix + 0.5) * res, org[1] + (iy + 0.5) * res
    dx, dy = Px - Cx[:, None], Py - Cy[:, None]
    c, s = c[:, None], s[:, None]
    g = np.maximum(np.abs(dx * c + dy * s) - hl, np.abs(dx * (-s) + dy * c) - w)
    g = np.where(ok[:, None], g, np.inf)
    return dict(ix=np.where(ok[:, None], ix, 0), iy=np.where(ok[:, None], iy, 0), g=g, point=point, iw=np.where(ok, iw, -1), ok=ok)


def _foot_reduce(t, ok, layers, kinds, cov, ix, iy):
    """one version (surely / possibly) of a footprint check query's outputs from its samples' covered columns cov (n, S) and their kinds (n, S)"""
    n = t.shape[0]
    hitcol = cov & ((kinds & layers) != 0)
    has = lambda bit: (cov & ((kinds & bit) != 0)).any(axis=1) if n else np.zeros(0, dtype=bool)
    kind = [has(FOOT_OCC_XY), has(FOOT_OCC_YAW), has(FOOT_OUTSIDE) | ~ok]
    m = (kind[0] * FOOT_OCC_XY + kind[1] * FOOT_OCC_YAW + kind[2] * FOOT_OUTSIDE) & layers
    hit = m != 0
    at = np.nonzero(hit)[0]
    out = dict(first_t=np.nan, last_t=np.nan, first_mask=0, first_cell=np.array([-1, -1], dtype=np.int32), hit=hit, hitcol=hitcol,
               counts=np.array([n, at.size] + [int(np.count_nonzero(k)) for k in kind], dtype=np.int32),
               cells=np.array([np.count_nonzero(cov), np.count_nonzero(hitcol)], dtype=np.int64))
    if at.size:
        j = at[0]
        out["first_t"], out["last_t"], out["first_mask"] = t[j], t[at[-1]], int(m[j])
        k = np.nonzero(hitcol[j])[0]
        if k.size:
            out["first_cell"] = np.array(min(zip(ix[j, k].tolist(), iy[j, k].tolist())), dtype=np.int32)
    return out


def footprint_check_rows(t, poses, yawn, shape, margin, grid, occ, occ_r2, layers=FOOT_ALL, tol=0.0, pad=1):
    """Host mirror of one uph_footprint_check_batch query, written from the rule: t (n,) the window's sample times, poses (n, 3) = X, Y, psi and yawn (n,) the
    states there (traj_states' columns 0, 1, 9 and 6), the shape inflated by margin, grid = footprint_grid(map), occ (nx_hold * ny * nyaw) and occ_r2
    (nx_hold * ny) the map's occupancy bytes, layers a non-empty subset of FOOT_ALL.  A column whose centre has the gap g of footprint_cover is SURELY covered
    when g < -tol (tol = 0: when g <= 0, the rule itself) and POSSIBLY covered when g <= tol; the point's own column is both.  Returns dict(sure=..., poss=...):
    each the query's outputs first_t, last_t, first_mask, first_cell (2,), counts (5,), cells (2,) under that reading, with hit (n,) the samples that are hits
    and hitcol (n, S) the hit columns; and cover = footprint_cover's dict (ix, iy index hitcol's columns)."""
    layers = int(layers)
    if not 1 <= layers <= FOOT_ALL:
        raise _lib.UnevenHipError("footprint_check_rows: layers must be a non-empty subset of FOOT_ALL")
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    cv = footprint_cover(np.asarray(poses, dtype=np.float64).reshape(-1, 3), yawn, shape, margin, grid, pad=pad)
    ix, iy, g, ok, iw = cv["ix"], cv["iy"], cv["g"], cv["ok"], cv["iw"]
    nx, ny, nyaw, x_off, nx_hold = (int(grid[k]) for k in ("nx", "ny", "nyaw", "x_off", "nx_hold"))
    occ, occ_r2 = np.asarray(occ).reshape(nx_hold, ny, nyaw), np.asarray(occ_r2).reshape(nx_hold, ny)
    ixh = ix - x_off
    inside = (ix >= 0) & (iy >= 0) & (ix <= nx - 1) & (iy <= ny - 1) & (ixh >= 0) & (ixh <= nx_hold - 1) & ((iw >= 0) & (iw <= nyaw - 1))[:, None]
    a, b, w = np.where(inside, ixh, 0), np.where(inside, iy, 0), np.broadcast_to(np.clip(iw, 0, nyaw - 1)[:, None], ix.shape)
    kinds = np.where(inside, (occ_r2[a, b] != 0) * FOOT_OCC_XY + (occ[a, b, w] != 0) * FOOT_OCC_YAW, FOOT_OUTSIDE)
    is_point = (ix == cv["point"][:, :1]) & (iy == cv["point"][:, 1:]) & ok[:, None]
    sure = is_point | ((g < -tol) if tol > 0.0 else (g <= 0.0))
    poss = is_point | (g <= tol)
    return dict(sure=_foot_reduce(t, ok, layers, kinds, sure, ix, iy), poss=_foot_reduce(t, ok, layers, kinds, poss, ix, iy), cover=cv)


# uph_delay_times / uph_delay_levels / uph_delays_batch (include/uneven_hip.h): numpy mirrors written from the rule
def delay_times(delay0, delay_step, D):
    """Host mirror of the table of start delays: delta_j = delay0 + j * delay_step (the product rounded, then the sum) for 0 <= j < D.  Raises for
    what the library refuses."""
    delay0, delay_step, D = float(delay0), float(delay_step), int(D)
    if not (np.isfinite(delay0) and np.isfinite(delay_step) and delay_step > 0.0 and D >= 1):
        raise _lib.UnevenHipError("delay_times: delay0 must be finite, delay_step positive and finite and D at least 1")
    if D > _lib.DELAY_MAX:
        raise _lib.UnevenHipError("delay_times: more than 4096 delays")
    with np.errstate(over="ignore"):
        p = np.arange(D, dtype=np.float64) * delay_step
        return delay0 + p


def delay_levels(pairs, n):
    """Host mirror of uph_delay_levels: the level of each of n vehicles among pairs (m, 2), i < j: 0 for a vehicle without a smaller partner, else
    1 + the largest level of its smaller partners.  The vehicles of one level do not depend on each other's choice."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.shape[0] and not ((0 <= pairs[:, 0]) & (pairs[:, 0] < pairs[:, 1]) & (pairs[:, 1] < n)).all():
        raise _lib.UnevenHipError("delay_levels: a pair does not have 0 <= i < j < n")
    level = np.zeros(n, dtype=np.int32)
    for j, i in sorted(map(tuple, pairs[:, ::-1].tolist())):        # by the larger index j: the levels of its smaller partners i are final
        level[j] = max(level[j], level[i] + 1)
    return level


def delay_schedule(sweep, pairs, n, n_delays=None, order=None):
    """Host mirror of uph_delays_batch's schedule, the sequential greedy: vehicles 0 .. n - 1 in priority order, pairs (m, 2) the kept pairs h < i.
    sweep(h, at_h, i) returns below (D,) of vehicle i swept against vehicle h standing at delay at_h = max(choice[h], 0) of the table; n_delays (n,)
    limits the delays a vehicle may use (None: all).  choice[i] is the smallest j < n_delays[i] with below == 0 against every partner h < i (0 without
    one); -1 when there is none -- the vehicle then counts at delay 0 for those behind it -- with blocker[i] the smallest h below at delay 0 (-1
    otherwise).  order: the sequence in which the vehicles are placed (None: 0 .. n - 1); every partner ahead must have been placed before."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ahead = [[] for _ in range(n)]
    for h, i in sorted(map(tuple, pairs.tolist())):
        ahead[i].append(h)
    choice, blocker = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    placed = np.zeros(n, dtype=bool)
    for i in (range(n) if order is None else order):
        assert all(placed[h] for h in ahead[i]), "delay_schedule: a vehicle ahead of %d is not placed yet" % i
        placed[i] = True
        if not ahead[i]:
            continue
        below = np.stack([np.asarray(sweep(h, max(int(choice[h]), 0), i)) for h in ahead[i]])
        nd = below.shape[1] if n_delays is None else int(n_delays[i])
        clear = np.nonzero((below[:, :nd] == 0).all(axis=0))[0]
        if clear.size:
            choice[i] = clear[0]
        else:
            choice[i] = -1
            blocker[i] = ahead[i][int(np.nonzero(below[:, 0] > 0)[0][0])]
    return dict(choice=choice, blocker=blocker)


class ALMTrajOpt:
    def __init__(self, uneven_map=None, params=None):
        self.L = _lib.load()
        q = dict(HILL_OPT_PARAMS)
        if params:
            q.update(params)
        for k, v in q.items():            # public parameter members, like the reference
            setattr(self, k, v)
        self._pnames = list(q.keys())
        self.h = None
        self.uneven_map = None
        self.in_opt = False
        self._B = 0
        self._sizes = []
        self._last = []
        if uneven_map is not None:
            self.setEnvironment(uneven_map)

    def __del__(self):
        try:
            if self.h:
                self.L.uph_ctx_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def setEnvironment(self, env):
        """ALMTrajOpt::setEnvironment (alm_traj_opt.h:127-130); creates the device context with the current parameter members."""
        self.uneven_map = env
        if self.h:
            self.L.uph_ctx_destroy(self.h)
            self.h = None
        self._clear_layer = None          # (a clearance term lived on the old context; released behind it: the layer cannot be closed while named)
        p = _lib.OptParams(**{k: (int(getattr(self, k)) if k in _INT_FIELDS else float(getattr(self, k))) for k in self._pnames})
        h = C.c_void_p()
        _lib.check(self.L.uph_ctx_create(env.h, C.byref(p), C.byref(h)), "uph_ctx_create")
        self.h = h

    def set_lanes(self, lanes):
        """64 / 128 / 256 lanes (one / two / four waves) per trajectory, 0 = automatic"""
        _lib.check(self.L.uph_ctx_set_lanes(self.h, int(lanes)), "uph_ctx_set_lanes")

    def set_xcd_locality(self, group):
        """experiment knob: per-XCD L2 locality of the launch order (uph_ctx_set_xcd_locality); takes effect at the next upload"""
        _lib.check(self.L.uph_ctx_set_xcd_locality(self.h, int(group)), "uph_ctx_set_xcd_locality")

    def set_wps(self, wps):
        _lib.check(self.L.uph_ctx_set_wps(self.h, int(wps)), "uph_ctx_set_wps")

    def set_sample_precision(self, bits):
        """32: fp32 arithmetic in the sample phase of the objective (configs[4] "fp32"; no 1e-9 parity with the double-only reference); 64: default"""
        _lib.check(self.L.uph_ctx_set_sample_precision(self.h, int(bits)), "uph_ctx_set_sample_precision")

    def set_clearance_term(self, layer, d_safe=0.0, weight=0.0):
        """The clearance term of the objective (uph_ctx_set_clearance_term): every sample closer than d_safe metres to an obstacle of the
        ClearanceLayer `layer` (polarity CLEAR_TO_OCCUPIED, of this context's map, fresh) adds weight * step * scale_fx * (d_safe - c)^2 to the cost.  It
        persists on the context (until setEnvironment makes a new one) and applies to every later evaluation, solve and penalty_batch, whoever uploaded
        the batch; layer = None switches it off.  The layer cannot be closed while the context names it.  See clearance.clearance_term_rows for the rule."""
        _lib.check(self.L.uph_ctx_set_clearance_term(self.h, None if layer is None else layer.h, float(d_safe), float(weight)), "uph_ctx_set_clearance_term")
        self._clear_layer = layer

    def clearance_term(self):
        """(layer, d_safe, weight) of the clearance term; layer is None when it is off"""
        h, d, w = C.c_void_p(), C.c_double(0), C.c_double(0)
        _lib.check(self.L.uph_ctx_clearance_term(self.h, C.byref(h), C.byref(d), C.byref(w)), "uph_ctx_clearance_term")
        return (getattr(self, "_clear_layer", None) if h.value else None), d.value, w.value

    def set_rho(self, rho):
        _lib.check(self.L.uph_ctx_set_rho(self.h, float(rho)), "uph_ctx_set_rho")

    def set_trial_abandon(self, on):
        """line-search trials stop once their Armijo rejection is certain (default on; uph_ctx_set_trial_abandon): off evaluates every trial in full"""
        _lib.check(self.L.uph_ctx_set_trial_abandon(self.h, 1 if on else 0), "uph_ctx_set_trial_abandon")

    def get_rho(self):
        r = C.c_double(0)
        _lib.check(self.L.uph_ctx_get_rho(self.h, C.byref(r)), "uph_ctx_get_rho")
        return r.value

    # ---- batch plumbing ---------------------------------------------------------------------------------------------
    def _make_problems(self, probs):
        arr, keep, self._sizes = pack_problems(probs, int(self.int_K), with_sizes=True)
        return arr, keep

    def upload(self, probs):
        arr, keep = self._make_problems(probs)
        self._B = 0
        _lib.check(self.L.uph_batch_upload(self.h, len(probs), arr), "uph_batch_upload")
        self._B = len(probs)
        self._trace_cap_up = getattr(self, "_trace_cap", 0)

    def solve(self):
        """Kernel only (inputs already resident in HBM)."""
        _lib.check(self.L.uph_batch_solve(self.h), "uph_batch_solve")

    def solve_async(self):
        """enqueue the solve on this context's stream and return (uph_batch_solve_async); pair with wait()"""
        _lib.check(self.L.uph_batch_solve_async(self.h), "uph_batch_solve_async")

    def wait(self):
        _lib.check(self.L.uph_batch_wait(self.h), "uph_batch_wait")

    def stats(self):
        ms = C.c_double(0)
        v = [C.c_int64(0) for _ in range(4)]
        _lib.check(self.L.uph_batch_stats(self.h, C.byref(ms), *[C.byref(x) for x in v]), "uph_batch_stats")
        pm = C.c_double(0)
        _lib.check(self.L.uph_batch_prepare_ms(self.h, C.byref(pm)), "uph_batch_prepare_ms")
        ab = (C.c_int64 * 5)()
        _lib.check(self.L.uph_batch_abandon_stats(self.h, ab), "uph_batch_abandon_stats")
        return dict(kernel_ms=ms.value, prepare_ms=pm.value, evals=v[0].value, sample_evals=v[1].value, lbfgs_iters=v[2].value, hist_bytes=v[3].value,
                    ls_rejected=ab[0], ls_guarded=ab[1], ls_abandoned=ab[2], chunks_skipped=ab[3], adjoints_skipped=ab[4])

    def cycles(self):
        """(B,16) shader-clock cycles per phase of the last solve (generate, samples, scatter, adjoint, two-loop, scaling, total, ...)"""
        out = np.zeros((max(0, self.L.uph_batch_count(self.h)), 16), dtype=np.int64)      # (sized from the context, not from this wrapper's bookkeeping)
        _lib.check(self.L.uph_batch_cycles(self.h, out.ctypes.data_as(C.POINTER(C.c_longlong))), "uph_batch_cycles")
        return out

    def origin(self):
        """caller's index of every problem this context holds (identity unless the batch came through optimize_batch_multi)"""
        idx = np.zeros(max(0, self.L.uph_batch_count(self.h)), dtype=np.int32)
        _lib.check(self.L.uph_batch_origin(self.h, _ip(idx)), "uph_batch_origin")
        return idx

    def download(self, full=True):
        """full = False pulls only x and the coefficients (what a planner reads); the per-sample arrays then stay on the device"""
        res, bufs = self._result_array(self._sizes, full)
        _lib.check(self.L.uph_batch_download(self.h, res), "uph_batch_download")
        self._last = self._collect(res, bufs)
        return self._last

    def optimize_batch(self, probs):
        self.upload(probs)
        self.solve()
        return self.download()

    def _result_array(self, sizes, full):
        """uph_result array with caller-owned output arrays: full = every array, else what a planner pulls (x, coefficients)"""
        res = (_lib.Result * len(sizes))()
        bufs = []
        for i, sz in enumerate(sizes):
            b = dict(x=np.zeros(sz["n"]), c_xy=np.zeros((6 * sz["Nxy"], 2)), c_yaw=np.zeros(6 * sz["Nyaw"]))
            r = res[i]
            r.x_final, r.c_xy, r.c_yaw = _dp(b["x"]), _dp(b["c_xy"]), _dp(b["c_yaw"])
            if full:
                b.update(hx=np.zeros(sz["S"]), gx=np.zeros(6 * sz["S"]), lam=np.zeros(sz["S"]), mu=np.zeros(6 * sz["S"]), scale_cx=np.zeros(7 * sz["S"]))
                r.hx, r.gx, r.lambda_, r.mu, r.scale_cx = _dp(b["hx"]), _dp(b["gx"]), _dp(b["lam"]), _dp(b["mu"]), _dp(b["scale_cx"])
            bufs.append(b)
        return res, bufs

    @staticmethod
    def _collect(res, bufs):
        out = []
        for i, b in enumerate(bufs):
            r = res[i]
            b.update(ret=r.ret_code, alm_iters=r.alm_iters, lbfgs_iters=r.lbfgs_iters, evals=r.evals, last_lbfgs_ret=r.last_lbfgs_ret,
                     cost=r.cost, jerk_cost=r.jerk_cost, T_xy=r.piece_T_xy, T_yaw=r.piece_T_yaw, rho_final=r.rho_final, scale_fx=r.scale_fx)
            out.append(b)
        return out

    def prepare_boundary(self, probs, full=False):
        arr, keep = self._make_problems(probs)
        res, bufs = self._result_array(self._sizes, full)
        return arr, keep, res, bufs

    def optimize_boundary(self, probs, full=False, prepared=None):
        """ONE uph_optimize_batch call -- upload + solve + download, the reference's synchronous contract (alm_traj_opt.h:92-98, result
        pulled afterwards :165-168) -- with pageable host arrays.  prepared = prepare_boundary(probs) keeps the ctypes packing out of a
        timed region."""
        arr, keep, res, bufs = prepared if prepared is not None else self.prepare_boundary(probs, full)
        self._B = 0
        import time
        t0 = time.perf_counter()
        rc = self.L.uph_optimize_batch(self.h, len(probs), arr, res)
        self.last_boundary_s = time.perf_counter() - t0
        _lib.check(rc, "uph_optimize_batch")
        self._B = len(probs)
        self._last = self._collect(res, bufs)
        return self._last

    @staticmethod
    def optimize_batch_multi(opts, probs, full=False):
        """uph_optimize_batch_multi: one batch over the contexts `opts` (one per device), results in the caller's order"""
        lead = opts[0]
        arr, keep = lead._make_problems(probs)
        sizes = list(lead._sizes)
        res, bufs = lead._result_array(sizes, full)
        hs = (C.c_void_p * len(opts))(*[o.h for o in opts])
        for o in opts:                     # whatever happens below, no wrapper keeps describing a batch its context no longer holds
            o._B, o._sizes, o._last = 0, [], None
        _lib.check(lead.L.uph_optimize_batch_multi(hs, len(opts), len(probs), arr, res), "uph_optimize_batch_multi")
        out = ALMTrajOpt._collect(res, bufs)
        # every context now holds its share: bring the wrappers' bookkeeping in step with the C contexts (sizes in share order)
        for o in opts:
            n = o.L.uph_batch_count(o.h)
            if n <= 0:
                continue
            idx = o.origin()
            o._B, o._sizes, o._last = int(n), [sizes[i] for i in idx], [out[i] for i in idx]
        return out

    # ---- goals -> trajectories in one call (uph_plan_upload) ---------------------------------------------------------
    def plan_goals_upload(self, kino, starts, goals, path_cap=0, **manager_params):
        """PlanManager::rcvWpsCallBack's chain (plan_manager.cpp:43-134) for a batch of goals with the paths kept on the device: the search of
        `kino` (a KinoAstar on the same map), a second search with room for every clipped path, PlanManager's resampling stage on the device
        (manager_params: resample.MANAGER_PARAMS keys, test_mode included) and the upload of the found goals' problems, in goal order.  Then
        solve() / solve_async() + wait() and download() work as after upload().  Returns dict of [B] arrays: status (UPH_KINO_*), traj_of (index in
        the resident batch, -1 without a path), n_inner_xy, n_inner_yaw.  A batch in which no goal has a path leaves the context empty (no raise);
        every failure of the call raises."""
        mp = self._manager_params("plan_goals", manager_params)
        s = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        if s.shape != g.shape or s.shape[0] == 0:
            raise _lib.UnevenHipError("plan_goals: starts and goals must be the same non-empty (B, 3)")
        B = s.shape[0]
        st, to = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
        nx, ny = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        self._B, self._sizes, self._last = 0, [], []
        rc = self.L.uph_plan_upload(kino.h, self.h, C.byref(mp), B, _dp(s), _dp(g), int(path_cap), _ip(st), _ip(to), _ip(nx), _ip(ny))
        return self._planned(rc, dict(status=st, traj_of=to, n_inner_xy=nx, n_inner_yaw=ny), "uph_plan_upload")

    @staticmethod
    def _manager_params(who, manager_params):
        from .resample import MANAGER_PARAMS
        unknown = set(manager_params) - set(MANAGER_PARAMS)
        if unknown:
            raise TypeError("%s: unknown manager parameter(s) %s" % (who, sorted(unknown)))
        mk = dict(MANAGER_PARAMS)
        mk.update(manager_params)
        return _lib.ManagerParams(**{k: (int(bool(v)) if k == "test_mode" else float(v)) for k, v in mk.items()})

    def _planned(self, rc, plan, who):
        """the outputs of uph_plan_upload / uph_replan_upload / uph_refine_upload -> the resident batch's sizes, or a raise"""
        st, to, nx, ny = plan["status"], plan["traj_of"], plan["n_inner_xy"], plan["n_inner_yaw"]
        self.last_plan = plan
        # "no goal produced a path" is the one UPH_ERR_INVALID returned with the outputs written (statuses no longer the -1 they were filled with)
        # and no UPH_KINO_OK among them: an empty batch, not an error.  Every other return code -- a HIP failure in the search included -- raises.
        no_path = rc == _lib.UPH_ERR_INVALID and (st >= 0).all() and not (st == _lib.UPH_KINO_OK).any()
        if rc != 0 and not no_path:
            _lib.check(rc, who)
        found = np.nonzero(to >= 0)[0]
        K1 = int(self.int_K) + 1
        self._sizes = [dict(Nxy=int(nx[b]) + 1, Nyaw=int(ny[b]) + 1, n=2 * int(nx[b]) + int(ny[b]) + 1, S=(int(nx[b]) + 1) * K1) for b in found]
        self._B = len(found)
        self._trace_cap_up = getattr(self, "_trace_cap", 0)
        return plan

    def plan_goals(self, kino, starts, goals, full=False, path_cap=0, **manager_params):
        """goals in, trajectories out (plan_goals_upload + solve + download): one dict per goal with its search `status`; a goal with a path also
        carries `traj_of` and the result dict optimize_batch returns.  The batch stays resident: rollout(), getMaxVxAxAyCurAttSig() and origin()
        (= the goal index of each resident trajectory) work afterwards."""
        return self._solve_planned(self.plan_goals_upload(kino, starts, goals, path_cap=path_cap, **manager_params), full)

    def _solve_planned(self, plan, full):
        out = [dict(status=int(v)) for v in plan["status"]]
        if self._B == 0:
            return out
        self.solve()
        found = np.nonzero(plan["traj_of"] >= 0)[0]
        res = self._download_block(plan["n_inner_xy"][found], plan["n_inner_yaw"][found], full)
        for j, b in enumerate(found):
            r = dict(res[j])
            r.update(status=int(plan["status"][b]), traj_of=j)
            out[b] = r
        return out

    # ---- re-plan from states on resident trajectories (uph_replan_upload) ------------------------------------------
    def replan_goals_upload(self, kino, src, src_traj, t_switch, goals=None, path_cap=0, **manager_params):
        """plan_goals_upload for a vehicle in motion: query q starts where trajectory src_traj[q] of `src`'s resident batch (an ALMTrajOpt on the same
        map, self included) is at t_switch[q] (the rollout's clock, clamped to [0, duration]), with that trajectory's velocity, acceleration, yaw rate and
        yaw acceleration as the new problem's start boundary; goals (B, 3), or None: each source problem's end pose.  The batch is uploaded to self.
        Returns plan_goals_upload's dict plus switch_states (B, 9): x, y, dx, dy, ddx, ddy, yaw (normSO2), dyaw, ddyaw."""
        mp = self._manager_params("replan_goals", manager_params)
        tr = np.ascontiguousarray(src_traj, dtype=np.int32).reshape(-1)
        ts = np.ascontiguousarray(t_switch, dtype=np.float64).reshape(-1)
        B = tr.shape[0]
        if B == 0 or ts.shape[0] != B:
            raise _lib.UnevenHipError("replan_goals: src_traj and t_switch must be the same non-empty length")
        g = None
        if goals is not None:
            g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
            if g.shape[0] != B:
                raise _lib.UnevenHipError("replan_goals: goals must be (B, 3)")
        st, to = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
        nx, ny = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        sw = np.full((B, 9), np.nan)
        rc = self.L.uph_replan_upload(kino.h, src.h, self.h, C.byref(mp), B, _ip(tr), _dp(ts), None if g is None else _dp(g), int(path_cap), _dp(sw),
                                      _ip(st), _ip(to), _ip(nx), _ip(ny))
        if rc not in (0, _lib.UPH_ERR_INVALID):        # a failure past the refusals (which leave self's batch as it was): no batch is resident
            self._B, self._sizes, self._last = 0, [], []
        return self._planned(rc, dict(status=st, traj_of=to, n_inner_xy=nx, n_inner_yaw=ny, switch_states=sw), "uph_replan_upload")

    def replan_goals(self, kino, src, src_traj, t_switch, goals=None, full=False, path_cap=0, **manager_params):
        """replan_goals_upload + solve + download, as plan_goals: one dict per query with its search `status` (and `traj_of` + the result dict when
        it has a path); the new batch stays resident on self.  The switch states are in self.last_plan["switch_states"]."""
        return self._solve_planned(self.replan_goals_upload(kino, src, src_traj, t_switch, goals=goals, path_cap=path_cap, **manager_params), full)

    # ---- resident trajectories at given times (uph_traj_states), their tails refined without a search (uph_refine_upload) --------------------------
    def traj_states(self, traj, t):
        """resident trajectory traj[q] at t[q] seconds from its start (clamped to [0, duration], the rollout's clock), evaluated on the device: (n, 10)
        rows x, y (map coordinates), dx, dy, ddx, ddy, yaw (normSO2), dyaw, ddyaw -- replan_goals_upload's switch states -- and the raw yaw"""
        tr = np.ascontiguousarray(traj, dtype=np.int32).reshape(-1)
        ts = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
        n = tr.shape[0]
        if n == 0 or ts.shape[0] != n:
            raise _lib.UnevenHipError("traj_states: traj and t must be the same non-empty length")
        out = np.zeros((n, _lib.TRAJ_STATE_COLS))
        _lib.check(self.L.uph_traj_states(self.h, n, _ip(tr), _dp(ts), _dp(out)), "uph_traj_states")
        return out

    def refine_upload(self, src, src_traj, t_switch):
        """the rest of trajectory src_traj[q] of `src`'s resident batch (an ALMTrajOpt on the same map, self included) after t_switch[q] as a new problem
        on self, without a search: start = its state at the switch time, end = its problem's uploaded end boundary, way-points = the trajectory itself
        (uph_refine_upload).  Returns plan_goals_upload's dict -- status UPH_KINO_OK, or UPH_REFINE_AT_END for a switch at or past the end (not
        uploaded) -- plus switch_states (B, 10) in traj_states' columns.  A batch in which every query is at its end leaves self empty (no raise)."""
        tr = np.ascontiguousarray(src_traj, dtype=np.int32).reshape(-1)
        ts = np.ascontiguousarray(t_switch, dtype=np.float64).reshape(-1)
        B = tr.shape[0]
        if B == 0 or ts.shape[0] != B:
            raise _lib.UnevenHipError("refine: src_traj and t_switch must be the same non-empty length")
        st, to = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
        nx, ny = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        sw = np.full((B, _lib.TRAJ_STATE_COLS), np.nan)
        rc = self.L.uph_refine_upload(src.h, self.h, B, _ip(tr), _dp(ts), _dp(sw), _ip(st), _ip(to), _ip(nx), _ip(ny))
        if rc != 0 and (rc != _lib.UPH_ERR_INVALID or (st >= 0).any()):      # past the refusals (which leave self's batch as it was): no batch is resident
            self._B, self._sizes, self._last = 0, [], []
        return self._planned(rc, dict(status=st, traj_of=to, n_inner_xy=nx, n_inner_yaw=ny, switch_states=sw), "uph_refine_upload")

    def refine(self, src, src_traj, t_switch, full=False):
        """refine_upload + solve + download, as replan_goals: one dict per query with its `status` (and `traj_of` + the result dict when it was
        uploaded); the new batch stays resident on self.  The switch states are in self.last_plan["switch_states"]."""
        return self._solve_planned(self.refine_upload(src, src_traj, t_switch), full)

    def _download_block(self, nxy, nyw, full):
        """download() for a whole resident batch into a few contiguous arrays: the uph_result array is a numpy record array whose pointer fields
        are filled at once (no per-problem ctypes work), every result dict holds views of the blocks.  Same dicts as download(full)."""
        nxy, nyw = np.asarray(nxy, dtype=np.int64), np.asarray(nyw, dtype=np.int64)
        F = nxy.shape[0]
        sizes = {"x": 2 * nxy + nyw + 1, "c_xy": 12 * (nxy + 1), "c_yaw": 6 * (nyw + 1)}
        if full:
            S = (nxy + 1) * (int(self.int_K) + 1)
            sizes.update(hx=S, gx=6 * S, lam=S, mu=6 * S, scale_cx=7 * S)
        field = dict(x="x_final", c_xy="c_xy", c_yaw="c_yaw", hx="hx", gx="gx", lam="lambda_", mu="mu", scale_cx="scale_cx")
        R_ = _lib.Result
        fmt = {C.c_int32: "<i4", C.c_double: "<f8"}
        dt = np.dtype(dict(names=[f for f, _ in R_._fields_], formats=[fmt.get(t, "<u8") for _, t in R_._fields_],
                           offsets=[getattr(R_, f).offset for f, _ in R_._fields_], itemsize=C.sizeof(R_)))
        rec = np.zeros(F, dtype=dt)
        blocks, offs = {}, {}
        for k, n in sizes.items():
            offs[k] = np.concatenate([[0], np.cumsum(n)])
            blocks[k] = np.zeros(max(1, int(offs[k][-1])))
            rec[field[k]] = blocks[k].ctypes.data + 8 * offs[k][:-1]
        _lib.check(self.L.uph_batch_download(self.h, rec.ctypes.data_as(C.POINTER(R_))), "uph_batch_download")
        sc = {k: rec[f].tolist() for k, f in (("ret", "ret_code"), ("alm_iters", "alm_iters"), ("lbfgs_iters", "lbfgs_iters"), ("evals", "evals"),
                                              ("last_lbfgs_ret", "last_lbfgs_ret"), ("cost", "cost"), ("jerk_cost", "jerk_cost"), ("T_xy", "piece_T_xy"),
                                              ("T_yaw", "piece_T_yaw"), ("rho_final", "rho_final"), ("scale_fx", "scale_fx"))}
        ol = {k: o.tolist() for k, o in offs.items()}
        out = []
        for j in range(F):
            d = {k: blocks[k][ol[k][j]:ol[k][j + 1]] for k in sizes}
            d["c_xy"] = d["c_xy"].reshape(-1, 2)
            d.update({k: v[j] for k, v in sc.items()})
            out.append(d)
        self._last = out
        return out

    def plan_staged(self, cap_xy=_lib.PLAN_STAGE_XY, cap_yaw=_lib.PLAN_STAGE_YAW):
        """test hook (uph_plan_staged): the resident problems of the last plan_goals_upload as the device staged them, resident order, in
        resample.resample_batch's dict layout plus the counts; complete = False marks a problem with more way-points than the staging holds
        (UPH_MAX_PIECE_* - 1: an UNSUPPORTED slot) or cap_*: its way-point arrays are then the first ones only"""
        B = max(0, self.L.uph_batch_count(self.h))
        ixy, exy, iyw, eyw = np.zeros((B, 6)), np.zeros((B, 6)), np.zeros((B, 3)), np.zeros((B, 3))
        oxy, oyw = np.zeros((B, 2 * max(cap_xy, 1))), np.zeros((B, max(cap_yaw, 1)))
        nxy, nyw, tt = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B)
        rc = self.L.uph_plan_staged(self.h, int(cap_xy), int(cap_yaw), _dp(ixy), _dp(exy), _dp(iyw), _dp(eyw), _dp(oxy), _dp(oyw), _ip(nxy), _ip(nyw), _dp(tt))
        if rc != _lib.UPH_ERR_LIMIT:      # a problem had more way-points than fit (complete = False below), the rest is written
            _lib.check(rc, "uph_plan_staged")
        kx, ky = min(cap_xy, _lib.PLAN_STAGE_XY), min(cap_yaw, _lib.PLAN_STAGE_YAW)
        return [dict(init_xy=ixy[b].reshape(3, 2).T.copy(), end_xy=exy[b].reshape(3, 2).T.copy(), inner_xy=oxy[b, :2 * min(nxy[b], kx)].reshape(-1, 2).T.copy(),
                     init_yaw=iyw[b].copy(), end_yaw=eyw[b].copy(), inner_yaw=oyw[b, :min(nyw[b], ky)].copy(), total_time=float(tt[b]),
                     n_inner_xy=int(nxy[b]), n_inner_yaw=int(nyw[b]), complete=bool(nxy[b] <= kx and nyw[b] <= ky)) for b in range(B)]

    # ---- the reference's entry point -------------------------------------------------------------------------------
    def optimizeSE2Traj(self, initStateXY, endStateXY, innerPtsXY, initYaw, endYaw, innerPtsYaw, totalTime):
        """ALMTrajOpt::optimizeSE2Traj (alm_traj_opt.h:92-98, alm_traj_opt.cpp:168-278).  Returns 0 / 1 / 2."""
        self.in_opt = True
        try:
            out = self.optimize_batch([dict(init_xy=initStateXY, end_xy=endStateXY, inner_xy=innerPtsXY, init_yaw=initYaw, end_yaw=endYaw,
                                            inner_yaw=innerPtsYaw, total_time=totalTime)])
        finally:
            self.in_opt = False
        return out[0]["ret"]

    def getTraj(self, i=0):
        r = self._last[i]
        return SE2Traj(r["c_xy"], r["c_yaw"], r["T_xy"], r["T_yaw"])

    def getTrajJerkCost(self, i=0):
        return self._last[i]["jerk_cost"]

    def getMaxVxAxAyCurAttSig(self):
        """Batched post-solve report (alm_traj_opt.h:170-229 + getNonHolError): (B,7) max vx, ax, ay, cur, att, sigma, non-hol error."""
        out = np.zeros((max(0, self.L.uph_batch_count(self.h)), 7))      # rows = this context's problems (see origin() after optimize_batch_multi)
        _lib.check(self.L.uph_report_batch(self.h, _dp(out)), "uph_report_batch")
        return out

    # ---- trajectory rollout ------------------------------------------------------------------------------------------
    def rollout_plan(self, dt=0.01, with_end=False):
        """uph_rollout_plan: row offsets [B + 1] of the resident batch (rows = the samples of `for (t = 0; t < total; t += dt)` [+ the end point])"""
        n = max(0, self.L.uph_batch_count(self.h))
        offs = np.zeros(n + 1, dtype=np.int64)
        _lib.check(self.L.uph_rollout_plan(self.h, float(dt), int(bool(with_end)), offs.ctypes.data_as(C.POINTER(C.c_int64))), "uph_rollout_plan")
        return offs

    def rollout(self, dt=0.01, channels=ROLLOUT_ALL, with_end=False, b0=0, b1=None, device=False):
        """The resident trajectories sampled every dt on the device (uph_rollout_batch): returns (offsets, rows).  offsets[b - b0] .. offsets[b + 1 - b0]
        are the rows of trajectory b of [b0, b1); rows [n, ncol] (columns: rollout_columns(channels)), positions in map coordinates.  device = True:
        rows is a torch.float64 tensor on the context's device, written there by uph_rollout_batch_dev."""
        offs_all = self.rollout_plan(dt, with_end)
        B = offs_all.shape[0] - 1
        b1 = B if b1 is None else int(b1)
        b0 = int(b0)
        if not (0 <= b0 <= b1 <= B):
            raise _lib.UnevenHipError("rollout: trajectory range [%d, %d) outside the batch of %d" % (b0, b1, B))
        offs = offs_all[b0:b1 + 1] - offs_all[b0]
        ncol = len(rollout_columns(int(channels)))
        if ncol == 0:
            raise _lib.UnevenHipError("rollout: empty channel mask")
        n = int(offs[-1])
        if device:
            import torch
            rows = torch.empty((n, ncol), dtype=torch.float64, device="cuda:%d" % self.uneven_map.device)
            ptr = C.c_void_p(rows.data_ptr() if n > 0 else 0)
            if n == 0:                    # (a null pointer is refused; nothing is written for an empty range)
                return offs, rows
            _lib.check(self.L.uph_rollout_batch_dev(self.h, float(dt), int(bool(with_end)), int(channels), b0, b1, ptr), "uph_rollout_batch_dev")
            return offs, rows
        rows = np.zeros((n, ncol))
        buf = rows if n > 0 else np.zeros((1, ncol))
        _lib.check(self.L.uph_rollout_batch(self.h, float(dt), int(bool(with_end)), int(channels), b0, b1, _dp(buf)), "uph_rollout_batch")
        return offs, rows

    @staticmethod
    def rollout_multi(opts, dt=0.01, channels=ROLLOUT_ALL, with_end=False):
        """rollout of a batch solved by optimize_batch_multi over the contexts `opts`: (offsets, rows) in the caller's order (uph_batch_origin
        maps each context's rows back, as for the report)"""
        parts = {}
        for o in opts:
            if o.L.uph_batch_count(o.h) <= 0:
                continue
            offs, rows = o.rollout(dt, channels, with_end)
            for k, i in enumerate(o.origin()):
                parts[int(i)] = rows[int(offs[k]):int(offs[k + 1])]
        B = len(parts)
        if sorted(parts) != list(range(B)):
            raise _lib.UnevenHipError("rollout_multi: the contexts do not hold one batch (origins %s)" % sorted(parts)[:8])
        counts = np.array([parts[i].shape[0] for i in range(B)], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        ncol = len(rollout_columns(int(channels)))
        rows = np.concatenate([parts[i] for i in range(B)]) if B else np.zeros((0, ncol))
        return offs, rows.reshape(-1, ncol)

    # ---- resident trajectories against the map as it is now (uph_check_batch) -----------------------------------------------------------------------
    def check_limits(self):
        """the default limits of check(): max_vel, max_acc_lon, max_acc_lat, max_kap, -min_cxi, max_sig of the context's parameters and +inf for the
        non-holonomic error (uph_check_limits)"""
        lim = np.zeros(7)
        _lib.check(self.L.uph_check_limits(self.h, _dp(lim)), "uph_check_limits")
        return lim

    def check(self, traj, t_from=0.0, t_to=None, dt=0.01, with_end=True, limits=None):
        """Reduce, on the device and on the bound map as it is now, the rollout(dt, with_end) samples of resident trajectory traj[q] with t in
        [t_from[q], t_to[q]] (scalars are broadcast; t_to = None: to the end) against `limits` (7 values, None: check_limits()).  Returns a dict of
        arrays over the queries: first_t (NaN: no violation), first_mask (bit k: term k of CHECK_TERMS, bit CHECK_OCC_BIT: occupied or outside the
        map), counts (n, 3: samples, violating, occupied), worst and worst_t (n, 7); see check_rows for the rule."""
        tr, n, tf, tt, _ = self._windows(traj, t_from, t_to, None, 0, "check")
        lim = None if limits is None else np.ascontiguousarray(limits, dtype=np.float64).reshape(7)
        out = dict(first_t=np.full(n, np.nan), first_mask=np.zeros(n, dtype=np.int32), counts=np.zeros((n, 3), dtype=np.int32),
                   worst=np.full((n, 7), -np.inf), worst_t=np.full((n, 7), np.nan))
        _lib.check(self.L.uph_check_batch(self.h, n, _ip(tr), _dp(tf), None if tt is None else _dp(tt), float(dt), int(bool(with_end)),
                                          None if lim is None else _dp(lim), _dp(out["first_t"]), _ip(out["first_mask"]), _ip(out["counts"]),
                                          _dp(out["worst"]), _dp(out["worst_t"])), "uph_check_batch")
        return out

    def _kernel_ms(self, fn_name):
        ms = C.c_double(0)
        _lib.check(getattr(self.L, fn_name)(self.h, C.byref(ms)), fn_name)
        return ms.value

    def check_kernel_ms(self):
        """milliseconds of uph_check_kernel in the last check() (events on the context's stream)"""
        return self._kernel_ms("uph_check_kernel_ms")

    # ---- poses located on resident trajectories, rects crossed by them (uph_locate_batch, uph_within_batch) ---------------------------------------
    def _windows(self, traj, t_from, t_to, rows, width, who):
        """the query arrays check / locate / within pass down: trajectories, broadcast window bounds and (rows not None) the n x width rows"""
        tr = np.ascontiguousarray(traj, dtype=np.int32).reshape(-1)
        n = tr.shape[0]
        if n == 0:
            raise _lib.UnevenHipError(who + ": no query")
        tf = np.ascontiguousarray(np.broadcast_to(np.asarray(t_from, dtype=np.float64), (n,)))
        tt = None if t_to is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t_to, dtype=np.float64), (n,)))
        rw = None if rows is None else np.ascontiguousarray(np.broadcast_to(np.asarray(rows, dtype=np.float64), (n, width)))
        return tr, n, tf, tt, rw

    def locate(self, traj, poses, t_from=0.0, t_to=None, dt=0.01, with_end=True):
        """Locate, on the device, pose poses[q] = (x, y, yaw) in map coordinates on resident trajectory traj[q] among its rollout(dt, with_end) samples
        with t in [t_from[q], t_to[q]] (scalars / one pose are broadcast; t_to = None: to the end): the nearest sample (near_t, near_d2, count), then the
        time t refined between its neighbours where the pose's offset is normal to the velocity (refined = 0: the sample itself was kept), the state
        there (n, 10: traj_states' columns), d2 and err (n, 3) = e_lon, e_lat, e_yaw of the pose against that state.  See locate_rows /
        locate_refine for the rule."""
        tr, n, tf, tt, ps = self._windows(traj, t_from, t_to, poses, 3, "locate")
        out = dict(near_t=np.full(n, np.nan), near_d2=np.full(n, np.inf), count=np.zeros(n, dtype=np.int32), t=np.full(n, np.nan),
                   refined=np.zeros(n, dtype=np.int32), state=np.full((n, _lib.TRAJ_STATE_COLS), np.nan), d2=np.full(n, np.inf), err=np.full((n, 3), np.nan))
        _lib.check(self.L.uph_locate_batch(self.h, n, _ip(tr), _dp(ps), _dp(tf), None if tt is None else _dp(tt), float(dt), int(bool(with_end)),
                                           _dp(out["near_t"]), _dp(out["near_d2"]), _ip(out["count"]), _dp(out["t"]), _ip(out["refined"]), _dp(out["state"]),
                                           _dp(out["d2"]), _dp(out["err"])), "uph_locate_batch")
        return out

    def within(self, traj, rects, t_from=0.0, t_to=None, dt=0.01, with_end=True):
        """Which rollout(dt, with_end) samples of resident trajectory traj[q] with t in [t_from[q], t_to[q]] lie inside the closed rect rects[q] =
        (x0, x1, y0, y1) in map coordinates (one rect is broadcast), on the device: enter_t / leave_t (t of the first / last sample inside, NaN: none)
        and counts (n, 2: samples, inside); see within_rows."""
        tr, n, tf, tt, rc = self._windows(traj, t_from, t_to, rects, 4, "within")
        out = dict(enter_t=np.full(n, np.nan), leave_t=np.full(n, np.nan), counts=np.zeros((n, 2), dtype=np.int32))
        _lib.check(self.L.uph_within_batch(self.h, n, _ip(tr), _dp(rc), _dp(tf), None if tt is None else _dp(tt), float(dt), int(bool(with_end)),
                                           _dp(out["enter_t"]), _dp(out["leave_t"]), _ip(out["counts"])), "uph_within_batch")
        return out

    def locate_kernel_ms(self):
        """milliseconds of the kernel(s) of the last locate() or within(), whichever came last (events on the context's stream)"""
        return self._kernel_ms("uph_locate_kernel_ms")

    # ---- resident trajectories against each other on a common clock (uph_extent_batch, uph_separation_batch, uph_conflicts_batch) ---------------------
    def _clock(self, traj, t_from, t_to, who, **per_query):
        """the query arrays of the common-clock calls: trajectories, the broadcast window bounds and the broadcast per-query values"""
        tr = np.ascontiguousarray(traj, dtype=np.int32).reshape(-1)
        n = tr.shape[0]
        if n == 0:
            raise _lib.UnevenHipError(who + ": no query")
        bc = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)))
        return tr, n, bc(t_from), bc(t_to), {k: bc(v) for k, v in per_query.items()}

    def _pair(self, traj_a, traj_b, t_from, t_to, other, who, **per_query):
        """_clock for the calls on pairs of vehicles, with traj_b broadcast against traj_a and the handle of b's context (None: self)"""
        tr, n, tf, tt, v = self._clock(traj_a, t_from, t_to, who, **per_query)
        tb = np.ascontiguousarray(np.broadcast_to(np.asarray(traj_b, dtype=np.int32), (n,)))
        return tr, tb, n, tf, tt, v, None if other is None else other.h

    @staticmethod
    def _conflict_list(call, n, cap, who):
        """the conflict list of a fleet call, call(room, pairs, rows, below, n_conflicts, n_candidates); cap = None: repeated with room for every conflict"""
        room = max(1024, 4 * n) if cap is None else int(cap)
        while True:
            pairs, rows, below = np.zeros((max(room, 1), 2), dtype=np.int32), np.full((max(room, 1), 4), np.nan), np.zeros(max(room, 1), dtype=np.int32)
            nc, nk = C.c_int64(0), C.c_int64(0)
            _lib.check(call(room, _ip(pairs), _dp(rows), _ip(below), C.byref(nc), C.byref(nk)), who)
            if cap is not None or nc.value <= room:
                break
            room = int(nc.value)
        m = min(room, int(nc.value))
        return dict(pairs=pairs[:m], rows=rows[:m], below=below[:m], n_conflicts=int(nc.value), n_candidates=int(nk.value))

    def extent(self, traj, t_from, t_to, t0=0.0, dt=0.01):
        """The bounding box, on the device, of vehicle q -- resident trajectory traj[q] started at t0[q] on a common clock -- over the samples
        tau_k = t_from[q] + k dt <= t_to[q] of that clock (scalars are broadcast): box (n, 4) = xmin, xmax, ymin, ymax in map coordinates and counts
        (n, 2: samples, NaN samples); see separation_times / extent_rows for the rule."""
        tr, n, tf, tt, v = self._clock(traj, t_from, t_to, "extent", t0=t0)
        out = dict(box=np.tile([np.inf, -np.inf, np.inf, -np.inf], (n, 1)), counts=np.zeros((n, 2), dtype=np.int32))
        _lib.check(self.L.uph_extent_batch(self.h, n, _ip(tr), _dp(v["t0"]), _dp(tf), _dp(tt), float(dt), _dp(out["box"]), _ip(out["counts"])), "uph_extent_batch")
        return out

    def separation(self, traj_a, traj_b, t_from, t_to, radius, t0_a=0.0, t0_b=0.0, other=None, dt=0.01):
        """How close, on the device, vehicle a -- trajectory traj_a[q] of self started at t0_a[q] on a common clock -- and vehicle b -- trajectory
        traj_b[q] of `other` (an ALMTrajOpt on the same device; None: self) started at t0_b[q] -- come over the samples tau_k = t_from[q] + k dt <=
        t_to[q]: min_d2 and min_t (the smallest squared distance and its tau), first_t / last_t (tau of the first / last sample with d2 < radius[q]^2,
        NaN: none) and counts (n, 2: samples, below).  A vehicle stands at its start before its t0 and at its goal after its end.  See separation_rows."""
        tr, tb, n, tf, tt, v, hb = self._pair(traj_a, traj_b, t_from, t_to, other, "separation", t0_a=t0_a, t0_b=t0_b, radius=radius)
        out = dict(min_d2=np.full(n, np.inf), min_t=np.full(n, np.nan), first_t=np.full(n, np.nan), last_t=np.full(n, np.nan), counts=np.zeros((n, 2), dtype=np.int32))
        _lib.check(self.L.uph_separation_batch(self.h, hb, n, _ip(tr), _ip(tb), _dp(v["t0_a"]), _dp(v["t0_b"]), _dp(tf), _dp(tt), float(dt), _dp(v["radius"]),
                                               _dp(out["min_d2"]), _dp(out["min_t"]), _dp(out["first_t"]), _dp(out["last_t"]), _ip(out["counts"])), "uph_separation_batch")
        return out

    def conflicts(self, traj, radius, t_from, t_to, t0=0.0, dt=0.05, cap=None):
        """The pairs of a fleet that come too close: vehicle i is resident trajectory traj[i] started at t0[i] on a common clock with a disc of
        radius[i] (scalars are broadcast), one window [t_from, t_to] for all.  Extents on the device, the broad phase on the host, the separation of
        its candidates on the device.  Returns pairs (m, 2) -- indices into traj, i < j, in (i, j) order, every pair with a sample of d2 <
        (radius[i] + radius[j])^2 or the first cap of them --, rows (m, 4) = min_d2, min_t, first_t, last_t, below (m,), n_conflicts (all of them) and
        n_candidates (pairs the broad phase kept).  See conflict_candidates / separation_rows."""
        tr, n, _, _, v = self._clock(traj, 0.0, 0.0, "conflicts", t0=t0, radius=radius)
        return self._conflict_list(lambda room, *out: self.L.uph_conflicts_batch(self.h, n, _ip(tr), _dp(v["t0"]), _dp(v["radius"]), float(t_from), float(t_to), float(dt),
                                                                                 room, *out), n, cap, "uph_conflicts_batch")

    def separation_kernel_ms(self):
        """milliseconds of the kernels of the last extent(), separation() or conflicts() (events on the context's stream)"""
        return self._kernel_ms("uph_separation_kernel_ms")

    # ---- the same with oriented rectangles for the vehicles (uph_footprint_separation_batch, uph_footprint_conflicts_batch) ---------------------------
    def footprint_separation(self, traj_a, traj_b, t_from, t_to, shape_a, shape_b, margin, t0_a=0.0, t0_b=0.0, other=None, dt=0.01):
        """separation() for vehicles that are rectangles: shape = (front, rear, half_width) in metres around the trajectory's point, turned by the raw yaw
        (one shape of (3,) is broadcast).  Over the samples tau_k = t_from[q] + k dt <= t_to[q]: min_c2 and min_t (the smallest squared distance between
        the two rectangles, 0 when they overlap, and its tau), first_t / last_t (tau of the first / last sample that overlaps or has c2 < margin[q]^2,
        NaN: none) and counts (n, 3: samples, below, overlapping).  Broadcasting and `other` as separation().  See footprint_rows."""
        tr, tb, n, tf, tt, v, hb = self._pair(traj_a, traj_b, t_from, t_to, other, "footprint_separation", t0_a=t0_a, t0_b=t0_b, margin=margin)
        sa, sb = (np.ascontiguousarray(np.broadcast_to(np.asarray(s, dtype=np.float64), (n, 3))) for s in (shape_a, shape_b))
        out = dict(min_c2=np.full(n, np.inf), min_t=np.full(n, np.nan), first_t=np.full(n, np.nan), last_t=np.full(n, np.nan), counts=np.zeros((n, 3), dtype=np.int32))
        _lib.check(self.L.uph_footprint_separation_batch(self.h, hb, n, _ip(tr), _ip(tb), _dp(v["t0_a"]), _dp(v["t0_b"]), _dp(tf), _dp(tt), float(dt), _dp(sa),
                                                         _dp(sb), _dp(v["margin"]), _dp(out["min_c2"]), _dp(out["min_t"]), _dp(out["first_t"]),
                                                         _dp(out["last_t"]), _ip(out["counts"])), "uph_footprint_separation_batch")
        return out

    def footprint_conflicts(self, traj, shape, margin, t_from, t_to, t0=0.0, dt=0.05, cap=None):
        """conflicts() for vehicles that are rectangles: vehicle i is resident trajectory traj[i] started at t0[i] with shape[i] = (front, rear,
        half_width) and margin[i] (a shape of (3,) and scalars are broadcast), one window for all.  Extents on the device, the broad phase on the host with
        footprint_radii, the footprint separation of its candidates on the device with the margin margin[i] + margin[j].  Returns pairs (m, 2), rows
        (m, 4) = min_c2, min_t, first_t, last_t, below (m,), n_conflicts and n_candidates as conflicts() does: every pair with a sample that overlaps
        or is closer than its margin, or the first cap of them."""
        tr, n, _, _, v = self._clock(traj, 0.0, 0.0, "footprint_conflicts", t0=t0, margin=margin)
        sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shape, dtype=np.float64), (n, 3)))
        return self._conflict_list(lambda room, *out: self.L.uph_footprint_conflicts_batch(self.h, n, _ip(tr), _dp(v["t0"]), _dp(sh), _dp(v["margin"]), float(t_from),
                                                                                           float(t_to), float(dt), room, *out), n, cap, "uph_footprint_conflicts_batch")

    def footprint_kernel_ms(self):
        """milliseconds of the kernels of the last footprint_separation() or footprint_conflicts() (events on the context's stream)"""
        return self._kernel_ms("uph_footprint_kernel_ms")

    # ---- the vehicle's rectangle swept over the map's occupancy as it is now (uph_footprint_check_batch) -----------------------------------------------
    def footprint_check(self, traj, shape, margin=0.0, t_from=0.0, t_to=None, dt=0.01, with_end=True, layers=FOOT_ALL):
        """check()'s occupancy read with the vehicle as a rectangle: over the rollout(dt, with_end) samples of resident trajectory traj[q] with t in [t_from[q],
        t_to[q]] (scalars and one shape of (3,) are broadcast; t_to = None: to the end), every column of the map whose centre lies in the rectangle shape[q] =
        (front, rear, half_width) inflated by margin[q] and turned by the raw yaw, and the column under the point itself, is looked up in the occupancy layers.
        A column's kinds are FOOT_OCC_XY, FOOT_OCC_YAW or FOOT_OUTSIDE; it is a hit when they intersect `layers`.  Returns a dict of arrays over the queries:
        first_t / last_t (t of the first / last sample with a hit column, NaN: none), first_mask (the kinds within layers at the first), first_cell (n, 2: the
        lexicographically smallest hit column of the first hit sample, (-1, -1): none), counts (n, 5: samples, hit samples, samples that cover a column of
        kind XY / YAW / OUTSIDE) and cells (n, 2: covered and hit columns summed over the samples).  See footprint_check_rows for the rule."""
        tr, n, tf, tt, _ = self._windows(traj, t_from, t_to, None, 0, "footprint_check")
        sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shape, dtype=np.float64), (n, 3)))
        mg = np.ascontiguousarray(np.broadcast_to(np.asarray(margin, dtype=np.float64), (n,)))
        out = dict(first_t=np.full(n, np.nan), last_t=np.full(n, np.nan), first_mask=np.zeros(n, dtype=np.int32), first_cell=np.full((n, 2), -1, dtype=np.int32),
                   counts=np.zeros((n, 5), dtype=np.int32), cells=np.zeros((n, 2), dtype=np.int64))
        _lib.check(self.L.uph_footprint_check_batch(self.h, n, _ip(tr), _dp(tf), None if tt is None else _dp(tt), float(dt), int(bool(with_end)), _dp(sh), _dp(mg),
                                                    int(layers), _dp(out["first_t"]), _dp(out["last_t"]), _ip(out["first_mask"]), _ip(out["first_cell"]),
                                                    _ip(out["counts"]), out["cells"].ctypes.data_as(C.POINTER(C.c_int64))), "uph_footprint_check_batch")
        return out

    def footprint_check_kernel_ms(self):
        """milliseconds of the kernel(s) of the last footprint_check() (events on the context's stream)"""
        return self._kernel_ms("uph_footprint_check_kernel_ms")

    # ---- how much room the body has along resident trajectories (uph_clearance_check_batch) ------------------------------------------------------------------
    def clearance(self, layer, traj, below=None, below2=None, t_from=0.0, t_to=None, dt=0.01, with_end=True):
        """Read the ClearanceLayer `layer` (of this context's map, fresh) at the rollout(dt, with_end) samples of resident trajectory traj[q] with t in
        [t_from[q], t_to[q]] (scalars are broadcast; t_to = None: to the end): per sample the value v = D at the cell of its point and yaw bin, 0 for a sample
        outside the grid.  `below` is a distance in metres, converted to below2 = ceil((below / res)^2); below2, in squared cells, is also accepted directly
        (exactly one of the two).  Returns a dict of arrays over the queries: min_d2 (-1: empty window), min_d = res * sqrt(min_d2) in metres (NaN: empty window,
        inf: CLEAR_FAR, nothing within rmax), min_t and min_cell (n, 3) of the earliest sample at the min, first_t / last_t of the samples with v < below2 (NaN:
        none), counts (n, 4: samples, below, outside, far) and below2 as used.  See clearance.clearance_check_rows for the rule."""
        from . import clearance as _cl
        tr, n, tf, tt, _ = self._windows(traj, t_from, t_to, None, 0, "clearance")
        if (below is None) == (below2 is None):
            raise _lib.UnevenHipError("clearance: give exactly one of below (metres) and below2 (squared cells)")
        res = float(layer.body_layer.uneven_map.xy_resolution)
        b2 = _cl.below2_of(below, res) if below2 is None else np.asarray(below2, dtype=np.int32)
        b2 = np.ascontiguousarray(np.broadcast_to(b2, (n,)), dtype=np.int32)
        out = dict(min_d2=np.full(n, -1, dtype=np.int32), min_t=np.full(n, np.nan), min_cell=np.full((n, 3), -1, dtype=np.int32), first_t=np.full(n, np.nan),
                   last_t=np.full(n, np.nan), counts=np.zeros((n, 4), dtype=np.int32))
        _lib.check(self.L.uph_clearance_check_batch(self.h, layer.h, n, _ip(tr), _dp(tf), None if tt is None else _dp(tt), float(dt), int(bool(with_end)), _ip(b2),
                                                    _ip(out["min_d2"]), _dp(out["min_t"]), _ip(out["min_cell"]), _dp(out["first_t"]), _dp(out["last_t"]),
                                                    _ip(out["counts"])), "uph_clearance_check_batch")
        d2 = out["min_d2"].astype(np.float64)
        out["min_d"] = np.where(d2 < 0, np.nan, np.where(d2 == _cl.CLEAR_FAR, np.inf, res * np.sqrt(np.maximum(d2, 0.0))))
        out["below2"] = b2
        return out

    def clearance_kernel_ms(self):
        """milliseconds of the kernel(s) of the last clearance() (events on the context's stream)"""
        return self._kernel_ms("uph_clearance_check_kernel_ms")

    # ---- start delays (uph_delay_sweep_batch, uph_delay_extent_batch, uph_delays_batch) ----------------------------------------------------------------
    def delay_sweep(self, traj_a, traj_b, t_from, t_to, radius, delay0, delay_step, D, t0_a=0.0, t0_b=0.0, other=None, dt=0.01):
        """separation() of vehicle a against vehicle b for every start t0_b[q] + delay_times(delay0, delay_step, D)[j] of b, on the device in one call:
        min_d2, min_t and below (n, D) -- each what separation() returns for that start --, first_clear (n,) = the smallest j with below == 0 (-1:
        none) and counts (n,) = the samples K of the window.  Broadcasting and `other` as separation()."""
        tr, tb, n, tf, tt, v, hb = self._pair(traj_a, traj_b, t_from, t_to, other, "delay_sweep", t0_a=t0_a, t0_b=t0_b, radius=radius)
        D = int(D)
        m = max(D, 1)
        out = dict(min_d2=np.full((n, m), np.inf), min_t=np.full((n, m), np.nan), below=np.zeros((n, m), dtype=np.int32), first_clear=np.full(n, -1, dtype=np.int32),
                   counts=np.zeros(n, dtype=np.int32))
        _lib.check(self.L.uph_delay_sweep_batch(self.h, hb, n, _ip(tr), _ip(tb), _dp(v["t0_a"]), _dp(v["t0_b"]), _dp(tf), _dp(tt), float(dt), _dp(v["radius"]),
                                                float(delay0), float(delay_step), D, _dp(out["min_d2"]), _dp(out["min_t"]), _ip(out["below"]),
                                                _ip(out["first_clear"]), _ip(out["counts"])), "uph_delay_sweep_batch")
        return out

    def delay_extent(self, traj, t_from, t_to, delay0, delay_step, D, t0=0.0, dt=0.01):
        """The hull over the delays of the table of extent(traj, t_from, t_to, t0 + delta_j), on the device in one call: box (n, 4) and counts (n, 2:
        samples K of the window, samples with a NaN position over all delays).  The input of a broad phase that holds under every delay."""
        tr, n, tf, tt, v = self._clock(traj, t_from, t_to, "delay_extent", t0=t0)
        out = dict(box=np.tile([np.inf, -np.inf, np.inf, -np.inf], (n, 1)), counts=np.zeros((n, 2), dtype=np.int32))
        _lib.check(self.L.uph_delay_extent_batch(self.h, n, _ip(tr), _dp(v["t0"]), _dp(tf), _dp(tt), float(dt), float(delay0), float(delay_step), int(D), _dp(out["box"]),
                                                 _ip(out["counts"])), "uph_delay_extent_batch")
        return out

    def delays(self, traj, radius, t_from, t_to, delay0, delay_step, D, t0=0.0, n_delays=None, dt=0.05):
        """Start delays that clear a fleet: vehicle i is resident trajectory traj[i] started at t0[i] with a disc of radius[i], in priority order (the
        smaller index goes first), one window for all.  Each vehicle gets the smallest delay of delay_times(delay0, delay_step, D) -- among its first
        n_delays[i] (None: all; a scalar is broadcast) -- at which it is never below r_h + r_i against any vehicle h ahead of it at ITS chosen start.
        Returns choice (n,; -1: no such delay, the vehicle stays at delay 0 and needs a new plan), start (n,) the effective starts, blocker (n,; the
        first vehicle in the way of an unresolved one, else -1), n_candidates, n_rounds and n_unresolved.  See delay_schedule."""
        tr, n, _, _, v = self._clock(traj, 0.0, 0.0, "delays", t0=t0, radius=radius)
        nd = None if n_delays is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_delays, dtype=np.int32), (n,)))
        out = dict(choice=np.zeros(n, dtype=np.int32), start=np.full(n, np.nan), blocker=np.full(n, -1, dtype=np.int32))
        nk, nr, nu = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        _lib.check(self.L.uph_delays_batch(self.h, n, _ip(tr), _dp(v["t0"]), _dp(v["radius"]), None if nd is None else _ip(nd), float(t_from), float(t_to), float(dt),
                                           float(delay0), float(delay_step), int(D), _ip(out["choice"]), _dp(out["start"]), _ip(out["blocker"]), C.byref(nk), C.byref(nr),
                                           C.byref(nu)), "uph_delays_batch")
        out.update(n_candidates=int(nk.value), n_rounds=int(nr.value), n_unresolved=int(nu.value))
        return out

    def delay_kernel_ms(self):
        """milliseconds of the kernels of the last delay_sweep(), delay_extent() or delays() -- or footprint_delay_sweep() / footprint_delays() -- (events on
        the context's stream)"""
        return self._kernel_ms("uph_delay_kernel_ms")

    # ---- start delays with oriented rectangles (uph_footprint_delay_sweep_batch, uph_footprint_delays_batch) -------------------------------------------
    def footprint_delay_sweep(self, traj_a, traj_b, t_from, t_to, shape_a, shape_b, margin, delay0, delay_step, D, t0_a=0.0, t0_b=0.0, other=None, dt=0.01):
        """footprint_separation() of vehicle a against vehicle b for every start t0_b[q] + delay_times(delay0, delay_step, D)[j] of b, on the device in one
        call: min_c2, min_t, below and overlapping (n, D) -- each what footprint_separation() returns for that start, bit for bit --, first_clear (n,) =
        the smallest j with below == 0 (-1: none) and counts (n,) = the samples K of the window.  Broadcasting and `other` as footprint_separation()."""
        tr, tb, n, tf, tt, v, hb = self._pair(traj_a, traj_b, t_from, t_to, other, "footprint_delay_sweep", t0_a=t0_a, t0_b=t0_b, margin=margin)
        sa, sb = (np.ascontiguousarray(np.broadcast_to(np.asarray(s, dtype=np.float64), (n, 3))) for s in (shape_a, shape_b))
        D = int(D)
        m = max(D, 1)
        out = dict(min_c2=np.full((n, m), np.inf), min_t=np.full((n, m), np.nan), below=np.zeros((n, m), dtype=np.int32), overlapping=np.zeros((n, m), dtype=np.int32),
                   first_clear=np.full(n, -1, dtype=np.int32), counts=np.zeros(n, dtype=np.int32))
        _lib.check(self.L.uph_footprint_delay_sweep_batch(self.h, hb, n, _ip(tr), _ip(tb), _dp(v["t0_a"]), _dp(v["t0_b"]), _dp(tf), _dp(tt), float(dt), _dp(sa), _dp(sb),
                                                          _dp(v["margin"]), float(delay0), float(delay_step), D, _dp(out["min_c2"]), _dp(out["min_t"]),
                                                          _ip(out["below"]), _ip(out["overlapping"]), _ip(out["first_clear"]), _ip(out["counts"])),
                   "uph_footprint_delay_sweep_batch")
        return out

    def footprint_delays(self, traj, shape, margin, t_from, t_to, delay0, delay_step, D, t0=0.0, n_delays=None, dt=0.05):
        """delays() for vehicles that are rectangles: vehicle i is resident trajectory traj[i] started at t0[i] with shape[i] = (front, rear, half_width) and
        margin[i] (a shape of (3,) and scalars are broadcast), in priority order, one window for all.  Each vehicle gets the smallest delay of the table --
        among its first n_delays[i] -- at which its rectangle never overlaps, nor comes closer than margin[h] + margin[i] to, that of any vehicle h ahead of
        it at ITS chosen start.  The broad phase takes footprint_radii on delay_extent's boxes.  Returns what delays() returns.  The remedy that goes with
        footprint_conflicts(): delays() on the circumscribed discs also postpones passes side by side that the rectangles allow."""
        tr, n, _, _, v = self._clock(traj, 0.0, 0.0, "footprint_delays", t0=t0, margin=margin)
        sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shape, dtype=np.float64), (n, 3)))
        nd = None if n_delays is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_delays, dtype=np.int32), (n,)))
        out = dict(choice=np.zeros(n, dtype=np.int32), start=np.full(n, np.nan), blocker=np.full(n, -1, dtype=np.int32))
        nk, nr, nu = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        _lib.check(self.L.uph_footprint_delays_batch(self.h, n, _ip(tr), _dp(v["t0"]), _dp(sh), _dp(v["margin"]), None if nd is None else _ip(nd), float(t_from),
                                                     float(t_to), float(dt), float(delay0), float(delay_step), int(D), _ip(out["choice"]), _dp(out["start"]),
                                                     _ip(out["blocker"]), C.byref(nk), C.byref(nr), C.byref(nu)), "uph_footprint_delays_batch")
        out.update(n_candidates=int(nk.value), n_rounds=int(nr.value), n_unresolved=int(nu.value))
        return out

    # ---- test / bench hooks -----------------------------------------------------------------------------------------
    def x0_packed(self, probs):
        xs = []
        for pr in probs:
            T = float(pr["total_time"])
            tau = (np.sqrt(2.0 * T - 1.0) - 1.0) if T > 1.0 else (1.0 - np.sqrt(2.0 / T - 1.0))      # logC2, alm_traj_opt.h:239-242
            xs.append(np.concatenate([[tau], np.asarray(pr["inner_xy"], dtype=np.float64).T.ravel(), np.asarray(pr["inner_yaw"], dtype=np.float64)]))
        return xs

    def eval_batch(self, xs=None, repeat=1):
        """One innerCallback evaluation per uploaded trajectory at xs (list of arrays; None = resident x)."""
        n_tot = sum(s["n"] for s in self._sizes)
        xp = np.concatenate(xs) if xs is not None else None
        f, g = np.zeros(self._B), np.zeros(n_tot)
        _lib.check(self.L.uph_eval_batch(self.h, _dp(xp) if xp is not None else None, _dp(f), _dp(g), int(repeat)), "uph_eval_batch")
        gs, o = [], 0
        for s in self._sizes:
            gs.append(g[o:o + s["n"]].copy())
            o += s["n"]
        return f, gs

    def penalty_batch(self, repeat=1, store_residuals=True):
        """calConstrainCostGrad alone (alm_traj_opt.cpp:663-991) on the resident coefficients / durations / duals / scales: per trajectory
        (cost, gdCxy (6 Nxy, 2), gdCyaw (6 Nyaw,), sum gdTxy, sum gdTyaw)"""
        ncx, ncy = sum(12 * s["Nxy"] for s in self._sizes), sum(6 * s["Nyaw"] for s in self._sizes)
        cost, gx, gy, gt = np.zeros(self._B), np.zeros(ncx), np.zeros(ncy), np.zeros((self._B, 2))
        _lib.check(self.L.uph_penalty_batch(self.h, int(repeat), int(bool(store_residuals)), _dp(cost), _dp(gx), _dp(gy), _dp(gt)), "uph_penalty_batch")
        out, ox, oy = [], 0, 0
        for b, s in enumerate(self._sizes):
            out.append(dict(cost=cost[b], gdCxy=gx[ox:ox + 12 * s["Nxy"]].reshape(-1, 2).copy(), gdCyaw=gy[oy:oy + 6 * s["Nyaw"]].copy(), gdTxy_sum=gt[b, 0], gdTyaw_sum=gt[b, 1]))
            ox += 12 * s["Nxy"]; oy += 6 * s["Nyaw"]
        return out

    def init_scaling_batch(self):
        _lib.check(self.L.uph_init_scaling_batch(self.h), "uph_init_scaling_batch")

    def set_state(self, lam=None, mu=None, scale_cx=None, scale_fx=None, rho=None):
        cat = lambda v: np.ascontiguousarray(np.concatenate(v), dtype=np.float64) if v is not None else None
        a, b, c = cat(lam), cat(mu), cat(scale_cx)
        d = np.ascontiguousarray(scale_fx, dtype=np.float64) if scale_fx is not None else None
        e = np.ascontiguousarray(rho, dtype=np.float64) if rho is not None else None
        p = lambda v: _dp(v) if v is not None else None
        _lib.check(self.L.uph_batch_set_state(self.h, p(a), p(b), p(c), p(d), p(e)), "uph_batch_set_state")

    # teacher-forced late-state hooks (states as oracle.OracleALM.capture() returns them) ---------------------------------
    MAX_PAST = 8

    def set_x(self, xs):
        xp = np.ascontiguousarray(np.concatenate(xs), dtype=np.float64)
        _lib.check(self.L.uph_batch_set_x(self.h, _dp(xp)), "uph_batch_set_x")

    def alm_passes(self, max_passes=0):
        """the ALM loop from the resident x / duals / scales / rho (no reset, no initScaling), at most max_passes passes"""
        _lib.check(self.L.uph_batch_alm_passes(self.h, int(max_passes)), "uph_batch_alm_passes")

    def set_lbfgs_state(self, states):
        """states: one dict per uploaded trajectory with x, g, d, pf, lm_ys, lm_s (mem, n), lm_y, step, fx, k, end, bound"""
        cat = lambda key: np.ascontiguousarray(np.concatenate([np.asarray(st[key], dtype=np.float64).ravel() for st in states]))
        pf = np.zeros((self._B, self.MAX_PAST))
        for i, st in enumerate(states):
            pf[i, :len(st["pf"])] = st["pf"]
        scal = np.array([[st["step"], st["fx"], st["k"], st["end"], st["bound"]] for st in states], dtype=np.float64)
        self.set_x([st["x"] for st in states])
        g, d, ls, ly, ys = cat("g"), cat("d"), cat("lm_s"), cat("lm_y"), cat("lm_ys")
        _lib.check(self.L.uph_batch_set_lbfgs_state(self.h, _dp(g), _dp(d), _dp(pf), _dp(ls), _dp(ly), _dp(ys), _dp(scal)), "uph_batch_set_lbfgs_state")

    def lbfgs_resume(self, budget, finish_pass=False):
        _lib.check(self.L.uph_batch_lbfgs_resume(self.h, int(budget), int(bool(finish_pass))), "uph_batch_lbfgs_resume")

    def get_lbfgs_state(self):
        """list of state dicts (same keys as set_lbfgs_state + code, accepted, converged); x and the duals via download()"""
        mem = int(self.mem_size)
        n_tot = sum(s["n"] for s in self._sizes)
        g, d = np.zeros(n_tot), np.zeros(n_tot)
        pf = np.zeros((self._B, self.MAX_PAST))
        ls, ly, ys = np.zeros(mem * n_tot), np.zeros(mem * n_tot), np.zeros((self._B, mem))
        scal = np.zeros((self._B, 8))
        _lib.check(self.L.uph_batch_get_lbfgs_state(self.h, _dp(g), _dp(d), _dp(pf), _dp(ls), _dp(ly), _dp(ys), _dp(scal)), "uph_batch_get_lbfgs_state")
        x = self.download()
        out, o, oh = [], 0, 0
        for i, s in enumerate(self._sizes):
            n = s["n"]
            out.append(dict(x=x[i]["x"], g=g[o:o + n].copy(), d=d[o:o + n].copy(), pf=pf[i, :max(1, int(self.past))].copy(), lm_ys=ys[i].copy(),
                            lm_s=ls[oh:oh + mem * n].reshape(mem, n).copy(), lm_y=ly[oh:oh + mem * n].reshape(mem, n).copy(),
                            step=scal[i, 0], fx=scal[i, 1], k=int(scal[i, 2]), end=int(scal[i, 3]), bound=int(scal[i, 4]), code=int(scal[i, 5]),
                            accepted=int(scal[i, 6]), converged=int(scal[i, 7]), hx=x[i]["hx"], gx=x[i]["gx"], lam=x[i]["lam"], mu=x[i]["mu"],
                            rho=x[i]["rho_final"]))
            o += n
            oh += mem * n
        return out

    def set_trace(self, cap):
        _lib.check(self.L.uph_ctx_set_trace(self.h, int(cap)), "uph_ctx_set_trace")
        self._trace_cap = int(cap)

    def get_trace(self):
        out = np.zeros((self._B, self._trace_cap_up))
        _lib.check(self.L.uph_ctx_get_trace(self.h, _dp(out)), "uph_ctx_get_trace")
        return out


# ---- a fleet of resident trajectories (uph_fleet_*) ---------------------------------------------------------------------------------------------------------
def fleet_bytes(slots, cap_xy=_lib.UPH_MAX_PIECE_XY, cap_yaw=_lib.UPH_MAX_PIECE_YAW):
    """device memory of a TrajFleet of that shape (uph_fleet_bytes; pure host arithmetic): slots * (96 cap_xy + 48 cap_yaw + FLEET_SLOT_ROW_BYTES)"""
    b = C.c_int64(0)
    _lib.check(_lib.load().uph_fleet_bytes(int(slots), int(cap_xy), int(cap_yaw), C.byref(b)), "uph_fleet_bytes")
    return int(b.value)


def _fleet_shape(slots, cap_xy, cap_yaw):
    """TrajFleet's argument check, before any device call: the shape as integers, or a raise"""
    try:
        s, cx, cy = int(slots), int(cap_xy), int(cap_yaw)
    except (TypeError, ValueError):
        raise _lib.UnevenHipError("TrajFleet: slots, cap_xy and cap_yaw must be integers")
    if s != slots or cx != cap_xy or cy != cap_yaw:
        raise _lib.UnevenHipError("TrajFleet: slots, cap_xy and cap_yaw must be integers")
    if s < 1 or not (1 <= cx <= _lib.UPH_MAX_PIECE_XY) or not (1 <= cy <= _lib.UPH_MAX_PIECE_YAW):
        raise _lib.UnevenHipError("TrajFleet: slots >= 1, 1 <= cap_xy <= %d and 1 <= cap_yaw <= %d" % (_lib.UPH_MAX_PIECE_XY, _lib.UPH_MAX_PIECE_YAW))
    return s, cx, cy


def _adopt_arrays(src_traj, slot, t0):
    """adopt()'s argument check, before any device call: (src_traj, slot, t0 or None) as the arrays the C call takes"""
    tr = np.ascontiguousarray(src_traj, dtype=np.int32).reshape(-1)
    sl = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
    n = tr.shape[0]
    if n == 0 or sl.shape[0] != n:
        raise _lib.UnevenHipError("adopt: src_traj and slot must be the same non-empty length")
    if np.unique(sl).shape[0] != n:
        raise _lib.UnevenHipError("adopt: a slot is named twice in one call")
    ts = None
    if t0 is not None:
        ts = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.float64), (n,)))
        if not np.isfinite(ts).all():
            raise _lib.UnevenHipError("adopt: t0 must be finite")
    return tr, sl, ts


class TrajFleet(ALMTrajOpt):
    """A long-lived set of resident trajectories on one map: `slots` slots of fixed stride (cap_xy / cap_yaw pieces at most) that solved trajectories of
    ALMTrajOpt objects on the same map -- or of another TrajFleet -- are adopted into on the device (uph_fleet_adopt: one kernel launch, no coefficient
    crosses the host).  It answers every query ALMTrajOpt answers on its resident batch -- traj_states, rollout, check, locate, within, extent, separation,
    conflicts, footprint_*, delay* --, is accepted as `other=` and as `src` of refine / replan_goals, and takes no upload or solve: those methods raise.
    In the fleet-wide wrappers (extent, conflicts, delays, their footprint and delay forms) t0 = None means the starts stored at adoption."""

    def __init__(self, uneven_map, slots, cap_xy=_lib.UPH_MAX_PIECE_XY, cap_yaw=_lib.UPH_MAX_PIECE_YAW, params=None):
        self.slots, self.cap_xy, self.cap_yaw = _fleet_shape(slots, cap_xy, cap_yaw)
        super().__init__(uneven_map, params)

    def setEnvironment(self, env):
        self.uneven_map = env
        if self.h:
            self.L.uph_ctx_destroy(self.h)
            self.h = None
        p = _lib.OptParams(**{k: (int(getattr(self, k)) if k in _INT_FIELDS else float(getattr(self, k))) for k in self._pnames})
        h = C.c_void_p()
        _lib.check(self.L.uph_fleet_create(env.h, C.byref(p), self.slots, self.cap_xy, self.cap_yaw, C.byref(h)), "uph_fleet_create")
        self.h = h

    # ---- slots ---------------------------------------------------------------------------------------------------------------------------------------------
    def adopt(self, src, src_traj, slot, t0=None):
        """trajectory src_traj[q] of `src`'s resident batch (an ALMTrajOpt or TrajFleet on the same map) into slot[q], started at t0[q] on the common clock
        (a scalar is broadcast; None: 0).  All or nothing: a refusal leaves the fleet as it was."""
        tr, sl, ts = _adopt_arrays(src_traj, slot, t0)
        if not isinstance(src, ALMTrajOpt) or src.h is None:
            raise _lib.UnevenHipError("adopt: src must be an ALMTrajOpt or a TrajFleet with a device context")
        _lib.check(self.L.uph_fleet_adopt(self.h, src.h, tr.shape[0], _ip(tr), _ip(sl), None if ts is None else _dp(ts)), "uph_fleet_adopt")

    def release(self, slot):
        """empty the slots (idempotent)"""
        sl = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        if sl.shape[0] == 0:
            raise _lib.UnevenHipError("release: no slot")
        _lib.check(self.L.uph_fleet_release(self.h, sl.shape[0], _ip(sl)), "uph_fleet_release")

    def _info(self):
        occ, t0 = np.zeros(self.slots, dtype=np.int32), np.zeros(self.slots)
        _lib.check(self.L.uph_fleet_info(self.h, None, None, None, _ip(occ), _dp(t0)), "uph_fleet_info")
        return occ.astype(bool), t0

    @property
    def occupied(self):
        """(slots,) bool: the slot holds a trajectory"""
        return self._info()[0]

    @property
    def t0(self):
        """(slots,) the start of each slot's trajectory on the common clock as stored at adoption (0 for an empty slot)"""
        return self._info()[1]

    def get(self, slot):
        """uph_fleet_get: dict of n_xy, n_yaw, T_xy, T_yaw, ret (n,) and the slots' WHOLE coefficient regions c_xy (n, 12 cap_xy), c_yaw (n, 6 cap_yaw), map
        coordinates; the first 12 n_xy / 6 n_yaw doubles of a row are the trajectory"""
        sl = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        n = sl.shape[0]
        if n == 0:
            raise _lib.UnevenHipError("get: no slot")
        out = dict(n_xy=np.zeros(n, dtype=np.int32), n_yaw=np.zeros(n, dtype=np.int32), T_xy=np.zeros(n), T_yaw=np.zeros(n), ret=np.zeros(n, dtype=np.int32),
                   c_xy=np.zeros((n, 12 * self.cap_xy)), c_yaw=np.zeros((n, 6 * self.cap_yaw)))
        _lib.check(self.L.uph_fleet_get(self.h, n, _ip(sl), _ip(out["n_xy"]), _ip(out["n_yaw"]), _dp(out["T_xy"]), _dp(out["T_yaw"]), _ip(out["ret"]),
                                        _dp(out["c_xy"]), _dp(out["c_yaw"])), "uph_fleet_get")
        return out

    def getTraj(self, slot=0):
        g = self.get([int(slot)])
        if g["n_xy"][0] == 0:
            raise _lib.UnevenHipError("getTraj: slot %d of the fleet is empty" % int(slot))
        nx, ny = int(g["n_xy"][0]), int(g["n_yaw"][0])
        return SE2Traj(g["c_xy"][0, :12 * nx].reshape(-1, 2).copy(), g["c_yaw"][0, :6 * ny].copy(), float(g["T_xy"][0]), float(g["T_yaw"][0]))

    def adopt_kernel_ms(self):
        """milliseconds of uph_fleet_adopt_kernel in the last adopt() (events on the fleet's stream)"""
        return self._kernel_ms("uph_fleet_kernel_ms")

    # ---- the fleet-wide wrappers: t0 = None means the stored starts ------------------------------------------------------------------------------------------
    def _starts(self, traj, t0):
        return self.t0[np.ascontiguousarray(traj, dtype=np.int32).reshape(-1)] if t0 is None else t0

    def extent(self, traj, t_from, t_to, t0=None, dt=0.01):
        return super().extent(traj, t_from, t_to, t0=self._starts(traj, t0), dt=dt)

    def conflicts(self, traj, radius, t_from, t_to, t0=None, dt=0.05, cap=None):
        return super().conflicts(traj, radius, t_from, t_to, t0=self._starts(traj, t0), dt=dt, cap=cap)

    def footprint_conflicts(self, traj, shape, margin, t_from, t_to, t0=None, dt=0.05, cap=None):
        return super().footprint_conflicts(traj, shape, margin, t_from, t_to, t0=self._starts(traj, t0), dt=dt, cap=cap)

    def delay_extent(self, traj, t_from, t_to, delay0, delay_step, D, t0=None, dt=0.01):
        return super().delay_extent(traj, t_from, t_to, delay0, delay_step, D, t0=self._starts(traj, t0), dt=dt)

    def delays(self, traj, radius, t_from, t_to, delay0, delay_step, D, t0=None, n_delays=None, dt=0.05):
        return super().delays(traj, radius, t_from, t_to, delay0, delay_step, D, t0=self._starts(traj, t0), n_delays=n_delays, dt=dt)

    def footprint_delays(self, traj, shape, margin, t_from, t_to, delay0, delay_step, D, t0=None, n_delays=None, dt=0.05):
        return super().footprint_delays(traj, shape, margin, t_from, t_to, delay0, delay_step, D, t0=self._starts(traj, t0), n_delays=n_delays, dt=dt)


def _fleet_refuses(name):
    def method(self, *args, **kwargs):
        raise _lib.UnevenHipError("%s: a TrajFleet takes no upload, solve, evaluation, report, download or batch state (adopt() fills its slots)" % name)
    method.__name__ = name
    method.__doc__ = "refused on a TrajFleet"
    return method


# the solve side of ALMTrajOpt: uploads, solves, evaluations, reports, downloads and the batch-state hooks
FLEET_REFUSED = ("set_lanes", "set_xcd_locality", "set_wps", "set_sample_precision", "set_rho", "set_trial_abandon", "upload", "solve", "solve_async", "wait", "stats",
                 "cycles", "origin", "download", "optimize_batch", "prepare_boundary", "optimize_boundary", "plan_goals_upload", "plan_goals", "replan_goals_upload",
                 "replan_goals", "refine_upload", "refine", "plan_staged", "optimizeSE2Traj", "getTrajJerkCost", "getMaxVxAxAyCurAttSig", "x0_packed", "eval_batch",
                 "penalty_batch", "init_scaling_batch", "set_state", "set_x", "alm_passes", "set_lbfgs_state", "lbfgs_resume", "get_lbfgs_state", "set_trace", "get_trace")
for _name in FLEET_REFUSED:
    setattr(TrajFleet, _name, _fleet_refuses(_name))
del _name
