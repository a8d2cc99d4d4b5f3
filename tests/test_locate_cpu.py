"""CPU tier of locating poses on resident trajectories and finding rect crossings (uph_locate_batch, uph_within_batch): the C-ABI and its binding, the
refusals that need no device, the adapter's entry points, and the numpy mirrors locate_rows / within_rows / locate_refine -- the rule of
include/uneven_hip.h that tests/test_gpu_locate.py holds the device against -- on hand-made rows and hand-made quintic trajectories."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from numpy.polynomial import Polynomial

from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import LOCATE_NEWTON, SE2Traj, locate_errors, locate_refine, locate_rows, norm_so2, within_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = C.POINTER(C.c_int32)
DP = _lib.DP
INF = float("inf")


def test_symbols_are_exported_with_the_binding_signatures():
    L = _lib.load()
    loc = _lib.SYMBOLS["uph_locate_batch"][1]
    wit = _lib.SYMBOLS["uph_within_batch"][1]
    ms = _lib.SYMBOLS["uph_locate_kernel_ms"][1]
    assert loc == [C.c_void_p, C.c_int32, I32P, DP, DP, DP, C.c_double, C.c_int32, DP, DP, I32P, DP, I32P, DP, DP, DP]
    assert wit == [C.c_void_p, C.c_int32, I32P, DP, DP, DP, C.c_double, C.c_int32, DP, DP, I32P]
    assert ms == [C.c_void_p, DP]
    for name, args in (("uph_locate_batch", loc), ("uph_within_batch", wit), ("uph_locate_kernel_ms", ms)):
        fn = getattr(L, name)
        assert fn.restype == C.c_int and fn.argtypes == args
    hdr = " ".join(open(os.path.join(ROOT, "include", "uneven_hip.h")).read().split())
    assert ("int uph_locate_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* poses /* [n][3] */, const double* t_from, "
            "const double* t_to /* NULL: to the end */, double dt, int32_t with_end, double* near_t") in hdr
    assert ("int uph_within_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* rects /* [n][4] */, const double* t_from, "
            "const double* t_to /* NULL: to the end */, double dt, int32_t with_end, double* enter_t") in hdr
    assert "int uph_locate_kernel_ms(const uph_ctx* c, double* kernel_ms);" in hdr


def test_refusals_without_a_device():
    L = _lib.load()
    one = np.zeros(1, dtype=np.int32)
    t0, pose, rect = np.zeros(1), np.zeros(3), np.array([0.0, 1.0, 0.0, 1.0])
    d = {k: np.full(s, -9.0) for k, s in (("near_t", 1), ("near_d2", 1), ("t", 1), ("state", 10), ("d2", 1), ("err", 3), ("enter_t", 1), ("leave_t", 1))}
    i = {k: np.full(s, -9, dtype=np.int32) for k, s in (("count", 1), ("refined", 1), ("counts", 2))}
    dp = lambda a: a.ctypes.data_as(DP)
    ip = lambda a: a.ctypes.data_as(I32P)
    assert L.uph_locate_batch(None, 1, ip(one), dp(pose), dp(t0), None, 0.01, 1, dp(d["near_t"]), dp(d["near_d2"]), ip(i["count"]), dp(d["t"]),
                              ip(i["refined"]), dp(d["state"]), dp(d["d2"]), dp(d["err"])) == _lib.UPH_ERR_INVALID
    assert b"uph_locate_batch" in L.uph_last_error()
    assert L.uph_within_batch(None, 1, ip(one), dp(rect), dp(t0), None, 0.01, 1, dp(d["enter_t"]), dp(d["leave_t"]), ip(i["counts"])) == _lib.UPH_ERR_INVALID
    assert b"uph_within_batch" in L.uph_last_error()
    ms = C.c_double(-9.0)
    assert L.uph_locate_kernel_ms(None, C.byref(ms)) == _lib.UPH_ERR_INVALID and ms.value == -9.0
    assert all((v == -9).all() for v in d.values()) and all((v == -9).all() for v in i.values())


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
int main() {
    uneven_hip::ALMTrajOpt* o = nullptr;
    if (o) {
        uneven_hip::ALMTrajOpt::TrajLocate r = o->locateSE2TrajBatch({0, 1}, {{{0.0, 0.0, 0.0}}, {{1.0, 2.0, 0.5}}}, {0.0, 0.5});
        r = o->locateSE2TrajBatch({0}, {{{0.0, 0.0, 0.0}}}, {0.0}, {1.0}, 0.03, false);
        uneven_hip::ALMTrajOpt::TrajWithin w = o->withinSE2TrajBatch({0, 1}, {{{0.0, 1.0, 0.0, 1.0}}, {{1.0, 2.0, 0.5, 0.7}}}, {0.0, 0.5});
        w = o->withinSE2TrajBatch({0}, {{{0.0, 1.0, 0.0, 1.0}}}, {0.0}, {1.0}, 0.03, false);
        return (int)r.near_t[0] + (int)r.near_d2[0] + r.count[0] + (int)r.t[0] + r.refined[0] + (int)r.state[9] + (int)r.d2[0] + (int)r.err[2] +
               (w.enters(0) ? (int)w.enter_t[0] + (int)w.leave_t[0] + w.counts[1] : 0);
    }
    return 0;
}
"""


def test_adapter_offers_locate_and_within(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "a.o")])


def _rows(n):
    t = 0.25 * np.arange(n)
    xy = np.stack([1.0 * np.arange(n), np.zeros(n)], axis=1)         # along the x axis, one metre per row
    return t, xy


def test_locate_rows_rule_on_hand_made_rows():
    t, xy = _rows(8)
    r = locate_rows(t, xy, [3.2, 0.5, 0.0])
    assert r["near_t"] == t[3] and r["count"] == 8 and r["j"] == 3
    assert r["near_d2"] == (3.0 - 3.2) * (3.0 - 3.2) + 0.5 * 0.5
    # a tie goes to the earlier sample: rows 3 and 4 are equally far from x = 3.5
    r = locate_rows(t, xy, [3.5, 0.0, 0.0])
    assert r["near_t"] == t[3] and r["near_d2"] == 0.25
    # ... also inside a window whose index 0 is not row 0
    r = locate_rows(t, xy, [3.5, 0.0, 0.0], t_from=t[2])
    assert r["near_t"] == t[3] and r["j"] == 1 and r["count"] == 6 and r["times"].tolist() == t[2:].tolist()
    # a NaN reads +inf: it loses against any finite row and ties with the other non-finite ones
    xy[3, 0] = np.nan
    r = locate_rows(t, xy, [3.0, 0.0, 0.0])
    assert r["near_t"] == t[2] and r["near_d2"] == 1.0                # 2 and 4 tie: the earlier
    xy[:, 1] = np.nan
    r = locate_rows(t, xy, [3.0, 0.0, 0.0])
    assert r["near_t"] == t[0] and r["near_d2"] == INF and r["j"] == 0
    # every d2 = +inf (a pose at 1e200): sample 0 of the window wins
    t, xy = _rows(8)
    r = locate_rows(t, xy, [1e200, 0.0, 0.0])
    assert r["near_t"] == t[0] and r["near_d2"] == INF and r["count"] == 8
    r = locate_rows(t, xy, [1e200, -1e200, 0.0], t_from=t[5])
    assert r["near_t"] == t[5] and r["near_d2"] == INF and r["count"] == 3


def test_locate_rows_windows():
    t, xy = _rows(8)
    for a, b in ((10.0, 20.0), (1.0, 0.5), (0.3, 0.4), (-2.0, -1.0), (0.0, -INF)):      # beyond, reversed, between rows, before 0
        r = locate_rows(t, xy, [3.0, 0.0, 0.0], a, b)
        assert r["count"] == 0 and np.isnan(r["near_t"]) and r["near_d2"] == INF and r["j"] == -1 and r["times"].shape == (0,)
        w = within_rows(t, xy, [-9.0, 9.0, -9.0, 9.0], a, b)
        assert w["counts"].tolist() == [0, 0] and np.isnan(w["enter_t"]) and np.isnan(w["leave_t"])
    r = locate_rows(t[:0], xy[:0], [0.0, 0.0, 0.0])
    assert r["count"] == 0 and r["j"] == -1
    # a point window on a sample
    r = locate_rows(t, xy, [0.0, 0.0, 0.0], t[6], t[6])
    assert r["count"] == 1 and r["near_t"] == t[6] and r["near_d2"] == 36.0 and r["j"] == 0
    assert within_rows(t, xy, [6.0, 6.0, 0.0, 0.0], t[6], t[6])["counts"].tolist() == [1, 1]
    # both bounds are inside
    r = locate_rows(t, xy, [0.0, 0.0, 0.0], t[2], t[4])
    assert r["count"] == 3 and r["near_t"] == t[2]
    r = locate_rows(t, xy, [0.0, 0.0, 0.0], np.nextafter(t[2], 9.0), np.nextafter(t[4], 0.0))
    assert r["count"] == 1 and r["near_t"] == t[3]


def test_within_rows_rule_on_hand_made_rows():
    t, xy = _rows(8)
    w = within_rows(t, xy, [2.5, 5.5, -1.0, 1.0])
    assert w["enter_t"] == t[3] and w["leave_t"] == t[5] and w["counts"].tolist() == [8, 3]
    # a rect edge exactly on a sample is inside (closed), on each of the four edges
    assert within_rows(t, xy, [3.0, 5.0, -1.0, 1.0])["counts"].tolist() == [8, 3]
    assert within_rows(t, xy, [np.nextafter(3.0, 9.0), np.nextafter(5.0, 0.0), -1.0, 1.0])["counts"].tolist() == [8, 1]
    assert within_rows(t, xy, [3.0, 5.0, 0.0, 1.0])["counts"].tolist() == [8, 3]
    assert within_rows(t, xy, [3.0, 5.0, -1.0, 0.0])["counts"].tolist() == [8, 3]
    assert within_rows(t, xy, [3.0, 5.0, np.nextafter(0.0, 1.0), 1.0])["counts"].tolist() == [8, 0]
    w = within_rows(t, xy, [4.0, 4.0, 0.0, 0.0])                      # a degenerate rect on a sample
    assert w["enter_t"] == w["leave_t"] == t[4] and w["counts"].tolist() == [8, 1]
    # a reversed rect is empty, in x or in y
    for rect in ([5.0, 3.0, -1.0, 1.0], [3.0, 5.0, 1.0, -1.0]):
        w = within_rows(t, xy, rect)
        assert w["counts"].tolist() == [8, 0] and np.isnan(w["enter_t"]) and np.isnan(w["leave_t"])
    # infinite bounds are a half plane; a NaN position is outside
    xy[4, 1] = np.nan
    w = within_rows(t, xy, [2.5, INF, -INF, INF])
    assert w["enter_t"] == t[3] and w["leave_t"] == t[7] and w["counts"].tolist() == [8, 4]
    # a path that leaves and comes back: first and last sample inside, every one inside counted
    t, xy = _rows(8)
    xy[:, 0] = [0.0, 1.0, 2.0, 3.0, 2.0, 1.0, 0.0, -1.0]
    w = within_rows(t, xy, [0.5, 1.5, -1.0, 1.0])
    assert w["enter_t"] == t[1] and w["leave_t"] == t[5] and w["counts"].tolist() == [8, 2]
    w = within_rows(t, xy, [0.5, 1.5, -1.0, 1.0], t_from=t[2])
    assert w["enter_t"] == t[5] and w["leave_t"] == t[5] and w["counts"].tolist() == [6, 1]


# one smooth planar curve cut into two position pieces of 2 s and three yaw pieces of 4/3 s: the pieces are Taylor shifts of one polynomial
PX = Polynomial([0.3, 0.4, 0.0, 0.01, -0.0005])
PY = Polynomial([-0.2, 0.0, 0.1, -0.01])
PW = Polynomial([0.3, 0.2, -0.01])
TOTAL = 4.0
SHIFT = (12.5, -7.25)


def _pieces(P, n):
    T = TOTAL / n
    out = []
    for i in range(n):
        c = P(Polynomial([i * T, 1.0])).coef
        out.append(np.concatenate([c, np.zeros(6 - c.shape[0])]))
    return np.array(out), T


@pytest.fixture(scope="module")
def curve():
    cx, Tx = _pieces(PX, 2)
    cy, _ = _pieces(PY, 2)
    cw, Tw = _pieces(PW, 3)
    c_xy = np.stack([cx, cy], axis=2).reshape(12, 2)                  # power k of dim d of piece i at row 6 i + k
    traj = SE2Traj(c_xy, cw.reshape(18), Tx, Tw)
    t, rows = 0.0, []
    while t < TOTAL:
        rows.append(t)
        t += 0.01
    rows = np.array(rows + [TOTAL])
    xy = np.array([[traj.getState(v)[0] + SHIFT[0], traj.getState(v)[1] + SHIFT[1]] for v in rows])      # as the rollout forms a STATE row
    return traj, rows, xy


def _kin(t):
    p = np.array([PX(t) + SHIFT[0], PY(t) + SHIFT[1]])
    v = np.array([PX.deriv()(t), PY.deriv()(t)])
    a = np.array([PX.deriv(2)(t), PY.deriv(2)(t)])
    return p, v, a


def _bar(v, e, a):
    """G: the project's per-evaluation bar 1e-9 on the scale of h = |v|^2 + e . a"""
    return 1e-9 * max(1.0, v @ v + np.hypot(*e) * np.hypot(*a))


def _d2(state, pose):
    ex, ey = state[0] - pose[0], state[1] - pose[1]
    return ex * ex + ey * ey


def _p2_p3(r, c, pose):
    """P2 and P3 of tests/test_gpu_locate.py on one mirror result r (coarse stage c)"""
    j, times = c["j"], c["times"]
    lo, hi = times[max(j - 1, 0)], times[min(j + 1, len(times) - 1)]
    assert r["lo"] == lo and r["hi"] == hi and lo <= r["t"] <= hi
    assert r["d2"] == _d2(r["state"], pose) and r["d2"] <= c["near_d2"]
    assert r["refined"] in (0, 1) and (r["refined"] == 1 or r["t"] == c["near_t"])
    assert 1 <= r["iters"] <= LOCATE_NEWTON
    s = r["state"]
    e = s[:2] - np.asarray(pose[:2])
    if lo < r["t"] < hi:
        assert abs(e @ s[2:4]) <= _bar(s[2:4], e, s[4:6]), (r["t"], e @ s[2:4])
    assert np.array_equal(r["err"], locate_errors(s, pose))


def test_locate_refine_known_answers_and_brute_force(curve):
    traj, rows, xy = curve
    rng = np.random.default_rng(5)
    used = 0
    for t0 in rng.uniform(0.2 * TOTAL, 0.8 * TOTAL, 24):
        p, v, a = _kin(t0)
        nrm = np.array([-v[1], v[0]]) / np.hypot(*v)
        for delta in (0.05, -0.05, 0.2, -0.2):
            pose = np.concatenate([p + delta * nrm, [PW(t0) + 0.1]])
            c = locate_rows(rows, xy, pose, t0 - 0.5, t0 + 0.5)
            assert 99 <= c["count"] <= 101 and abs(c["near_t"] - t0) <= 0.011
            r = locate_refine(traj, SHIFT, pose, c["times"], c["j"])
            _p2_p3(r, c, pose)
            assert r["refined"] == 1 and r["lo"] < r["t"] < r["hi"]
            # P4: the answer is t0, to the bar expressed in time
            e0 = p - pose[:2]
            h0 = v @ v + e0 @ a
            assert np.hypot(*v) >= 0.1 and h0 >= 0.5 * (v @ v)
            assert abs(r["t"] - t0) * h0 <= _bar(v, e0, a), (t0, delta, r["t"] - t0)
            # dense brute force over the bracket: nothing on it is nearer
            dense = min(_d2([PX(u) + SHIFT[0], PY(u) + SHIFT[1]], pose) for u in np.linspace(r["lo"], r["hi"], 401))
            assert r["d2"] <= dense * (1.0 + 1e-12)
            # the tracking error of a pose on the normal: no longitudinal part, delta across, the yaw offset
            psi = r["state"][9]
            side = np.sign(np.cos(psi) * nrm[1] - np.sin(psi) * nrm[0])
            assert abs(r["err"][0]) <= 0.2 * abs(np.sin(psi - np.arctan2(v[1], v[0]))) + 1e-9
            assert abs(np.hypot(r["err"][0], r["err"][1]) - abs(delta)) <= 1e-9 and np.sign(r["err"][1]) == side * np.sign(delta)
            assert abs(r["err"][2] - norm_so2(pose[2] - psi)) == 0.0 and abs(r["err"][2] - 0.1) <= 1e-6
            used += 1
    assert used == 96


def test_locate_refine_small_windows_and_winners_at_the_ends(curve):
    traj, rows, xy = curve
    k = 137
    pose_mid = np.array([*(0.3 * xy[k] + 0.7 * xy[k + 1]), 0.0])     # between rows k and k + 1, nearer to k + 1
    # windows of 1, 2 and 3 samples
    for lo_k, hi_k in ((k + 1, k + 1), (k, k + 1), (k + 1, k + 2), (k, k + 2), (k - 1, k + 1)):
        c = locate_rows(rows, xy, pose_mid, rows[lo_k], rows[hi_k])
        assert c["count"] == hi_k - lo_k + 1 and c["near_t"] == rows[k + 1]
        r = locate_refine(traj, SHIFT, pose_mid, c["times"], c["j"])
        _p2_p3(r, c, pose_mid)
        if lo_k == hi_k:                                             # one sample: the bracket is a point
            assert r["t"] == rows[k + 1] and r["d2"] == c["near_d2"] and r["iters"] == 1
        elif lo_k <= k:                                              # the bracket holds the foot of the pose
            assert r["refined"] == 1 and rows[k] < r["t"] < rows[k + 1] and r["d2"] < c["near_d2"]
        else:                                                        # the foot lies before the window: the winner is its first sample and stays
            assert r["t"] == rows[k + 1] and r["lo"] == rows[k + 1]
    # a winner at either end of a longer window, the foot outside it
    for a_k, b_k, pose_k, want in ((k, k + 60, k - 30, k), (k - 60, k, k + 30, k)):
        pose = np.array([*xy[pose_k], 0.0])
        c = locate_rows(rows, xy, pose, rows[a_k], rows[b_k])
        assert c["near_t"] == rows[want] and c["j"] in (0, 60)
        r = locate_refine(traj, SHIFT, pose, c["times"], c["j"])
        _p2_p3(r, c, pose)
        assert r["t"] == rows[want] and r["d2"] == c["near_d2"]
    # a pose exactly on a sample: g = 0 there at once
    pose = np.array([*xy[k], 0.0])
    c = locate_rows(rows, xy, pose)
    r = locate_refine(traj, SHIFT, pose, c["times"], c["j"])
    _p2_p3(r, c, pose)
    assert r["t"] == rows[k] and r["d2"] == 0.0 and r["refined"] == 1
    # an empty window answers NaN
    r = locate_refine(traj, SHIFT, pose, rows[:0], -1)
    assert np.isnan(r["t"]) and r["refined"] == 0 and r["d2"] == INF and np.isnan(r["state"]).all() and np.isnan(r["err"]).all()
    # a pose at 1e200: every d2 is +inf, sample 0 is kept
    far = np.array([1e200, 0.0, 0.0])
    c = locate_rows(rows, xy, far)
    r = locate_refine(traj, SHIFT, far, c["times"], c["j"])
    assert c["j"] == 0 and c["near_t"] == rows[0] and r["d2"] == INF and r["lo"] == rows[0] <= r["t"] <= r["hi"] == rows[1]
