"""CPU tier of re-planning from states on resident trajectories (uph_replan_upload: a vehicle that follows a solved trajectory gets a new goal, or
learns that the map changed, and its next plan starts from the state it will have at the switch time): the C-ABI and its binding, argument refusals
that need no device, the host mirror SE2Traj.getState of the device's switch state, and the C++ adapter's replanSE2TrajBatch.  The GPU tier is
tests/test_gpu_replan.py."""
import ctypes as C
import math
import os
import subprocess
import types

import numpy as np
import pytest

from uneven_planner_amd import _lib
from uneven_planner_amd import resample as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dp(a):
    return a.ctypes.data_as(_lib.DP)


def test_symbol_is_exported_with_the_binding_signature():
    L = _lib.load()
    args = _lib.SYMBOLS["uph_replan_upload"][1]
    assert args[:4] == [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_lib.ManagerParams)] and len(args) == 14
    assert args[5] == C.POINTER(C.c_int32) and args[6] == args[7] == args[9] == _lib.DP and args[8] == C.c_int32
    fn = L.uph_replan_upload
    assert fn.restype == C.c_int and fn.argtypes == args
    hdr = open(os.path.join(ROOT, "include", "uneven_hip.h")).read()
    assert "int uph_replan_upload(uph_kino* k, uph_ctx* src, uph_ctx* dst, const uph_manager_params* mp, int32_t B, const int32_t* src_traj," in hdr


def test_refusals_need_no_device():
    """null handles and arrays, B <= 0, a negative path_cap and manager parameters the stage cannot walk with are refused before any HIP call:
    UPH_ERR_INVALID, every output untouched"""
    L = _lib.load()
    mp = _lib.ManagerParams(**R.MANAGER_PARAMS)
    tr, ts, g = np.zeros(4, dtype=np.int32), np.zeros(4), np.ones((4, 3))
    sw = np.full((4, 9), 7.0)
    st, to, nx, ny = (np.full(4, 7, dtype=np.int32) for _ in range(4))
    fake = C.c_void_p(0x1000)            # never dereferenced: every call below fails its argument check first
    full = [fake, fake, fake, C.byref(mp), 4, _ip(tr), _dp(ts), _dp(g), 0, _dp(sw), _ip(st), _ip(to), _ip(nx), _ip(ny)]
    for i in (0, 1, 2, 3, 5, 6, 10, 11, 12, 13):           # each required pointer NULL in turn (goals and switch_states may be NULL)
        a = list(full)
        a[i] = None
        assert L.uph_replan_upload(*a) == -1, i
        assert b"uph_replan_upload" in L.uph_last_error()
    for B in (0, -2):
        a = list(full)
        a[4] = B
        assert L.uph_replan_upload(*a) == -1
    a = list(full)
    a[8] = -1
    assert L.uph_replan_upload(*a) == -1
    for kw in (dict(piece_len=0.0), dict(yaw_piece_times=-1.0), dict(mean_vel=0.0), dict(test_mode=1, test_max_vel=0.0)):
        q = dict(R.MANAGER_PARAMS)
        q.update(kw)
        bad = _lib.ManagerParams(**q)
        a = list(full)
        a[3] = C.byref(bad)
        assert L.uph_replan_upload(*a) == -1, kw
    assert (st == 7).all() and (to == 7).all() and (nx == 7).all() and (ny == 7).all() and (sw == 7.0).all()


# ---- SE2Traj.getState: the host mirror of the device's switch state ----------------------------------------------------------------------------
def _traj(seed, nxy, nyaw, Txy, Tyaw):
    from uneven_planner_amd.alm_traj_opt import SE2Traj
    rng = np.random.default_rng(seed)
    c_xy = rng.normal(size=(6 * nxy, 2)) * np.array([1.0, 0.7])          # C-ABI layout: row 6 i + k = power k of piece i, columns x, y
    c_yaw = rng.normal(size=6 * nyaw) * 2.0
    c_yaw[0] += 9.0                                                       # an unwrapped yaw beyond pi: normSO2 must fold it
    return SE2Traj(c_xy, c_yaw, Txy, Tyaw), c_xy, c_yaw


def _locate(T, n, t):
    """the reference's PolyTrajectory::locatePieceIdx (se2traj.hpp:343-361) for n pieces of duration T"""
    idx = 0
    while idx < n and t > T:
        t -= T
        idx += 1
    if idx == n:
        idx -= 1
        t += T
    return idx, t


def _numpy_state(c_xy, c_yaw, nxy, nyaw, Txy, Tyaw, t):
    tot = min(sum([Txy] * nxy), sum([Tyaw] * nyaw))
    t = min(max(t, 0.0), tot)
    ix, tl = _locate(Txy, nxy, t)
    iw, tw = _locate(Tyaw, nyaw, t)
    out = []
    for d in range(2):
        p = c_xy[6 * ix:6 * ix + 6, d][::-1]                               # np.polyval wants the highest power first
        out.append([np.polyval(p, tl), np.polyval(np.polyder(p), tl), np.polyval(np.polyder(p, 2), tl)])
    py = c_yaw[6 * iw:6 * iw + 6][::-1]
    w = np.polyval(py, tw)
    return np.array([out[0][0], out[1][0], out[0][1], out[1][1], out[0][2], out[1][2], math.atan2(math.sin(w), math.cos(w)),
                     np.polyval(np.polyder(py), tw), np.polyval(np.polyder(py, 2), tw)])


def _close(a, b, tol):
    d = np.abs(np.asarray(a) - np.asarray(b))
    d[6] = abs(math.remainder(a[6] - b[6], 2 * math.pi))                  # yaw modulo 2 pi (normSO2 vs atan2 at +-pi)
    return (d <= tol * np.maximum(1.0, np.abs(b))).all(), d


def test_get_state_matches_numpy_evaluation():
    """getState against np.polyval on the same coefficients with the piece located by locatePieceIdx: at every piece boundary (the boundary
    belongs to the earlier piece), inside pieces, at 0, at the duration and clamped beyond both ends (durations 0.37 and 0.185 are not binary
    fractions: the running sums round)"""
    for seed, (nxy, nyaw, Txy, Tyaw) in enumerate([(5, 10, 0.37, 0.185), (1, 2, 0.8, 0.4), (7, 7, 0.25, 0.25), (3, 9, 0.6, 0.21)]):
        tr, c_xy, c_yaw = _traj(seed, nxy, nyaw, Txy, Tyaw)
        tot = tr.getTotalDuration()
        ts = [0.0, -1.0, -1e-300, tot, tot + 5.0, 1e9, 0.5 * tot, 0.999 * tot]
        ts += [i * Txy for i in range(1, nxy)] + [i * Tyaw for i in range(1, nyaw)]
        ts += [i * Txy + 1e-9 for i in range(nxy)] + [(i + 0.5) * Tyaw for i in range(nyaw)]
        ts += list(np.random.default_rng(seed).uniform(0, tot, 25))
        for t in ts:
            got, want = tr.getState(t), _numpy_state(c_xy, c_yaw, nxy, nyaw, Txy, Tyaw, t)
            ok, d = _close(got, want, 1e-11)
            assert ok, (seed, t, d)
        assert np.array_equal(tr.getState(-3.0), tr.getState(0.0)) and np.array_equal(tr.getState(tot + 1.0), tr.getState(tot))
        assert -math.pi <= tr.getState(0.0)[6] <= math.pi


def test_get_state_derivatives_agree_with_central_differences():
    tr, _, _ = _traj(11, 6, 12, 0.41, 0.205)
    h = 1e-6
    for t in np.linspace(0.05, tr.getTotalDuration() - 0.05, 37):
        if min(abs(t / 0.205 - round(t / 0.205)), abs(t / 0.41 - round(t / 0.41))) < 1e-4:
            continue                                                      # (a difference across a piece boundary sees two polynomials)
        a, b, s = tr.getState(t - h), tr.getState(t + h), tr.getState(t)
        fd_v = (b[:2] - a[:2]) / (2 * h)
        fd_a = (b[2:4] - a[2:4]) / (2 * h)
        fd_w = math.remainder(b[6] - a[6], 2 * math.pi) / (2 * h)
        fd_ww = (b[7] - a[7]) / (2 * h)
        assert np.allclose(fd_v, s[2:4], rtol=1e-6, atol=1e-6) and np.allclose(fd_a, s[4:6], rtol=1e-6, atol=1e-6), t
        assert abs(fd_w - s[7]) <= 1e-6 * max(1.0, abs(s[7])) and abs(fd_ww - s[8]) <= 1e-6 * max(1.0, abs(s[8])), t


def test_norm_so2_is_the_devices_loop():
    from uneven_planner_amd.alm_traj_opt import norm_so2
    for y in (0.0, math.pi, -math.pi, 3.2, -3.2, 9.0, -20.5, 1e3):
        v = y
        while v < -math.pi:
            v += 2 * math.pi
        while v > math.pi:
            v -= 2 * math.pi
        assert norm_so2(y) == v


# ---- the Python door and the C++ adapter --------------------------------------------------------------------------------------------------------
class _FakeLib:
    """stands in for the library behind ALMTrajOpt.replan_goals_upload: returns `rc` and, when `write` is given, writes those statuses and the switch
    states (as uph_replan_upload writes its outputs: all together)"""

    def __init__(self, rc, write=None):
        self.rc, self.write = rc, write

    def uph_replan_upload(self, kh, src, dst, mp, B, tr, ts, g, cap, sw, st, to, nx, ny):
        if self.write is not None:
            for b, v in enumerate(self.write):
                st[b], to[b], nx[b], ny[b] = v, (b if v == 0 else -1), 0, 0
                for k in range(9):
                    sw[9 * b + k] = float(k)
        return self.rc

    def uph_last_error(self):
        return _lib.load().uph_last_error()


def _fake_opt(fake):
    import uneven_planner_amd as U
    opt = U.ALMTrajOpt.__new__(U.ALMTrajOpt)      # (no device: the contexts are never touched, only the return code and the outputs are read)
    opt.L, opt.h, opt.int_K = fake, None, 16
    opt._B, opt._sizes, opt._last = 5, [None] * 5, [None] * 5
    return opt


def test_replan_goals_raises_on_every_failure_but_no_path():
    """only "no query produced a path" (UPH_ERR_INVALID with the outputs written, no UPH_KINO_OK among them) is an empty batch; a refusal raises and
    leaves the object's batch bookkeeping as it was (the library leaves dst's batch as it was); argument shapes are checked before the call"""
    kino, src = types.SimpleNamespace(h=None), types.SimpleNamespace(h=None)
    opt = _fake_opt(_FakeLib(-1, write=[3, 1]))
    plan = opt.replan_goals_upload(kino, src, [0, 1], [0.5, 1.0])
    assert plan["status"].tolist() == [3, 1] and (plan["traj_of"] == -1).all() and opt._B == 0
    assert np.array_equal(plan["switch_states"], np.tile(np.arange(9.0), (2, 1)))
    out = _fake_opt(_FakeLib(-1, write=[3, 6])).replan_goals(kino, src, [0, 1], [0.5, 1.0])
    assert [r["status"] for r in out] == [3, 6]
    refused = _fake_opt(_FakeLib(-1))
    with pytest.raises(_lib.UnevenHipError):
        refused.replan_goals_upload(kino, src, [0, 1], [0.5, 1.0])
    assert refused._B == 5
    for fake in (_FakeLib(-2), _FakeLib(-4, write=[0, 3]), _FakeLib(-1, write=[0, 3])):
        with pytest.raises(_lib.UnevenHipError):
            _fake_opt(fake).replan_goals_upload(kino, src, [0, 1], [0.5, 1.0])
    for bad in (dict(src_traj=[], t_switch=[]), dict(src_traj=[0, 1], t_switch=[0.5]), dict(src_traj=[0], t_switch=[0.5], goals=np.zeros((2, 3)))):
        with pytest.raises(_lib.UnevenHipError):
            _fake_opt(_FakeLib(0)).replan_goals_upload(kino, src, **bad)
    with pytest.raises(TypeError):
        _fake_opt(_FakeLib(0)).replan_goals_upload(kino, src, [0], [0.5], pice_len=0.3)


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
int replan(uneven_hip::UnevenMapHandle* map) {
    uneven_hip::KinoAstar kino;
    kino.setEnvironment(map);
    uneven_hip::ALMTrajOpt opt;
    opt.setEnvironment(map);
    std::vector<std::array<double, 3>> starts(2, std::array<double, 3>{{0.0, 0.0, 0.0}}), goals(2, std::array<double, 3>{{2.0, 1.0, 0.5}});
    uph_manager_params mgr{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5};
    uneven_hip::ALMTrajOpt::GoalPlan p = opt.planSE2TrajBatch(kino, starts, goals, mgr);
    std::vector<int> traj;
    std::vector<double> ts;
    for (size_t b = 0; b < p.traj_of.size(); b++) if (p.traj_of[b] >= 0) { traj.push_back(p.traj_of[b]); ts.push_back(0.5 * p.total_time[b]); }
    std::vector<std::array<double, 3>> next(traj.size(), std::array<double, 3>{{-1.0, 2.0, 1.0}});
    uneven_hip::ALMTrajOpt::GoalPlan q = opt.replanSE2TrajBatch(kino, traj, ts, &next, mgr);           // new goal while driving
    uneven_hip::ALMTrajOpt::GoalPlan r = opt.replanSE2TrajBatch(kino, traj, ts, nullptr, mgr, 512);     // map changed, same goal
    int n = 0;
    for (size_t b = 0; b < q.ret.size(); b++) n += q.traj_of[b] >= 0 && q.ret[b] == 0 ? 1 : 0;
    for (size_t b = 0; b < r.ret.size(); b++) n += r.traj[b].getTotalDuration() > 0.0 ? 1 : 0;
    return n;
}
"""


def test_adapter_replan_se2_traj_batch_compiles(tmp_path):
    src = tmp_path / "replan.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "replan.o")])
