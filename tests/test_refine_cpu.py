"""CPU tier of refining resident trajectories without a new search (uph_refine_upload: the rest of each trajectory after a switch time becomes a new
problem, started from the state there, seeded with the trajectory itself) and of evaluating them at given times (uph_traj_states): the C-ABI and
its binding, the refusals that need no device, the host rule for the remaining time, the piece counts and the way-point times (refine_counts, which
tests/test_gpu_refine.py reuses), the Python door and the C++ adapter's refineSE2TrajBatch.  The GPU tier is tests/test_gpu_refine.py."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from uneven_planner_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dp(a):
    return a.ctypes.data_as(_lib.DP)


def refine_counts(T_xy, n_xy, T_yaw, n_yaw, t_switch):
    """uph_refine_upload's host rule for one query on a trajectory of n_xy pieces of T_xy and n_yaw pieces of T_yaw: the duration D as the rollout
    forms it (running sums of the piece durations, the smaller one), tc = t_switch clamped to [0, D], R = D - tc.  R <= 0: None (UPH_REFINE_AT_END).
    Otherwise N' = max(1, nearbyint(R / T_xy)), M' = max(N', nearbyint(R / T_yaw)) and the way-point times tc + k (R / N'), k = 1 .. N' - 1, and
    tc + k (R / M'), k = 1 .. M' - 1, formed as the library forms them (one rounding per operation, no contraction)"""
    T_xy, T_yaw = float(T_xy), float(T_yaw)
    dx = dy = 0.0
    for _ in range(int(n_xy)):
        dx += T_xy
    for _ in range(int(n_yaw)):
        dy += T_yaw
    D = dx if dx < dy else dy
    t = float(t_switch)
    tc = 0.0 if t <= 0.0 else (D if t >= D else t)
    R = D - tc
    if not R > 0.0:
        return None
    n = max(1, int(np.rint(R / T_xy)))
    m = max(n, int(np.rint(R / T_yaw)))
    hx, hy = R / n, R / m
    return dict(D=D, tc=tc, R=R, n_xy=n, n_yaw=m, t_xy=np.array([tc + k * hx for k in range(1, n)]), t_yaw=np.array([tc + k * hy for k in range(1, m)]))


def test_symbols_are_exported_with_the_binding_signatures():
    L = _lib.load()
    a = _lib.SYMBOLS["uph_traj_states"][1]
    assert a == [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), _lib.DP, _lib.DP]
    r = _lib.SYMBOLS["uph_refine_upload"][1]
    assert r[:5] == [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), _lib.DP] and r[5] == _lib.DP and len(r) == 10
    assert all(x == C.POINTER(C.c_int32) for x in r[6:])
    for name, args in (("uph_traj_states", a), ("uph_refine_upload", r)):
        fn = getattr(L, name)
        assert fn.restype == C.c_int and fn.argtypes == args
    hdr = open(os.path.join(ROOT, "include", "uneven_hip.h")).read()
    assert "int uph_traj_states(uph_ctx* c, int32_t n, const int32_t* traj, const double* t, double* out10);" in hdr
    assert "int uph_refine_upload(uph_ctx* src, uph_ctx* dst, int32_t B, const int32_t* src_traj, const double* t_switch," in hdr
    assert "#define UPH_REFINE_AT_END 7" in hdr and _lib.UPH_REFINE_AT_END == 7 and _lib.TRAJ_STATE_COLS == 10


def test_refusals_need_no_device():
    """null handles and arrays and n / B <= 0 are refused before any HIP call: UPH_ERR_INVALID, every output untouched"""
    L = _lib.load()
    fake = C.c_void_p(0x1000)            # never dereferenced: every call below fails its argument check first
    tr, ts = np.zeros(4, dtype=np.int32), np.zeros(4)
    out = np.full((4, 10), 7.0)
    full = [fake, 4, _ip(tr), _dp(ts), _dp(out)]
    for i in (0, 2, 3, 4):
        a = list(full)
        a[i] = None
        assert L.uph_traj_states(*a) == -1, i
        assert b"uph_traj_states" in L.uph_last_error()
    for n in (0, -3):
        a = list(full)
        a[1] = n
        assert L.uph_traj_states(*a) == -1
    sw = np.full((4, 10), 7.0)
    st, to, nx, ny = (np.full(4, 7, dtype=np.int32) for _ in range(4))
    full = [fake, fake, 4, _ip(tr), _dp(ts), _dp(sw), _ip(st), _ip(to), _ip(nx), _ip(ny)]
    for i in (0, 1, 3, 4, 6, 7, 8, 9):                     # each required pointer NULL in turn (switch_states may be NULL)
        a = list(full)
        a[i] = None
        assert L.uph_refine_upload(*a) == -1, i
        assert b"uph_refine_upload" in L.uph_last_error()
    for B in (0, -2):
        a = list(full)
        a[2] = B
        assert L.uph_refine_upload(*a) == -1
    assert (out == 7.0).all() and (sw == 7.0).all() and (st == 7).all() and (to == 7).all() and (nx == 7).all() and (ny == 7).all()


# (n_xy, T_xy, n_yaw, T_yaw): both blocks share the total time, as a solved trajectory's do; durations that are not binary fractions, so that
# the running sums round
TRAJS = [(5, 0.37, 10, 0.185), (7, 0.41, 12, 0.41 * 7 / 12), (1, 0.8, 2, 0.4), (4, 0.3, 9, 1.2 / 9), (3, 0.6, 9, 0.2), (128, 0.3, 256, 0.15),
         (31, 0.2937, 62, 0.2937 / 2)]


def _check(c, nxy, Txy, nyw, Tyw):
    n, m = c["n_xy"], c["n_yaw"]
    assert 1 <= n <= nxy and n <= m <= nyw
    assert n <= 1 or abs(n - c["R"] / Txy) <= 0.5 + 1e-12
    assert n == max(1, int(np.rint(c["R"] / Txy))) and m == max(n, int(np.rint(c["R"] / Tyw)))
    for tt, k in ((c["t_xy"], n), (c["t_yaw"], m)):
        assert tt.shape == (k - 1,)
        if k > 1:
            assert c["tc"] < tt[0] and (np.diff(tt) > 0).all() and tt[-1] < c["D"]
            assert np.allclose(np.diff(np.concatenate([[c["tc"]], tt, [c["D"]]])), c["R"] / k, rtol=1e-12, atol=1e-12)


def test_count_rule():
    """refine_counts at t = 0 (and before it: the source's counts), at xy knots (N' = Nxy - k), at yaw-only knots (M' = Nyaw - k), halfway through a
    piece, within 1e-12 of the end (one piece each, no way-point), at the end and past it (nothing left)"""
    for nxy, Txy, nyw, Tyw in TRAJS:
        for t0 in (0.0, -1.0, -1e-300):
            c = refine_counts(Txy, nxy, Tyw, nyw, t0)
            assert (c["tc"], c["n_xy"], c["n_yaw"], c["R"]) == (0.0, nxy, nyw, c["D"])
            _check(c, nxy, Txy, nyw, Tyw)
        for k in range(1, nxy):
            c = refine_counts(Txy, nxy, Tyw, nyw, k * Txy)
            assert c["n_xy"] == nxy - k and c["n_yaw"] == max(nxy - k, int(np.rint(c["R"] / Tyw))), (nxy, k)
            _check(c, nxy, Txy, nyw, Tyw)
        for k in range(1, nyw):
            if (k * Tyw / Txy) % 1.0 < 1e-9 or (k * Tyw / Txy) % 1.0 > 1 - 1e-9:
                continue                                        # (an xy knot too)
            c = refine_counts(Txy, nxy, Tyw, nyw, k * Tyw)
            assert c["n_yaw"] == max(c["n_xy"], nyw - k), (nyw, k)
            _check(c, nxy, Txy, nyw, Tyw)
        for k in range(nxy):
            c = refine_counts(Txy, nxy, Tyw, nyw, (k + 0.5) * Txy)
            assert c["n_xy"] in (max(1, nxy - k - 1), nxy - k)
            _check(c, nxy, Txy, nyw, Tyw)
        D = refine_counts(Txy, nxy, Tyw, nyw, 0.0)["D"]
        c = refine_counts(Txy, nxy, Tyw, nyw, D - 1e-12)
        assert c["n_xy"] == c["n_yaw"] == 1 and c["t_xy"].size == c["t_yaw"].size == 0 and 0.0 < c["R"] < 2e-12
        for t in (D, D + 1e-12, D + 5.0, 1e300):
            assert refine_counts(Txy, nxy, Tyw, nyw, t) is None
    assert _lib.UPH_REFINE_AT_END == 7


# ---- the Python door and the C++ adapter --------------------------------------------------------------------------------------------------------
class _FakeLib:
    """stands in for the library behind ALMTrajOpt.refine_upload: returns `rc` and, when `write` is given, writes those statuses and the switch
    states (as uph_refine_upload writes its outputs: all together)"""

    def __init__(self, rc, write=None):
        self.rc, self.write = rc, write

    def uph_refine_upload(self, src, dst, B, tr, ts, sw, st, to, nx, ny):
        if self.write is not None:
            for b, v in enumerate(self.write):
                st[b], to[b], nx[b], ny[b] = v, (b if v == 0 else -1), 0, 0
                for k in range(10):
                    sw[10 * b + k] = float(k)
        return self.rc

    def uph_last_error(self):
        return _lib.load().uph_last_error()


def _fake_opt(fake):
    import uneven_planner_amd as U
    opt = U.ALMTrajOpt.__new__(U.ALMTrajOpt)      # (no device: the contexts are never touched, only the return code and the outputs are read)
    opt.L, opt.h, opt.int_K = fake, None, 16
    opt._B, opt._sizes, opt._last = 5, [None] * 5, [None] * 5
    return opt


def test_refine_raises_on_every_failure_but_all_at_end():
    """only "no query left to refine" (UPH_ERR_INVALID with the outputs written, every status UPH_REFINE_AT_END) is an empty batch; a refusal raises
    and leaves the object's batch bookkeeping as it was; a failure after the outputs were written raises and leaves no batch; shapes are checked
    before the call"""
    src = types.SimpleNamespace(h=None)
    opt = _fake_opt(_FakeLib(-1, write=[7, 7]))
    plan = opt.refine_upload(src, [0, 1], [5.0, 9.0])
    assert plan["status"].tolist() == [7, 7] and (plan["traj_of"] == -1).all() and opt._B == 0
    assert np.array_equal(plan["switch_states"], np.tile(np.arange(10.0), (2, 1)))
    assert [r["status"] for r in _fake_opt(_FakeLib(-1, write=[7, 7])).refine(src, [0, 1], [5.0, 9.0])] == [7, 7]
    refused = _fake_opt(_FakeLib(-1))
    with pytest.raises(_lib.UnevenHipError):
        refused.refine_upload(src, [0, 1], [0.5, 1.0])
    assert refused._B == 5
    for fake in (_FakeLib(-2), _FakeLib(-4, write=[0, 7]), _FakeLib(-1, write=[0, 7])):
        o = _fake_opt(fake)
        with pytest.raises(_lib.UnevenHipError):
            o.refine_upload(src, [0, 1], [0.5, 1.0])
        assert o._B == 0
    for bad in (dict(src_traj=[], t_switch=[]), dict(src_traj=[0, 1], t_switch=[0.5])):
        with pytest.raises(_lib.UnevenHipError):
            _fake_opt(_FakeLib(0)).refine_upload(src, **bad)
    with pytest.raises(_lib.UnevenHipError):
        _fake_opt(_FakeLib(0)).traj_states([0, 1], [0.5])


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
int refine(uneven_hip::UnevenMapHandle* map) {
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
    uneven_hip::ALMTrajOpt::GoalPlan r = opt.refineSE2TrajBatch(traj, ts);                         // map changed, same goal, same route
    int n = 0;
    for (size_t q = 0; q < r.ret.size(); q++) {
        if (r.status[q] == UPH_REFINE_AT_END) continue;
        n += r.ret[q] == 0 ? 1 : 0;
    }
    if (n < (int)r.ret.size()) r = opt.replanSE2TrajBatch(kino, traj, ts, nullptr, mgr);     // the fallback: search again
    return n;
}
"""


def test_adapter_refine_se2_traj_batch_compiles(tmp_path):
    src = tmp_path / "refine.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "refine.o")])
