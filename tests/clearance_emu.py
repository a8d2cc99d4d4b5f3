"""TEST SCAFFOLDING: the CPU emulator of the workgroup program (tests/emu_bridge.py) built from tests/emu/emu_clearance.cpp, which adds one objective
evaluation of the program instantiated WITH the clearance term (Solver<HostWG, double, true>) and the shared field function on the emulator's grid."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu_bridge as E

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBS = {}


def lib(late=False):
    """the emulator's library; late: the build with -DEMU_CLEAR_LOADS_LATE (ClearLoadsLate<HostWG> true: the statement order of the 512-lane device kernels)"""
    _L = _LIBS.get(bool(late))
    if _L is None:
        so = os.path.join(_HERE, "emu", "libemu_clearance_late.so" if late else "libemu_clearance.so")
        srcs = [os.path.join(_HERE, "emu", f) for f in ("emu_clearance.cpp", "emu_solver.cpp")]
        csrc = os.path.join(_HERE, "..", "uneven_planner_amd", "csrc")
        deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + (["-DEMU_CLEAR_LOADS_LATE"] if late else []) + ["-o", so, srcs[0]])
        L = C.CDLL(so)
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint16)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [dp, dp, dp]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_set_lanes.argtypes = [C.c_int]
        L.emu_clear_field.argtypes = [C.c_void_p, up, C.c_int, dp, C.c_int, dp, dp]
        L.emu_clear_eval.argtypes = [C.c_void_p, C.c_int, up, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int] + [dp] * 12
        L.emu_clear_run.argtypes = [C.c_void_p, C.c_int, up, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int] + [dp] * 14 + [C.POINTER(C.c_longlong)]
        L.emu_clear_set_trial_abandon.argtypes = [C.c_void_p, C.c_int]
        L.emu_clear_loads_late.restype = C.c_int
        assert L.emu_clear_loads_late() == int(bool(late))
        _L = _LIBS[bool(late)] = L
    return _L


class ClearanceEmu(E.Emu):
    def __init__(self, cells, map_params_vec, opt_params_vec, lanes=128, late=False):
        self.L = lib(late)
        self.lanes = int(lanes)
        self.cells = np.ascontiguousarray(cells, dtype=np.float64)
        self.mp = np.ascontiguousarray(map_params_vec, dtype=np.float64)
        self.op = np.ascontiguousarray(opt_params_vec, dtype=np.float64)
        self.K = int(self.op[20])
        self.h = self.L.emu_create(E._dp(self.mp), E._dp(self.cells), E._dp(self.op))

    def field(self, D, rmax, pos):
        D = np.ascontiguousarray(D, dtype=np.uint16)
        p = np.ascontiguousarray(np.asarray(pos, dtype=np.float64).reshape(-1, 3))
        c, g = np.zeros(p.shape[0]), np.zeros((p.shape[0], 2))
        self.L.emu_clear_field(self.h, D.ctypes.data_as(C.POINTER(C.c_uint16)), int(rmax), E._dp(p), p.shape[0], E._dp(c), E._dp(g))
        return c, g

    def eval(self, prob, x, term=None, lam=None, mu=None, scale_cx=None, rho=1.0, scale_fx=1.0):
        """one objective evaluation at x; term = None (the plain program) or (D, rmax, d_safe, weight).  Returns f, g, c_xy, c_yaw, T_xy, T_yaw."""
        self.L.emu_set_lanes(self.lanes)
        nxy, nyaw = prob["inner_xy"].shape[1], prob["inner_yaw"].shape[0]
        S, n = (nxy + 1) * (self.K + 1), 2 * nxy + nyaw + 1
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        x = f64(x).copy()
        g = np.zeros(n)
        lam = np.zeros(S) if lam is None else f64(lam)
        mu = np.zeros(6 * S) if mu is None else f64(mu)
        sc = np.ones(7 * S) if scale_cx is None else f64(scale_cx)
        cxy, cyaw = np.zeros((6 * (nxy + 1), 2)), np.zeros(6 * (nyaw + 1))
        scal = np.zeros(8)
        scal[0], scal[1] = rho, scale_fx
        if term is None:
            D, rmax, d_safe, weight, on = np.zeros(1, dtype=np.uint16), 1, 0.0, 0.0, 0
        else:
            D, rmax, d_safe, weight = term
            D, on = np.ascontiguousarray(D, dtype=np.uint16), 1
        ixy, exy, iy, ey = f64(prob["init_xy"].T), f64(prob["end_xy"].T), f64(prob["init_yaw"]), f64(prob["end_yaw"])
        self.L.emu_clear_eval(self.h, on, D.ctypes.data_as(C.POINTER(C.c_uint16)), int(rmax), float(d_safe), float(weight), nxy, nyaw, E._dp(ixy), E._dp(exy),
                              E._dp(iy), E._dp(ey), E._dp(x), E._dp(g), E._dp(lam), E._dp(mu), E._dp(sc), E._dp(cxy), E._dp(cyaw), E._dp(scal))
        return dict(f=scal[2], g=g, c_xy=cxy, c_yaw=cyaw, T_xy=scal[4], T_yaw=scal[5])

    def run_term(self, mode, prob, x, term, lam=None, mu=None, scale_cx=None, rho=1.0, scale_fx=1.0):
        """emu_bridge.Emu.run's modes 0 (one evaluation at x) and 2 (the solve from x) with the program instantiated WITH the term = (D, rmax, d_safe, weight);
        the same dict: x, f, g, hx, gx, c_xy, c_yaw, T_xy, T_yaw, ret, lbfgs_iters, evals, ..."""
        assert mode in (0, 2)
        self.L.emu_set_lanes(self.lanes)
        nxy, nyaw = prob["inner_xy"].shape[1], prob["inner_yaw"].shape[0]
        S, n = (nxy + 1) * (self.K + 1), 2 * nxy + nyaw + 1
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        x = f64(x).copy()
        g = np.zeros(n)
        lam = np.zeros(S) if lam is None else f64(lam).copy()
        mu = np.zeros(6 * S) if mu is None else f64(mu).copy()
        sc = np.ones(7 * S) if scale_cx is None else f64(scale_cx).copy()
        hx, gx = np.zeros(S), np.zeros(6 * S)
        cxy, cyaw = np.zeros((6 * (nxy + 1), 2)), np.zeros(6 * (nyaw + 1))
        scal = np.zeros(8)
        scal[0], scal[1] = rho, scale_fx
        istat = np.zeros(6, dtype=np.int64)
        D, rmax, d_safe, weight = term
        D = np.ascontiguousarray(D, dtype=np.uint16)
        ixy, exy, iy, ey = f64(prob["init_xy"].T), f64(prob["end_xy"].T), f64(prob["init_yaw"]), f64(prob["end_yaw"])
        self.L.emu_clear_run(self.h, int(mode), D.ctypes.data_as(C.POINTER(C.c_uint16)), int(rmax), float(d_safe), float(weight), nxy, nyaw, E._dp(ixy), E._dp(exy),
                             E._dp(iy), E._dp(ey), E._dp(x), E._dp(g), E._dp(lam), E._dp(mu), E._dp(sc), E._dp(hx), E._dp(gx), E._dp(cxy), E._dp(cyaw), E._dp(scal),
                             istat.ctypes.data_as(C.POINTER(C.c_longlong)))
        return dict(x=x, g=g, lam=lam, mu=mu, scale_cx=sc, hx=hx, gx=gx, c_xy=cxy, c_yaw=cyaw, rho=scal[0], scale_fx=scal[1], f=scal[2], jerk_cost=scal[3],
                    T_xy=scal[4], T_yaw=scal[5], ret=int(istat[0]), alm_iters=int(istat[1]), lbfgs_iters=int(istat[2]), evals=int(istat[3]), last_lbfgs_ret=int(istat[4]))
