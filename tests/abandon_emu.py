"""TEST SCAFFOLDING: the CPU emulator of the workgroup program (tests/emu_bridge.py) built from tests/emu/emu_abandon.cpp, which adds the
trial-abandonment switch, the line-search counters of the last run and the may-abandon rule as the product states it."""
import ctypes as C
import os
import subprocess

import emu_bridge as E

_HERE = os.path.dirname(os.path.abspath(__file__))
_L = None
COUNTERS = ("ls_rejected", "ls_guarded", "ls_abandoned", "chunks_skipped", "adjoints_skipped")


def lib():
    global _L
    if _L is None:
        so = os.path.join(_HERE, "emu", "libemu_abandon.so")
        srcs = [os.path.join(_HERE, "emu", f) for f in ("emu_abandon.cpp", "emu_solver.cpp")]
        csrc = os.path.join(_HERE, "..", "uneven_planner_amd", "csrc")
        deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [dp, dp, dp]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [dp] * 14 + [C.POINTER(C.c_longlong), dp]
        L.emu_set_hook.argtypes = [C.c_int, C.c_int, C.c_int] + [dp] * 7
        L.emu_set_lanes.argtypes = [C.c_int]
        L.emu_set_trial_abandon.argtypes = [C.c_void_p, C.c_int]
        L.emu_abandon_counters.argtypes = [C.POINTER(C.c_longlong)]
        L.emu_may_abandon.restype = C.c_int
        L.emu_may_abandon.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double]
        _L = L
    return _L


class AbandonEmu(E.Emu):
    def __init__(self, cells, map_params_vec, opt_params_vec, lanes=128):
        import numpy as np
        self.L = lib()
        self.L.emu_set_lanes(lanes)
        self.cells = np.ascontiguousarray(cells, dtype=np.float64)
        self.mp = np.ascontiguousarray(map_params_vec, dtype=np.float64)
        self.op = np.ascontiguousarray(opt_params_vec, dtype=np.float64)
        self.K = int(self.op[20])
        self.h = self.L.emu_create(E._dp(self.mp), E._dp(self.cells), E._dp(self.op))

    def set_trial_abandon(self, on):
        self.L.emu_set_trial_abandon(self.h, 1 if on else 0)
        return self

    def counters(self):
        out = (C.c_longlong * 5)()
        self.L.emu_abandon_counters(out)
        return dict(zip(COUNTERS, [int(v) for v in out]))
