"""CPU tier of the fleet of resident trajectories (include/uneven_hip.h uph_fleet_*, uneven_planner_amd.TrajFleet, uneven_hip::TrajFleet): the symbols are
exported and bound, uph_fleet_bytes follows the documented slot layout, the refusals that need no device, no host fall-back, the wrapper's argument checks that
raise before any device call, and the adapter's TrajFleet compiles as plain C++17.  The device side is tests/test_gpu_fleet.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLEET_SYMBOLS = ("uph_fleet_bytes", "uph_fleet_create", "uph_fleet_adopt", "uph_fleet_release", "uph_fleet_info", "uph_fleet_get", "uph_fleet_kernel_ms")
INVALID, NO_DEVICE = -1, -3


def _lib():
    import uneven_planner_amd as U
    return U, U._lib.load()


def _err(L):
    return L.uph_last_error().decode()


def _params(U):
    from uneven_planner_amd.alm_traj_opt import HILL_OPT_PARAMS, _INT_FIELDS
    return U._lib.OptParams(**{k: (int(v) if k in _INT_FIELDS else float(v)) for k, v in HILL_OPT_PARAMS.items()})


def test_fleet_symbols_are_exported_and_bound():
    U, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "uneven_hip.h")).read()
    for s in FLEET_SYMBOLS:
        assert s in U._lib.SYMBOLS and hasattr(L, s) and ("int %s(" % s) in hdr, s
        assert getattr(L, s).argtypes == U._lib.SYMBOLS[s][1]
    assert hasattr(U, "TrajFleet") and issubclass(U.TrajFleet, U.ALMTrajOpt)
    assert "#define UPH_FLEET_SLOT_ROW_BYTES %d" % U._lib.FLEET_SLOT_ROW_BYTES in hdr


@pytest.mark.parametrize("slots, cap_xy, cap_yaw", [(1, 1, 1), (1, 128, 256), (7, 3, 5), (64, 17, 34), (4096, 128, 256), (4096, 1, 256), (100000, 128, 1),
                                                    (2 ** 31 - 1, 128, 256)])
def test_fleet_bytes_follows_the_slot_layout(slots, cap_xy, cap_yaw):
    """slot s owns 12 cap_xy doubles of c_xy, 6 cap_yaw doubles of c_yaw and the two rows: no rounding, no slack, 64-bit arithmetic"""
    U, L = _lib()
    b = C.c_int64(-1)
    assert L.uph_fleet_bytes(slots, cap_xy, cap_yaw, C.byref(b)) == 0
    assert b.value == slots * (8 * 12 * cap_xy + 8 * 6 * cap_yaw + U._lib.FLEET_SLOT_ROW_BYTES)
    from uneven_planner_amd.alm_traj_opt import fleet_bytes
    assert fleet_bytes(slots, cap_xy, cap_yaw) == b.value


def test_fleet_bytes_at_the_largest_caps_is_24_KiB_of_coefficients_per_slot():
    from uneven_planner_amd.alm_traj_opt import fleet_bytes
    U, _ = _lib()
    assert fleet_bytes(1) - U._lib.FLEET_SLOT_ROW_BYTES == 24 * 1024
    assert fleet_bytes(4096) - 4096 * U._lib.FLEET_SLOT_ROW_BYTES == 96 << 20


@pytest.mark.parametrize("shape", [(0, 4, 8), (-1, 4, 8), (4, 0, 8), (4, 129, 8), (4, 4, 0), (4, 4, 257), (4, -3, 8)])
def test_bad_shapes_are_refused_without_a_device(shape):
    U, L = _lib()
    b = C.c_int64(-7)
    assert L.uph_fleet_bytes(*shape, C.byref(b)) == INVALID and b.value == -7 and "uph_fleet_bytes" in _err(L)
    # uph_fleet_create checks the shape before it looks at the map or the device: the map handle below is never read
    p, h = _params(U), C.c_void_p(0)
    fake_map = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert L.uph_fleet_create(fake_map, C.byref(p), *shape, C.byref(h)) == INVALID and not h.value and "uph_fleet_create" in _err(L)


def test_null_arguments_are_refused_without_a_device():
    U, L = _lib()
    p, h = _params(U), C.c_void_p(0)
    fake_map = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert L.uph_fleet_bytes(4, 4, 8, None) == INVALID
    assert L.uph_fleet_create(None, C.byref(p), 4, 4, 8, C.byref(h)) == INVALID and "uph_fleet_create" in _err(L)
    assert L.uph_fleet_create(fake_map, None, 4, 4, 8, C.byref(h)) == INVALID
    assert L.uph_fleet_create(fake_map, C.byref(p), 4, 4, 8, None) == INVALID
    # the calls on a fleet, without one
    one = np.zeros(1, dtype=np.int32)
    ip = one.ctypes.data_as(C.POINTER(C.c_int32))
    ms = C.c_double(-1.0)
    assert L.uph_fleet_adopt(None, None, 1, ip, ip, None) == INVALID and "uph_fleet_adopt" in _err(L)
    assert L.uph_fleet_release(None, 1, ip) == INVALID and "uph_fleet_release" in _err(L)
    assert L.uph_fleet_info(None, None, None, None, None, None) == INVALID and "uph_fleet_info" in _err(L)
    assert L.uph_fleet_get(None, 1, ip, None, None, None, None, None, None, None) == INVALID and "uph_fleet_get" in _err(L)
    assert L.uph_fleet_kernel_ms(None, C.byref(ms)) == INVALID and ms.value == -1.0


def test_no_host_fall_back_without_a_device():
    """valid arguments on a machine without a GPU: UPH_ERR_NO_DEVICE before the map is read, nothing created"""
    U, L = _lib()
    if L.uph_device_count() > 0:
        return          # with a device the same call is the GPU tier's (tests/test_gpu_fleet.py), on a real map
    p, h = _params(U), C.c_void_p(0)
    fake_map = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert L.uph_fleet_create(fake_map, C.byref(p), 4, 4, 8, C.byref(h)) == NO_DEVICE and not h.value
    assert "no HIP device" in _err(L)


def test_wrapper_argument_checks_raise_before_any_device_call():
    import uneven_planner_amd as U
    from uneven_planner_amd.alm_traj_opt import _adopt_arrays
    E = U._lib.UnevenHipError
    # the shape is checked before the map is touched: the map argument here is not one
    for bad in ((0, 4, 8), (4, 0, 8), (4, 129, 8), (4, 4, 257), (2.5, 4, 8), ("many", 4, 8)):
        with pytest.raises(E, match="TrajFleet"):
            U.TrajFleet(object(), *bad)
    with pytest.raises(E, match="same non-empty length"):
        _adopt_arrays([0, 1], [0], None)
    with pytest.raises(E, match="same non-empty length"):
        _adopt_arrays([], [], None)
    with pytest.raises(E, match="twice"):
        _adopt_arrays([0, 1, 2], [3, 4, 3], None)
    with pytest.raises(E, match="finite"):
        _adopt_arrays([0, 1], [0, 1], [0.0, np.nan])
    with pytest.raises(E, match="finite"):
        _adopt_arrays([0, 1], [0, 1], np.inf)
    tr, sl, ts = _adopt_arrays([5, 5], [1, 0], 2.5)          # the same source twice is fine; a scalar start is broadcast
    assert tr.dtype == np.int32 and sl.dtype == np.int32 and tr.tolist() == [5, 5] and sl.tolist() == [1, 0] and ts.tolist() == [2.5, 2.5]
    assert _adopt_arrays([1], [0], None)[2] is None
    # the solve side raises on a fleet (no device is reached: the object below has no context)
    f = U.TrajFleet.__new__(U.TrajFleet)
    f.h = None                                               # (for __del__)
    for name in ("upload", "solve", "solve_async", "wait", "download", "optimize_batch", "eval_batch", "plan_goals", "refine", "replan_goals", "set_rho", "set_state",
                 "getMaxVxAxAyCurAttSig", "optimizeSE2Traj"):
        with pytest.raises(E, match="TrajFleet"):
            getattr(f, name)()


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
using namespace uneven_hip;
// adopt what two optimisers solved, ask the fleet, hand a trajectory on
int cycle(UnevenMapHandle& map, ALMTrajOpt& a, ALMTrajOpt& b, std::vector<double>& out) {
    TrajFleet fleet;
    fleet.setEnvironment(&map, 8, 64, 128);
    fleet.adoptSE2TrajBatch(a, {0, 1}, {0, 1}, {0.0, 1.5});
    fleet.adoptSE2TrajBatch(b, {0}, {5});
    std::vector<int32_t> occ = fleet.occupied();
    std::vector<double> t0 = fleet.startTimes();
    ALMTrajOpt::TrajConflicts c = fleet.conflictsSE2TrajBatch({0, 1, 5}, {t0[0], t0[1], t0[5]}, {0.3, 0.3, 0.3}, 0.0, 20.0, 0.05);
    ALMTrajOpt::TrajSeparation s = a.separationSE2TrajBatch({0}, {5}, {0.0}, {t0[5]}, {0.0}, {20.0}, {0.6}, 0.01, &fleet);      // the fleet as `other`
    if (s.conflicts(0)) fleet.releaseSlots({5});
    out = fleet.trajStates({0, 5}, {0.5, 0.5});
    SE2Trajectory t = fleet.getTraj(5);
    fleet.releaseSlots({1});
    return (int)c.pairs.size() + t.pos_traj.getPieceNum() + (int)occ.size() + fleet.slots();
}
"""


def test_cpp_adapter_fleet_compiles(tmp_path):
    src = tmp_path / "fleet_consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "f.o")])
