"""CPU tier: the host half of the trajectory rollout (include/uneven_hip.h uph_rollout_*).  uph_rollout_sizes needs no device: its row counts
are checked against the reference's own loop `for (t = 0; t < total; t += dt)` run literally in Python on the same durations."""
import ctypes as C

import numpy as np
import pytest

UPH_OK, UPH_ERR_INVALID, UPH_ERR_LIMIT = 0, -1, -4


def _total(n_xy, T_xy, n_yaw, T_yaw):
    """getTotalDuration as the device report forms it: running sums piece by piece, the smaller of position and yaw"""
    dx = 0.0
    for _ in range(n_xy):
        dx += T_xy
    dy = 0.0
    for _ in range(n_yaw):
        dy += T_yaw
    return dx if dx < dy else dy


def _loop_count(total, dt):
    t, n = 0.0, 0
    while t < total:
        n += 1
        t += dt
    return n


def _sizes(n_xy, T_xy, n_yaw, T_yaw, dt, with_end):
    from uneven_planner_amd import _lib
    L = _lib.load()
    n_xy, n_yaw = np.ascontiguousarray(n_xy, dtype=np.int32), np.ascontiguousarray(n_yaw, dtype=np.int32)
    T_xy, T_yaw = np.ascontiguousarray(T_xy, dtype=np.float64), np.ascontiguousarray(T_yaw, dtype=np.float64)
    offs = np.zeros(len(n_xy) + 1, dtype=np.int64)
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.uph_rollout_sizes(len(n_xy), pi(n_xy), pd(T_xy), pi(n_yaw), pd(T_yaw), float(dt), int(with_end), offs.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, offs


def _expected(n_xy, T_xy, n_yaw, T_yaw, dt, with_end):
    cnt = [_loop_count(_total(a, b, c, d), dt) + (1 if with_end else 0) for a, b, c, d in zip(n_xy, T_xy, n_yaw, T_yaw)]
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)


def test_rollout_symbols_and_signatures():
    from uneven_planner_amd import _lib
    L = _lib.load()
    for name in ("uph_rollout_sizes", "uph_rollout_plan", "uph_rollout_batch", "uph_rollout_batch_dev"):
        assert hasattr(L, name), name
        res, args = _lib.SYMBOLS[name]
        assert getattr(L, name).restype is res and list(getattr(L, name).argtypes) == list(args)
    assert _lib.SYMBOLS["uph_rollout_sizes"][1][5] is C.c_double          # dt
    assert _lib.SYMBOLS["uph_rollout_batch_dev"][1][-1] is C.c_void_p      # device pointer (torch data_ptr)
    from uneven_planner_amd import alm_traj_opt as A
    assert len(A.rollout_columns(A.ROLLOUT_ALL)) == 28
    assert A.rollout_columns(A.ROLLOUT_STATE | A.ROLLOUT_POSE)[:4] == ["t", "x", "y", "yaw"]
    assert len(A.rollout_columns(A.ROLLOUT_TERRAIN)) == 7 and len(A.rollout_columns(A.ROLLOUT_POSE)) == 12


@pytest.mark.parametrize("dt", [0.03, 0.01, 0.07])
@pytest.mark.parametrize("with_end", [0, 1])
def test_rollout_sizes_random(dt, with_end):
    rng = np.random.default_rng(17)
    B = 120
    n_xy = rng.integers(1, 60, B)
    n_yaw = n_xy + rng.integers(0, 40, B)
    T_xy = rng.uniform(0.05, 0.9, B)
    T_yaw = rng.uniform(0.05, 0.9, B)
    rc, offs = _sizes(n_xy, T_xy, n_yaw, T_yaw, dt, with_end)
    assert rc == UPH_OK
    assert np.array_equal(offs, _expected(n_xy, T_xy, n_yaw, T_yaw, dt, with_end))


@pytest.mark.parametrize("dt", [0.03, 0.01, 0.07, 0.25])
def test_rollout_sizes_exact_multiples_and_edges(dt):
    # total an exact (decimal) multiple of dt: whether the running sum lands below or on it decides one sample -- only the literal loop knows
    n_xy, T_xy, n_yaw, T_yaw = [], [], [], []
    for k in range(1, 60):
        n_xy.append(k); T_xy.append(dt); n_yaw.append(k); T_yaw.append(dt)             # total = k additions of dt
        n_xy.append(4); T_xy.append(k * dt / 4.0); n_yaw.append(5); T_yaw.append(k * dt)  # position shorter than yaw
        n_xy.append(3); T_xy.append(k * dt); n_yaw.append(6); T_yaw.append(k * dt / 7.0)  # yaw shorter than position
    n_xy += [1, 2, 1]; T_xy += [0.3 * dt, 0.2 * dt, 0.0]; n_yaw += [1, 2, 1]; T_yaw += [0.5 * dt, 0.4 * dt, 0.0]    # total < dt; total = 0
    for with_end in (0, 1):
        rc, offs = _sizes(n_xy, T_xy, n_yaw, T_yaw, dt, with_end)
        assert rc == UPH_OK
        assert np.array_equal(offs, _expected(n_xy, T_xy, n_yaw, T_yaw, dt, with_end))
    # total < dt: one sample (t = 0), the end point makes it two; total = 0: none (+ the end point)
    rc, offs = _sizes([1, 1], [0.5 * dt, 0.0], [1, 1], [0.5 * dt, 0.0], dt, 0)
    assert list(np.diff(offs)) == [1, 0]
    rc, offs = _sizes([1, 1], [0.5 * dt, 0.0], [1, 1], [0.5 * dt, 0.0], dt, 1)
    assert list(np.diff(offs)) == [2, 1]


def test_rollout_sizes_yaw_shorter_uses_minimum():
    rc, offs = _sizes([10], [0.5], [12], [0.25], 0.01, 0)       # position 5 s, yaw 3 s
    # 300 additions of 0.01 stay below 3.0: the loop runs a 301st time -- which q * dt would not show
    assert rc == UPH_OK and offs[1] == _loop_count(_total(10, 0.5, 12, 0.25), 0.01) == 301


def test_rollout_sizes_limit_and_stall():
    # more samples than UPH_ROLLOUT_MAX_SAMPLES
    from uneven_planner_amd import alm_traj_opt as A
    rc, _ = _sizes([10], [1.0], [10], [1.0], 1e-5, 0)
    assert rc == UPH_ERR_LIMIT
    # a duration the running sum could only reach after it has stopped growing (t + dt == t long before 1e300): refused, not looped
    rc, _ = _sizes([1], [1e300], [1], [1e300], 1.0, 0)
    assert rc == UPH_ERR_LIMIT
    # just below the cap is fine, at the cap + 1 is not
    dt = 1.0 / 1024.0                                        # exact binary steps: t_q = q dt exactly
    m = A.ROLLOUT_MAX_SAMPLES
    rc, offs = _sizes([1], [m * dt], [1], [m * dt], dt, 1)
    assert rc == UPH_OK and offs[1] == m + 1
    rc, _ = _sizes([1], [(m + 1) * dt], [1], [(m + 1) * dt], dt, 0)
    assert rc == UPH_ERR_LIMIT


def test_rollout_sizes_refusals():
    for dt in (0.0, -0.01, float("nan"), float("inf")):
        rc, _ = _sizes([3], [0.5], [3], [0.5], dt, 0)
        assert rc == UPH_ERR_INVALID, dt
    rc, _ = _sizes([-1], [0.5], [3], [0.5], 0.01, 0)
    assert rc == UPH_ERR_INVALID
    from uneven_planner_amd import _lib
    L = _lib.load()
    offs = np.zeros(2, dtype=np.int64)
    assert L.uph_rollout_sizes(1, None, None, None, None, 0.01, 0, offs.ctypes.data_as(C.POINTER(C.c_int64))) == UPH_ERR_INVALID
    assert L.uph_rollout_sizes(0, None, None, None, None, 0.01, 0, None) == UPH_ERR_INVALID
    # a NaN duration has no samples, exactly as `t < NaN` ends the loop at once
    rc, offs = _sizes([2], [float("nan")], [2], [float("nan")], 0.01, 0)
    assert rc == UPH_OK and offs[1] == 0


def test_rollout_sizes_python_wrapper():
    from uneven_planner_amd import alm_traj_opt as A
    offs = A.rollout_sizes([5, 7], [0.4, 0.3], [6, 7], [0.35, 0.31], dt=0.03, with_end=True)
    assert np.array_equal(offs, _expected([5, 7], [0.4, 0.3], [6, 7], [0.35, 0.31], 0.03, 1))
    views = A.split_rollout(offs, np.arange(int(offs[-1]) * 2, dtype=np.float64).reshape(-1, 2))
    assert [v.shape[0] for v in views] == list(np.diff(offs))
