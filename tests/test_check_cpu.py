"""CPU tier of checking resident trajectories against the current map (uph_check_batch): the C-ABI and its binding, the refusals that need no
device, the host window rule (uph_check_window) against the reference's sampling loop run literally, and the numpy mirror check_rows -- the rule of
include/uneven_hip.h that tests/test_gpu_check.py holds the device against -- on hand-made rows.  The GPU tier is tests/test_gpu_check.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import CHECK_OCC_BIT, check_rows, check_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = C.POINTER(C.c_int32)


def loop_rows(total, dt, with_end):
    """the t of a trajectory's rollout rows: `t = 0; while t < total: t += dt` (alm_traj_opt.h:182), + the end row"""
    t, out = 0.0, []
    while t < total:
        out.append(t)
        t += dt
    return out + ([total] if with_end else [])


def loop_window(total, dt, with_end, t_from, t_to):
    """(q_lo, q_hi, end_row) by walking the loop: the comparisons t_from <= t and t <= t_to are literal"""
    rows = loop_rows(total, dt, False)
    inside = [q for q, t in enumerate(rows) if t_from <= t and t <= t_to]
    end = bool(with_end and t_from <= total and total <= t_to)
    return inside, end


def _same_window(total, dt, with_end, t_from, t_to):
    inside, end = loop_window(total, dt, with_end, t_from, t_to)
    lo, hi, e = check_window(dt, with_end, total, t_from, t_to)
    assert hi >= lo >= 0
    assert list(range(lo, hi)) == inside, (total, dt, t_from, t_to, lo, hi, inside[:3], inside[-3:])
    assert e == end, (total, dt, with_end, t_from, t_to)
    return len(inside) + int(end)


def test_symbols_are_exported_with_the_binding_signatures():
    L = _lib.load()
    lim = _lib.SYMBOLS["uph_check_limits"][1]
    win = _lib.SYMBOLS["uph_check_window"][1]
    bat = _lib.SYMBOLS["uph_check_batch"][1]
    assert lim == [C.c_void_p, _lib.DP]
    assert win == [C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, I32P, I32P, I32P]
    assert bat == [C.c_void_p, C.c_int32, I32P, _lib.DP, _lib.DP, C.c_double, C.c_int32, _lib.DP, _lib.DP, I32P, I32P, _lib.DP, _lib.DP]
    for name, args in (("uph_check_limits", lim), ("uph_check_window", win), ("uph_check_batch", bat)):
        fn = getattr(L, name)
        assert fn.restype == C.c_int and fn.argtypes == args
    hdr = " ".join(open(os.path.join(ROOT, "include", "uneven_hip.h")).read().split())
    assert "#define UPH_CHECK_OCC_BIT 7" in hdr and CHECK_OCC_BIT == 7 == _lib.UPH_CHECK_OCC_BIT
    assert "int uph_check_limits(const uph_ctx* c, double* lim7);" in hdr
    assert ("int uph_check_window(double dt, int32_t with_end, double total, double t_from, double t_to, int32_t* q_lo, int32_t* q_hi, "
            "int32_t* end_row);") in hdr
    assert "int uph_check_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t_from, const double* t_to" in hdr


def test_refusals_without_a_device():
    L = _lib.load()
    v = [C.c_int32(-7) for _ in range(3)]
    ref = [C.byref(x) for x in v]
    for dt in (0.0, -0.01, float("inf"), float("nan")):
        assert L.uph_check_window(dt, 1, 3.0, 0.0, 1.0, *ref) == _lib.UPH_ERR_INVALID
    assert L.uph_check_window(0.01, 1, 3.0, float("nan"), 1.0, *ref) == _lib.UPH_ERR_INVALID
    assert L.uph_check_window(0.01, 1, 3.0, 0.0, float("nan"), *ref) == _lib.UPH_ERR_INVALID
    assert L.uph_check_window(0.01, 1, 3.0, 0.0, 1.0, None, ref[1], ref[2]) == _lib.UPH_ERR_INVALID
    assert L.uph_check_window(1e-6, 1, 3.0, 0.0, 1.0, *ref) == _lib.UPH_ERR_LIMIT            # 3e6 samples > UPH_ROLLOUT_MAX_SAMPLES
    assert [x.value for x in v] == [-7, -7, -7]
    lim = np.full(7, -3.0)
    assert L.uph_check_limits(None, _lib.DP(C.c_double(0))) == _lib.UPH_ERR_INVALID
    one = np.zeros(1, dtype=np.int32)
    t0 = np.zeros(1)
    assert L.uph_check_batch(None, 1, one.ctypes.data_as(I32P), t0.ctypes.data_as(_lib.DP), None, 0.01, 1, None, None, None, None, None, None) == _lib.UPH_ERR_INVALID
    assert (lim == -3.0).all()


def test_window_equals_the_loop_on_random_totals():
    rng = np.random.default_rng(11)
    for _ in range(60):
        total = float(rng.uniform(0.02, 9.0))
        dt = float(rng.choice([0.01, 0.03, 0.05, 0.0173]))
        a, b = sorted(rng.uniform(-1.0, total + 1.0, 2))
        for with_end in (0, 1):
            _same_window(total, dt, with_end, a, b)
            _same_window(total, dt, with_end, 0.0, float("inf"))


@pytest.mark.parametrize("dt", [0.01, 0.03])
def test_window_edges(dt):
    total = 2.3456
    rows = loop_rows(total, dt, False)
    n = len(rows)
    t7, t8, tl = rows[7], rows[8], rows[-1]
    mid = 0.5 * (t7 + t8)
    for with_end in (0, 1):
        assert _same_window(total, dt, with_end, t7, tl) == n - 7 + 0             # starts and ends exactly on a sample; the end row is beyond
        assert _same_window(total, dt, with_end, np.nextafter(t7, 9.0), tl) == n - 8
        assert _same_window(total, dt, with_end, 0.0, t8) == 9
        assert _same_window(total, dt, with_end, 0.0, np.nextafter(t8, -9.0)) == 8
        assert _same_window(total, dt, with_end, mid, mid + 2.5 * dt) in (2, 3)   # between samples
        assert _same_window(total, dt, with_end, mid, mid) == 0                   # a point between two samples
        assert _same_window(total, dt, with_end, t7, t7) == 1                     # a point on a sample
        assert _same_window(total, dt, with_end, -5.0, -1.0) == 0                 # before 0
        assert _same_window(total, dt, with_end, -5.0, 0.0) == 1
        assert _same_window(total, dt, with_end, -5.0, 99.0) == n + with_end      # beyond both ends
        assert _same_window(total, dt, with_end, total + 1.0, total + 2.0) == 0   # beyond the total
        assert _same_window(total, dt, with_end, 1.5, 0.5) == 0                   # t_to < t_from
        assert _same_window(total, dt, with_end, float("-inf"), float("inf")) == n + with_end
        assert _same_window(total, dt, with_end, 1.0, float("-inf")) == 0
        # the end row in and out of the window
        assert _same_window(total, dt, with_end, tl, total) == 1 + with_end
        assert _same_window(total, dt, with_end, total, total) == with_end
        assert _same_window(total, dt, with_end, tl, np.nextafter(total, 0.0)) == 1
        assert _same_window(total, dt, with_end, np.nextafter(total, 9.0), 99.0) == 0


def test_window_of_short_and_degenerate_trajectories():
    for with_end in (0, 1):
        assert _same_window(0.004, 0.01, with_end, 0.0, 1.0) == 1 + with_end       # total < dt: the sample at 0 (+ the end row)
        assert _same_window(0.004, 0.01, with_end, 0.001, 1.0) == with_end
        assert _same_window(0.0, 0.01, with_end, -1.0, 1.0) == with_end            # no sample of the loop; the end row at t = 0
        assert _same_window(0.03, 0.01, with_end, 0.0, 1.0) == len(loop_rows(0.03, 0.01, False)) + with_end
    lo, hi, e = check_window(0.01, 1, float("nan"), 0.0, 1.0)                       # a NaN duration has no samples, as in the loop
    assert (lo, hi, e) == (0, 0, False)


def _rows(n):
    t = 0.25 * np.arange(n)
    terms = np.zeros((n, 7))
    terms[:, 4] = -1.0                      # att = -cos xi of level ground: inside LIM
    return t, terms, np.zeros(n, dtype=np.int32)


LIM = np.array([1.0, 2.0, 3.0, 4.0, -0.8, 0.05, np.inf])


def test_check_rows_rule_on_hand_made_rows():
    t, T, occ = _rows(8)
    r = check_rows(t, T, occ, LIM)
    assert np.isnan(r["first_t"]) and r["first_mask"] == 0 and r["counts"].tolist() == [8, 0, 0]
    assert r["worst"].tolist() == [0, 0, 0, 0, -1.0, 0, 0] and (r["worst_t"] == 0.0).all()        # every tie goes to the earliest sample
    # |v| for the first four terms, v for the others; exactly at the limit is no violation
    T[2, 0], T[3, 1], T[5, 1], T[4, 4], T[6, 5], T[1, 6] = -1.0, -2.5, 2.5, -0.8, 0.06, 1e30
    r = check_rows(t, T, occ, LIM)
    assert r["first_t"] == t[3] and r["first_mask"] == 1 << 1 and r["counts"].tolist() == [8, 3, 0]
    assert r["worst"].tolist() == [1.0, 2.5, 0, 0, -0.8, 0.06, 1e30]
    assert r["worst_t"].tolist() == [t[2], t[3], 0.0, 0.0, t[4], t[6], t[1]]                       # 2.5 twice: the earlier one
    T[4, 4] = np.nextafter(-0.8, 0.0)
    r = check_rows(t, T, occ, LIM)
    assert r["counts"][1] == 4 and r["worst"][4] == T[4, 4]
    # two terms at one sample
    T[3, 3] = -4.5
    assert check_rows(t, T, occ, LIM)["first_mask"] == (1 << 1) | (1 << 3)
    # a negative value of a one-sided term never violates
    T[0, 5] = -9.0
    assert check_rows(t, T, occ, LIM, t_to=0.0)["first_mask"] == 0


def test_check_rows_nan_violates_and_reads_inf():
    t, T, occ = _rows(6)
    T[:, 2] = [0.5, 7.0, np.nan, 8.0, np.nan, 0.0]
    T[4, 6] = np.nan
    T[5, 5] = -np.inf
    r = check_rows(t, T, occ, LIM)
    assert r["first_t"] == t[1] and r["first_mask"] == 1 << 2
    assert r["worst"][2] == np.inf and r["worst_t"][2] == t[2]                 # the FIRST non-finite sample
    assert r["worst"][6] == np.inf and r["worst_t"][6] == t[4]                 # NaN violates even an infinite limit
    assert r["worst"][5] == np.inf and r["worst_t"][5] == t[5]                 # -inf is non-finite too (but violates nothing)
    assert r["counts"].tolist() == [6, 4, 0]
    r = check_rows(t, T, occ, LIM, t_from=t[2], t_to=t[2])
    assert r["first_t"] == t[2] and r["first_mask"] == 1 << 2 and r["counts"].tolist() == [1, 1, 0]


def test_check_rows_empty_window():
    t, T, occ = _rows(5)
    T[:, 0] = 9.0
    for a, b in ((10.0, 20.0), (1.0, 0.5), (0.3, 0.4), (-2.0, -1.0)):
        r = check_rows(t, T, occ, LIM, t_from=a, t_to=b)
        assert r["counts"].tolist() == [0, 0, 0] and np.isnan(r["first_t"]) and r["first_mask"] == 0
        assert (r["worst"] == -np.inf).all() and np.isnan(r["worst_t"]).all()
    r = check_rows(t[:0], T[:0], occ[:0], LIM)
    assert r["counts"].tolist() == [0, 0, 0] and (r["worst"] == -np.inf).all()


def test_check_rows_occupancy_bit_and_window():
    t, T, occ = _rows(8)
    occ[[3, 5]] = [1, -1]                                                      # occupied; outside the map counts as occupied
    T[5, 0] = 2.0
    r = check_rows(t, T, occ, LIM)
    assert r["first_t"] == t[3] and r["first_mask"] == 1 << CHECK_OCC_BIT == 128 and r["counts"].tolist() == [8, 2, 2]
    r = check_rows(t, T, occ, LIM, t_from=t[4])
    assert r["first_t"] == t[5] and r["first_mask"] == 128 | 1 and r["counts"].tolist() == [4, 1, 1]
    r = check_rows(t, T, occ, LIM, t_from=t[3], t_to=t[5])                     # both bounds are inside
    assert r["counts"].tolist() == [3, 2, 2] and r["worst_t"][0] == t[5]
    r = check_rows(t, T, occ, LIM, t_from=np.nextafter(t[3], 9.0), t_to=np.nextafter(t[5], 0.0))
    assert r["counts"].tolist() == [1, 0, 0]


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
int main() {
    uneven_hip::ALMTrajOpt* o = nullptr;
    if (o) {
        uneven_hip::ALMTrajOpt::TrajCheck r = o->checkSE2TrajBatch({0, 1}, {0.0, 0.5});
        r = o->checkSE2TrajBatch({0}, {0.0}, {1.0}, 0.03, false, o->checkLimits().data());
        return r.violates(0) ? (int)r.first_t[0] + r.first_mask[0] + r.counts[2] + (int)r.worst[6] + (int)r.worst_t[6] : 0;
    }
    return 0;
}
"""


def test_adapter_offers_the_check(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "a.o")])
