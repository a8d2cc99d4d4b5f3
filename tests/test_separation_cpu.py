"""CPU tier of the queries between resident trajectories on a common clock (uph_separation_times, uph_extent_batch, uph_separation_batch,
uph_conflict_candidates, uph_conflicts_batch): the C-ABI and its binding, the refusals that need no device, the adapter's entry points, the host-only
calls against the numpy mirrors separation_times / conflict_candidates, and the mirrors separation_rows / extent_rows -- the rule of
include/uneven_hip.h that tests/test_gpu_separation.py holds the device against -- on hand-made rows with known answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import conflict_candidates, extent_rows, separation_rows, separation_times

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = C.POINTER(C.c_int32)
I64P = C.POINTER(C.c_int64)
DP = _lib.DP
INF = float("inf")
NAN = float("nan")
dp = lambda a: a.ctypes.data_as(DP)
ip = lambda a: a.ctypes.data_as(I32P)


def test_symbols_are_exported_with_the_binding_signatures():
    L = _lib.load()
    want = {
        "uph_separation_times": [C.c_double, C.c_double, C.c_double, I64P],
        "uph_extent_batch": [C.c_void_p, C.c_int32, I32P, DP, DP, DP, C.c_double, DP, I32P],
        "uph_separation_batch": [C.c_void_p, C.c_void_p, C.c_int32, I32P, I32P, DP, DP, DP, DP, C.c_double, DP, DP, DP, DP, DP, I32P],
        "uph_conflict_candidates": [C.c_int32, DP, DP, C.c_int64, I32P, I64P],
        "uph_conflicts_batch": [C.c_void_p, C.c_int32, I32P, DP, DP, C.c_double, C.c_double, C.c_double, C.c_int64, I32P, DP, I32P, I64P, I64P],
        "uph_separation_kernel_ms": [C.c_void_p, DP],
    }
    for name, args in want.items():
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
        fn = getattr(L, name)
        assert fn.restype == C.c_int and fn.argtypes == args, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "uneven_hip.h")).read().split())
    assert "int uph_separation_times(double t_from, double t_to, double dt, int64_t* K);" in hdr
    assert ("int uph_extent_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* t_from, const double* t_to, double dt, "
            "double* box /* [n][4]: xmin, xmax, ymin, ymax */, int32_t* counts /* [n][2]: samples, NaN samples */);") in hdr
    assert ("int uph_separation_batch(uph_ctx* ca, uph_ctx* cb /* NULL: ca */, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, "
            "const double* t0_b, const double* t_from, const double* t_to, double dt, const double* radius, double* min_d2") in hdr
    assert "int uph_conflict_candidates(int32_t n, const double* box /* [n][4] */, const double* radius /* [n] */, int64_t cap, int32_t* pairs" in hdr
    assert ("int uph_conflicts_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* radius /* [n]: per vehicle */, double t_from, "
            "double t_to, double dt, int64_t cap, int32_t* pairs") in hdr
    assert "int uph_separation_kernel_ms(const uph_ctx* c, double* kernel_ms);" in hdr
    assert _lib.SEPARATION_MAX_SAMPLES == 1 << 22


def test_refusals_without_a_device():
    L = _lib.load()
    one, z, w1, r = np.zeros(1, dtype=np.int32), np.zeros(1), np.ones(1), np.full(1, 0.5)
    d = {k: np.full(s, -9.0) for k, s in (("box", 4), ("min_d2", 1), ("min_t", 1), ("first_t", 1), ("last_t", 1), ("rows", 4))}
    i = {k: np.full(s, -9, dtype=np.int32) for k, s in (("ecounts", 2), ("scounts", 2), ("pairs", 2), ("below", 1))}
    nc, nk = C.c_int64(-9), C.c_int64(-9)
    assert L.uph_extent_batch(None, 1, ip(one), dp(z), dp(z), dp(w1), 0.01, dp(d["box"]), ip(i["ecounts"])) == _lib.UPH_ERR_INVALID
    assert b"uph_extent_batch" in L.uph_last_error()
    assert L.uph_separation_batch(None, None, 1, ip(one), ip(one), dp(z), dp(z), dp(z), dp(w1), 0.01, dp(r), dp(d["min_d2"]), dp(d["min_t"]), dp(d["first_t"]),
                                  dp(d["last_t"]), ip(i["scounts"])) == _lib.UPH_ERR_INVALID
    assert b"uph_separation_batch" in L.uph_last_error()
    assert L.uph_conflicts_batch(None, 1, ip(one), dp(z), dp(r), 0.0, 1.0, 0.05, 1, ip(i["pairs"]), dp(d["rows"]), ip(i["below"]), C.byref(nc),
                                 C.byref(nk)) == _lib.UPH_ERR_INVALID
    assert b"uph_conflicts_batch" in L.uph_last_error()
    ms = C.c_double(-9.0)
    assert L.uph_separation_kernel_ms(None, C.byref(ms)) == _lib.UPH_ERR_INVALID and ms.value == -9.0
    assert b"uph_separation_kernel_ms" in L.uph_last_error()
    assert all((v == -9).all() for v in d.values()) and all((v == -9).all() for v in i.values()) and nc.value == -9 and nk.value == -9
    # the host-only calls refuse what the rule excludes, outputs untouched
    K = C.c_int64(-9)
    for a, b, dt in ((0.0, 1.0, 0.0), (0.0, 1.0, -0.1), (0.0, 1.0, INF), (0.0, 1.0, NAN), (NAN, 1.0, 0.1), (0.0, NAN, 0.1), (-INF, 1.0, 0.1), (0.0, INF, 0.1)):
        assert L.uph_separation_times(a, b, dt, C.byref(K)) == _lib.UPH_ERR_INVALID and K.value == -9, (a, b, dt)
        assert b"uph_separation_times" in L.uph_last_error()
    assert L.uph_separation_times(0.0, 1.0, 0.1, None) == _lib.UPH_ERR_INVALID
    box, rad = np.array([[0.0, 1.0, 0.0, 1.0], [0.5, 1.5, 0.5, 1.5]]), np.array([0.1, 0.1])
    n = C.c_int64(-9)
    for bad_box, bad_rad in ((np.array([[0.0, 1.0, NAN, 1.0], [0.5, 1.5, 0.5, 1.5]]), rad), (box, np.array([0.1, -0.1])), (box, np.array([INF, 0.1])), (box, np.array([0.1, NAN]))):
        assert L.uph_conflict_candidates(2, dp(bad_box), dp(bad_rad), 1, ip(i["pairs"]), C.byref(n)) == _lib.UPH_ERR_INVALID and n.value == -9
        assert b"uph_conflict_candidates" in L.uph_last_error() and (i["pairs"] == -9).all()
    assert L.uph_conflict_candidates(2, None, dp(rad), 1, ip(i["pairs"]), C.byref(n)) == _lib.UPH_ERR_INVALID
    assert L.uph_conflict_candidates(2, dp(box), dp(rad), -1, ip(i["pairs"]), C.byref(n)) == _lib.UPH_ERR_INVALID
    assert L.uph_conflict_candidates(2, dp(box), dp(rad), 1, None, C.byref(n)) == _lib.UPH_ERR_INVALID and n.value == -9


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
int main() {
    uneven_hip::ALMTrajOpt* o = nullptr;
    uneven_hip::ALMTrajOpt* fleet = nullptr;
    if (o) {
        uneven_hip::ALMTrajOpt::TrajExtent e = o->extentSE2TrajBatch({0, 1}, {0.0, 2.5}, {0.0, 0.0}, {9.0, 9.0});
        e = o->extentSE2TrajBatch({0}, {1000.0}, {1000.0}, {1005.0}, 0.05);
        uneven_hip::ALMTrajOpt::TrajSeparation s = o->separationSE2TrajBatch({0, 1}, {1, 2}, {0.0, 0.0}, {1.0, 2.0}, {0.0, 0.0}, {9.0, 9.0}, {0.5, 0.5});
        s = o->separationSE2TrajBatch({0}, {3}, {0.5}, {0.0}, {0.0}, {9.0}, {0.6}, 0.05, fleet);
        uneven_hip::ALMTrajOpt::TrajConflicts c = o->conflictsSE2TrajBatch({0, 1, 2}, {0.0, 1.0, 2.0}, {0.3, 0.3, 0.3}, 0.0, 20.0);
        c = o->conflictsSE2TrajBatch({0, 1, 2}, {0.0, 1.0, 2.0}, {0.3, 0.3, 0.3}, 0.0, 20.0, 0.1, 16);
        return (int)e.box[3] + e.counts[1] + (s.conflicts(0) ? (int)s.min_d2[0] + (int)s.min_t[0] + (int)s.first_t[0] + (int)s.last_t[0] + s.counts[0] : 0) +
               (int)c.n_conflicts + (int)c.n_candidates + (c.pairs.empty() ? 0 : c.pairs[0][1] + c.below[0] + (int)c.min_d2[0] + (int)c.min_t[0] + (int)c.first_t[0] + (int)c.last_t[0]);
    }
    return 0;
}
"""


def test_adapter_offers_extent_separation_and_conflicts(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "a.o")])


def _K(t_from, t_to, dt):
    K = C.c_int64(-9)
    rc = _lib.load().uph_separation_times(t_from, t_to, dt, C.byref(K))
    return rc, K.value


def test_separation_times_against_the_mirror():
    # K = 0: a reversed window, also by one ulp
    for a, b in ((1.0, 0.5), (1.0, np.nextafter(1.0, 0.0)), (1000.0, 999.0)):
        assert _K(a, b, 0.1) == (0, 0) and separation_times(a, b, 0.1).shape == (0,)
    # K = 1: a point window, and a window shorter than dt
    for a, b, dt in ((1.0, 1.0, 0.1), (0.0, 0.0, 0.01), (2.0, 2.05, 0.1), (-3.0, np.nextafter(-2.9, -9.0), 0.1)):
        assert _K(a, b, dt) == (0, 1) and separation_times(a, b, dt).tolist() == [a]
    # t_to exactly on a sample: that sample counts, one ulp less and it does not
    for a, dt, k in ((0.0, 0.1, 3), (0.0, 0.1, 10), (1000.0, 0.1, 50), (1000.0, 0.05, 100), (-7.25, 0.01, 257), (0.3, 0.25, 1025)):
        tk = a + k * dt                                             # the product rounded, then the sum
        assert _K(a, tk, dt) == (0, k + 1) and _K(a, np.nextafter(tk, -INF), dt) == (0, k)
        tau = separation_times(a, tk, dt)
        assert tau.shape == (k + 1,) and tau[-1] == tk and tau[0] == a and separation_times(a, np.nextafter(tk, -INF), dt).shape == (k,)
    # t_from = 1000.0 and dt = 0.1: tau is t_from + k * dt, not a running sum and not one fused operation
    tau = separation_times(1000.0, 1005.0, 0.1)
    assert tau.tolist() == [1000.0 + k * 0.1 for k in range(len(tau))] and _K(1000.0, 1005.0, 0.1) == (0, len(tau)) and len(tau) in (50, 51)
    run, t = [], 1000.0
    while t <= 1005.0:
        run.append(t)
        t += 0.1
    assert run != tau.tolist()                                      # (the rollout's additive table differs on this clock)
    # random windows
    rng = np.random.default_rng(11)
    for _ in range(200):
        a = float(rng.choice([0.0, 1000.0, -12.5, rng.uniform(-50.0, 50.0)]))
        dt = float(rng.choice([0.1, 0.01, 0.05, 0.25, rng.uniform(1e-3, 0.5)]))
        b = a + float(rng.uniform(-1.0, 30.0))
        tau = separation_times(a, b, dt)
        assert _K(a, b, dt) == (0, tau.shape[0])
        if tau.shape[0]:
            assert tau[-1] <= b < a + tau.shape[0] * dt and np.array_equal(tau, a + np.arange(tau.shape[0]) * dt)
    # large clocks absorb small steps: the count follows the rounded tau, not (t_to - t_from) / dt
    for a, b, dt in ((1e16, 1e16, 0.5), (1e16, 1e16 + 4.0, 0.5), (2.0 ** 53, 2.0 ** 53, 1.0)):
        tau = separation_times(a, b, dt)
        assert _K(a, b, dt) == (0, tau.shape[0]) and tau.shape[0] > (b - a) / dt + 1
    # K > 2^22 is refused, K = 2^22 is not
    top = 1 << 22
    assert _K(0.0, float(top - 1), 1.0) == (0, top) and separation_times(0.0, float(top - 1), 1.0).shape == (top,)
    rc, K = _K(0.0, float(top), 1.0)
    assert rc == _lib.UPH_ERR_LIMIT and K == -9 and b"2^22" in _lib.load().uph_last_error()
    assert _K(0.0, 1.0, 1e-8)[0] == _lib.UPH_ERR_LIMIT and _K(1e16, 1e16, 1e-7)[0] == _lib.UPH_ERR_LIMIT
    for a, b, dt in ((0.0, float(top), 1.0), (0.0, 1.0, 1e-8)):
        with pytest.raises(_lib.UnevenHipError):
            separation_times(a, b, dt)
    for a, b, dt in ((0.0, 1.0, 0.0), (0.0, INF, 0.1), (NAN, 1.0, 0.1), (0.0, 1.0, NAN)):
        with pytest.raises(_lib.UnevenHipError):
            separation_times(a, b, dt)


def test_separation_rows_on_hand_made_rows():
    # two straight lines that cross: a along x at 1 m/s, b along y at 1 m/s through (4, 0) at tau = 4
    tau = separation_times(0.0, 8.0, 0.5)
    a = np.stack([tau, np.zeros_like(tau)], axis=1)
    b = np.stack([np.full_like(tau, 4.0), tau - 4.0], axis=1)
    r = separation_rows(tau, a, b, 1.5)
    assert r["min_d2"] == 0.0 and r["min_t"] == 4.0 and r["counts"].tolist() == [17, 5]              # d2 = 2 (tau - 4)^2 < 2.25: |tau - 4| <= 1
    assert r["first_t"] == 3.0 and r["last_t"] == 5.0
    r = separation_rows(tau, a, b, np.sqrt(0.5))                   # d2 = 0.5 at |tau - 4| = 0.5, R * R rounded
    R2 = np.sqrt(0.5) * np.sqrt(0.5)
    assert r["counts"].tolist() == [17, 3 if 0.5 < R2 else 1]
    # strictly below: d2 == R2 exactly is not below
    assert separation_rows(tau, a, b, 2.0)["counts"].tolist() == [17, 5]                               # d2 = 2, 0.5, 0 ... < 4; d2 = 4.5 at 1.5 is not
    r = separation_rows([0.0, 1.0], [[0.0, 0.0], [3.0, 0.0]], [[0.0, 4.0], [0.0, 4.0]], 5.0)         # d2 = 16, 25 against R2 = 25
    assert r["counts"].tolist() == [2, 1] and r["first_t"] == 0.0 and r["last_t"] == 0.0 and r["min_d2"] == 16.0
    # a tie: the earlier sample wins (b mirrors a about tau = 2)
    t5 = np.arange(5.0)
    r = separation_rows(t5, np.stack([t5, np.zeros(5)], axis=1), np.tile([2.0, 1.0], (5, 1)), 0.0)
    assert r["min_d2"] == 1.0 and r["min_t"] == 2.0
    r = separation_rows(t5, np.stack([np.abs(t5 - 2.0), np.zeros(5)], axis=1), np.zeros((5, 2)), 1.5)  # d2 = 4, 1, 0, 1, 4
    assert r["min_t"] == 2.0 and r["first_t"] == 1.0 and r["last_t"] == 3.0 and r["counts"].tolist() == [5, 3]
    r = separation_rows(t5, np.tile([1.0, 0.0], (5, 1)), np.zeros((5, 2)), 2.0)                       # all equal: sample 0
    assert r["min_t"] == 0.0 and r["min_d2"] == 1.0 and r["counts"].tolist() == [5, 5] and r["last_t"] == 4.0
    # a NaN row: +inf for the minimum, never below; it may not hide the samples around it
    xa = np.stack([t5, np.zeros(5)], axis=1)
    xa[2, 0] = NAN
    r = separation_rows(t5, xa, np.tile([2.0, 0.0], (5, 1)), 1.5)
    assert r["min_d2"] == 1.0 and r["min_t"] == 1.0 and r["counts"].tolist() == [5, 2] and r["first_t"] == 1.0 and r["last_t"] == 3.0
    r = separation_rows(t5, np.full((5, 2), NAN), np.zeros((5, 2)), 9.0)
    assert r["min_d2"] == INF and r["min_t"] == 0.0 and r["counts"].tolist() == [5, 0] and np.isnan(r["first_t"]) and np.isnan(r["last_t"])
    r = separation_rows(t5, np.full((5, 2), 1e200), np.zeros((5, 2)), 9.0)                             # d2 overflows: +inf, sample 0
    assert r["min_d2"] == INF and r["min_t"] == 0.0 and r["counts"].tolist() == [5, 0]
    # radius = 0 is never below, even at d2 = 0
    r = separation_rows(t5, np.ones((5, 2)), np.ones((5, 2)), 0.0)
    assert r["min_d2"] == 0.0 and r["min_t"] == 0.0 and r["counts"].tolist() == [5, 0] and np.isnan(r["first_t"])
    assert separation_rows(t5, np.ones((5, 2)), np.ones((5, 2)), 1e-300)["counts"].tolist() == [5, 0]  # R * R rounds to 0
    assert separation_rows(t5, np.ones((5, 2)), np.ones((5, 2)), 1e-150)["counts"].tolist() == [5, 5]
    # an empty window
    r = separation_rows(np.zeros(0), np.zeros((0, 2)), np.zeros((0, 2)), 1.0)
    assert r["min_d2"] == INF and np.isnan(r["min_t"]) and np.isnan(r["first_t"]) and np.isnan(r["last_t"]) and r["counts"].tolist() == [0, 0]


def test_extent_rows_on_hand_made_rows():
    xy = np.array([[1.0, -2.0], [3.0, 0.5], [-1.5, 4.0], [0.0, 0.0]])
    e = extent_rows(xy)
    assert e["box"].tolist() == [-1.5, 3.0, -2.0, 4.0] and e["counts"].tolist() == [4, 0]
    xy[2, 1] = NAN                                                 # the whole sample leaves the box, x included
    e = extent_rows(xy)
    assert e["box"].tolist() == [0.0, 3.0, -2.0, 0.5] and e["counts"].tolist() == [4, 1]
    e = extent_rows(np.full((3, 2), NAN))
    assert e["box"].tolist() == [INF, -INF, INF, -INF] and e["counts"].tolist() == [3, 3]
    e = extent_rows(np.zeros((0, 2)))
    assert e["box"].tolist() == [INF, -INF, INF, -INF] and e["counts"].tolist() == [0, 0]
    e = extent_rows([[2.0, 3.0]])
    assert e["box"].tolist() == [2.0, 2.0, 3.0, 3.0] and e["counts"].tolist() == [1, 0]


def _brute(box, rad):
    """the rule, pair by pair"""
    keep = []
    with np.errstate(invalid="ignore"):
        for i in range(len(box)):
            for j in range(i + 1, len(box)):
                R = rad[i] + rad[j]
                if box[i, 0] - box[j, 1] > R or box[j, 0] - box[i, 1] > R or box[i, 2] - box[j, 3] > R or box[j, 2] - box[i, 3] > R:
                    continue
                keep.append((i, j))
    return keep


def _native(box, rad, cap=None):
    L = _lib.load()
    box, rad = np.ascontiguousarray(box, dtype=np.float64), np.ascontiguousarray(rad, dtype=np.float64)
    n = C.c_int64(-9)
    if cap is None:
        assert L.uph_conflict_candidates(len(rad), dp(box), dp(rad), 0, None, C.byref(n)) == 0
        cap = n.value
    pairs = np.full((max(cap, 1), 2), -9, dtype=np.int32)
    assert L.uph_conflict_candidates(len(rad), dp(box), dp(rad), cap, ip(pairs), C.byref(n)) == 0
    return pairs, n.value


def _random_boxes(rng, n, span):
    lo = rng.uniform(-span, span, (n, 2))
    size = rng.uniform(0.0, 3.0, (n, 2)) * (rng.uniform(size=(n, 2)) < 0.8)        # some are points or segments
    box = np.stack([lo[:, 0], lo[:, 0] + size[:, 0], lo[:, 1], lo[:, 1] + size[:, 1]], axis=1)
    return box, rng.uniform(0.0, 0.6, n) * (rng.uniform(size=n) < 0.9)


def test_candidates_equal_the_mirror_and_the_brute_force():
    rng = np.random.default_rng(7)
    box, rad = _random_boxes(rng, 200, 14.0)
    empty = rng.choice(200, 12, replace=False)
    box[empty] = [INF, -INF, INF, -INF]
    empty = empty[empty != 5]
    box[5] = [-INF, INF, -INF, INF]                                 # the whole plane: no gap to any box is > R (to an empty box it is inf - inf), kept with all
    want = _brute(box, rad)
    assert 150 < len(want) < 200 * 199 // 2 // 4 and sum(1 for p in want if 5 in p) == 199
    assert not any(5 not in (i, j) and (i in empty or j in empty) for i, j in want) and len(empty) >= 11
    got, n = _native(box, rad)
    assert n == len(want) and got.tolist() == [list(p) for p in want]
    assert conflict_candidates(box, rad).tolist() == got.tolist() and conflict_candidates(box, rad).dtype == np.int32
    # a cap smaller than the count: the first cap pairs of the same order, the full count, nothing written beyond
    got, n = _native(box, rad, cap=37)
    assert n == len(want) and got.tolist() == [list(p) for p in want[:37]]
    big = np.full((60, 2), -9, dtype=np.int32)
    k = C.c_int64(0)
    assert _lib.load().uph_conflict_candidates(200, dp(box), dp(rad), 37, ip(big), C.byref(k)) == 0 and (big[37:] == -9).all() and (big[:37] >= 0).all()
    # all in one place (every pair), far apart (none), none at all
    same = np.tile([0.0, 1.0, 0.0, 1.0], (30, 1))
    got, n = _native(same, np.zeros(30))
    assert n == 435 and got.tolist() == [[i, j] for i in range(30) for j in range(i + 1, 30)]
    far = np.stack([10.0 * np.arange(30), 10.0 * np.arange(30) + 1.0, np.zeros(30), np.ones(30)], axis=1)
    assert _native(far, np.full(30, 4.4))[1] == 0 and _native(far, np.full(30, 4.5))[1] == 29
    assert _native(np.zeros((0, 4)), np.zeros(0), cap=0)[1] == 0 and conflict_candidates(np.zeros((0, 4)), np.zeros(0)).shape == (0, 2)
    # radii that differ a lot: the sweep may not stop at a small neighbour in front of a large one
    box = np.array([[0.0, 1.0, 0.0, 1.0], [3.0, 4.0, 0.0, 1.0], [6.0, 7.0, 0.0, 1.0], [9.0, 10.0, 0.0, 1.0]])
    rad = np.array([0.1, 0.1, 0.1, 8.0])
    assert _native(box, rad)[0].tolist() == [[0, 3], [1, 3], [2, 3]] == [list(p) for p in _brute(box, rad)] and conflict_candidates(box, rad).tolist() == [[0, 3], [1, 3], [2, 3]]


def test_boxes_that_touch_at_exactly_R_are_kept():
    # gap == R is not > R: kept; one ulp more: dropped -- in x and in y, on either side
    R = 0.75
    for axis in (0, 1):
        for side in (0, 1):
            for gap, kept in ((R, True), (np.nextafter(R, 9.0), False), (np.nextafter(R, 0.0), True)):
                a = np.array([-1.0, 0.0, -1.0, 0.0])
                b = a.copy()
                b[2 * axis:2 * axis + 2] = [gap, 1.0 + gap]
                assert b[2 * axis] - a[2 * axis + 1] == gap
                box = np.stack([a, b] if side == 0 else [b, a])
                rad = np.array([0.25, 0.5])
                assert rad[0] + rad[1] == R
                want = [[0, 1]] if kept else []
                assert [list(p) for p in _brute(box, rad)] == want and _native(box, rad)[0][:len(want)].tolist() == want and _native(box, rad)[1] == len(want)
                assert conflict_candidates(box, rad).tolist() == want
    # R = r_i + r_j is one rounded add: 0.1 + 0.2 is 0.30000000000000004, a gap of 0.3 < R is kept and so is the gap R itself
    box = np.array([[0.0, 1.0, 0.0, 1.0], [1.0 + 0.3, 2.0, 0.0, 1.0]])
    gap = box[1, 0] - box[0, 1]
    for r0, r1 in ((0.1, 0.2), (0.2, 0.1)):
        kept = not gap > r0 + r1
        assert (_native(box, [r0, r1])[1] == 1) == kept == (len(conflict_candidates(box, [r0, r1])) == 1)


def test_a_dropped_pair_is_never_below():
    """the pruning argument on numbers: points sampled inside (and on the corners of) the boxes of a dropped pair never have d2 < R * R, with the
    device's d2 -- and the argument needs no epsilon: pairs whose gap exceeds R by one ulp are among them"""
    rng = np.random.default_rng(19)
    box, rad = _random_boxes(rng, 120, 6.0)
    for k in range(0, 40, 2):                                       # pairs of neighbours whose gap in x is R exactly, or one ulp more
        R = rad[k] + rad[k + 1]
        box[k + 1, 0] = box[k, 1] + R
        if box[k + 1, 0] - box[k, 1] <= R and k % 4 == 0:
            box[k + 1, 0] = np.nextafter(box[k + 1, 0], INF)
        box[k + 1, 1] = box[k + 1, 0] + 1.0
        box[k + 1, 2:] = box[k, 2:]
    kept = set(_brute(box, rad))
    assert set(map(tuple, conflict_candidates(box, rad).tolist())) == kept
    dropped = [(i, j) for i in range(120) for j in range(i + 1, 120) if (i, j) not in kept]
    assert len(dropped) > 3000 and sum(1 for i, j in dropped if j == i + 1 and i < 40 and i % 2 == 0) >= 5
    u = np.concatenate([rng.uniform(size=(28, 2)), [[0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0]]])

    def points(b):
        return np.stack([b[0] + u[:, 0] * (b[1] - b[0]), b[2] + u[:, 1] * (b[3] - b[2])], axis=1).clip([b[0], b[2]], [b[1], b[3]])

    least = INF
    for i, j in dropped:
        pa, pb = points(box[i]), points(box[j])
        ex, ey = pa[:, None, 0] - pb[None, :, 0], pa[:, None, 1] - pb[None, :, 1]
        d2 = ex * ex + ey * ey
        R = rad[i] + rad[j]
        assert not (d2 < R * R).any(), (i, j)
        least = min(least, float((d2 - R * R).min()))
    assert least >= 0.0
    # and the rule is not vacuous: kept pairs do have such points
    close = 0
    for i, j in sorted(kept):
        pa, pb = points(box[i]), points(box[j])
        ex, ey = pa[:, None, 0] - pb[None, :, 0], pa[:, None, 1] - pb[None, :, 1]
        R = rad[i] + rad[j]
        close += bool((ex * ex + ey * ey < R * R).any())
    assert close >= len(kept) // 2
