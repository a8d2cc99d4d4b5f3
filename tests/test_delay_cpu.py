"""CPU tier of the start delays (uph_delay_times, uph_delay_levels, uph_delay_sweep_batch, uph_delay_extent_batch, uph_delays_batch): the C-ABI and its
binding, the adapter's entry points, the refusals that need no device, the host-only calls against the numpy mirrors delay_times / delay_levels, and the
mirror delay_schedule -- the sequential greedy that tests/test_gpu_delay.py holds uph_delays_batch against -- on hand-made tables with known answers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import delay_levels, delay_schedule, delay_times

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
    D, I, V = C.c_double, C.c_int32, C.c_void_p
    want = {
        "uph_delay_times": [D, D, I, DP],
        "uph_delay_levels": [I, C.c_int64, I32P, I32P],
        "uph_delay_sweep_batch": [V, V, I, I32P, I32P, DP, DP, DP, DP, D, DP, D, D, I, DP, DP, I32P, I32P, I32P],
        "uph_delay_extent_batch": [V, I, I32P, DP, DP, DP, D, D, D, I, DP, I32P],
        "uph_delays_batch": [V, I, I32P, DP, DP, I32P, D, D, D, D, D, I, I32P, DP, I32P, I64P, I32P, I32P],
        "uph_delay_kernel_ms": [V, DP],
    }
    for name, args in want.items():
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
        fn = getattr(L, name)
        assert fn.restype == C.c_int and fn.argtypes == args, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "uneven_hip.h")).read().split())
    assert "int uph_delay_times(double delay0, double delay_step, int32_t D, double* delta);" in hdr
    assert "int uph_delay_levels(int32_t n, int64_t n_pairs, const int32_t* pairs /* [n_pairs][2] */, int32_t* level /* [n] */);" in hdr
    assert ("int uph_delay_sweep_batch(uph_ctx* ca, uph_ctx* cb /* NULL: ca */, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, "
            "const double* t0_b, const double* t_from, const double* t_to, double dt, const double* radius, double delay0, double delay_step, int32_t D, "
            "double* min_d2 /* [n][D] */, double* min_t /* [n][D] */, int32_t* below /* [n][D] */, int32_t* first_clear /* [n] */, int32_t* counts /* [n]: K */);") in hdr
    assert ("int uph_delay_extent_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* t_from, const double* t_to, double dt, "
            "double delay0, double delay_step, int32_t D, double* box /* [n][4] */, int32_t* counts") in hdr
    assert ("int uph_delays_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* radius, const int32_t* n_delays /* may be NULL */, "
            "double t_from, double t_to, double dt, double delay0, double delay_step, int32_t D, int32_t* choice /* [n] */, double* start /* [n] */, "
            "int32_t* blocker /* [n] */, int64_t* n_candidates, int32_t* n_rounds, int32_t* n_unresolved);") in hdr
    assert "int uph_delay_kernel_ms(const uph_ctx* c, double* kernel_ms);" in hdr
    # the rules the header states: the table is formed on the host, the swept broad phase is the unchanged proof, no epsilon
    text_of = " ".join(re.sub(r"\n \* +", " ", open(os.path.join(ROOT, "include", "uneven_hip.h")).read()).split())         # (without the comment's line breaks)
    for text in ("delta_j = delay0 + j * delay_step", "the product rounded, then the sum", "no multiply on the device", "drops no pair that is below at any sample for any "
                 "combination of delays", "with no epsilon", "K * D > 2^26", "D > 4096", "2^20 sweep rows", "#define UPH_DELAY_TILE %d" % _lib.DELAY_TILE):
        assert text in text_of, text
    assert (_lib.DELAY_MAX, _lib.DELAY_MAX_WORK, _lib.DELAY_ROWS) == (4096, 1 << 26, 1 << 20)
    src = open(os.path.join(ROOT, "uneven_planner_amd", "csrc", "traj_query.hip")).read()
    assert "constexpr int DELAY_TILE = %d;" % _lib.DELAY_TILE in src


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
int main() {
    uneven_hip::ALMTrajOpt* o = nullptr;
    uneven_hip::ALMTrajOpt* fleet = nullptr;
    if (o) {
        uneven_hip::ALMTrajOpt::TrajDelaySweep s = o->delaySweepSE2TrajBatch({0, 1}, {1, 2}, {0.0, 0.0}, {1.0, 2.0}, {0.0, 0.0}, {9.0, 9.0}, {0.5, 0.5}, 0.0, 0.5, 8);
        s = o->delaySweepSE2TrajBatch({0}, {3}, {0.5}, {0.0}, {0.0}, {9.0}, {0.6}, -1.0, 0.25, 16, 0.05, fleet);
        uneven_hip::ALMTrajOpt::TrajExtent e = o->delayExtentSE2TrajBatch({0, 1}, {0.0, 2.5}, {0.0, 0.0}, {9.0, 9.0}, 0.0, 0.5, 8);
        e = o->delayExtentSE2TrajBatch({0}, {1000.0}, {1000.0}, {1005.0}, 0.0, 0.5, 8, 0.05);
        uneven_hip::ALMTrajOpt::TrajDelays d = o->delaysSE2TrajBatch({0, 1, 2}, {0.0, 1.0, 2.0}, {0.3, 0.3, 0.3}, 0.0, 20.0, 0.0, 0.5, 16);
        d = o->delaysSE2TrajBatch({0, 1, 2}, {0.0, 1.0, 2.0}, {0.3, 0.3, 0.3}, 0.0, 20.0, 0.0, 0.5, 16, {1, 16, 16}, 0.1);
        return s.D + (int)s.min_d2[0] + (int)s.min_t[0] + s.below[0] + s.first_clear[0] + s.counts[0] + (int)e.box[3] + e.counts[1] + d.choice[0] + (int)d.start[0] +
               d.blocker[0] + (int)d.n_candidates + d.n_rounds + d.n_unresolved;
    }
    return 0;
}
"""


def test_adapter_offers_the_delay_calls(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "a.o")])


def _times(delay0, step, D, room=None):
    out = np.full(max(D, 1) if room is None else room, -9.0)
    return _lib.load().uph_delay_times(delay0, step, D, dp(out)), out


def test_delay_times_against_the_mirror():
    # delay0 around 1000 s with a step of 0.1: delta_j = delay0 + j * step, not a running sum
    rc, got = _times(1000.0, 0.1, 64)
    assert rc == 0 and got.tolist() == [1000.0 + j * 0.1 for j in range(64)] and np.array_equal(got, delay_times(1000.0, 0.1, 64))
    run, t = [], 1000.0
    for _ in range(64):
        run.append(t)
        t += 0.1
    assert run != got.tolist()
    # steps a large delay0 absorbs: the table follows the rounded sum and does not decrease
    for d0, step in ((1e16, 0.5), (2.0 ** 53, 1.0), (-1e16, 0.75)):
        rc, got = _times(d0, step, 32)
        assert rc == 0 and np.array_equal(got, delay_times(d0, step, 32)) and (np.diff(got) >= 0.0).all() and got[1] == d0 and got.tolist() == [d0 + j * step for j in range(32)]
    # D = 1, a negative delay0, the largest table; nothing is written beyond D
    rc, got = _times(-2.5, 0.5, 1, room=3)
    assert rc == 0 and got.tolist() == [-2.5, -9.0, -9.0] and delay_times(-2.5, 0.5, 1).tolist() == [-2.5]
    rc, got = _times(-3.0, 0.3, 4096)
    assert rc == 0 and np.array_equal(got, delay_times(-3.0, 0.3, 4096)) and got[10] == -3.0 + 10 * 0.3
    rng = np.random.default_rng(3)
    for _ in range(100):
        d0, step, D = float(rng.uniform(-50.0, 1500.0)), float(rng.choice([0.1, 0.5, 0.05, rng.uniform(1e-3, 2.0)])), int(rng.integers(1, 300))
        rc, got = _times(d0, step, D)
        assert rc == 0 and np.array_equal(got, delay_times(d0, step, D)) and np.array_equal(got, d0 + np.arange(D) * step)
    # a table that overflows is a table: the starts it makes are refused where they are used
    rc, got = _times(0.0, 1e308, 4)
    assert rc == 0 and got.tolist() == [0.0, 1e308, INF, INF] and np.array_equal(got, delay_times(0.0, 1e308, 4))


def test_refusals_without_a_device():
    L = _lib.load()
    # the table
    for d0, step, D, code in ((0.0, 0.0, 4, -1), (0.0, -0.5, 4, -1), (0.0, INF, 4, -1), (0.0, NAN, 4, -1), (NAN, 0.5, 4, -1), (INF, 0.5, 4, -1), (-INF, 0.5, 4, -1),
                              (0.0, 0.5, 0, -1), (0.0, 0.5, -3, -1), (0.0, 0.5, 4097, _lib.UPH_ERR_LIMIT)):
        rc, out = _times(d0, step, D, room=8)
        assert rc == code and (out == -9).all(), (d0, step, D)
        assert b"uph_delay_times" in L.uph_last_error()
        with pytest.raises(_lib.UnevenHipError):
            delay_times(d0, step, D)
    assert L.uph_delay_times(0.0, 0.5, 4, None) == _lib.UPH_ERR_INVALID
    # the device calls without a context, outputs untouched
    one, z, w1, r = np.zeros(1, dtype=np.int32), np.zeros(1), np.ones(1), np.full(1, 0.5)
    d = {k: np.full(s, -9.0) for k, s in (("min_d2", 4), ("min_t", 4), ("box", 4), ("start", 1))}
    i = {k: np.full(s, -9, dtype=np.int32) for k, s in (("below", 4), ("first", 1), ("K", 1), ("ecounts", 2), ("choice", 1), ("blocker", 1))}
    nk, nr, nu = C.c_int64(-9), C.c_int32(-9), C.c_int32(-9)
    assert L.uph_delay_sweep_batch(None, None, 1, ip(one), ip(one), dp(z), dp(z), dp(z), dp(w1), 0.01, dp(r), 0.0, 0.5, 4, dp(d["min_d2"]), dp(d["min_t"]), ip(i["below"]),
                                   ip(i["first"]), ip(i["K"])) == _lib.UPH_ERR_INVALID
    assert b"uph_delay_sweep_batch" in L.uph_last_error()
    assert L.uph_delay_extent_batch(None, 1, ip(one), dp(z), dp(z), dp(w1), 0.01, 0.0, 0.5, 4, dp(d["box"]), ip(i["ecounts"])) == _lib.UPH_ERR_INVALID
    assert b"uph_delay_extent_batch" in L.uph_last_error()
    assert L.uph_delays_batch(None, 1, ip(one), dp(z), dp(r), None, 0.0, 1.0, 0.05, 0.0, 0.5, 4, ip(i["choice"]), dp(d["start"]), ip(i["blocker"]), C.byref(nk), C.byref(nr),
                              C.byref(nu)) == _lib.UPH_ERR_INVALID
    assert b"uph_delays_batch" in L.uph_last_error()
    ms = C.c_double(-9.0)
    assert L.uph_delay_kernel_ms(None, C.byref(ms)) == _lib.UPH_ERR_INVALID and ms.value == -9.0
    assert b"uph_delay_kernel_ms" in L.uph_last_error()
    assert all((v == -9).all() for v in d.values()) and all((v == -9).all() for v in i.values()) and (nk.value, nr.value, nu.value) == (-9, -9, -9)
    # the levels
    lv = np.full(4, -9, dtype=np.int32)
    for bad in ([[0, 1], [2, 1]], [[0, 1], [1, 1]], [[-1, 2]], [[0, 4]], [[3, 0]]):
        pr = np.array(bad, dtype=np.int32)
        assert L.uph_delay_levels(4, len(bad), ip(pr), ip(lv)) == _lib.UPH_ERR_INVALID and (lv == -9).all(), bad
        assert b"uph_delay_levels" in L.uph_last_error()
        with pytest.raises(_lib.UnevenHipError):
            delay_levels(bad, 4)
    pr = np.array([[0, 1]], dtype=np.int32)
    assert L.uph_delay_levels(-1, 0, None, ip(lv)) == _lib.UPH_ERR_INVALID and L.uph_delay_levels(4, -1, ip(pr), ip(lv)) == _lib.UPH_ERR_INVALID
    assert L.uph_delay_levels(4, 1, None, ip(lv)) == _lib.UPH_ERR_INVALID and L.uph_delay_levels(4, 1, ip(pr), None) == _lib.UPH_ERR_INVALID and (lv == -9).all()


def _levels(pairs, n):
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    lv = np.full(max(n, 1), -9, dtype=np.int32)
    assert _lib.load().uph_delay_levels(n, pr.shape[0], ip(pr) if pr.shape[0] else None, ip(lv)) == 0
    return lv[:n]


def _random_pairs(rng, n, m):
    got = set()
    while len(got) < m:
        i, j = sorted(rng.choice(n, 2, replace=False).tolist())
        got.add((i, j))
    return [list(p) for p in got]                                   # (in no particular order)


def test_delay_levels_against_the_mirror():
    assert _levels([], 5).tolist() == [0] * 5 == delay_levels([], 5).tolist() and delay_levels([], 5).dtype == np.int32
    assert _levels([], 0).shape == (0,) and delay_levels(np.zeros((0, 2)), 0).shape == (0,)
    chain = [[k, k + 1] for k in range(9)]
    assert _levels(chain, 10).tolist() == list(range(10)) == delay_levels(chain, 10).tolist()
    assert _levels(chain[::-1], 10).tolist() == list(range(10)) == delay_levels(chain[::-1], 10).tolist()
    star = [[0, k] for k in range(1, 8)]
    assert _levels(star, 8).tolist() == [0] + [1] * 7 == delay_levels(star, 8).tolist()
    into = [[k, 7] for k in range(7)]                               # a star whose hub comes last: every spoke is free, the hub waits for them all
    assert _levels(into, 8).tolist() == [0] * 7 + [1] == delay_levels(into, 8).tolist()
    assert _levels([[0, 2], [1, 2], [0, 1], [2, 5]], 6).tolist() == [0, 1, 2, 0, 0, 3]
    rng = np.random.default_rng(23)
    for n in (40, 60):
        pairs = _random_pairs(rng, n, 200)
        want = np.zeros(n, dtype=int)
        for j in range(n):                                          # the definition, vehicle by vehicle
            want[j] = max([want[i] + 1 for i, k in pairs if k == j], default=0)
        assert _levels(pairs, n).tolist() == want.tolist() == delay_levels(pairs, n).tolist() and want.max() >= 3
    # a pair named twice changes nothing
    assert _levels(chain + chain, 10).tolist() == list(range(10))


def _table_sweep(below):
    """sweep() on a hand-made table below[(h, i)][at_h] = (D,) counts"""
    return lambda h, at, i: below[(h, i)][at]


def test_delay_schedule_on_hand_made_tables():
    D = 6
    # a chain in which every vehicle must yield one step more than the one ahead: i is below h unless it starts at least one step later than h does
    n = 5
    pairs = [[k, k + 1] for k in range(n - 1)]
    below = {(k, k + 1): np.array([[0 if j > at else 3 for j in range(D)] for at in range(D)]) for k in range(n - 1)}
    got = delay_schedule(_table_sweep(below), pairs, n)
    assert got["choice"].tolist() == [0, 1, 2, 3, 4] and got["blocker"].tolist() == [-1] * 5 and got["choice"].dtype == np.int32
    # ... and with D too small for the chain the last vehicles find nothing: each stays at 0 for the next, which then clears at 1 again
    got = delay_schedule(_table_sweep(below), pairs, n, n_delays=[6, 6, 2, 6, 6])
    assert got["choice"].tolist() == [0, 1, -1, 1, 2] and got["blocker"].tolist() == [-1, -1, 1, -1, -1]
    # cleared only by the last allowed j; one fewer and it is unresolved
    b2 = {(0, 1): np.tile([2, 2, 2, 2, 2, 0], (D, 1))}
    assert delay_schedule(_table_sweep(b2), [[0, 1]], 2)["choice"].tolist() == [0, 5]
    assert delay_schedule(_table_sweep(b2), [[0, 1]], 2, n_delays=[6, 6])["choice"].tolist() == [0, 5]
    got = delay_schedule(_table_sweep(b2), [[0, 1]], 2, n_delays=[6, 5])
    assert got["choice"].tolist() == [0, -1] and got["blocker"].tolist() == [-1, 0]
    # n_delays = 1: choice is 0 or -1, and the blocker is the SMALLEST h that is below at j = 0 (1 is clear of 3 at j = 0, 0 and 2 are not)
    b3 = {(0, 3): np.tile([4, 0, 0, 0, 0, 0], (D, 1)), (1, 3): np.tile([0, 5, 5, 5, 5, 5], (D, 1)), (2, 3): np.tile([1, 1, 0, 0, 0, 0], (D, 1)),
          (0, 1): np.tile([0, 0, 0, 0, 0, 0], (D, 1))}
    p3 = [[2, 3], [0, 3], [1, 3], [0, 1]]
    got = delay_schedule(_table_sweep(b3), p3, 4, n_delays=[1, 1, 1, 1])
    assert got["choice"].tolist() == [0, 0, 0, -1] and got["blocker"].tolist() == [-1, -1, -1, 0]
    b3[(0, 3)] = np.tile([0, 0, 0, 0, 0, 0], (D, 1))
    assert delay_schedule(_table_sweep(b3), p3, 4, n_delays=[1, 1, 1, 1])["blocker"].tolist() == [-1, -1, -1, 2]
    # every partner has to be clear at the SAME j: 0 allows all, 1 allows 0 alone, 2 allows 2.. -> nothing within 6
    assert delay_schedule(_table_sweep(b3), p3, 4)["choice"].tolist() == [0, 0, 0, -1]
    b3[(1, 3)] = np.tile([0, 5, 5, 0, 5, 0], (D, 1))
    assert delay_schedule(_table_sweep(b3), p3, 4)["choice"].tolist() == [0, 0, 0, 3]
    # a vehicle behind an unresolved one avoids it at ITS j = 0 position: row `at` = 0 of the table is the one asked for
    asked = []

    def sweep(h, at, i):
        asked.append((h, at, i))
        return {(0, 1): [7, 7, 7], (1, 2): [[9, 0, 0], [9, 9, 9], [9, 9, 9]][at], (0, 2): [0, 0, 0]}[(h, i)]

    got = delay_schedule(sweep, [[0, 1], [1, 2], [0, 2]], 3)
    assert got["choice"].tolist() == [0, -1, 1] and got["blocker"].tolist() == [-1, 0, -1] and (1, 0, 2) in asked and all(at == 0 for _, at, _ in asked)
    # no partners at all, and a vehicle without one among others
    got = delay_schedule(lambda *a: 1 / 0, [], 4)
    assert got["choice"].tolist() == [0] * 4 and got["blocker"].tolist() == [-1] * 4
    got = delay_schedule(_table_sweep(b2), [[0, 1]], 3)
    assert got["choice"].tolist() == [0, 5, 0]


def test_levels_give_the_sequential_result_on_random_tables():
    rng = np.random.default_rng(41)
    some_wait = some_fail = 0
    for case in range(50):
        n, D = int(rng.integers(6, 30)), int(rng.integers(2, 9))
        pairs = _random_pairs(rng, n, int(rng.integers(n // 2, 3 * n)))
        table = {(h, i): rng.integers(0, 3, (D, D)) * (rng.uniform(size=(D, D)) < 0.45) for h, i in pairs}
        nd = rng.integers(1, D + 1, n) if case % 2 else None
        want = delay_schedule(_table_sweep(table), pairs, n, n_delays=nd)
        level = delay_levels(pairs, n)
        order = np.argsort(level, kind="stable")
        got = delay_schedule(_table_sweep(table), pairs, n, n_delays=nd, order=order.tolist())
        assert np.array_equal(got["choice"], want["choice"]) and np.array_equal(got["blocker"], want["blocker"]), case
        # any order inside a level, too
        shuffled = np.concatenate([rng.permutation(np.nonzero(level == lv)[0]) for lv in range(level.max() + 1)])
        got = delay_schedule(_table_sweep(table), pairs, n, n_delays=nd, order=shuffled.tolist())
        assert np.array_equal(got["choice"], want["choice"]) and np.array_equal(got["blocker"], want["blocker"]), case
        some_wait += int((want["choice"] > 0).any())
        some_fail += int((want["choice"] < 0).any())
        assert ((want["blocker"] >= 0) == (want["choice"] < 0)).all()
    assert some_wait >= 25 and some_fail >= 10
