"""CPU tier of the start delays with oriented rectangles (uph_footprint_delay_sweep_batch, uph_footprint_delays_batch): the C-ABI and its binding, the rules the
header states, the adapter's entry points, the refusals that need no device -- shape, margin, delay table, D, n_delays: all of them come before a context is
read --, and the schedule mirror delay_schedule driven by a `below` table that footprint_rows fills from hand-made poses: three cars on straight lines where
the circumscribed discs need a delay and the rectangles need none."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import delay_schedule, delay_times, footprint_radii, footprint_rows, separation_rows, separation_times

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
        "uph_footprint_delay_sweep_batch": [V, V, I, I32P, I32P, DP, DP, DP, DP, D, DP, DP, DP, D, D, I, DP, DP, I32P, I32P, I32P, I32P],
        "uph_footprint_delays_batch": [V, I, I32P, DP, DP, DP, I32P, D, D, D, D, D, I, I32P, DP, I32P, I64P, I32P, I32P],
    }
    for name, args in want.items():
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
        fn = getattr(L, name)
        assert fn.restype == C.c_int and fn.argtypes == args, name
    raw = open(os.path.join(ROOT, "include", "uneven_hip.h")).read()
    hdr = " ".join(raw.split())
    assert ("int uph_footprint_delay_sweep_batch(uph_ctx* ca, uph_ctx* cb /* NULL: ca */, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, "
            "const double* t0_b, const double* t_from, const double* t_to, double dt, const double* shape_a /* [n][3] */, const double* shape_b /* [n][3] */, "
            "const double* margin /* [n] */, double delay0, double delay_step, int32_t D, double* min_c2 /* [n][D] */, double* min_t /* [n][D] */, "
            "int32_t* below /* [n][D] */, int32_t* overlapping /* [n][D] */, int32_t* first_clear /* [n] */, int32_t* counts /* [n]: K */);") in hdr
    assert ("int uph_footprint_delays_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* shape /* [n][3] */, "
            "const double* margin /* [n] */, const int32_t* n_delays /* may be NULL */, double t_from, double t_to, double dt, double delay0, double delay_step, "
            "int32_t D, int32_t* choice /* [n] */, double* start /* [n] */, int32_t* blocker /* [n] */, int64_t* n_candidates, int32_t* n_rounds, "
            "int32_t* n_unresolved);") in hdr
    # the rules the header states: the row is footprint_separation's bit for bit, the device only adds, the schedule is unchanged, the broad phase is the two
    # existing arguments one after the other with no new epsilon, the refusals are the union and come before any output
    text_of = " ".join(re.sub(r"\n \* +", " ", raw).split())         # (without the comment's line breaks)
    for text in ("row (q, j) holds min_c2, min_t, below and overlapping of uph_footprint_separation_batch", "over the same window, dt and margin, bit for bit",
                 "K = 0 gives +inf, NaN, 0, 0", "the device performs only the add t0_b + delta_j", "first_clear[q] is the smallest j with below == 0 (-1: none)",
                 "counts[q] = K", "the schedule above, unchanged in every rule", "M = margin[h] + margin[i], one rounded add as in uph_footprint_conflicts_batch",
                 "uph_conflict_candidates on the swept boxes of uph_delay_extent_batch with uph_footprint_radii's radii",
                 "every position a vehicle takes at any sample under any delay of the table lies in its swept box", "share of 2^-40", "No new epsilon",
                 "The refusals are the union of the refusals of uph_footprint_separation_batch / uph_footprint_conflicts_batch and of uph_delay_sweep_batch / "
                 "uph_delays_batch", "UPH_ERR_LIMIT for D > 4096 and for a query with K * D > 2^26", "each before any output is written",
                 "the shape and margin checks come first", "last uph_footprint_delay_sweep_batch or uph_footprint_delays_batch"):
        assert text in text_of, text
    # ... and what was there before is still there, word for word (tests/test_delay_cpu.py and tests/test_footprint_cpu.py search it)
    for text in ("milliseconds of the kernels of the last uph_delay_sweep_batch, uph_delay_extent_batch or uph_delays_batch of c (events on the context's stream)",
                 "uph_conflict_candidates with these radii therefore drops no pair that is below at any sample"):
        assert text in text_of, text
    src = open(os.path.join(ROOT, "uneven_planner_amd", "csrc", "traj_query.hip")).read()
    assert "void uph_footprint_sweep_kernel(PairArgs<FootQuery, FootSweepOut> a)" in src and "sizeof(FootSweepOut) == 32" in src


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
int main() {
    uneven_hip::ALMTrajOpt* o = nullptr;
    uneven_hip::ALMTrajOpt* fleet = nullptr;
    if (o) {
        const std::array<double, 3> car{0.45, 0.15, 0.15};
        uneven_hip::ALMTrajOpt::TrajFootprintDelaySweep s = o->footprintDelaySweepSE2TrajBatch({0, 1}, {1, 2}, {0.0, 0.0}, {1.0, 2.0}, {0.0, 0.0}, {9.0, 9.0}, {car, car},
                                                                                               {car, car}, {0.1, 0.0}, 0.0, 0.5, 8);
        s = o->footprintDelaySweepSE2TrajBatch({0}, {3}, {0.5}, {0.0}, {0.0}, {9.0}, {car}, {car}, {0.2}, -1.0, 0.25, 16, 0.05, fleet);
        uneven_hip::ALMTrajOpt::TrajDelays d = o->footprintDelaysSE2TrajBatch({0, 1, 2}, {0.0, 1.0, 2.0}, {car, car, car}, {0.05, 0.05, 0.05}, 0.0, 20.0, 0.0, 0.5, 16);
        d = o->footprintDelaysSE2TrajBatch({0, 1, 2}, {0.0, 1.0, 2.0}, {car, car, car}, {0.05, 0.05, 0.05}, 0.0, 20.0, 0.0, 0.5, 16, {1, 16, 16}, 0.1);
        return s.D + (int)s.min_c2[0] + (int)s.min_t[0] + s.below[0] + s.overlapping[0] + s.first_clear[0] + s.counts[0] + d.choice[0] + (int)d.start[0] + d.blocker[0] +
               (int)d.n_candidates + d.n_rounds + d.n_unresolved;
    }
    return 0;
}
"""


def test_adapter_offers_the_footprint_delay_calls(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "a.o")])


class _Calls:
    """the two calls through ctypes on pre-filled outputs.  ctx: None, or a block of zeros that stands for a context -- every refusal asked for here comes before
    the call reads its context, which is the point of the test"""

    def __init__(self):
        self.L = _lib.load()
        self.block = C.create_string_buffer(1 << 16)

    def run(self, call, ctx=True, n=2, shape=None, shape_b=None, margin=None, delay0=0.0, step=0.5, D=4, nd=None, null=()):
        tr, z, w = np.zeros(2, dtype=np.int32), np.zeros(2), np.ones(2)
        sh = np.ascontiguousarray(np.tile([0.45, 0.15, 0.15], (2, 1)) if shape is None else shape, dtype=np.float64)
        sb = np.ascontiguousarray(sh if shape_b is None else shape_b, dtype=np.float64)
        m = np.ascontiguousarray(np.full(2, 0.1) if margin is None else margin, dtype=np.float64)
        nd = None if nd is None else np.ascontiguousarray(nd, dtype=np.int32)
        h = C.cast(self.block, C.c_void_p) if ctx else None
        arg = lambda name, v: None if name in null else v
        rows = 2 * max(1, min(D, 4096))
        if call == "sweep":
            o = dict(min_c2=np.full(rows, -9.0), min_t=np.full(rows, -9.0), below=np.full(rows, -9, dtype=np.int32), over=np.full(rows, -9, dtype=np.int32),
                     first=np.full(2, -9, dtype=np.int32), K=np.full(2, -9, dtype=np.int32))
            rc = self.L.uph_footprint_delay_sweep_batch(h, None, n, ip(tr), ip(tr), dp(z), dp(z), dp(z), dp(w), 0.01, arg("shape_a", dp(sh)), arg("shape_b", dp(sb)),
                                                        arg("margin", dp(m)), delay0, step, D, dp(o["min_c2"]), dp(o["min_t"]), ip(o["below"]), ip(o["over"]),
                                                        ip(o["first"]), ip(o["K"]))
        else:
            o = dict(choice=np.full(2, -9, dtype=np.int32), start=np.full(2, -9.0), blocker=np.full(2, -9, dtype=np.int32), nk=np.full(1, -9, dtype=np.int64),
                     nr=np.full(1, -9, dtype=np.int32), nu=np.full(1, -9, dtype=np.int32))
            rc = self.L.uph_footprint_delays_batch(h, n, arg("traj", ip(tr)), arg("t0", dp(z)), arg("shape", dp(sh)), arg("margin", dp(m)), None if nd is None else ip(nd),
                                                   0.0, 1.0, 0.05, delay0, step, D, ip(o["choice"]), dp(o["start"]), ip(o["blocker"]),
                                                   o["nk"].ctypes.data_as(I64P), ip(o["nr"]), ip(o["nu"]))
        return rc, o, self.L.uph_last_error()


def test_refusals_without_a_device():
    T = _Calls()
    names = {"sweep": b"uph_footprint_delay_sweep_batch", "delays": b"uph_footprint_delays_batch"}

    def refused(call, word=None, code=_lib.UPH_ERR_INVALID, **kw):
        rc, o, err = T.run(call, **kw)
        assert rc == code and all((v == -9).all() for v in o.values()), (call, kw, rc, err)
        assert names[call] in err and (word is None or word in err), (call, kw, err)

    car = np.tile([0.45, 0.15, 0.15], (2, 1))
    for call in ("sweep", "delays"):
        # no context, no query, a missing array
        refused(call, b"bad arguments", ctx=False)
        for n in (0, -2):
            refused(call, b"bad arguments", n=n)
        for null in (("shape_a", "shape_b", "margin") if call == "sweep" else ("traj", "t0", "shape", "margin")):
            refused(call, b"bad arguments", null=(null,))
        # the shapes and the margins, first of all: also with a table that would be refused
        for bad in (-1e-9, NAN, INF, -INF):
            for col in range(3):
                s = car.copy()
                s[1, col] = bad
                refused(call, b"shape", shape=s)
                refused(call, b"shape", shape=s, D=0, step=-1.0)
                if call == "sweep":
                    refused(call, b"shape_b", shape_b=s)
            refused(call, b"margin", margin=[0.1, bad])
            refused(call, b"margin", margin=[0.1, bad], D=5000)
        if call == "delays":                                        # a shape and margin whose radius overflows
            refused(call, b"radius", shape=[[1e308, 0.0, 1e308], [0.45, 0.15, 0.15]], margin=[1e308, 0.1])
        # the delay table and D
        for step in (0.0, -0.5, INF, NAN):
            refused(call, b"delay_step", step=step)
        for d0 in (NAN, INF, -INF):
            refused(call, b"delay0", delay0=d0)
        for D in (0, -3):
            refused(call, b"D must be at least 1", D=D)
        refused(call, b"4096", code=_lib.UPH_ERR_LIMIT, D=4097)
    # n_delays outside [1, D]
    for nd in ([1, 0], [5, 1], [-1, 1], [1, 4097]):
        refused("delays", b"n_delays", nd=nd)
    refused("delays", b"4096", code=_lib.UPH_ERR_LIMIT, nd=[1, 4097], D=4097)      # (the table before the limits)


# ---- the schedule on hand-made poses.  Three cars of 0.6 m x 0.3 m (the trajectory's point 0.15 m ahead of the rear bumper) at 0.5 m/s on straight lines: car 0
# along the x axis, cars 1 and 2 along x = 0 and x = 2 towards +y, each crossing car 0's line LAG = 1.3 m behind it.  Where the three rectangles are nearest (car
# 0's point 0.5 m past the crossing) the facing corners are 0.2 m apart along each axis: 0.283 m, more than the margin M = 0.1 m, so no car has to wait.  The
# circumscribed discs (rho + m = 0.524 m, R = 1.049 m for a pair) see the points 1.3 / sqrt(2) = 0.919 m apart and make cars 1 and 2 wait; one step of 1 s
# (0.5 m more lag: 1.273 m) clears them.
CAR, M_EACH, SPEED, TOTAL, LAG = (0.45, 0.15, 0.15), 0.05, 0.5, 16.0, 1.3
LINES = (((-3.0, 0.0), 0.0), ((0.0, -3.0 - LAG), np.pi / 2), ((2.0, -5.0 - LAG), np.pi / 2))          # start point and heading


def _pose(i, tau, start):
    """car i started at `start` on the common clock: it stands at its first point before and at its last after (uph_separation_batch's clamp)"""
    (x0, y0), yaw = LINES[i]
    s = SPEED * np.clip(tau - start, 0.0, TOTAL)
    return np.stack([x0 + s * np.cos(yaw), y0 + s * np.sin(yaw)], axis=1), np.full(tau.shape[0], yaw)


def test_the_rectangles_need_no_delay_where_the_discs_do():
    D, step = 4, 1.0
    delta = delay_times(0.0, step, D)
    tau = separation_times(0.0, 24.0, 0.05)
    pairs = [[0, 1], [0, 2], [1, 2]]
    r = footprint_radii(np.tile(CAR, (3, 1)), M_EACH)
    assert abs(r[0] - (np.hypot(0.45, 0.15) + 0.05)) < 1e-9
    c2_at_0 = {}

    def rect_sweep(h, at, i):
        below = np.zeros(D, dtype=np.int32)
        for j in range(D):
            (pa, wa), (pb, wb) = _pose(h, tau, delta[at]), _pose(i, tau, delta[j])
            row = footprint_rows(tau, pa, wa, CAR, pb, wb, CAR, M_EACH + M_EACH)
            below[j] = row["counts"][1]
            if j == 0 and at == 0:
                c2_at_0[(h, i)] = row["min_c2"]
        return below

    def disc_sweep(h, at, i):
        return np.array([separation_rows(tau, _pose(h, tau, delta[at])[0], _pose(i, tau, delta[j])[0], r[h] + r[i])["counts"][1] for j in range(D)], dtype=np.int32)

    rect = delay_schedule(rect_sweep, pairs, 3)
    disc = delay_schedule(disc_sweep, pairs, 3)
    assert rect["choice"].tolist() == [0, 0, 0] and rect["blocker"].tolist() == [-1, -1, -1]
    assert disc["choice"].tolist() == [0, 1, 1] and disc["blocker"].tolist() == [-1, -1, -1]
    # the numbers behind it: the rectangles' closest approach is the corner distance worked out above, the discs' is LAG / sqrt(2)
    assert abs(np.sqrt(c2_at_0[(0, 1)]) - np.hypot(0.2, 0.2)) < 1e-3 and abs(np.sqrt(c2_at_0[(0, 2)]) - np.hypot(0.2, 0.2)) < 1e-3 and c2_at_0[(1, 2)] > 1.0
    assert disc_sweep(0, 0, 1).tolist()[0] > 0 and disc_sweep(0, 0, 1).tolist()[1:] == [0, 0, 0] and (rect_sweep(0, 0, 1) == 0).all()
    # a margin the rectangles do not keep either: then they wait too, and one step clears them as well (the corners are then 0.45 m apart along each axis)
    wide = lambda h, at, i: np.array([footprint_rows(tau, *_pose(h, tau, delta[at]), CAR, *_pose(i, tau, delta[j]), CAR, 0.3)["counts"][1] for j in range(D)])
    assert delay_schedule(wide, pairs, 3)["choice"].tolist() == [0, 1, 1]
    # with one delay each the discs leave cars 1 and 2 unresolved, blocked by car 0; the rectangles leave nobody
    one = delay_schedule(disc_sweep, pairs, 3, n_delays=[1, 1, 1])
    assert one["choice"].tolist() == [0, -1, -1] and one["blocker"].tolist() == [-1, 0, 0]
    assert delay_schedule(rect_sweep, pairs, 3, n_delays=[1, 1, 1])["choice"].tolist() == [0, 0, 0]
