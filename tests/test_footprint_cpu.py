"""CPU tier of the oriented-rectangle footprints between resident trajectories (uph_footprint_radii, uph_footprint_separation_batch,
uph_footprint_conflicts_batch, uph_footprint_kernel_ms): the C-ABI and its binding, the host-only radii against the numpy mirror, the refusals that need
no device, the adapter's entry points, and the mirrors footprint_clearance2 / footprint_rows -- the rule of include/uneven_hip.h that
tests/test_gpu_footprint.py holds the device against -- on hand-made cases with known answers, against a geometry written independently of the rule
(sampled boundaries, segment intersection) on random rectangles, and the broad-phase argument on numbers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import conflict_candidates, footprint_clearance2, footprint_radii, footprint_rows

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
        "uph_footprint_radii": [C.c_int32, DP, DP, DP],
        "uph_footprint_separation_batch": [C.c_void_p, C.c_void_p, C.c_int32, I32P, I32P, DP, DP, DP, DP, C.c_double, DP, DP, DP, DP, DP, DP, DP, I32P],
        "uph_footprint_conflicts_batch": [C.c_void_p, C.c_int32, I32P, DP, DP, DP, C.c_double, C.c_double, C.c_double, C.c_int64, I32P, DP, I32P, I64P, I64P],
        "uph_footprint_kernel_ms": [C.c_void_p, DP],
    }
    for name, args in want.items():
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
        fn = getattr(L, name)
        assert fn.restype == C.c_int and fn.argtypes == args, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "uneven_hip.h")).read().split())
    assert "int uph_footprint_radii(int32_t n, const double* shape /* [n][3]: front, rear, half_width */, const double* margin /* [n] */, double* r /* [n] */);" in hdr
    assert ("int uph_footprint_separation_batch(uph_ctx* ca, uph_ctx* cb /* NULL: ca */, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, "
            "const double* t0_b, const double* t_from, const double* t_to, double dt, const double* shape_a /* [n][3] */, const double* shape_b /* [n][3] */, "
            "const double* margin /* [n] */, double* min_c2") in hdr
    assert ("int uph_footprint_conflicts_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* shape /* [n][3] */, "
            "const double* margin /* [n]: per vehicle */, double t_from, double t_to, double dt, int64_t cap, int32_t* pairs") in hdr
    assert "int uph_footprint_kernel_ms(const uph_ctx* c, double* kernel_ms);" in hdr


def _radii(shape, margin, n=None, null=()):
    shape, margin = np.ascontiguousarray(shape, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(margin, dtype=np.float64)
    r = np.full(max(1, margin.size), -9.0)
    arg = lambda name, v: None if name in null else v
    rc = _lib.load().uph_footprint_radii(margin.size if n is None else n, arg("shape", dp(shape)), arg("margin", dp(margin)), arg("r", dp(r)))
    return rc, r


def test_radii_equal_the_mirror_bit_for_bit_and_refuse_what_the_rule_excludes():
    rng = np.random.default_rng(3)
    shape = rng.uniform(0.0, 1.5, (500, 3)) * (rng.uniform(size=(500, 3)) < 0.85)      # zeros among them
    margin = rng.uniform(0.0, 0.5, 500) * (rng.uniform(size=500) < 0.8)
    shape[:4] = [[0.0, 0.0, 0.0], [0.4, 0.2, 0.15], [0.2, 0.4, 0.15], [3.0, 0.0, 4.0]]
    margin[:4] = [0.0, 0.0, 0.1, 0.0]
    rc, r = _radii(shape, margin)
    want = footprint_radii(shape, margin)
    assert rc == 0 and np.array_equal(r, want)
    k = 1.0 + 2.0 ** -40
    assert r[0] == 0.0 and r[1] == np.hypot(0.4, 0.15) * k and r[2] == (np.hypot(0.4, 0.15) + 0.1) * k and r[3] == 5.0 * k
    # the radius covers the rectangle and the margin: every corner lies within hypot(max(front, rear), half_width) of the point
    far = np.sqrt(np.maximum(shape[:, 0], shape[:, 1]) ** 2 + shape[:, 2] ** 2)
    assert (r >= far + margin).all() and (r <= (far + margin) * (1.0 + 2.0 ** -39) + 1e-300).all()
    assert np.array_equal(footprint_radii([0.4, 0.2, 0.15], 0.1), r[1:2] * 0 + (np.hypot(0.4, 0.15) + 0.1) * k)
    L = _lib.load()
    for bad in (-1e-9, NAN, INF, -INF):
        for col in range(3):
            s = shape[:5].copy()
            s[3, col] = bad
            rc, r = _radii(s, margin[:5])
            assert rc == _lib.UPH_ERR_INVALID and (r == -9.0).all() and b"shape" in L.uph_last_error() and b"uph_footprint_radii" in L.uph_last_error(), (bad, col)
            with pytest.raises(_lib.UnevenHipError):
                footprint_radii(s, margin[:5])
        m = margin[:5].copy()
        m[2] = bad
        rc, r = _radii(shape[:5], m)
        assert rc == _lib.UPH_ERR_INVALID and (r == -9.0).all() and b"margin" in L.uph_last_error(), bad
        with pytest.raises(_lib.UnevenHipError):
            footprint_radii(shape[:5], m)
    for null in ("shape", "margin", "r"):
        rc, r = _radii(shape[:5], margin[:5], null=(null,))
        assert rc == _lib.UPH_ERR_INVALID and (r == -9.0).all() and b"uph_footprint_radii" in L.uph_last_error()
    assert _radii(shape[:5], margin[:5], n=-1)[0] == _lib.UPH_ERR_INVALID
    assert L.uph_footprint_radii(0, None, None, None) == 0


def test_refusals_without_a_device():
    L = _lib.load()
    one, z, w1, m = np.zeros(1, dtype=np.int32), np.zeros(1), np.ones(1), np.full(1, 0.1)
    sh = np.array([[0.4, 0.2, 0.15]])
    d = {k: np.full(s, -9.0) for k, s in (("min_c2", 1), ("min_t", 1), ("first_t", 1), ("last_t", 1), ("rows", 4))}
    i = {k: np.full(s, -9, dtype=np.int32) for k, s in (("counts", 3), ("pairs", 2), ("below", 1))}
    nc, nk = C.c_int64(-9), C.c_int64(-9)
    assert L.uph_footprint_separation_batch(None, None, 1, ip(one), ip(one), dp(z), dp(z), dp(z), dp(w1), 0.01, dp(sh), dp(sh), dp(m), dp(d["min_c2"]), dp(d["min_t"]),
                                            dp(d["first_t"]), dp(d["last_t"]), ip(i["counts"])) == _lib.UPH_ERR_INVALID
    assert b"uph_footprint_separation_batch" in L.uph_last_error()
    assert L.uph_footprint_conflicts_batch(None, 1, ip(one), dp(z), dp(sh), dp(m), 0.0, 1.0, 0.05, 1, ip(i["pairs"]), dp(d["rows"]), ip(i["below"]), C.byref(nc),
                                           C.byref(nk)) == _lib.UPH_ERR_INVALID
    assert b"uph_footprint_conflicts_batch" in L.uph_last_error()
    ms = C.c_double(-9.0)
    assert L.uph_footprint_kernel_ms(None, C.byref(ms)) == _lib.UPH_ERR_INVALID and ms.value == -9.0
    assert b"uph_footprint_kernel_ms" in L.uph_last_error()
    assert all((v == -9).all() for v in d.values()) and all((v == -9).all() for v in i.values()) and nc.value == -9 and nk.value == -9


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
int main() {
    uneven_hip::ALMTrajOpt* o = nullptr;
    uneven_hip::ALMTrajOpt* fleet = nullptr;
    if (o) {
        const std::array<double, 3> car{0.4, 0.2, 0.15};
        uneven_hip::ALMTrajOpt::TrajFootprintSeparation s = o->footprintSeparationSE2TrajBatch({0, 1}, {1, 2}, {0.0, 0.0}, {1.0, 2.0}, {0.0, 0.0}, {9.0, 9.0}, {car, car},
                                                                                               {car, car}, {0.1, 0.0});
        s = o->footprintSeparationSE2TrajBatch({0}, {3}, {0.5}, {0.0}, {0.0}, {9.0}, {car}, {car}, {0.2}, 0.05, fleet);
        uneven_hip::ALMTrajOpt::TrajFootprintConflicts c = o->footprintConflictsSE2TrajBatch({0, 1, 2}, {0.0, 1.0, 2.0}, {car, car, car}, {0.05, 0.05, 0.05}, 0.0, 20.0);
        c = o->footprintConflictsSE2TrajBatch({0, 1, 2}, {0.0, 1.0, 2.0}, {car, car, car}, {0.05, 0.05, 0.05}, 0.0, 20.0, 0.1, 16);
        return (s.conflicts(0) ? (int)s.min_c2[0] + (int)s.min_t[0] + (int)s.first_t[0] + (int)s.last_t[0] + s.counts[0] + s.overlaps(0) : 0) + (int)c.n_conflicts +
               (int)c.n_candidates + (c.pairs.empty() ? 0 : c.pairs[0][1] + c.below[0] + (int)c.min_c2[0] + (int)c.min_t[0] + (int)c.first_t[0] + (int)c.last_t[0]);
    }
    return 0;
}
"""


def test_adapter_offers_footprint_separation_and_conflicts(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "a.o")])


def _c2(pa, wa, sa, pb, wb, sb):
    c2, over, g = footprint_clearance2([pa], [wa], sa, [pb], [wb], sb, gap=True)
    return float(c2[0]), bool(over[0]), float(g[0])


def test_clearance_on_hand_made_cases():
    sq = (0.5, 0.5, 0.5)                                            # the unit square about its point
    # axis-aligned, a gap along x: a spans x in [-0.5, 0.25], b (front 0.75, rear 0.25) at x = 2 spans [1.75, 2.75]
    c2, over, g = _c2((0.0, 0.0), 0.0, (0.25, 0.5, 0.125), (2.0, 0.25), 0.0, (0.75, 0.25, 0.5))
    assert c2 == 1.5 ** 2 and not over and g == 1.5
    c2, over, g = _c2((2.0, 0.25), 0.0, (0.75, 0.25, 0.5), (0.0, 0.0), 0.0, (0.25, 0.5, 0.125))
    assert c2 == 1.5 ** 2 and not over and g == 1.5
    # ... and the same turned by pi (cos = -1 exactly, sin of the order of 1e-16): front and rear change sides
    c2, over, _ = _c2((0.0, 0.0), np.pi, (0.5, 0.25, 0.125), (2.0, 0.25), 0.0, (0.75, 0.25, 0.5))
    assert abs(c2 - 2.25) <= 1e-15 * 2.25 and not over
    # corner to corner on the diagonal: unit squares about (0, 0) and (2, 2), the corners (0.5, 0.5) and (1.5, 1.5)
    c2, over, g = _c2((0.0, 0.0), 0.0, sq, (2.0, 2.0), 0.0, sq)
    assert c2 == 2.0 and not over and g == 1.0
    # a corner against a square turned by 45 degrees: its edge faces the corner, 1.5 sqrt 2 - 0.5 away
    c2, over, g = _c2((0.0, 0.0), 0.0, sq, (2.0, 2.0), np.pi / 4, sq)
    want = (1.5 * np.sqrt(2.0) - 0.5) ** 2
    assert abs(c2 - want) <= 4e-15 * want and not over and abs(g - np.sqrt(want)) <= 1e-14
    # a cross: two bars of 4 x 0.25 at right angles and at 45 degrees -- no corner of either lies inside the other
    bar = (2.0, 2.0, 0.125)
    for yaw in (np.pi / 2, np.pi / 4, -1.0):
        c2, over, g = _c2((0.0, 0.0), 0.0, bar, (0.3, 0.0), yaw, bar)
        assert c2 == 0.0 and over and g < -0.09
    # the same bars side by side do not overlap: 0.5 apart, 0.25 wide
    c2, over, g = _c2((0.0, 0.0), 0.0, bar, (0.3, 0.5), 0.0, bar)
    assert c2 == 0.25 ** 2 == g * g and not over
    # one inside the other
    for yaw in (0.0, 0.7, 3.0):
        c2, over, g = _c2((0.0, 0.0), 0.0, (1.0, 1.0, 1.0), (0.25, 0.125), yaw, (0.125, 0.125, 0.125))
        assert c2 == 0.0 and over and g < -0.5
        c2, over, g = _c2((0.25, 0.125), yaw, (0.125, 0.125, 0.125), (0.0, 0.0), 0.0, (1.0, 1.0, 1.0))
        assert c2 == 0.0 and over
    # touching edges count as overlapping, one ulp apart does not
    c2, over, g = _c2((0.0, 0.0), 0.0, sq, (1.0, 0.25), 0.0, sq)
    assert c2 == 0.0 and over and g == 0.0
    c2, over, g = _c2((0.0, 0.0), 0.0, sq, (np.nextafter(1.0, 2.0), 0.25), 0.0, sq)
    assert not over and 0.0 < g < 1e-15 and c2 == g * g
    c2, over, g = _c2((0.0, 0.0), 0.0, sq, (1.0, 1.0), 0.0, sq)     # touching corners
    assert c2 == 0.0 and over and g == 0.0
    # a point against a rectangle: outside a corner, beside an edge, inside
    pt = (0.0, 0.0, 0.0)
    box = (0.5, 0.5, 0.25)
    c2, over, _ = _c2((2.0, 1.0), 0.3, pt, (0.0, 0.0), 0.0, box)
    assert c2 == 1.5 ** 2 + 0.75 ** 2 and not over
    c2, over, _ = _c2((0.0, 0.0), 0.0, box, (0.25, -1.0), 2.0, pt)
    assert c2 == 0.75 ** 2 and not over
    c2, over, _ = _c2((0.25, 0.125), 1.0, pt, (0.0, 0.0), 0.0, box)
    assert c2 == 0.0 and over
    c2, over, _ = _c2((0.5, 0.25), 1.0, pt, (0.0, 0.0), 0.0, box)   # on the corner
    assert c2 == 0.0 and over
    # a segment (half_width 0) against a segment
    c2, over, _ = _c2((0.0, 0.0), 0.0, (1.0, 1.0, 0.0), (0.0, 0.5), 0.0, (1.0, 0.0, 0.0))
    assert c2 == 0.25 and not over
    # a point against a point: the distance comes out in the other point's turned axes, to rounding
    rng = np.random.default_rng(5)
    for _ in range(50):
        pa, pb = rng.uniform(-1.0, 1.0, 2), rng.uniform(-1.0, 1.0, 2)
        c2, over, _ = _c2(pa, rng.uniform(-7.0, 7.0), pt, pb, rng.uniform(-7.0, 7.0), pt)
        want = (pa[0] - pb[0]) ** 2 + (pa[1] - pb[1]) ** 2
        assert abs(c2 - want) <= 1e-15 * want and not over
    c2, over, g = _c2((0.5, 0.5), 1.0, pt, (0.5, 0.5), 2.0, pt)     # the same point: touching
    assert c2 == 0.0 and over and g == 0.0
    # a pose that is not finite: NaN, neither overlapping nor anything else -- in any of the six values
    for k in range(6):
        for bad in (NAN, INF):
            v = [0.0, 0.0, 0.0, 0.1, 0.1, 0.0]
            v[k] = bad
            c2, over, g = _c2(v[0:2], v[2], sq, v[3:5], v[5], sq)
            assert np.isnan(c2) and not over and np.isnan(g), (k, bad)
    # the rule is symmetric in the two vehicles up to rounding and does not move with the place on the map
    for _ in range(50):
        pa, pb, wa, wb = rng.uniform(-1.0, 1.0, 2), rng.uniform(-1.0, 1.0, 2), rng.uniform(-7.0, 7.0), rng.uniform(-7.0, 7.0)
        sa, sb = rng.uniform(0.0, 0.5, 3), rng.uniform(0.0, 0.5, 3)
        x, y = _c2(pa, wa, sa, pb, wb, sb), _c2(pb, wb, sb, pa, wa, sa)
        assert x[1] == y[1] and abs(x[0] - y[0]) <= 1e-14 and abs(x[2] - y[2]) <= 1e-14
        z = _c2(pa + 64.0, wa, sa, (pb + 64.0), wb, sb)
        assert x[1] == z[1] and abs(x[0] - z[0]) <= 1e-13


def _corners(p, w, s):
    f, r, h = s
    c, sn = np.cos(w), np.sin(w)
    loc = np.array([[f, h], [-r, h], [-r, -h], [f, -h]])
    return np.stack([p[0] + loc[:, 0] * c - loc[:, 1] * sn, p[1] + loc[:, 0] * sn + loc[:, 1] * c], axis=1)


def _boundary(cs, m):
    t = np.linspace(0.0, 1.0, m, endpoint=False)[:, None]
    return np.concatenate([cs[k] + t * (cs[(k + 1) % 4] - cs[k]) for k in range(4)])


def _cross(o, a, b):
    return (a[..., 0] - o[..., 0]) * (b[..., 1] - o[..., 1]) - (a[..., 1] - o[..., 1]) * (b[..., 0] - o[..., 0])


def _polygons_meet(P, Q):
    """two convex quadrilaterals (corners in order) share a point: an edge of one crosses an edge of the other, or a corner of one lies inside the other
    -- written without any separating axis"""
    for i in range(4):
        a, b = P[i], P[(i + 1) % 4]
        for j in range(4):
            c, d = Q[j], Q[(j + 1) % 4]
            if _cross(a, b, c) * _cross(a, b, d) <= 0.0 and _cross(c, d, a) * _cross(c, d, b) <= 0.0:
                return True
    for X, Y in ((P, Q), (Q, P)):
        s = np.array([_cross(Y[j], Y[(j + 1) % 4], X[0]) for j in range(4)])
        if (s >= 0.0).all() or (s <= 0.0).all():
            return True
    return False


def test_clearance_against_sampled_boundaries_on_random_rectangles():
    """2000 random pairs in the shape range of a small car.  The distance between points sampled on the two boundaries is an upper bound of the true
    distance and exceeds it by at most the sampling pitch; whether the rectangles overlap is decided by segment crossings and containment.  The sandwich
    g <= sqrt(c2) ties the separating-axis half of the rule to the distance half."""
    rng = np.random.default_rng(17)
    n, per_edge = 2000, 128
    worst, n_over, worst_sandwich = 0.0, 0, -INF
    for _ in range(n):
        pa, pb = rng.uniform(-1.0, 1.0, 2), rng.uniform(-1.0, 1.0, 2)
        wa, wb = rng.uniform(-7.0, 7.0, 2)
        sa = np.array([rng.uniform(0.1, 0.5), rng.uniform(0.0, 0.3), rng.uniform(0.05, 0.25)])
        sb = np.array([rng.uniform(0.1, 0.5), rng.uniform(0.0, 0.3), rng.uniform(0.05, 0.25)])
        c2, over, g = _c2(pa, wa, sa, pb, wb, sb)
        A, B = _corners(pa, wa, sa), _corners(pb, wb, sb)
        assert over == _polygons_meet(A, B), (pa, wa, sa, pb, wb, sb)
        n_over += over
        if over:
            assert c2 == 0.0 and g <= 0.0
            continue
        ba, bb = _boundary(A, per_edge), _boundary(B, per_edge)
        pitch = max(2.0 * sa[2], sa[0] + sa[1], 2.0 * sb[2], sb[0] + sb[1]) / per_edge
        sampled = np.sqrt(((ba[:, None, :] - bb[None, :, :]) ** 2).sum(axis=2).min())
        diff = sampled - np.sqrt(c2)
        assert -1e-12 <= diff <= pitch, (diff, pitch, pa, wa, sa, pb, wb, sb)
        worst = max(worst, diff)
        assert 0.0 < g <= np.sqrt(c2) + 1e-14, (g, c2)
        worst_sandwich = max(worst_sandwich, g - np.sqrt(c2))
    print("random rectangles: %d of %d overlap; sampled - sqrt(c2) at most %.3g m; g - sqrt(c2) at most %.3g" % (n_over, n, worst, worst_sandwich))
    assert 0.1 * n < n_over < 0.3 * n


def test_footprint_rows_on_hand_made_rows():
    car, pt = (0.5, 0.25, 0.125), (0.0, 0.0, 0.0)
    t5 = np.arange(5.0)
    z5 = np.zeros(5)
    # b passes a along x, 1 m to the side: a spans x in [-0.25, 0.5], y in +-0.125; b the same about (x, 1): the gap is 0.75 in y while they are abreast
    xa, xb = np.zeros((5, 2)), np.stack([t5 - 2.0, np.ones(5)], axis=1)
    r = footprint_rows(t5, xa, z5, car, xb, z5, car, 0.5)
    assert r["min_c2"] == 0.75 ** 2 and r["min_t"] == 2.0 and r["counts"].tolist() == [5, 0, 0] and np.isnan(r["first_t"]) and np.isnan(r["last_t"])
    r = footprint_rows(t5, xa, z5, car, xb, z5, car, 0.8)           # abreast at tau = 2 (c2 = 0.5625) and, nose to tail by 0.25 in x, at 1 and 3 (0.625)
    assert r["counts"].tolist() == [5, 3, 0] and r["first_t"] == 1.0 and r["last_t"] == 3.0 and r["min_t"] == 2.0
    assert footprint_rows(t5, xa, z5, car, xb, z5, car, 0.75)["counts"].tolist() == [5, 0, 0]          # strictly below: c2 == M2 is not
    assert footprint_rows(t5, xa, z5, car, xb, z5, car, np.nextafter(0.75, 1.0))["counts"].tolist() == [5, 1, 0]
    # a tie goes to the earlier sample: equal c2 at tau = 1 and 3 once tau = 2 is a NaN pose; a NaN sample is never below and hides nothing around it
    wa = z5.copy()
    wa[2] = NAN
    r = footprint_rows(t5, xa, wa, car, xb, z5, car, 0.8)
    assert r["min_c2"] == 0.25 ** 2 + 0.75 ** 2 and r["min_t"] == 1.0 and r["counts"].tolist() == [5, 2, 0] and r["first_t"] == 1.0 and r["last_t"] == 3.0
    r = footprint_rows(t5, np.full((5, 2), NAN), z5, car, xb, z5, car, 9.0)
    assert r["min_c2"] == INF and r["min_t"] == 0.0 and r["counts"].tolist() == [5, 0, 0] and np.isnan(r["first_t"]) and np.isnan(r["last_t"])
    # overlapping samples: c2 = 0, the first of them is the minimum; with a margin of 0 "below" means "overlapping"
    xb = np.stack([0.5 * (t5 - 2.0), np.full(5, 0.25)], axis=1)     # touching in y (0.125 + 0.125) while the spans in x meet: tau = 1, 2 and 3 (0.75 long, 0.5 apart)
    r = footprint_rows(t5, xa, z5, car, xb, z5, car, 0.0)
    assert r["min_c2"] == 0.0 and r["min_t"] == 1.0 and r["counts"].tolist() == [5, 3, 3] and r["first_t"] == 1.0 and r["last_t"] == 3.0
    r = footprint_rows(t5, xa, z5, car, xb, z5, car, 0.3)           # tau = 0 and 4: 0.25 apart in x
    assert r["counts"].tolist() == [5, 5, 3] and r["first_t"] == 0.0 and r["last_t"] == 4.0 and r["min_t"] == 1.0
    assert footprint_rows(t5, xa, z5, car, xb, z5, car, 0.25)["counts"].tolist() == [5, 3, 3]
    # points: a margin of 0 is never below unless they coincide, which counts as touching
    r = footprint_rows(t5, np.ones((5, 2)), z5, pt, np.ones((5, 2)), z5 + 1.0, pt, 0.0)
    assert r["min_c2"] == 0.0 and r["min_t"] == 0.0 and r["counts"].tolist() == [5, 5, 5]
    r = footprint_rows(t5, np.ones((5, 2)), z5, pt, np.ones((5, 2)) + [0.0, 0.5], z5, pt, 0.0)
    assert r["min_c2"] == 0.25 and r["counts"].tolist() == [5, 0, 0]
    assert footprint_rows(t5, np.ones((5, 2)), z5, pt, np.ones((5, 2)) + [0.0, 0.5], z5, pt, 1e-300)["counts"].tolist() == [5, 0, 0]     # M * M rounds to 0
    # an empty window
    r = footprint_rows(np.zeros(0), np.zeros((0, 2)), np.zeros(0), car, np.zeros((0, 2)), np.zeros(0), car, 1.0)
    assert r["min_c2"] == INF and np.isnan(r["min_t"]) and np.isnan(r["first_t"]) and np.isnan(r["last_t"]) and r["counts"].tolist() == [0, 0, 0]
    for bad in (-0.1, NAN, INF):
        with pytest.raises(_lib.UnevenHipError):
            footprint_rows(t5, xa, z5, car, xb, z5, car, bad)
        with pytest.raises(_lib.UnevenHipError):
            footprint_rows(t5, xa, z5, (0.5, bad, 0.1), xb, z5, car, 0.1)


SHAPES = np.array([[0.4, 0.2, 0.15], [0.1, 0.5, 0.05], [0.0, 0.0, 0.0], [0.3, 0.0, 0.25]])


def _reach_yaw(shape, toward):
    """the yaw that points the rectangle's farthest corner along +x (toward = 0) or -x (toward = pi)"""
    f, r, h = shape
    return toward - (np.arctan2(h, f) if f >= r else np.arctan2(h, -r))


def test_a_pair_the_broad_phase_drops_is_never_below():
    """random fleets of 200 boxes: vehicles take positions inside (and on the corners of) their boxes at any yaw; no pair that conflict_candidates drops with
    footprint_radii is below at any sample in the mirror, M = margin_i + margin_j.  Among them pairs whose boxes are the least more than R apart, the rectangles'
    farthest corners pointing at each other from the facing edges: the clearance is then M within the 2^-40 the radii carry."""
    rng = np.random.default_rng(23)
    K = 24
    u = np.concatenate([rng.uniform(size=(K - 4, 2)), [[0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0]]])
    dropped_total, least = 0, INF
    for fleet in range(3):
        n = 200
        lo = rng.uniform(-9.0, 9.0, (n, 2))
        size = rng.uniform(0.0, 2.0, (n, 2)) * (rng.uniform(size=(n, 2)) < 0.8)
        box = np.stack([lo[:, 0], lo[:, 0] + size[:, 0], lo[:, 1], lo[:, 1] + size[:, 1]], axis=1)
        kind = rng.integers(0, len(SHAPES), n)
        margin = rng.uniform(0.0, 0.3, n) * (rng.uniform(size=n) < 0.8)
        rad = footprint_radii(SHAPES[kind], margin)
        yaw = rng.uniform(-7.0, 7.0, (n, K))
        for k in range(0, 60, 2):                                   # neighbours in x whose gap is the smallest above R; the corner samples reach for each other
            R = rad[k] + rad[k + 1]
            box[k + 1, 0] = box[k, 1] + R
            while not box[k + 1, 0] - box[k, 1] > R:                # the smallest xmin the rule drops
                box[k + 1, 0] = np.nextafter(box[k + 1, 0], INF)
            box[k + 1, 1] = box[k + 1, 0] + 1.0
            box[k + 1, 2:] = box[k, 2:]
            yaw[k, -2:] = _reach_yaw(SHAPES[kind[k]], 0.0)         # samples (1, 0) and (1, 1): the edge x = xmax
            yaw[k + 1, -4:-2] = _reach_yaw(SHAPES[kind[k + 1]], np.pi)
        pos = np.stack([box[:, None, 0] + u[None, :, 0] * (box[:, None, 1] - box[:, None, 0]), box[:, None, 2] + u[None, :, 1] * (box[:, None, 3] - box[:, None, 2])], axis=2)
        pos = np.clip(pos, box[:, None, [0, 2]], box[:, None, [1, 3]])
        kept = set(map(tuple, conflict_candidates(box, rad).tolist()))
        ii, jj = np.triu_indices(n, 1)
        drop = np.array([(i, j) not in kept for i, j in zip(ii.tolist(), jj.tolist())])
        ii, jj = ii[drop], jj[drop]
        assert sum(1 for k in range(0, 60, 2) if (k, k + 1) not in kept) == 30 and len(kept) > 100
        dropped_total += ii.size
        for ka in range(len(SHAPES)):
            for kb in range(len(SHAPES)):
                sel = np.nonzero((kind[ii] == ka) & (kind[jj] == kb))[0]
                if sel.size == 0:
                    continue
                i, j = ii[sel], jj[sel]
                M = margin[i] + margin[j]
                # every sample of i against every sample of j would be K * K: sample s of i against samples s and K - 1 - s of j, and the facing pairs
                for other in (np.arange(K), np.arange(K)[::-1], np.r_[np.arange(K - 2), K - 4, K - 3]):
                    c2, over = footprint_clearance2(pos[i].reshape(-1, 2), yaw[i].reshape(-1), SHAPES[ka], pos[j][:, other].reshape(-1, 2), yaw[j][:, other].reshape(-1), SHAPES[kb])
                    c2, over = c2.reshape(-1, K), over.reshape(-1, K)
                    assert not over.any() and not (c2 < (M * M)[:, None]).any(), (fleet, ka, kb)
                    least = min(least, float((np.sqrt(c2) - M[:, None]).min()))
    print("broad phase: %d dropped pairs, the smallest sqrt(c2) - M among their samples: %.3g m" % (dropped_total, least))
    assert dropped_total > 3 * 15000 and 0.0 <= least < 1e-9        # the near pairs do come within the slack, and none crosses it
