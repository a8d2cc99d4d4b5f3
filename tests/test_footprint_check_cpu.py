"""CPU tier of the footprint check (uph_footprint_check_columns, uph_footprint_check_batch, uph_footprint_check_kernel_ms): the C-ABI and its binding, the
header's text, the refusals that need no device, the host-only column bound against its mirror and its limit, the adapter's entry point, and the mirrors
footprint_cover / footprint_check_rows -- the rule of include/uneven_hip.h that tests/test_gpu_footprint_check.py holds the device against -- on hand-made
cases with known answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import (FOOT_ALL, FOOT_OCC_XY, FOOT_OCC_YAW, FOOT_OUTSIDE, ALMTrajOpt, TrajFleet, footprint_check_columns,
                                             footprint_check_rows, footprint_cover)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = C.POINTER(C.c_int32)
I64P = C.POINTER(C.c_int64)
DP = _lib.DP
INF = float("inf")
NAN = float("nan")
dp = lambda a: a.ctypes.data_as(DP)
ip = lambda a: a.ctypes.data_as(I32P)
lp = lambda a: a.ctypes.data_as(I64P)
# a 10 m x 10 m grid at 0.05 m with 64 yaw bins of 0.1 rad, as the hill map's
GRID = dict(origin=np.array([-5.0, -5.0, -(2.0 * np.pi + 5e-2) / 2.0]), res=0.05, yaw_res=0.1, nx=200, ny=200, nyaw=64, x_off=0, nx_hold=200)


def test_symbols_are_exported_with_the_binding_signatures():
    L = _lib.load()
    want = {
        "uph_footprint_check_columns": [C.POINTER(_lib.MapParams), C.c_int32, DP, DP, I64P],
        "uph_footprint_check_batch": [C.c_void_p, C.c_int32, I32P, DP, DP, C.c_double, C.c_int32, DP, DP, C.c_int32, DP, DP, I32P, I32P, I32P, I64P],
        "uph_footprint_check_kernel_ms": [C.c_void_p, DP],
    }
    for name, args in want.items():
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
        fn = getattr(L, name)
        assert fn.restype == C.c_int and fn.argtypes == args, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "uneven_hip.h")).read().split())
    assert ("int uph_footprint_check_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t_from, const double* t_to /* NULL: to the end */, double dt, "
            "int32_t with_end, const double* shape /* [n][3] */, const double* margin /* [n], NULL: 0 */, int32_t layers, double* first_t") in hdr
    assert "int uph_footprint_check_columns(const uph_map_params* mp, int32_t n, const double* shape" in hdr
    assert "int uph_footprint_check_kernel_ms(const uph_ctx* c, double* kernel_ms);" in hdr
    for k, v in (("UPH_FOOT_OCC_XY", 1), ("UPH_FOOT_OCC_YAW", 2), ("UPH_FOOT_OUTSIDE", 4), ("UPH_FOOT_ALL", 7)):
        assert "#define %s %d" % (k, v) in hdr and getattr(_lib, k) == v
    assert (FOOT_OCC_XY, FOOT_OCC_YAW, FOOT_OUTSIDE, FOOT_ALL) == (1, 2, 4, 7)
    # the rule's load-bearing sentences: cell centres and how to ask for whole cells, the point's column, the pad, the limit, the fleet
    for text in ("The test is on CELL CENTRES", "adds res * sqrt(2) / 2 to the margin", "The rule is the membership test; the box is the implementation",
                 "No float-to-int conversion of such a value is executed", "exceed 2^14 columns", "uph_footprint_delays_batch, uph_footprint_check_batch, every"):
        assert text in hdr, text
    for cls in (ALMTrajOpt, TrajFleet):
        assert callable(cls.footprint_check) and callable(cls.footprint_check_kernel_ms)


def test_refusals_without_a_device():
    L = _lib.load()
    one, z, sh, mg = np.zeros(1, dtype=np.int32), np.zeros(1), np.array([[0.4, 0.2, 0.15]]), np.full(1, 0.05)
    d = {k: np.full(s, -9.0) for k, s in (("first_t", 1), ("last_t", 1))}
    i = {k: np.full(s, -9, dtype=np.int32) for k, s in (("first_mask", 1), ("first_cell", 2), ("counts", 5))}
    cells = np.full(2, -9, dtype=np.int64)
    assert L.uph_footprint_check_batch(None, 1, ip(one), dp(z), None, 0.01, 1, dp(sh), dp(mg), 7, dp(d["first_t"]), dp(d["last_t"]), ip(i["first_mask"]),
                                       ip(i["first_cell"]), ip(i["counts"]), lp(cells)) == _lib.UPH_ERR_INVALID
    assert b"uph_footprint_check_batch" in L.uph_last_error()
    ms = C.c_double(-9.0)
    assert L.uph_footprint_check_kernel_ms(None, C.byref(ms)) == _lib.UPH_ERR_INVALID and ms.value == -9.0
    assert b"uph_footprint_check_kernel_ms" in L.uph_last_error()
    assert all((v == -9).all() for v in d.values()) and all((v == -9).all() for v in i.values()) and (cells == -9).all()


def _columns(shape, margin, res=0.05, n=None, null=()):
    shape = np.ascontiguousarray(shape, dtype=np.float64).reshape(-1, 3)
    margin = None if margin is None else np.ascontiguousarray(np.broadcast_to(np.asarray(margin, dtype=np.float64), (shape.shape[0],)))
    mp = _lib.MapParams(iter_num=2, map_size_x=10.0, map_size_y=10.0, ellipsoid_x=0.2, ellipsoid_y=0.1, ellipsoid_z=0.1, xy_resolution=res, yaw_resolution=0.1,
                        min_cnormal=0.8, max_rho=0.05, gravity=9.81)
    cols = np.full(max(1, shape.shape[0]), -9, dtype=np.int64)
    arg = lambda name, v: None if name in null else v
    rc = _lib.load().uph_footprint_check_columns(arg("mp", C.byref(mp)), shape.shape[0] if n is None else n, arg("shape", dp(shape)),
                                                 None if margin is None else dp(margin), arg("cols", lp(cols)))
    return rc, cols


def test_columns_equal_the_mirror_and_bound_the_box():
    rng = np.random.default_rng(11)
    shape = rng.uniform(0.0, 2.5, (300, 3)) * (rng.uniform(size=(300, 3)) < 0.85)
    margin = rng.uniform(0.0, 0.5, 300) * (rng.uniform(size=300) < 0.8)
    shape[:3] = [[0.0, 0.0, 0.0], [0.45, 0.15, 0.3], [0.12, 0.12, 0.07]]
    margin[:3] = [0.0, 0.05, 0.0]
    for res in (0.05, 0.25):
        rc, cols = _columns(shape, margin, res)
        want = [footprint_check_columns(s, m, res) for s, m in zip(shape, margin)]
        assert rc == 0 and cols.tolist() == want
        if res == 0.05:
            assert cols[0] == 16 and cols[1] == (int(np.floor(2.0 * np.hypot(0.35, 0.35) * (1.0 + 2.0 ** -40) / 0.05)) + 4) ** 2 == 23 * 23
        # the bound holds: the box the rule's implementation enumerates at any heading has no more columns
        grid = dict(GRID, res=res)
        for q in range(0, 300, 7):
            psi = rng.uniform(-7.0, 7.0, 40)
            pose = np.stack([rng.uniform(-4.0, 4.0, 40), rng.uniform(-4.0, 4.0, 40), psi], axis=1)
            hl, o, w = 0.5 * (shape[q, 0] + shape[q, 1]) + margin[q], 0.5 * (shape[q, 0] - shape[q, 1]), shape[q, 2] + margin[q]
            c, s = np.cos(psi), np.sin(psi)
            Cx, Cy = pose[:, 0] + o * c, pose[:, 1] + o * s
            ex, ey = hl * np.abs(c) + w * np.abs(s), hl * np.abs(s) + w * np.abs(c)
            inv = 1.0 / res
            nbx = (np.floor(((Cx + ex) + 5.0) * inv) + 1.0) - (np.floor(((Cx - ex) + 5.0) * inv) - 1.0) + 1.0
            nby = (np.floor(((Cy + ey) + 5.0) * inv) + 1.0) - (np.floor(((Cy - ey) + 5.0) * inv) - 1.0) + 1.0
            assert (nbx * nby <= cols[q]).all(), (q, res)
            assert grid["res"] == res
    # margin == NULL is a margin of 0
    assert np.array_equal(_columns(shape, None)[1], _columns(shape, 0.0)[1])
    # the limit of uph_footprint_check_batch: 2^14 columns is a side of 128
    assert footprint_check_columns((3.0, 3.0, 0.5), 0.0, 0.05) <= _lib.FOOT_CHECK_MAX_COLUMNS < footprint_check_columns((3.0, 3.0, 1.0), 0.0, 0.05)
    assert _columns([[1e300, 0.0, 0.0]], 0.0)[1][0] == 1 << 62
    L = _lib.load()
    for bad in (-1e-9, NAN, INF, -INF):
        for col in range(3):
            s = shape[:5].copy()
            s[3, col] = bad
            rc, cols = _columns(s, margin[:5])
            assert rc == _lib.UPH_ERR_INVALID and (cols == -9).all() and b"shape" in L.uph_last_error() and b"uph_footprint_check_columns" in L.uph_last_error()
            with pytest.raises(_lib.UnevenHipError):
                footprint_check_columns(s[3], 0.0, 0.05)
        m = margin[:5].copy()
        m[2] = bad
        rc, cols = _columns(shape[:5], m)
        assert rc == _lib.UPH_ERR_INVALID and (cols == -9).all() and b"margin" in L.uph_last_error()
        with pytest.raises(_lib.UnevenHipError):
            footprint_check_columns(shape[2], bad, 0.05)
    rc, cols = _columns([[1e308, 0.0, 1e308]], 1e308)
    assert rc == _lib.UPH_ERR_INVALID and (cols == -9).all() and b"not finite" in L.uph_last_error()
    for null in ("mp", "shape", "cols"):
        rc, cols = _columns(shape[:5], margin[:5], null=(null,))
        assert rc == _lib.UPH_ERR_INVALID and (cols == -9).all()
    for res in (0.0, -0.05, NAN, INF):
        assert _columns(shape[:5], margin[:5], res)[0] == _lib.UPH_ERR_INVALID
    assert _columns(shape[:5], margin[:5], n=-1)[0] == _lib.UPH_ERR_INVALID
    assert L.uph_footprint_check_columns(C.byref(_lib.MapParams(xy_resolution=0.05)), 0, None, None, None) == 0


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
int main() {
    uneven_hip::ALMTrajOpt* o = nullptr;
    if (o) {
        const std::array<double, 3> car{0.45, 0.15, 0.3};
        uneven_hip::ALMTrajOpt::TrajFootprintCheck r = o->footprintCheckSE2TrajBatch({0, 1}, {0.0, 0.5}, {}, {car, car});
        r = o->footprintCheckSE2TrajBatch({0}, {0.0}, {9.0}, {car}, {0.05}, UPH_FOOT_OCC_XY | UPH_FOOT_OUTSIDE, 0.03, false);
        return (r.hits(0) ? (int)r.first_t[0] + (int)r.last_t[0] + r.first_mask[0] + r.first_cell[0][0] + r.first_cell[0][1] + r.counts[4] : 0) + (int)r.cells[1];
    }
    return 0;
}
"""


def test_adapter_offers_the_footprint_check(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "a.o")])


def _covered(cv, k=0):
    on = (cv["g"][k] <= 0.0) | ((cv["ix"][k] == cv["point"][k, 0]) & (cv["iy"][k] == cv["point"][k, 1]))
    return set(zip(cv["ix"][k][on].tolist(), cv["iy"][k][on].tolist()))


def test_cover_on_known_cases():
    # psi = 0, C on the centre of column (100, 100): centres at multiples of 0.05 from it, |dx| <= 0.12 keeps 5, |dy| <= 0.07 keeps 3
    cv = footprint_cover([0.025, 0.025, 0.0], 0.0, (0.12, 0.12, 0.07), 0.0, GRID)
    got = _covered(cv)
    assert got == {(100 + a, 100 + b) for a in range(-2, 3) for b in range(-1, 2)} and cv["point"][0].tolist() == [100, 100] and cv["ok"][0]
    assert cv["iw"][0] == int(np.floor((0.0 - GRID["origin"][2]) / 0.1))
    # psi = pi / 2 swaps the counts
    got = _covered(footprint_cover([0.025, 0.025, np.pi / 2], 0.0, (0.12, 0.12, 0.07), 0.0, GRID))
    assert got == {(100 + a, 100 + b) for a in range(-1, 2) for b in range(-2, 3)}
    # the margin inflates both half extents; front != rear moves the centre along the heading
    got = _covered(footprint_cover([0.025, 0.025, 0.0], 0.0, (0.07, 0.07, 0.02), 0.05, GRID))
    assert got == {(100 + a, 100 + b) for a in range(-2, 3) for b in range(-1, 2)}
    got = _covered(footprint_cover([0.025, 0.025, 0.0], 0.0, (0.22, 0.02, 0.07), 0.0, GRID))     # hl = 0.12, o = 0.1: the centre sits on column 102
    assert got == {(102 + a, 100 + b) for a in range(-2, 3) for b in range(-1, 2)}
    got = _covered(footprint_cover([0.025, 0.025, np.pi], 0.0, (0.22, 0.02, 0.07), 0.0, GRID))
    assert got == {(98 + a, 100 + b) for a in range(-2, 3) for b in range(-1, 2)}
    # an all-zero shape: the point's column alone, wherever the point lies in it, and also where no centre is covered
    rng = np.random.default_rng(2)
    pose = np.stack([rng.uniform(-4.9, 4.9, 200), rng.uniform(-4.9, 4.9, 200), rng.uniform(-7.0, 7.0, 200)], axis=1)
    cv = footprint_cover(pose, 0.0, (0.0, 0.0, 0.0), 0.0, GRID)
    for k in range(200):
        assert _covered(cv, k) == {tuple(np.floor((pose[k, :2] + 5.0) * (1.0 / 0.05)).astype(int).tolist())}
    got = _covered(footprint_cover([0.001, 0.001, 0.3], 0.0, (0.01, 0.01, 0.01), 0.0, GRID))        # no centre within 0.01 m of the point
    assert got == {(100, 100)}
    # growing the margin never loses a column
    for k in range(0, 200, 5):
        sh = (rng.uniform(0.0, 0.5), rng.uniform(0.0, 0.3), rng.uniform(0.0, 0.3))
        prev = set()
        for mg in (0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.21):
            now = _covered(footprint_cover(pose[k], 0.0, sh, mg, GRID))
            assert prev <= now, (k, mg)
            prev = now
    # degenerate poses cover nothing
    bad = np.array([[NAN, 0.0, 0.0], [0.0, INF, 0.0], [0.0, 0.0, NAN], [1e9, 0.0, 0.0], [0.0, -1e9, 0.0], [0.0, 0.0, 0.0]])
    cv = footprint_cover(bad, [0.0, 0.0, 0.0, 0.0, 0.0, NAN], (0.3, 0.3, 0.2), 0.0, GRID)
    assert not cv["ok"].any() and np.isinf(cv["g"]).all() and all(not _covered(cv, k) - {(0, 0)} for k in range(6))
    assert footprint_cover([5e7, 0.0, 0.0], 0.0, (0.3, 0.3, 0.2), 0.0, GRID)["ok"][0]                 # 1e9 columns fit, 2e10 do not


def test_no_column_of_the_outer_ring_of_a_two_column_pad_passes():
    """the enumeration box of the kernel is the hull's box with one column of pad: on 10 000 random poses no column of the ring a second column of pad adds
    is covered, and neither is one of the first ring by more than a rounding -- the box loses nothing"""
    rng = np.random.default_rng(7)
    n = 10000
    pose = np.stack([rng.uniform(-4.0, 4.0, n), rng.uniform(-4.0, 4.0, n), rng.uniform(-7.0, 7.0, n)], axis=1)
    for sh, mg in (((0.45, 0.15, 0.3), 0.05), ((0.0, 0.0, 0.0), 0.0), ((0.5, 0.0, 0.0), 0.0), ((0.13, 0.31, 0.22), 0.017)):
        cv1, cv2 = footprint_cover(pose, 0.0, sh, mg, GRID, pad=1), footprint_cover(pose, 0.0, sh, mg, GRID, pad=2)
        on1, on2 = cv1["g"] <= 0.0, cv2["g"] <= 0.0
        assert np.array_equal(on1.sum(axis=1), on2.sum(axis=1))
        # the ring: columns of the pad = 2 box that the pad = 1 box of the same pose does not hold
        x0, x1 = cv1["ix"].min(axis=1)[:, None], cv1["ix"].max(axis=1)[:, None]
        y0, y1 = cv1["iy"].min(axis=1)[:, None], cv1["iy"].max(axis=1)[:, None]
        ring = (cv2["ix"] < x0) | (cv2["ix"] > x1) | (cv2["iy"] < y0) | (cv2["iy"] > y1)
        assert ring.any(axis=1).all() and not (on2 & ring).any()
        assert cv2["g"][ring].min() > 0.9 * GRID["res"] - 1e-9        # outside by nearly a whole column


def _grid_case():
    """a 40 x 30 grid with 8 yaw bins, a vehicle driving along +x through row iy = 10; hand-placed occupancy"""
    grid = dict(origin=np.array([0.0, 0.0, -3.2]), res=0.5, yaw_res=0.8, nx=40, ny=30, nyaw=8, x_off=0, nx_hold=40)
    occ, occ_r2 = np.zeros((40, 30, 8), dtype=np.int8), np.zeros((40, 30), dtype=np.int8)
    t = np.arange(12) * 0.1
    poses = np.stack([2.25 + 1.0 * np.arange(12), np.full(12, 5.25), np.zeros(12)], axis=1)      # on the centres of columns (4 + 2 k, 10)
    return grid, occ, occ_r2, t, poses


def test_check_rows_on_a_hand_made_grid():
    grid, occ, occ_r2, t, poses = _grid_case()
    iw0 = int(np.floor((0.0 + 3.2) / 0.8))
    car = (0.6, 0.6, 0.6)                                               # covers 3 x 3 columns around the point's
    run = lambda **kw: footprint_check_rows(t, poses, 0.0, kw.pop("shape", car), kw.pop("margin", 0.0), grid, occ, occ_r2, **kw)
    r = run()
    for v in (r["sure"], r["poss"]):
        assert np.isnan(v["first_t"]) and np.isnan(v["last_t"]) and v["first_mask"] == 0 and v["first_cell"].tolist() == [-1, -1]
        assert v["counts"].tolist() == [12, 0, 0, 0, 0] and v["cells"].tolist() == [12 * 9, 0]
    # an XY obstacle beside the path: the point never sees it, the body does at samples 3 and 4 (columns 10 +- 1 and 12 +- 1 hold ix = 11)
    occ_r2[11, 11] = 1
    occ_r2[11, 9] = 1
    occ[13, 9, iw0] = 1                                                 # YAW kind at the heading's bin: samples 4 and 5
    occ[15, 10, (iw0 + 1) % 8] = 1                                      # another bin: never read
    r = run()["sure"]
    assert r["first_t"] == t[3] and r["last_t"] == t[5] and r["first_mask"] == FOOT_OCC_XY and r["first_cell"].tolist() == [11, 9]
    assert r["counts"].tolist() == [12, 3, 2, 2, 0] and r["cells"].tolist() == [108, 2 + 3 + 1]
    assert r["hit"].tolist() == [False] * 3 + [True] * 3 + [False] * 6
    assert run(shape=(0.0, 0.0, 0.0))["sure"]["counts"].tolist() == [12, 0, 0, 0, 0]      # the point alone: what check reads
    assert run(shape=(0.6, 0.6, 0.1))["sure"]["counts"].tolist() == [12, 0, 0, 0, 0]      # a narrow body passes between
    # layers: subsets select the hits, the kind counters stay
    r = run(layers=FOOT_OCC_YAW)["sure"]
    assert r["first_t"] == t[4] and r["last_t"] == t[5] and r["first_mask"] == FOOT_OCC_YAW and r["first_cell"].tolist() == [13, 9]
    assert r["counts"].tolist() == [12, 2, 2, 2, 0] and r["cells"].tolist() == [108, 2]
    r = run(layers=FOOT_OUTSIDE)["sure"]
    assert np.isnan(r["first_t"]) and r["counts"].tolist() == [12, 0, 2, 2, 0]
    r = run(layers=FOOT_OCC_XY | FOOT_OCC_YAW)["sure"]
    assert r["counts"].tolist() == [12, 3, 2, 2, 0]
    # sample 4 is the first when the window starts there: both kinds, the smaller cell wins the tie between (11, 9), (11, 11), (13, 9)
    r = footprint_check_rows(t[4:], poses[4:], 0.0, car, 0.0, grid, occ, occ_r2)["sure"]
    assert r["first_t"] == t[4] and r["first_mask"] == (FOOT_OCC_XY | FOOT_OCC_YAW) and r["first_cell"].tolist() == [11, 9] and r["counts"][0] == 8
    occ_r2[11, 9] = 0
    r = footprint_check_rows(t[4:], poses[4:], 0.0, car, 0.0, grid, occ, occ_r2)["sure"]
    assert r["first_cell"].tolist() == [11, 11]
    # a column that is both XY and YAW is one hit column with both kinds
    occ_r2[13, 9] = 1
    r = footprint_check_rows(t[5:6], poses[5:6], 0.0, car, 0.0, grid, occ, occ_r2)["sure"]
    assert r["first_mask"] == 3 and r["cells"].tolist() == [9, 1] and r["counts"].tolist() == [1, 1, 1, 1, 0]
    # outside: a yaw bin beyond the grid makes every covered column OUTSIDE; a body over the border makes some
    r = footprint_check_rows(t[:2], poses[:2], 3.3, car, 0.0, grid, occ, occ_r2)["sure"]
    assert r["first_mask"] == FOOT_OUTSIDE and r["counts"].tolist() == [2, 2, 0, 0, 2] and r["cells"].tolist() == [18, 18] and r["first_cell"].tolist() == [3, 9]
    edge = np.array([[0.25, 5.25, 0.0]])
    r = footprint_check_rows(t[:1], edge, 0.0, car, 0.0, grid, occ, occ_r2)["sure"]
    assert r["first_mask"] == FOOT_OUTSIDE and r["cells"].tolist() == [9, 3] and r["first_cell"].tolist() == [-1, 9]
    tile = dict(grid, x_off=6, nx_hold=20)                            # a tile holding rows 6 .. 25: the rows before it are outside
    r = footprint_check_rows(t[:3], poses[:3], 0.0, car, 0.0, tile, occ[6:26], occ_r2[6:26])["sure"]
    assert r["counts"].tolist() == [3, 2, 0, 0, 2] and r["cells"].tolist() == [27, 9 + 3] and r["first_cell"].tolist() == [3, 9]
    # an empty window
    r = footprint_check_rows(t[:0], poses[:0], 0.0, car, 0.0, grid, occ, occ_r2)
    for v in (r["sure"], r["poss"]):
        assert np.isnan(v["first_t"]) and np.isnan(v["last_t"]) and v["first_mask"] == 0 and v["first_cell"].tolist() == [-1, -1]
        assert v["counts"].tolist() == [0] * 5 and v["cells"].tolist() == [0, 0]
    # a NaN pose: covers nothing, of kind OUTSIDE, a hit iff layers holds OUTSIDE, without a cell
    bad = poses.copy()
    bad[1, 0] = NAN
    r = footprint_check_rows(t, bad, 0.0, car, 0.0, grid, occ, occ_r2)["sure"]
    assert r["first_t"] == t[1] and r["first_mask"] == FOOT_OUTSIDE and r["first_cell"].tolist() == [-1, -1]
    assert r["counts"].tolist() == [12, 4, 3, 2, 1] and r["cells"][0] == 11 * 9      # (by now (11, 11) and (13, 9) are XY: samples 3, 4, 5)
    r = footprint_check_rows(t, bad, 0.0, car, 0.0, grid, occ, occ_r2, layers=FOOT_OCC_XY)["sure"]
    assert r["first_t"] == t[3] and r["counts"].tolist() == [12, 3, 3, 2, 1]
    yn = np.zeros(12)
    yn[2] = NAN
    assert footprint_check_rows(t, poses, yn, car, 0.0, grid, occ, occ_r2)["sure"]["first_t"] == t[2]
    for layers in (0, 8, -1):
        with pytest.raises(_lib.UnevenHipError):
            run(layers=layers)


def test_check_rows_sure_and_possible_readings():
    """a centre exactly on the rectangle's edge is covered by the rule (<=); with a tolerance it is possibly covered and not surely"""
    grid, occ, occ_r2, t, poses = _grid_case()
    occ_r2[12, 12] = 1                                                  # centre (6.25, 6.25): 1.0 above the path
    sh = (0.1, 0.1, 1.0)                                                # a bar across the heading whose end lies exactly on that centre at sample 4
    r = footprint_check_rows(t, poses, 0.0, sh, 0.0, grid, occ, occ_r2)
    assert r["sure"]["counts"][1] == 1 and r["poss"]["counts"][1] == 1 and r["sure"]["first_t"] == t[4]
    r = footprint_check_rows(t, poses, 0.0, sh, 0.0, grid, occ, occ_r2, tol=1e-9)
    assert r["sure"]["counts"][1] == 0 and r["poss"]["counts"][1] == 1 and np.isnan(r["sure"]["first_t"]) and r["poss"]["first_t"] == t[4]
    assert r["sure"]["cells"][0] == 12 * 3 and r["poss"]["cells"][0] == 12 * 5 and r["poss"]["first_cell"].tolist() == [12, 12]
    assert footprint_check_rows(t, poses, 0.0, (0.1, 0.1, 0.99), 0.0, grid, occ, occ_r2, tol=1e-9)["poss"]["counts"][1] == 0
