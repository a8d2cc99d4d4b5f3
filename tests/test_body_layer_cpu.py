"""CPU tier of the body layer (uph_body_stencil, uph_body_layer_margin, uph_body_layer_*, uph_kino_set_body_layer): the C-ABI and its binding, the header's
text, the host-only stencil against its numpy mirror bit for bit, the properties the kernel's interval form rests on (rows are contiguous, the R box is never
touched), known stencils, the conservative margin's guarantee against footprint_cover on random in-cell poses, the layer mirror body_layer_rows on a hand-made
grid, the refusals that need no device, and the adapter's entry points."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from uneven_planner_amd import _lib, body_layer as BL
from uneven_planner_amd.alm_traj_opt import footprint_check_columns, footprint_cover
from uneven_planner_amd.body_layer import FOOT_OCC_XY, FOOT_OUTSIDE, body_layer_margin, body_layer_rows, body_stencil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = C.POINTER(C.c_int32)
DP = _lib.DP
VP = C.c_void_p
NAN, INF = float("nan"), float("inf")
CAR = (0.45, 0.15, 0.3)
GRIDS = ((0.05, 0.1), (0.1, 0.2), (0.04, 0.05))


def _params(res, yaw_res):
    return dict(xy_resolution=res, yaw_resolution=yaw_res)


def _raw_stencil(shape, margin, res=0.05, yaw_res=0.1):
    """the bare call, return code and R left as they were on a refusal"""
    mp = BL._map_params(_params(res, yaw_res))
    sh = np.ascontiguousarray(shape, dtype=np.float64)
    R, nyaw = C.c_int32(-9), C.c_int32(-9)
    rc = _lib.load().uph_body_stencil(C.byref(mp), sh.ctypes.data_as(DP), float(margin), C.byref(R), C.byref(nyaw), None, None, None)
    return rc, R.value, nyaw.value


def test_symbols_are_exported_with_the_binding_signatures():
    L = _lib.load()
    MP = C.POINTER(_lib.MapParams)
    want = {
        "uph_body_stencil": [MP, DP, C.c_double, I32P, I32P, DP, I32P, I32P],
        "uph_body_layer_margin": [MP, DP, DP],
        "uph_body_layer_create": [VP, DP, C.c_double, C.c_int32, C.POINTER(VP)],
        "uph_body_layer_build": [VP],
        "uph_body_layer_update": [VP, I32P],
        "uph_body_layer_get": [VP, C.c_char_p],
        "uph_body_layer_set": [VP, C.c_char_p],
        "uph_body_layer_info": [VP, DP, DP, I32P, I32P, I32P, I32P],
        "uph_body_layer_kernel_ms": [VP, DP],
        "uph_body_layer_destroy": [VP],
        "uph_kino_set_body_layer": [VP, VP],
    }
    for name, args in want.items():
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
        fn = getattr(L, name)
        assert fn.restype == C.c_int and fn.argtypes == args, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "uneven_hip.h")).read().split())
    for decl in ("int uph_body_stencil(const uph_map_params* mp, const double* shape", "int uph_body_layer_margin(const uph_map_params* mp, const double* shape",
                 "int uph_body_layer_create(uph_map* m, const double* shape", "int uph_body_layer_build(uph_body_layer* l);",
                 "int uph_body_layer_update(uph_body_layer* l, const int32_t rect[4]);", "int uph_body_layer_get(uph_body_layer* l, char* bytes",
                 "int uph_body_layer_set(uph_body_layer* l, const char* bytes);", "int uph_body_layer_info(const uph_body_layer* l,",
                 "int uph_body_layer_kernel_ms(const uph_body_layer* l, double* kernel_ms);", "int uph_body_layer_destroy(uph_body_layer* l);",
                 "int uph_kino_set_body_layer(uph_kino* k, uph_body_layer* layer);", "typedef struct uph_body_layer uph_body_layer;"):
        assert decl in hdr, decl
    assert "#define UPH_BODY_MAX_R 64" in hdr and _lib.UPH_BODY_MAX_R == 64
    # the rule's load-bearing sentences
    for text in ("|qx * c + qy * s| <= hl'", "|qx * (-s) + qy * c| <= w'", "The rule IS the interval per row", "an empty row has lo = 1, hi = 0",
                 "UPH_FOOT_OCC_YAW is refused", "makes every yaw slice equal to occ_r2", "2 r sin(e / 2)", "exactly one write behind",
                 "The start test stays on occ", "R = floor(hypot(max(front, rear) + m, half_width + m) * (1 + 2^-40) / res) + 1"):
        assert text in hdr, text
    import uneven_planner_amd as U
    assert U.BodyLayer is BL.BodyLayer and callable(U.KinoAstar.set_body_layer)
    for meth in ("build", "update", "get", "set", "stencil", "info", "kernel_ms", "close"):
        assert callable(getattr(U.BodyLayer, meth)), meth


def _random_shapes(rng, n, res):
    """shapes and margins up to ~40 columns of reach, some components zero, a few fixed ones first"""
    shape = rng.uniform(0.0, 25.0 * res, (n, 3)) * (rng.uniform(size=(n, 3)) < 0.85)
    margin = rng.uniform(0.0, 6.0 * res, n) * (rng.uniform(size=n) < 0.8)
    shape[:4] = [[0.0, 0.0, 0.0], CAR, [0.12, 0.12, 0.07], [0.9, 0.0, 0.02]]
    margin[:4] = [0.0, 0.062, 0.0, 0.01]
    return shape, margin


@pytest.mark.parametrize("res,yaw_res", GRIDS)
def test_stencil_equals_the_mirror_rows_are_intervals_and_the_box_is_never_touched(res, yaw_res):
    rng = np.random.default_rng(int(res * 1000))
    shape, margin = _random_shapes(rng, 300, res)
    nyaw_want = int(math.ceil((2.0 * math.pi + 5e-2) / yaw_res))
    n_cols = 0
    for sh, mg in zip(shape, margin):
        st = BL.stencil(_params(res, yaw_res), sh, mg)
        R, lo, hi = body_stencil(st["cs"], res, sh, mg)
        assert st["R"] == R and st["nyaw"] == nyaw_want and np.array_equal(st["lo"], lo) and np.array_equal(st["hi"], hi)
        assert st["lo"].dtype == np.int32 and st["lo"].shape == (nyaw_want, 2 * R + 1)
        # the bin poses: one multiply and one add from the yaw origin, the host's cosine
        psi = -(2.0 * math.pi + 5e-2) / 2.0 + (np.arange(nyaw_want) + 0.5) * yaw_res
        assert np.abs(st["cs"][:, 0] - np.cos(psi)).max() < 1e-15 and np.abs(st["cs"][:, 1] - np.sin(psi)).max() < 1e-15
        # per row the interval IS the set of covered dy computed pointwise: no row is non-contiguous
        cov = BL.covered(st["cs"], res, sh, mg, R)
        dy = np.arange(-R, R + 1)
        interval = (dy[None, None, :] >= lo[:, :, None]) & (dy[None, None, :] <= hi[:, :, None])
        assert np.array_equal(cov, interval)
        # no covered offset on the border of the R box
        assert not cov[:, 0, :].any() and not cov[:, -1, :].any() and not cov[:, :, 0].any() and not cov[:, :, -1].any()
        # the cell itself is covered once the rectangle has an interior around the pose (a zero width or a pose on the rear edge leaves (0, 0) to a rounding of
        # o c s - o s c and o (c c + s s): the rule as written, and such a shape at margin 0 is not one a caller builds a layer for)
        if mg > 0.0 or not (sh[0] != sh[1]):
            assert cov[:, R, R].all()
        n_cols += int(cov.sum())
    assert n_cols > 300 * nyaw_want


def test_known_stencils():
    p = _params(0.05, 0.1)
    st = BL.stencil(p, (0.0, 0.0, 0.0), 0.0)
    assert st["R"] == 1 and st["nyaw"] == 64
    assert (st["lo"][:, 1] == 0).all() and (st["hi"][:, 1] == 0).all() and (st["lo"][:, [0, 2]] == 1).all() and (st["hi"][:, [0, 2]] == 0).all()
    # hl' = 0.12, w' = 0.07, o = 0 (tests/test_footprint_check_cpu.py's footprint_cover case): 5 x 3 near psi = 0, 3 x 5 near pi / 2
    st = BL.stencil(p, (0.12, 0.12, 0.07), 0.0)
    psi = -(2.0 * math.pi + 5e-2) / 2.0 + (np.arange(64) + 0.5) * 0.1
    cov = BL.covered(st["cs"], 0.05, (0.12, 0.12, 0.07), 0.0)
    R = st["R"]
    off = lambda iw: {(a - R, b - R) for a, b in zip(*np.nonzero(cov[iw]))}
    i0, i90 = int(np.argmin(np.abs(psi))), int(np.argmin(np.abs(psi - math.pi / 2)))
    assert off(i0) == {(a, b) for a in range(-2, 3) for b in range(-1, 2)}
    assert off(i90) == {(a, b) for a in range(-1, 2) for b in range(-2, 3)}
    # the same rectangle from a smaller shape and a margin
    st_m = BL.stencil(p, (0.07, 0.07, 0.02), 0.05)
    assert st_m["R"] == R and np.array_equal(st_m["lo"][[i0, i90]], st["lo"][[i0, i90]]) and np.array_equal(st_m["hi"][[i0, i90]], st["hi"][[i0, i90]])
    # front != rear shifts the set along the heading: hl = 0.12, o = 0.1 puts the centre two columns ahead
    cov2 = BL.covered(BL.stencil(p, (0.22, 0.02, 0.07), 0.0)["cs"], 0.05, (0.22, 0.02, 0.07), 0.0)
    R2 = (cov2.shape[1] - 1) // 2
    got = {(a - R2, b - R2) for a, b in zip(*np.nonzero(cov2[i0]))}
    assert got == {(2 + a, b) for a in range(-2, 3) for b in range(-1, 2)}
    ipi = int(np.argmin(np.abs(np.abs(psi) - math.pi)))
    got = {(a - R2, b - R2) for a, b in zip(*np.nonzero(cov2[ipi]))}
    assert got == {(-2 + a, b) for a in range(-2, 3) for b in range(-1, 2)}
    # a growing margin never loses an offset
    rng = np.random.default_rng(5)
    for _ in range(20):
        sh = (rng.uniform(0.0, 0.5), rng.uniform(0.0, 0.3), rng.uniform(0.0, 0.3))
        prev = None
        for mg in (0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.21):
            s = BL.stencil(p, sh, mg)
            now = BL.covered(s["cs"], 0.05, sh, mg, 20)
            assert s["R"] <= 20 and (prev is None or not (prev & ~now).any())
            prev = now
    # the car of the issue
    st = BL.stencil(p, CAR, 0.062)
    assert st["R"] == 13
    per_bin = (st["hi"] - st["lo"] + 1).clip(min=0).sum(axis=1)
    assert 200 <= per_bin.min() and per_bin.max() <= 230


def test_margin_equals_its_formula():
    L = _lib.load()
    rng = np.random.default_rng(3)
    for res, yaw_res in GRIDS:
        for _ in range(50):
            sh = rng.uniform(0.0, 1.0, 3)
            got = BL.layer_margin(_params(res, yaw_res), sh)
            assert got == body_layer_margin(res, yaw_res, sh)
            want = (res * math.sqrt(2.0) / 2.0 + 2.0 * float(np.hypot(max(sh[0], sh[1]), sh[2])) * math.sin(yaw_res / 4.0)) * (1.0 + 2.0 ** -40)
            assert got == want
    assert abs(BL.layer_margin(_params(0.05, 0.1), CAR) - 0.0624) < 2e-4
    m = C.c_double(-9.0)
    mp = BL._map_params(_params(0.05, 0.1))
    for bad in ([-0.1, 0.1, 0.1], [0.1, NAN, 0.1], [0.1, 0.1, INF]):
        sh = np.array(bad)
        assert L.uph_body_layer_margin(C.byref(mp), sh.ctypes.data_as(DP), C.byref(m)) == _lib.UPH_ERR_INVALID and m.value == -9.0
    assert L.uph_body_layer_margin(None, np.zeros(3).ctypes.data_as(DP), C.byref(m)) == _lib.UPH_ERR_INVALID


def test_the_conservative_margin_covers_every_pose_inside_the_cell():
    """10 000 random poses inside random cells of a 40 x 30 grid, four shapes: every column footprint_cover(pose, margin 0) covers surely (by more than 1e-9 m)
    lies in the cell's stencil at the conservative margin.  Zero exceptions."""
    res, yaw_res, nx, ny = 0.5, 0.8, 40, 30
    p = _params(res, yaw_res)
    rng = np.random.default_rng(17)
    n = 10000
    origin = np.array([0.0, 0.0, -(2.0 * math.pi + 5e-2) / 2.0])
    for sh in ((0.45, 0.15, 0.3), (0.0, 0.0, 0.0), (2.6, 0.4, 0.2), (0.7, 1.9, 1.1)):
        mg = BL.layer_margin(p, sh)
        st = BL.stencil(p, sh, mg)
        R, nyaw = st["R"], st["nyaw"]
        grid = dict(origin=origin, res=res, yaw_res=yaw_res, nx=nx, ny=ny, nyaw=nyaw, x_off=0, nx_hold=nx)
        cell = np.stack([rng.integers(0, nx, n), rng.integers(0, ny, n), rng.integers(0, nyaw, n)], axis=1)
        u = rng.uniform(0.0, 1.0, (n, 3))
        u[:400] = rng.integers(0, 2, (400, 3)) * (1.0 - 1e-9) + 0.5e-9         # the cell's corners, where the bound is tight
        pose = origin[None, :] + (cell + u) * np.array([res, res, yaw_res])[None, :]
        cv = footprint_cover(pose, pose[:, 2], sh, 0.0, grid)
        assert cv["ok"].all() and np.array_equal(cv["point"], cell[:, :2]) and np.array_equal(cv["iw"], cell[:, 2])
        sure = cv["g"] < -1e-9
        k, c = np.nonzero(sure)
        dx, dy = cv["ix"][k, c] - cell[k, 0], cv["iy"][k, c] - cell[k, 1]
        assert (np.abs(dx) <= R).all() and (np.abs(dy) <= R).all()
        lo, hi = st["lo"][cell[k, 2], dx + R], st["hi"][cell[k, 2], dx + R]
        assert ((dy >= lo) & (dy <= hi)).all()
        assert sh == (0.0, 0.0, 0.0) or sure.sum() > n
        # the pose's own column, which footprint_cover counts whatever the shape: offset (0, 0) is in every bin's stencil
        assert (st["lo"][:, R] <= 0).all() and (st["hi"][:, R] >= 0).all()


def test_layer_rows_on_a_hand_made_grid():
    res, yaw_res, nx, ny = 0.5, 0.8, 40, 30
    p = _params(res, yaw_res)
    sh, mg = (1.2, 0.4, 0.6), 0.1
    st = BL.stencil(p, sh, mg)
    R, nyaw, lo, hi = st["R"], st["nyaw"], st["lo"], st["hi"]
    cov = BL.covered(st["cs"], res, sh, mg, R)
    both = FOOT_OCC_XY | FOOT_OUTSIDE
    empty, full = np.zeros((nx, ny), dtype=np.int8), np.ones((nx, ny), dtype=np.int8)
    # empty occupancy: nothing with XY; with OUTSIDE the band of cells whose stencil leaves the grid
    assert not body_layer_rows(empty, lo, hi, FOOT_OCC_XY).any()
    band = body_layer_rows(empty, lo, hi, FOOT_OUTSIDE)
    want = np.zeros((nx, ny, nyaw), dtype=np.int8)
    for iw in range(nyaw):
        for a, b in zip(*np.nonzero(cov[iw])):
            dx, dy = a - R, b - R
            ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
            want[:, :, iw] |= ((ix + dx < 0) | (ix + dx >= nx) | (iy + dy < 0) | (iy + dy >= ny)).astype(np.int8)
    assert np.array_equal(band, want) and band.any() and not band[R:nx - R, R:ny - R].any()
    assert np.array_equal(body_layer_rows(empty, lo, hi, both), band)
    # full occupancy: everything with XY (the cell itself is covered); OUTSIDE alone ignores it
    assert body_layer_rows(full, lo, hi, FOOT_OCC_XY).all() and body_layer_rows(full, lo, hi, both).all()
    assert np.array_equal(body_layer_rows(full, lo, hi, FOOT_OUTSIDE), band)
    # one column: the stencil reflected through it
    for cx, cy in ((0, 0), (0, ny - 1), (nx - 1, 0), (nx - 1, ny - 1), (nx // 2, ny // 2)):
        occ = empty.copy()
        occ[cx, cy] = 1
        got = body_layer_rows(occ, lo, hi, FOOT_OCC_XY)
        want = np.zeros_like(got)
        for iw in range(nyaw):
            for a, b in zip(*np.nonzero(cov[iw])):
                ix, iy = cx - (a - R), cy - (b - R)
                if 0 <= ix < nx and 0 <= iy < ny:
                    want[ix, iy, iw] = 1
        assert np.array_equal(got, want), (cx, cy)
        assert np.array_equal(body_layer_rows(occ, lo, hi, both), want | band)
    # the all-zero shape: every slice is occ_r2; non-zero bytes other than 1 count as occupied
    rng = np.random.default_rng(4)
    occ = (rng.uniform(size=(nx, ny)) < 0.05).astype(np.int8) * rng.integers(1, 100, (nx, ny)).astype(np.int8)
    z = BL.stencil(p, (0.0, 0.0, 0.0), 0.0)
    got = body_layer_rows(occ, z["lo"], z["hi"], FOOT_OCC_XY)
    assert np.array_equal(got, np.repeat((occ != 0).astype(np.int8)[:, :, None], nyaw, axis=2))
    assert not body_layer_rows(occ, z["lo"], z["hi"], FOOT_OUTSIDE).any()
    # a random layer against the pointwise definition
    got = body_layer_rows(occ, lo, hi, both)
    pad = np.ones((nx + 2 * R, ny + 2 * R), dtype=bool)
    pad[R:R + nx, R:R + ny] = occ != 0
    want = np.zeros_like(got)
    for iw in range(nyaw):
        for a, b in zip(*np.nonzero(cov[iw])):
            want[:, :, iw] |= pad[a:a + nx, b:b + ny].astype(np.int8)
    assert np.array_equal(got, want)


def test_refusals_without_a_device():
    L = _lib.load()
    # the 2^14 bound of uph_footprint_check_columns, from both sides
    assert footprint_check_columns((3.0, 3.0, 0.5), 0.0, 0.05) <= _lib.FOOT_CHECK_MAX_COLUMNS < footprint_check_columns((3.0, 3.0, 1.0), 0.0, 0.05)
    rc, R, _ = _raw_stencil((3.0, 3.0, 0.5), 0.0)
    assert rc == 0 and R == int(math.floor(float(np.hypot(3.0, 0.5)) * (1.0 + 2.0 ** -40) / 0.05)) + 1 <= _lib.UPH_BODY_MAX_R
    rc, R, nyaw = _raw_stencil((3.0, 3.0, 1.0), 0.0)
    assert rc == _lib.UPH_ERR_LIMIT and (R, nyaw) == (-9, -9) and b"2^14" in L.uph_last_error() and b"uph_body_stencil" in L.uph_last_error()
    # a one-sided shape passes the column bound (it is on (front + rear) / 2) and not the radius
    assert footprint_check_columns((6.0, 0.0, 0.0), 0.0, 0.1) <= _lib.FOOT_CHECK_MAX_COLUMNS
    rc, R, _ = _raw_stencil((6.0, 0.0, 0.0), 0.0, res=0.1)
    assert rc == 0 and R == 61
    rc, R, _ = _raw_stencil((12.0, 0.0, 0.0), 0.0, res=0.1)
    assert footprint_check_columns((12.0, 0.0, 0.0), 0.0, 0.1) <= _lib.FOOT_CHECK_MAX_COLUMNS
    assert rc == _lib.UPH_ERR_LIMIT and R == -9 and b"UPH_BODY_MAX_R" in L.uph_last_error()
    for bad in (-1e-9, NAN, INF, -INF):
        for col in range(3):
            s = list(CAR)
            s[col] = bad
            assert _raw_stencil(s, 0.05)[:2] == (_lib.UPH_ERR_INVALID, -9)
        assert _raw_stencil(CAR, bad)[:2] == (_lib.UPH_ERR_INVALID, -9)
    for res in (0.0, -0.05, NAN, INF):
        assert _raw_stencil(CAR, 0.05, res=res)[0] == _lib.UPH_ERR_INVALID
    for yr in (0.0, -0.1, NAN, INF):
        assert _raw_stencil(CAR, 0.05, yaw_res=yr)[0] == _lib.UPH_ERR_INVALID
    sh = np.array(CAR)
    assert L.uph_body_stencil(None, sh.ctypes.data_as(DP), 0.0, None, None, None, None, None) == _lib.UPH_ERR_INVALID
    assert L.uph_body_stencil(C.byref(BL._map_params(None)), None, 0.0, None, None, None, None, None) == _lib.UPH_ERR_INVALID
    # objects: NULL handles are refused before anything else
    h = VP()
    assert L.uph_body_layer_create(None, sh.ctypes.data_as(DP), 0.0, 1, C.byref(h)) == _lib.UPH_ERR_INVALID and not h.value
    assert L.uph_body_layer_build(None) == _lib.UPH_ERR_INVALID
    assert L.uph_body_layer_update(None, (C.c_int32 * 4)(0, 1, 0, 1)) == _lib.UPH_ERR_INVALID
    assert L.uph_body_layer_get(None, None) == _lib.UPH_ERR_INVALID and L.uph_body_layer_set(None, None) == _lib.UPH_ERR_INVALID
    assert L.uph_body_layer_info(None, None, None, None, None, None, None) == _lib.UPH_ERR_INVALID
    ms = C.c_double(-9.0)
    assert L.uph_body_layer_kernel_ms(None, C.byref(ms)) == _lib.UPH_ERR_INVALID and ms.value == -9.0
    assert L.uph_kino_set_body_layer(None, None) == _lib.UPH_ERR_INVALID and b"uph_kino_set_body_layer" in L.uph_last_error()
    assert L.uph_body_layer_destroy(None) == 0


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
int main() {
    uneven_hip::UnevenMapHandle* m = nullptr;
    uneven_hip::KinoAstar* k = nullptr;
    if (m && k) {
        const std::array<double, 3> car{0.45, 0.15, 0.3};
        const double mg = uneven_hip::BodyLayer::conservativeMargin(uph_map_params{2, 10.0, 10.0, 0.2, 0.1, 0.1, 0.05, 0.1, 0.8, 0.05, 9.81}, car);
        uneven_hip::BodyLayer layer(*m, car, mg, UPH_FOOT_OCC_XY | UPH_FOOT_OUTSIDE);
        layer.build();
        layer.update({0, 4, 0, 4});
        layer.updateChanged(uph_map_update_info{});
        std::vector<char> b = layer.get();
        layer.set(b);
        const uneven_hip::BodyLayer::Info i = layer.info();
        k->setBodyLayer(&layer);
        k->setBodyLayer(nullptr);
        return (int)b.size() + i.R + i.dims[2] + i.behind + i.layers + (int)i.margin + (int)i.shape[0] + (int)layer.kernelMs();
    }
    return 0;
}
"""


def test_adapter_offers_the_body_layer(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "a.o")])
