"""CPU tier of the clearance term (include/uneven_hip.h uph_ctx_set_clearance_term / uph_clearance_field, csrc/clearance_dev.hpp): the header and
the bindings, the numpy mirror of the field against its own rule, and the workgroup program instantiated with the term in the CPU emulator
(tests/emu/emu_clearance.cpp) against the mirror and against central differences.  No device is needed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import clearance_emu as CE
from uneven_planner_amd import _lib, clearance as CL, scenes
from uneven_planner_amd.resample import make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the 40 x 30 x 63 grid: sizes that are whole multiples of a resolution with an exact binary form, a yaw resolution that gives 63 bins
RES, YRES, SX, SY = 0.125, 0.101, 5.0, 3.75
DIMS = (40, 30, 63)
GEOM = (np.array([-SX / 2.0, -SY / 2.0, -(2.0 * math.pi + 5e-2) / 2.0]), RES, YRES)
RMAX, D_SAFE, WEIGHT, K = 6, 0.5, 50.0, 16
# the objective's other terms are kept small so that cost(on) - cost(off) is not the difference of two large numbers: no time cost to speak of, no
# scaling trick on the jerk, a small rho
PRM = dict(rho_T=1.0, use_scaling=0.0)
RHO = 1e-3


def _layer():
    """hand-set body bytes: a block beside every test path, a column that is an obstacle in every other yaw slice, one that is an obstacle in a band of slices"""
    body = np.zeros(DIMS, dtype=np.uint8)
    body[6:8, 14:16, :] = 1
    body[18:21, 13:16, :] = 1
    body[30, 5, ::2] = 1
    body[8, 22, 10:40] = 1
    return CL.clearance_rows(body, RMAX)


def _problem(pieces):
    for length in np.arange(0.5, 4.5, 0.01):
        p = make_problem((-2.2, -0.35, 0.1), (-2.2 + length * math.cos(0.1), -0.35 + length * math.sin(0.1), 0.3))
        if p["inner_xy"].shape[1] + 1 == pieces:
            return p
    raise AssertionError(pieces)


@pytest.fixture(scope="module")
def emu(oracle):
    cells = scenes.analytic_cells(size_x=SX, size_y=SY, xy_res=RES, yaw_res=YRES)
    assert scenes.grid_dims(SX, SY, RES, YRES) == DIMS
    mp = oracle.map_params_vec(dict(map_size_x=SX, map_size_y=SY, xy_resolution=RES, yaw_resolution=YRES))
    return CE.ClearanceEmu(cells, mp, oracle.params_vec(PRM), lanes=128), cells


def _x0(oracle, cells, prob):
    og = oracle.OracleGrid(SX, SY, RES, YRES)
    og.set_cells(cells)
    return oracle.OracleALM(og, PRM).setup(prob)


def test_symbols_signatures_and_header_text():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "uneven_hip.h")).read()
    names = ("uph_ctx_set_clearance_term", "uph_ctx_clearance_term", "uph_clearance_field")
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n, nargs in zip(names, (4, 4, 5)):
        assert n in _lib.SYMBOLS and hasattr(L, n) and re.search(r"\bint %s\(" % n, hdr), n
        args = re.search(r"\bint %s\((.*?)\);" % n, flat, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib.SYMBOLS[n][1]) == nargs, n
    for phrase in ("piecewise constant in yaw", "res * sqrt(min(D, rmax^2 + 1))", "u = (x - origin_x) / res - 0.5", "clamped to the grid", "exact gradient of the bilinear patch",
                   "no float-to-int conversion", "g = d_safe - c", "om * g^2", "no multiplier", "d_safe > res * rmax", "rebuild", "64 lanes", "fp32 sample mode",
                   "local frames", "refused while a context names the layer"):
        assert phrase.lower() in hdr.lower(), phrase
    import uneven_planner_amd as U
    assert callable(U.ALMTrajOpt.set_clearance_term) and callable(U.ALMTrajOpt.clearance_term) and callable(U.ClearanceLayer.field)
    assert callable(CL.clearance_field) and callable(CL.clearance_term_rows)
    # null handles
    assert L.uph_ctx_set_clearance_term(None, None, 0.1, 1.0) == _lib.UPH_ERR_INVALID and b"uph_ctx_set_clearance_term" in L.uph_last_error()
    assert L.uph_ctx_clearance_term(None, None, None, None) == _lib.UPH_ERR_INVALID
    assert L.uph_clearance_field(None, 1, None, None, None) == _lib.UPH_ERR_INVALID and b"uph_clearance_field" in L.uph_last_error()


def _centres(ix, iy, iw):
    o, res, yres = GEOM
    return np.stack([o[0] + (ix + 0.5) * res, o[1] + (iy + 0.5) * res, o[2] + (iw + 0.5) * yres], axis=-1)


def test_mirror_values_at_cell_centres_and_continuity():
    D = _layer()
    assert (D == CL.CLEAR_FAR).any() and (D == 0).any()
    ix, iy, iw = np.meshgrid(np.arange(DIMS[0]), np.arange(DIMS[1]), np.arange(0, DIMS[2], 7), indexing="ij")
    c, g = CL.clearance_field(D, GEOM, RMAX, _centres(ix, iy, iw).reshape(-1, 3))
    want = RES * np.sqrt(np.minimum(D[ix, iy, iw].astype(np.int64), RMAX * RMAX + 1).astype(np.float64))
    assert np.array_equal(c.reshape(want.shape), want)           # (RES has an exact binary form: fx = fy = 0 exactly at a centre)
    assert c.max() == RES * math.sqrt(RMAX * RMAX + 1)
    # continuity across the borders of the bilinear patches (the lines through cell centres) and of the cells (half-way): a step of 1e-9 m changes the value by
    # at most the largest slope (one cell value per cell: < sqrt(rmax^2 + 1) here) times the step
    rng = np.random.default_rng(3)
    n = 4000
    p = np.stack([rng.uniform(-SX / 2, SX / 2, n), rng.uniform(-SY / 2, SY / 2, n), rng.uniform(-3.0, 3.0, n)], axis=1)
    onx = GEOM[0][0] + (np.floor((p[:, 0] - GEOM[0][0]) / RES * 2) / 2) * RES          # snapped to centre lines and cell borders alike
    for axis, snapped in ((0, onx), (1, GEOM[0][1] + (np.floor((p[:, 1] - GEOM[0][1]) / RES * 2) / 2) * RES)):
        a, b = p.copy(), p.copy()
        a[:, axis], b[:, axis] = snapped - 1e-9, snapped + 1e-9
        ca, cb = CL.clearance_field(D, GEOM, RMAX, a)[0], CL.clearance_field(D, GEOM, RMAX, b)[0]
        assert np.abs(ca - cb).max() <= 2e-9 * math.sqrt(RMAX * RMAX + 1) * 1.001


def test_mirror_gradient_against_central_differences_inside_patches():
    D = _layer()
    rng = np.random.default_rng(5)
    n = 6000
    # points well inside a patch: fractions in [0.2, 0.8] of the patch between four centres
    i0, j0 = rng.integers(0, DIMS[0] - 1, n), rng.integers(0, DIMS[1] - 1, n)
    x = GEOM[0][0] + (i0 + 0.5 + rng.uniform(0.2, 0.8, n)) * RES
    y = GEOM[0][1] + (j0 + 0.5 + rng.uniform(0.2, 0.8, n)) * RES
    p = np.stack([x, y, rng.uniform(-3.0, 3.0, n)], axis=1)
    c, g = CL.clearance_field(D, GEOM, RMAX, p)
    h = 1e-3 * RES
    scale = np.abs(g).max()
    assert scale > 0.5
    for axis in (0, 1):
        a, b = p.copy(), p.copy()
        a[:, axis] += h
        b[:, axis] -= h
        fd = (CL.clearance_field(D, GEOM, RMAX, a)[0] - CL.clearance_field(D, GEOM, RMAX, b)[0]) / (2 * h)
        # the patch is bilinear: the central difference is exact up to the rounding of values of order 1 divided by 2 h
        assert np.abs(fd - g[:, axis]).max() <= 1e-6 * scale, float(np.abs(fd - g[:, axis]).max() / scale)


def test_mirror_clamps_at_the_borders_and_zeroes_degenerate_poses():
    D = _layer().copy()
    D[0, :, :], D[-1, :, :], D[:, 0, :], D[:, -1, :] = 1, 4, 9, 16           # distinct values along the four borders (the corners take the later ones)
    o = GEOM[0]
    yaw = 0.3
    iw = int(math.floor((yaw - o[2]) / YRES))
    val = lambda d: RES * math.sqrt(min(int(d), RMAX * RMAX + 1))
    y_mid, x_mid = o[1] + 10.5 * RES, o[0] + 10.5 * RES
    for pos, want in (((o[0] - 3.0, y_mid, yaw), val(D[0, 10, iw])), ((o[0] + SX + 3.0, y_mid, yaw), val(D[-1, 10, iw])),
                      ((x_mid, o[1] - 3.0, yaw), val(D[10, 0, iw])), ((x_mid, o[1] + SY + 7.0, yaw), val(D[10, -1, iw])),
                      ((o[0] + 0.2 * RES, y_mid, yaw), val(D[0, 10, iw])), ((o[0] + SX - 0.2 * RES, y_mid, yaw), val(D[-1, 10, iw]))):
        c, g = CL.clearance_field(D, GEOM, RMAX, [pos])
        assert c[0] == want, (pos, c[0], want)
    # outside in x: both x corners are the border row, no x slope
    c, g = CL.clearance_field(D, GEOM, RMAX, [(o[0] - 3.0, y_mid + 0.3 * RES, yaw)])
    assert g[0, 0] == 0.0
    bad = [(float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, float("nan")), (0.0, 0.0, float("-inf")), (1e12, 0.0, 0.0), (0.0, -1e12, 0.0)]
    c, g = CL.clearance_field(D, GEOM, RMAX, bad)
    assert np.array_equal(c, np.zeros(6)) and np.array_equal(g, np.zeros((6, 2)))
    # yaw wraps by whole turns into the same slice
    a = CL.clearance_field(D, GEOM, RMAX, [(0.3, 0.2, 0.5)])
    b = CL.clearance_field(D, GEOM, RMAX, [(0.3, 0.2, 0.5 + 2 * math.pi)])
    assert abs(a[0][0] - b[0][0]) <= 1e-12


def test_emulated_field_is_the_mirror(emu):
    e, _ = emu
    D = _layer()
    rng = np.random.default_rng(9)
    n = 3000
    p = np.stack([rng.uniform(-SX / 2 - 0.5, SX / 2 + 0.5, n), rng.uniform(-SY / 2 - 0.5, SY / 2 + 0.5, n), rng.uniform(-7.0, 7.0, n)], axis=1)
    p[:5] = [(float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, float("nan")), (2e12, 0, 0), (0, 0, 0)]
    c, g = e.field(D, RMAX, p)
    cm, gm = CL.clearance_field(D, GEOM, RMAX, p)
    assert np.array_equal(c, cm) and np.array_equal(g, gm)


@pytest.mark.parametrize("pieces", [3, 7, 8])
def test_emulated_added_cost_is_the_mirrors_sum(oracle, emu, pieces):
    """cost(on) - cost(off) of one evaluation against clearance_term_rows at 1e-12 relative.  At 8 pieces a 128-lane chunk of 7 whole pieces ends inside
    the trajectory (two chunks)."""
    e, cells = emu
    D = _layer()
    prob = _problem(pieces)
    x0 = _x0(oracle, cells, prob)
    off = e.eval(prob, x0, rho=RHO)
    on = e.eval(prob, x0, term=(D, RMAX, D_SAFE, WEIGHT), rho=RHO)
    assert np.array_equal(on["c_xy"], off["c_xy"]) and on["T_xy"] == off["T_xy"]
    rows = CL.clearance_term_rows(D, GEOM, RMAX, D_SAFE, WEIGHT, on["c_xy"], on["c_yaw"], on["T_xy"], on["T_yaw"], K)
    assert rows["below"].sum() >= 10 and not rows["below"].all() and rows["cost"] > 0.1
    added = on["f"] - off["f"]
    print("pieces %d: f off %.6g, added %.15g, mirror %.15g, samples below %d" % (pieces, off["f"], added, rows["cost"], rows["below"].sum()))
    assert abs(off["f"]) < 1e3 * rows["cost"]                  # (the subtraction loses at most three digits)
    assert abs(added - rows["cost"]) <= 1e-12 * rows["cost"], (added, rows["cost"])


def _tau_grad(tau):
    return tau + 1.0 if tau > 0 else (1.0 - tau) / ((0.5 * tau - 1.0) * tau + 1.0) ** 2


@pytest.mark.parametrize("pieces", [7, 8])
def test_emulated_added_gradient_against_central_differences(oracle, emu, pieces):
    """grad(on) - grad(off) with respect to every entry of x (tau, way-points, yaw way-points) against central differences (h = 1e-6) of cost(on) - cost(off).
    The bound is four times the worst relative error the same procedure shows for the term-off objective at the same points and step.

    The time entry.  The term's time part is om g^2 / K per sample -- the reference's quirk Q3 for its own user cost, kept for the term as the issue of the
    term asks -- where the derivative of the cost has om g^2 / T_xy.  A finite-difference test on tau has to allow for it: the entry is
    compared after the known difference, cost * (1 / T_xy - 1 / K) / Nxy * dT/dtau, is added.  For the term-off objective the same quirk is below its
    own error (the user cost is a 1e-7 part of that gradient), so its error is taken as it is.

    Measured: term-off 1.16e-8 (7 pieces) and 1.58e-8 (8 pieces) of the largest entry; the added part 4.5e-10 and 4.8e-10."""
    e, cells = emu
    D = _layer()
    prob = _problem(pieces)
    x0 = _x0(oracle, cells, prob)
    term = (D, RMAX, D_SAFE, WEIGHT)
    off, on = e.eval(prob, x0, rho=RHO), e.eval(prob, x0, term=term, rho=RHO)
    n, h = x0.shape[0], 1e-6
    fd_off, fd_add = np.zeros(n), np.zeros(n)
    for i in range(n):
        xp, xm = x0.copy(), x0.copy()
        xp[i] += h
        xm[i] -= h
        a, b = e.eval(prob, xp, rho=RHO), e.eval(prob, xm, rho=RHO)
        c, d = e.eval(prob, xp, term=term, rho=RHO), e.eval(prob, xm, term=term, rho=RHO)
        fd_off[i] = (a["f"] - b["f"]) / (2 * h)
        fd_add[i] = ((c["f"] - a["f"]) - (d["f"] - b["f"])) / (2 * h)
    e_off = np.abs(off["g"] - fd_off).max() / np.abs(off["g"]).max()
    dg = on["g"] - off["g"]
    rows = CL.clearance_term_rows(D, GEOM, RMAX, D_SAFE, WEIGHT, on["c_xy"], on["c_yaw"], on["T_xy"], on["T_yaw"], K)
    q3 = rows["cost"] * (1.0 / on["T_xy"] - 1.0 / K) / pieces * _tau_grad(x0[0])
    assert abs(q3) > 0.1 * np.abs(dg).max()                    # (the allowance is not a detail here: without it the time entry is off by this much)
    dg[0] += q3
    e_add = np.abs(dg - fd_add).max() / np.abs(dg).max()
    print("pieces %d: relative error of the procedure, term-off %.3g, added part %.3g (largest added entry %.4g, time entry %.4g of which Q3 %.4g)"
          % (pieces, e_off, e_add, np.abs(dg).max(), dg[0], q3))
    assert np.abs(dg[1:]).max() > 1.0 and e_off > 0.0
    assert e_add <= 4.0 * e_off, (e_add, e_off)


def test_emulated_no_sample_below_is_term_off(oracle, emu):
    """a layer set, but no sample within d_safe: every cell far, and a layer whose obstacles all lie further than d_safe from every sample"""
    e, cells = emu
    prob = _problem(8)
    x0 = _x0(oracle, cells, prob)
    off = e.eval(prob, x0, rho=RHO)
    far = np.full(DIMS, CL.CLEAR_FAR, dtype=np.uint16)
    body = np.zeros(DIMS, dtype=np.uint8)
    body[30, 5, ::2] = 1
    body[8, 20, 10:40] = 1
    D = CL.clearance_rows(body, RMAX)
    rows = CL.clearance_term_rows(D, GEOM, RMAX, D_SAFE, WEIGHT, off["c_xy"], off["c_yaw"], off["T_xy"], off["T_yaw"], K)
    assert not rows["below"].any() and D_SAFE < rows["c"].min() < RES * math.sqrt(RMAX * RMAX + 1)       # (near enough to read a distance, not near enough to pay)
    for term in ((far, RMAX, D_SAFE, WEIGHT), (D, RMAX, D_SAFE, WEIGHT)):
        on = e.eval(prob, x0, term=term, rho=RHO)
        assert abs(on["f"] - off["f"]) <= 1e-13 * abs(off["f"])
        assert np.abs(on["g"] - off["g"]).max() <= 1e-13 * np.abs(off["g"]).max()


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
int main() {
    uneven_hip::BodyLayer* b = nullptr;
    uneven_hip::ALMTrajOpt* o = nullptr;
    if (b && o) {
        uneven_hip::ClearanceLayer layer(*b, 20);
        o->setClearanceTerm(&layer, 0.1, 200.0);
        const uneven_hip::ALMTrajOpt::ClearanceTerm t = o->clearanceTerm();
        const uneven_hip::ClearanceLayer::Field f = layer.field({{0.0, 0.0, 0.0}, {1.0, 2.0, 3.0}});
        o->setClearanceTerm(nullptr);
        return (t.layer == layer.handle() ? 1 : 0) + (int)t.d_safe + (int)t.weight + (int)f.value[0] + (int)f.grad[1][1];
    }
    return 0;
}
"""


def test_adapter_offers_the_clearance_term(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "a.o")])
