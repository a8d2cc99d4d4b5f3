"""GPU tier of the clearance term (include/uneven_hip.h uph_ctx_set_clearance_term / uph_clearance_field): the field kernel against the numpy
mirror (G1), the term in the penalty kernel against clearance_term_rows at every lane count (G2), determinism (G3), off means off (G4), every refusal (G5),
the loop check -> refine closed on the disc scene of sections 7t / 7u (G6), the C++ adapter against ctypes (G7)."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_clearance import CAR, GRIDS, POINT, _beside, _flat, _map, _patterns, _tilt_discs
from test_gpu_replan import _hill_map, _queries, _source
from test_gpu_separation import _totals, _valid
from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import FOOT_OCC_XY, footprint_radii
from uneven_planner_amd.clearance import CLEAR_FAR, CLEAR_TO_FREE, clearance_field, clearance_rows, clearance_term_rows, grow_rect, layer_geometry
from uneven_planner_amd.resample import make_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
RMAX = 20
# G6's weight, chosen on the device: the smallest power of ten at which the refined victim leaves D = 0 of the car's layer (the sweep is in the test's docstring)
WEIGHT = 1.0e7


# ---- G1 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
def test_field_on_the_device_against_the_mirror(grid):
    """G1: uph_clearance_field on both small grids with the seven hand-set patterns, 4096 poses: random ones inside and outside the grid, poses on cell edges and
    on the lines through cell centres, all four borders, degenerate poses, far cells.  A handful of fp64 operations on values of order 1 to 50, performed in the
    mirror's order without contraction: 1e-12 relative."""
    import uneven_planner_amd as U
    params, dims = GRIDS[grid]
    m = _flat(_map(params))
    assert tuple(int(v) for v in m.voxel_num) == dims
    geom = layer_geometry(m)
    o, res = geom[0], geom[1]
    sx, sy = dims[0] * res, dims[1] * res
    rng = np.random.default_rng(dims[0])
    n = 4096
    p = np.stack([rng.uniform(o[0] - 0.3, o[0] + sx + 0.3, n), rng.uniform(o[1] - 0.3, o[1] + sy + 0.3, n), rng.uniform(-7.0, 7.0, n)], axis=1)
    k = np.arange(n)
    edge = o[0] + rng.integers(0, 2 * dims[0] + 1, n) * 0.5 * res          # cell edges and centre lines in x ...
    p[k % 8 == 1, 0] = edge[k % 8 == 1]
    edge = o[1] + rng.integers(0, 2 * dims[1] + 1, n) * 0.5 * res          # ... and in y
    p[k % 8 == 2, 1] = edge[k % 8 == 2]
    p[k % 64 == 3, 0], p[k % 64 == 4, 0] = o[0] + 0.1 * res, o[0] + sx - 0.1 * res      # inside the half cell along each border
    p[k % 64 == 5, 1], p[k % 64 == 6, 1] = o[1] + 0.1 * res, o[1] + sy - 0.1 * res
    p[7], p[71], p[135], p[199], p[263] = (np.nan, 0, 0), (0, np.inf, 0), (0, 0, np.nan), (3e12, 0, 0), (0, -3e12, 0.5)
    body = U.BodyLayer(m, POINT, 0.0, FOOT_OCC_XY)
    n_far = n_near = n_zero_grad = 0
    for name, b in _patterns(dims).items():
        body.set(b)
        for rmax in (3, 13):
            layer = U.ClearanceLayer(body, rmax)
            D = layer.get()
            c, g = layer.field(p)
            cm, gm = clearance_field(D, geom, rmax, p)
            assert np.all(np.abs(c - cm) <= 1e-12 * np.abs(cm)) and np.all(np.abs(g - gm) <= 1e-12 * np.abs(gm)), (name, rmax, float(np.abs(c - cm).max()), float(np.abs(g - gm).max()))
            assert c[7] == c[71] == c[135] == c[199] == c[263] == 0.0 and not g[[7, 71, 135, 199, 263]].any()
            n_far += int((c == res * math.sqrt(rmax * rmax + 1)).sum())
            n_near += int(((c > 0) & (c < res * rmax)).sum())
            n_zero_grad += int((~g.any(axis=1)).sum())
            layer.close()
    assert n_far > 0 and n_near > 0 and n_zero_grad > 0
    depth = U.ClearanceLayer(body, 5, CLEAR_TO_FREE)
    with pytest.raises(_lib.UnevenHipError, match="UPH_CLEAR_TO_OCCUPIED"):
        depth.field(p[:4])
    depth.close()
    body.close()


# ---- the disc scene of DESIGN.md 7t / 7u (tests/test_gpu_footprint_check.py C3) ---------------------------------------------------------------------------------
def make_scene():
    """64 hill goals solved, then a disc of 0.1 m tilted 0.2 m to the side of one clean trajectory's mid pose (the victim), the car's conservative body layer
    and its clearance layer at rmax 20"""
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array([j for j in _valid(res) if res[j]["ret"] == 0], dtype=np.int32)
    total = _totals(src)
    before = src.footprint_check(ok, CAR, 0.05)
    clean = np.nonzero((before["counts"][:, 1] == 0) & (src.check(ok, limits=np.full(7, INF))["counts"][:, 2] == 0))[0]
    v = int(clean[0])
    mid = src.traj_states([ok[v]], [0.5 * total[ok[v]]])[0]
    p0 = _beside(mid, 0.2)
    offs, rows = src.rollout(0.01, 1, with_end=True)
    blk = lambda q: rows[int(offs[ok[q]]):int(offs[ok[q] + 1])]
    dist = np.array([np.hypot(*(blk(q)[:, 1:3] - p0).T).min() for q in range(len(ok))])
    _tilt_discs(m, [p0], 0.1)
    after = src.footprint_check(ok, CAR, 0.05)
    assert after["counts"][v, 1] > 0
    car = U.BodyLayer(m, CAR)
    layer = U.ClearanceLayer(car, RMAX)
    return dict(m=m, ka=ka, src=src, res=res, ok=ok, total=total, v=v, p0=p0, dist=dist, first_t=float(after["first_t"][v]), car=car, layer=layer, D=layer.get(),
                geom=layer_geometry(m))


@pytest.fixture(scope="module")
def scene():
    return make_scene()


def _near_problems(scene):
    """problems of 3, 8 and more than 23 pieces whose straight initial path passes 0.27 m beside the disc, and two of 3 and 8 pieces at least 2.5 m away from it;
    all of them further than 1 m from the border, which the car's layer marks as well (odd coordinates: no sample on a patch border)"""
    p0 = scene["p0"]
    out = []
    for shift, wanted in ((0.27, (3, 8, 24)), (2.5, (3, 8))):
        for pieces in wanted:
            length = {3: 0.77, 8: 2.23, 24: 7.07}[pieces]
            found = None
            for ang in np.arange(-3.05, 3.1, 0.173):
                a = np.array([math.cos(ang), math.sin(ang)])
                for side in (1.0, -1.0):
                    q = p0 + side * shift * np.array([-a[1], a[0]])
                    for t1 in np.linspace(0.31, length - 0.31, 9):
                        s, g = q - t1 * a, q + (length - t1) * a
                        if np.abs(np.concatenate([s, g])).max() > 3.9 or (shift > 1.0 and min(np.hypot(*(s - p0)), np.hypot(*(g - p0))) < shift):
                            continue
                        if shift > 1.0:         # ... and from whatever else the map holds: the field along the straight path, with room to spare
                            line = np.linspace(0.0, 1.0, 200)[:, None] * (g - s)[None, :] + s[None, :]
                            if clearance_field(scene["D"], scene["geom"], RMAX, np.column_stack([line, np.full(200, ang)]))[0].min() < 0.6:
                                continue
                        pr = make_problem((s[0], s[1], ang), (g[0], g[1], ang))
                        n = pr["inner_xy"].shape[1] + 1
                        if n == pieces or (pieces == 24 and n > 23):
                            found = pr
                            break
                    if found:
                        break
                if found:
                    break
            assert found is not None, (pieces, shift)
            out.append(found)
    return out


def _penalty(scene, lanes, probs, term):
    """the resident trajectory of one evaluation at x0, then uph_penalty_batch without and with the term; (off, on, download)"""
    import uneven_planner_amd as U
    opt = U.ALMTrajOpt(scene["m"])
    opt.set_rho(1.0)
    opt.set_lanes(lanes)
    opt.upload(probs)
    opt.eval_batch(opt.x0_packed(probs))
    dl = opt.download(full=False)
    off = opt.penalty_batch(store_residuals=False)
    opt.set_clearance_term(scene["layer"], *term)
    on = opt.penalty_batch(store_residuals=False)
    on2 = opt.penalty_batch(store_residuals=False)
    opt.set_clearance_term(None)
    return off, on, on2, dl


# ---- G2, G3 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [128, 256, 512])
def test_penalty_on_minus_off_is_the_mirrors_rows(scene, lanes):
    """G2 and G3: the differences of cost, gdCxy and the time gradients of uph_penalty_batch with and without the term against clearance_term_rows, at 1e-9 of each
    array's largest magnitude (the tolerance the penalty kernel is held to against the oracle); the same launch twice; the batch permuted."""
    probs = _near_problems(scene)
    res = scene["m"].xy_resolution
    term = (6 * res, 2.0e4)
    off, on, on2, dl = _penalty(scene, lanes, probs, term)
    pieces = [p["inner_xy"].shape[1] + 1 for p in probs]
    assert pieces[0] == 3 and pieces[1] == 8 and pieces[2] > 23
    n_below = []
    for b, pr in enumerate(probs):
        rows = clearance_term_rows(scene["D"], scene["geom"], RMAX, term[0], term[1], dl[b]["c_xy"], dl[b]["c_yaw"], dl[b]["T_xy"], dl[b]["T_yaw"], 16, dl[b]["scale_fx"])
        n_below.append(int(rows["below"].sum()))
        d_cost, d_gc, d_gt = on[b]["cost"] - off[b]["cost"], on[b]["gdCxy"] - off[b]["gdCxy"], on[b]["gdTxy_sum"] - off[b]["gdTxy_sum"]
        e = (abs(d_cost - rows["cost"]) / abs(on[b]["cost"]), np.abs(d_gc - rows["gdCxy"]).max() / np.abs(on[b]["gdCxy"]).max(),
             abs(d_gt - rows["gdT"]) / max(abs(on[b]["gdTxy_sum"]), abs(on[b]["gdTyaw_sum"])))
        print("G2 lanes %d, %d pieces: %d samples below, added cost %.6g of %.6g, errors %.2e %.2e %.2e" % (lanes, pieces[b], n_below[-1], rows["cost"], on[b]["cost"], *e))
        assert max(e) <= 1e-9, (b, e)
        assert np.array_equal(on[b]["gdCyaw"], off[b]["gdCyaw"]) and on[b]["gdTyaw_sum"] == off[b]["gdTyaw_sum"]          # no yaw gradient
        if n_below[-1] == 0:
            assert d_cost == 0.0 and not d_gc.any() and d_gt == 0.0
        else:
            assert rows["cost"] > 1e-6 * abs(on[b]["cost"]) and np.abs(rows["gdCxy"]).max() > 1e-6 * np.abs(on[b]["gdCxy"]).max()
        for k in ("cost", "gdCxy", "gdCyaw", "gdTxy_sum", "gdTyaw_sum"):
            assert np.array_equal(on[b][k], on2[b][k]), k                                                                 # G3: the same launch twice
    assert min(n_below[:3]) > 0 and max(n_below[3:]) == 0, n_below
    perm = [4, 2, 0, 1, 3]
    _, pon, _, _ = _penalty(scene, lanes, [probs[i] for i in perm], term)
    for j, i in enumerate(perm):
        for k in ("cost", "gdCxy", "gdCyaw", "gdTxy_sum", "gdTyaw_sum"):
            assert np.array_equal(pon[j][k], on[i][k]), (k, i)                                                            # G3: the batch permuted


# ---- G4 -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(scene):
    """G4: a context whose term was set and then switched off solves bit for bit as one that never had a term; weight 0 evaluates within 1e-13 of off."""
    import uneven_planner_amd as U
    probs = _near_problems(scene)[:3]
    never = U.ALMTrajOpt(scene["m"])
    never.set_rho(1.0)
    a = never.optimize_batch(probs)
    had = U.ALMTrajOpt(scene["m"])
    had.set_rho(1.0)
    had.set_clearance_term(scene["layer"], 0.1, 1.0e4)
    assert had.clearance_term() == (scene["layer"], 0.1, 1.0e4)
    had.upload(probs)
    had.eval_batch(had.x0_packed(probs))
    had.set_clearance_term(None)
    assert had.clearance_term() == (None, 0.0, 0.0)
    b = had.optimize_batch(probs)
    for ra, rb in zip(a, b):
        for k in ("x", "c_xy", "c_yaw", "cost", "ret", "evals", "lam", "mu", "hx", "gx"):
            assert np.array_equal(ra[k], rb[k]), k
    zero = U.ALMTrajOpt(scene["m"])
    zero.set_rho(1.0)
    zero.set_clearance_term(scene["layer"], 0.3, 0.0)
    c = zero.optimize_batch(probs)
    for ra, rc in zip(a, c):
        dev = (abs(rc["cost"] - ra["cost"]) / abs(ra["cost"]), np.abs(rc["x"] - ra["x"]).max() / np.abs(ra["x"]).max())
        print("G4 weight 0: ret %d / %d, cost and way-points differ by %.2e, %.2e" % (ra["ret"], rc["ret"], *dev))
        assert rc["ret"] == ra["ret"] and max(dev) <= 1e-13, dev


# ---- G5 -----------------------------------------------------------------------------------------------------------------------------------------------------
def _refused(fn, text):
    with pytest.raises(_lib.UnevenHipError, match=text):
        fn()


def test_every_refusal(scene):
    """G5: refused with UPH_ERR_INVALID and a message, nothing launched, resident data untouched; the layer's lifetime; a stale layer; the chain of updates"""
    import uneven_planner_amd as U
    import map_update_cases as MU
    m, layer, res = _hill_map(), None, scene["m"].xy_resolution
    car = U.BodyLayer(m, CAR)
    layer = U.ClearanceLayer(car, RMAX)
    probs = _near_problems(scene)[:2]
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    # the values and the layer, when the term is set
    depth = U.ClearanceLayer(car, 5, CLEAR_TO_FREE)
    _refused(lambda: opt.set_clearance_term(depth, 0.1, 1.0), "UPH_CLEAR_TO_OCCUPIED")
    depth.close()
    for d_safe, weight, text in ((0.0, 1.0, "d_safe must be positive"), (-0.1, 1.0, "d_safe must be positive"), (0.1, -1.0, "weight must not be negative"),
                                 (float("nan"), 1.0, "finite"), (0.1, float("inf"), "finite"), (res * RMAX * 1.001, 1.0, "never be penalised")):
        _refused(lambda: opt.set_clearance_term(layer, d_safe, weight), text)
    _refused(lambda: opt.set_clearance_term(scene["layer"], 0.1, 1.0), "another map")
    assert opt.clearance_term() == (None, 0.0, 0.0)
    opt.set_clearance_term(layer, res * RMAX, 1.0)                # (the largest d_safe is accepted)
    # the layer cannot be destroyed while the context names it
    _refused(layer.close, "still names the layer")
    opt.set_clearance_term(None)
    # what depends on the batch and the context's switches: at the launch, and nothing is launched
    base = opt.optimize_batch(probs)
    x_res = [r["x"].copy() for r in opt.download(full=False)]

    def untouched():
        for r, x in zip(opt.download(full=False), x_res):
            assert np.array_equal(r["x"], x)

    opt.set_clearance_term(layer, 0.1, 1.0e4)
    opt.set_lanes(64)
    opt.upload(probs)
    for call in (opt.solve, lambda: opt.eval_batch(opt.x0_packed(probs)), lambda: opt.penalty_batch()):
        _refused(call, "not for 64")
    opt.set_lanes(0)
    opt.set_clearance_term(None)
    assert all(np.array_equal(r["x"], b["x"]) for r, b in zip(opt.optimize_batch(probs), base))         # (and the context works as before)
    opt.set_clearance_term(layer, 0.1, 1.0e4)
    opt.set_sample_precision(32)
    _refused(opt.solve, "fp32 sample mode")
    untouched()
    opt.set_sample_precision(64)
    n = [s["n"] for s in opt._sizes]
    mem = int(opt.mem_size)
    opt.set_clearance_term(None)
    opt.set_lbfgs_state([dict(x=x, g=np.zeros(k), d=np.zeros(k), pf=np.zeros(1), lm_ys=np.ones(mem), lm_s=np.zeros((mem, k)), lm_y=np.zeros((mem, k)), step=1.0, fx=0.0,
                              k=1, end=0, bound=0) for x, k in zip(x_res, n)])
    opt.set_clearance_term(layer, 0.1, 1.0e4)
    _refused(lambda: opt.lbfgs_resume(1), "resume hook")
    untouched()
    # a batch with per-trajectory local frames: a flat strip that reaches 40 m from its origin
    strip = _flat(_map(dict(map_size_x=80.0, map_size_y=4.0, xy_resolution=0.25)))
    sbody = U.BodyLayer(strip, POINT, 0.0, FOOT_OCC_XY)
    slayer = U.ClearanceLayer(sbody, 4)
    sopt = U.ALMTrajOpt(strip)
    sopt.set_rho(1.0)
    sopt.set_clearance_term(slayer, 0.5, 1.0)
    sopt.upload([make_problem((35.0, -0.5, 0.1), (37.0, 0.5, 0.2))])
    _refused(sopt.solve, "local frames")
    sopt.set_clearance_term(None)
    sopt.solve()
    # a stale layer: the map changes, the body layer follows, the clearance layer is behind ("rebuild"); then the chain, and the next solve reads the new field
    opt.upload(probs)
    info = m.update(MU.BOX, MU.scan(mound=0.6, sigma=0.07))
    _refused(opt.solve, "rebuild")                               # the body layer is behind the map
    car.update(info["changed"])
    _refused(opt.solve, "rebuild")                               # the clearance layer is behind its body layer
    _refused(lambda: U.ALMTrajOpt(m).set_clearance_term(layer, 0.1, 1.0), "rebuild")
    nx, ny = int(m.voxel_num[0]), int(m.voxel_num[1])
    old = layer.get()
    layer.update(grow_rect((nx, ny), info["changed"], car.info()["R"]))
    new = layer.get()
    assert layer.info()["fresh"] and not np.array_equal(old, new)
    # a problem across the rewritten rect: the penalty with the term reads the new values (the mirror with the old ones disagrees)
    x0, x1, y0, y1 = grow_rect((nx, ny), info["changed"], car.info()["R"])
    cx, cy = m.map_origin[0] + 0.5 * (x0 + x1) * res, m.map_origin[1] + 0.5 * (y0 + y1) * res
    pr = make_problem((cx - 0.613, cy - 0.291, 0.4), (cx + 0.587, cy + 0.317, 0.5))
    opt.set_clearance_term(None)
    opt.upload([pr])
    opt.eval_batch(opt.x0_packed([pr]))
    dl = opt.download(full=False)[0]
    off = opt.penalty_batch(store_residuals=False)[0]
    opt.set_clearance_term(layer, 0.5, 1.0e3)
    on = opt.penalty_batch(store_residuals=False)[0]
    rows = [clearance_term_rows(D, layer_geometry(m), RMAX, 0.5, 1.0e3, dl["c_xy"], dl["c_yaw"], dl["T_xy"], dl["T_yaw"], 16, dl["scale_fx"]) for D in (new, old)]
    added = on["cost"] - off["cost"]
    assert rows[0]["cost"] > 0 and abs(added - rows[0]["cost"]) <= 1e-9 * abs(on["cost"]) and abs(rows[1]["cost"] - rows[0]["cost"]) > 1e-6 * abs(on["cost"])
    opt.set_clearance_term(None)
    layer.close()                                                # accepted once no context names it


# ---- G6 -----------------------------------------------------------------------------------------------------------------------------------------------------
def loop_figures(scene, weight, d_safe=None, term_layer=None):
    """the victim refined from 0.5 s before first_t, together with the trajectory farthest from the disc refined from 0.3 s, without and with the term: per
    solve the results and what clearance() and footprint_check() read back"""
    import uneven_planner_amd as U
    src, ok, v, layer, m = scene["src"], scene["ok"], scene["v"], scene["layer"], scene["m"]
    term_layer = layer if term_layer is None else term_layer
    term_D = scene["D"] if term_layer is layer else term_layer.get()
    d_safe = 2 * m.xy_resolution if d_safe is None else d_safe
    far = int(np.argmax(scene["dist"]))
    tr, ts = [ok[v], ok[far]], [max(scene["first_t"] - 0.5, 0.0), 0.3]
    out = {}
    for tag, term in (("off", None), ("on", (d_safe, weight))):
        dst = U.ALMTrajOpt(m)
        dst.set_rho(1.0)
        if term:
            dst.set_clearance_term(term_layer, *term)
        r = dst.refine(src, tr, ts)
        assert all(q["status"] == 0 for q in r)
        ids = [q["traj_of"] for q in r]
        cl = dst.clearance(layer, ids, below2=1)
        fc = dst.footprint_check(ids, CAR, 0.0)
        rows = [clearance_term_rows(term_D, scene["geom"], term_layer.rmax, d_safe, 1.0, q["c_xy"], q["c_yaw"], q["T_xy"], q["T_yaw"], 16) for q in r]
        out[tag] = dict(res=r, min_d2=cl["min_d2"].copy(), zero=cl["counts"][:, 1].copy(), samples=cl["counts"][:, 0].copy(), hits=fc["counts"][:, 1].copy(),
                        below=[int(q["below"].sum()) for q in rows])
    return out


def test_the_loop_closes(scene):
    """G6: the disc scene of sections 7t / 7u.  The term reads the clearance of the POINT body layer -- the distance to the obstacle itself -- and d_safe stands for the
    body: 12 cells = 0.6 m, the car's circumscribed radius hypot(0.45, 0.3) = 0.54 m and a cell, rounded up to cells (within res * rmax = 1 m); weight 1e7.  Both solves
    are read back with the clearance of the CAR's conservative layer and with footprint_check.  Inequalities against the solve without the term, not thresholds.

    Measured (one MI355X).  Without the term the refined victim has min_d2 0, 181 of 1007 samples with D = 0 and 152 footprint hits at margin 0 (ret 0, cost 2.3348).
    With it: min_d2 2, 0 of 1232 samples with D = 0, 0 footprint hits (ret 2, cost 3.05856): it reaches zero.  The sweep, same scene (samples with D = 0 / hits):
    d_safe 0.45 m, weight 1e6: 184 / 140, 1e7: 58 / 9 (ret 0, min_d2 still 0);  d_safe 0.6 m, 1e5: 180 / 151, 1e6: 143 / 41, 1e7: 0 / 0.
    What does NOT work, and why the term's layer is the point layer: with the car's own layer (d_safe two cells up to 1 m, weight 1e5 up to 1e9) the victim never leaves
    D = 0 -- it passes 0.2 m beside the disc, deep inside the plateau D = 0 of the dilated layer, where the field and so its gradient are 0; only a sample within a cell
    of the rim feels a slope.  The far trajectory of the same batch has no sample below d_safe and keeps its way-points (difference 0)."""
    import uneven_planner_amd as U
    m = scene["m"]
    point = U.BodyLayer(m, POINT, 0.0)
    room = U.ClearanceLayer(point, RMAX)
    f = loop_figures(scene, WEIGHT, 12 * m.xy_resolution, room)
    off, on = f["off"], f["on"]
    for tag in ("off", "on"):
        print("G6 %s: victim ret %d cost %.6g, min_d2 %d, samples with D = 0: %d of %d, footprint hits at margin 0: %d; far trajectory ret %d, quadrature samples below d_safe %d"
              % (tag, f[tag]["res"][0]["ret"], f[tag]["res"][0]["cost"], f[tag]["min_d2"][0], f[tag]["zero"][0], f[tag]["samples"][0], f[tag]["hits"][0],
                 f[tag]["res"][1]["ret"], f[tag]["below"][1]))
    for q in on["res"]:
        assert np.isfinite(q["cost"]) and q["ret"] in (0, 1, 2), (q["ret"], q["cost"])
    assert off["zero"][0] > 0                                    # (the parent's behaviour: the refined victim touches the disc)
    assert on["min_d2"][0] > off["min_d2"][0]
    assert on["zero"][0] < off["zero"][0]
    assert on["hits"][0] <= off["hits"][0]
    # the trajectory far from every disc: no sample below d_safe with or without the term, and the same way-points
    assert on["below"][1] == 0 and off["below"][1] == 0
    dx = np.abs(on["res"][1]["x"] - off["res"][1]["x"]).max()
    print("G6 far trajectory: way-points differ by %.3g" % dx)
    assert dx <= 1e-9


# ---- G7 -----------------------------------------------------------------------------------------------------------------------------------------------------
CPP = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
#include <cstdio>
using namespace uneven_hip;
int main(int argc, char** argv) {
    // in: {ncell, B, n}, cells, B x {start, goal}, n poses; out: field values and gradients, then per goal {status, ret, jerk_cost, total_time}, then the term read back
    FILE* f = std::fopen(argv[1], "rb");
    long long hdr[3];
    if (!f || fread(hdr, 8, 3, f) != 3) return 2;
    std::vector<double> cells((size_t)hdr[0] * 4), sg((size_t)hdr[1] * 6);
    std::vector<std::array<double, 3>> pos((size_t)hdr[2]);
    if (fread(cells.data(), 8, cells.size(), f) != cells.size() || fread(sg.data(), 8, sg.size(), f) != sg.size() || fread(pos.data(), 24, pos.size(), f) != pos.size()) return 2;
    std::fclose(f);
    uph_map_params mp = {2, 10.0, 10.0, 0.2, 0.1, 0.1, 0.05, 0.1, 0.8, 0.05, 9.81};
    UnevenMapHandle map(mp, 0);
    map.setCells(cells.data());
    KinoAstar kino;
    kino.setEnvironment(&map);
    const std::array<double, 3> car{0.45, 0.15, 0.3};
    BodyLayer body(map, car, BodyLayer::conservativeMargin(mp, car));
    ClearanceLayer layer(body, 20);
    FILE* o = std::fopen(argv[2], "wb");
    const ClearanceLayer::Field fld = layer.field(pos);
    fwrite(fld.value.data(), 8, fld.value.size(), o);
    fwrite(fld.grad.data(), 16, fld.grad.size(), o);
    {
        ALMTrajOpt opt;
        opt.setEnvironment(&map);
        opt.setClearanceTerm(&layer, 0.1, 1.0e5);
        std::vector<std::array<double, 3>> starts((size_t)hdr[1]), goals((size_t)hdr[1]);
        for (long long b = 0; b < hdr[1]; b++) for (int k = 0; k < 3; k++) { starts[b][k] = sg[6 * b + k]; goals[b][k] = sg[6 * b + 3 + k]; }
        uph_manager_params mgr{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5};
        ALMTrajOpt::GoalPlan p = opt.planSE2TrajBatch(kino, starts, goals, mgr);
        for (long long b = 0; b < hdr[1]; b++) {
            const bool has = p.traj_of[b] >= 0;
            double h[4] = {(double)p.status[b], has ? (double)p.ret[b] : -1.0, has ? p.jerk_cost[b] : 0.0, has ? p.total_time[b] : 0.0};
            fwrite(h, 8, 4, o);
        }
        const ALMTrajOpt::ClearanceTerm t = opt.clearanceTerm();
        bool refused = false;
        try { opt.setClearanceTerm(&layer, -1.0, 1.0); } catch (const std::runtime_error&) { refused = true; }
        opt.setClearanceTerm(nullptr);
        double tail[5] = {t.layer == layer.handle() ? 1.0 : 0.0, t.d_safe, t.weight, refused ? 1.0 : 0.0, opt.clearanceTerm().layer == nullptr ? 1.0 : 0.0};
        fwrite(tail, 8, 5, o);
    }
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_matches_ctypes(tmp_path, analytic_cells):
    """G7: ClearanceLayer::field and ALMTrajOpt::setClearanceTerm from a compiled C++ consumer (-Wall -Werror) against the ctypes binding, bit for bit"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    rng = np.random.default_rng(31)
    cells = np.array(analytic_cells, dtype=np.float64).reshape(200, 200, -1, 4)
    xs = (np.arange(200) + 0.5) * 0.05 - 5.0
    near = np.zeros((200, 200), dtype=bool)
    for p in rng.uniform(-4.5, 4.5, (40, 2)):
        near |= np.hypot(xs[:, None] - p[0], xs[None, :] - p[1]) < 0.12
    cells[near, :, 2], cells[near, :, 3] = 0.8, 0.0
    cells = np.ascontiguousarray(cells.reshape(-1, 4))
    m = U.UnevenMap()
    m.set_cells(cells)
    ka = U.KinoAstar(m)
    S, G = scenes.random_queries(6, seed0=9900)
    B = S.shape[0]
    pos = np.stack([rng.uniform(-5.2, 5.2, 500), rng.uniform(-5.2, 5.2, 500), rng.uniform(-7, 7, 500)], axis=1)
    car = U.BodyLayer(m, CAR)
    layer = U.ClearanceLayer(car, 20)
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    opt.set_clearance_term(layer, 0.1, 1.0e5)
    plan = opt.plan_goals(ka, S, G)
    src_ = tmp_path / "term.cpp"
    src_.write_text(CPP)
    exe = str(tmp_path / "term")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src_), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3q", cells.shape[0], B, pos.shape[0]))
        f.write(cells.tobytes())
        f.write(np.ascontiguousarray(np.concatenate([S, G], axis=1), dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(pos).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.frombuffer(open(fout, "rb").read(), dtype=np.float64)
    n = pos.shape[0]
    c, g = layer.field(pos)
    assert np.array_equal(raw[:n], c) and np.array_equal(raw[n:3 * n].reshape(n, 2), g) and (c < 0.05 * math.sqrt(401)).any()
    rows = raw[3 * n:3 * n + 4 * B].reshape(B, 4)
    solved = 0
    for b in range(B):
        assert rows[b, 0] == plan[b]["status"]
        if plan[b]["status"] == 0:
            assert rows[b, 1] == plan[b]["ret"] and rows[b, 2] == plan[b]["jerk_cost"], (b, rows[b], plan[b]["ret"], plan[b]["jerk_cost"])
            solved += 1
    assert solved >= 3
    assert raw[3 * n + 4 * B:].tolist() == [1.0, 0.1, 1.0e5, 1.0, 1.0]
