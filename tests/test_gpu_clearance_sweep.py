"""The clearance term's evaluation, penalty and solve kernels -- uph_solver_kernel<NT, 1, MODE, false, CLR = true>, MODE 0 / 8 / 2 at 128, 256 and 512 lanes --
against the oracle with the term (oracle/alm.hpp, pinned on the CPU by tests/test_clearance_sweep_cpu.py) over the piece-count sweep (tests/piece_sweep.py):
every Nxy in 1..128, the oversize class included.  Everything goes through the C-ABI; the body bytes are set by hand; layer.get() is the D the oracle receives.
S1 one evaluation, S2 the penalty alone, S3 capped solves, S4 the descriptor, S5 edges inside an evaluation, S6 other geometries.
tools/clearance_sweep_report.py runs this file and writes the worst errors to profiles/clearance_sweep.txt."""
import numpy as np
import pytest

import grid_cases as GC
import piece_sweep as PS
from test_gpu_clearance import POINT
from test_gpu_pieces import AUTO, _check, _ctx, _eval_bar, _upload, _vid
from uneven_planner_amd.alm_traj_opt import FOOT_OCC_XY

pytestmark = pytest.mark.gpu

TERM = (PS.CLR_RMAX, PS.CLR_D_SAFE, PS.CLR_WEIGHT)
SOLVE_TERM = (PS.CLR_RMAX, PS.CLR_D_SAFE, PS.CLR_SOLVE_WEIGHT)
LANES = (128, 256, 512)
VARIANTS = [(128, 0), (256, 0), (512, 0), AUTO]
_SOLVED = {}


def _layer(m, lattice, rmax):
    """(body layer, clearance layer, its values) of hand-set lattice bytes on the map m; the values must be the host mirror's"""
    import uneven_planner_amd as U
    dims = tuple(int(v) for v in m.voxel_num)
    body = U.BodyLayer(m, POINT, 0.0, FOOT_OCC_XY)
    body.set(PS.lattice_body(dims, lattice))
    layer = U.ClearanceLayer(body, rmax)
    D = layer.get()
    want = PS.clearance_layer(dims, lattice, rmax)
    assert np.array_equal(D, want)
    return body, layer, want                     # (the cached array: the oracle's answers are keyed by it)


@pytest.fixture(scope="module")
def dev(analytic_cells):
    import uneven_planner_amd as U
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    return m


@pytest.fixture(scope="module")
def lay(dev):
    body, layer, D = _layer(dev, PS.CLR_LATTICE, PS.CLR_RMAX)
    return dict(body=body, layer=layer, D=D)


def _term_ctx(dev, lay, variant, term, params=None):
    opt = _ctx(dev, variant, params)
    opt.set_clearance_term(lay["layer"], term[1], term[2])
    return opt


def _evaluate(opt, probs, states, variant):
    _upload(opt, probs, variant)
    opt.set_state(lam=[s["lam"] for s in states], mu=[s["mu"] for s in states], scale_cx=[s["scale_cx"] for s in states],
                  scale_fx=np.array([s["scale_fx"] for s in states]), rho=np.array([s["rho"] for s in states]))
    f, gs = opt.eval_batch(opt.x0_packed(probs))
    out = opt.download()
    return [dict(out[i], f=f[i], g=gs[i]) for i in range(len(probs))]


def _pen(d):
    return dict(cost=d["cost"], gdCxy=d["gdCxy"], gdCyaw=d["gdCyaw"], gdTxy_sum=d["gdTxy_sum"], gdTyaw_sum=d["gdTyaw_sum"])


# ---- S1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_s1_single_evaluation_with_the_term(dev, lay, oracle, oracle_grid, variant):
    """S1, MODE 0: f, grad f, hx, gx, c_xy, c_yaw and T of one evaluation with the term, every case of the sweep as one heterogeneous batch, at
    test_gpu_pieces._eval_bar.  The automatic selection (256 lanes for this batch size) is bit for bit the forced 256-lane variant."""
    cases = PS.all_cases()
    for lanes in ([variant[0]] if variant != AUTO else LANES):
        PS.assert_chunk_coverage([n for n, r in cases if r == 2.0], lanes)
    ref = PS.oracle_evals_term(oracle, oracle_grid, cases, lay["D"], TERM)
    probs, states = [PS.sweep_problem(*c) for c in cases], [PS.case_state(*c) for c in cases]
    got = _evaluate(_term_ctx(dev, lay, variant, TERM), probs, states, variant)
    _SOLVED[("s1", variant)] = got
    _check("s1_single_evaluation", variant, cases, [PS.eval_errors(ref[c], g) for c, g in zip(cases, got)], _eval_bar)
    if variant == AUTO:
        assert 256 < len(cases) < 512
        forced = _SOLVED.get(("s1", (256, 0))) or _evaluate(_term_ctx(dev, lay, (256, 0), TERM), probs, states, (256, 0))
        diff = [PS.pieces(p) for p, a, b in zip(probs, got, forced) if not (a["f"] == b["f"] and np.array_equal(a["g"], b["g"]))]
        assert not diff, diff[:8]


# ---- S2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_s2_penalty_alone_with_the_term(dev, lay, oracle, oracle_grid, lanes):
    """S2, MODE 8: uph_penalty_batch(repeat = 2, store_residuals) with the term, ratio 2, every Nxy: cost, gdCxy, gdCyaw, the two gdT sums, hx, gx at 1e-9
    against the oracle's calConstrainCostGrad with the term"""
    variant = (lanes, 0)
    cases = [c for c in PS.all_cases() if c[1] == 2.0]
    assert [c[0] for c in cases] == PS.NXY_ALL
    ref = PS.oracle_evals_term(oracle, oracle_grid, cases, lay["D"], TERM)
    opt = _term_ctx(dev, lay, variant, TERM)
    _evaluate(opt, [PS.sweep_problem(*c) for c in cases], [PS.case_state(*c) for c in cases], variant)
    pen = opt.penalty_batch(repeat=2, store_residuals=True)
    out = opt.download()
    got = [PS.penalty_errors(ref[c], d, o["hx"], o["gx"]) for c, d, o in zip(cases, pen, out)]
    _check("s2_penalty", variant, cases, got, lambda q, nxy: 1e-9)


# ---- S3 ---------------------------------------------------------------------------------------------------------------------------------
def _solve_nxy():
    return [n for n in PS.SOLVE_NXY if n not in PS.CLR_SOLVE_LEFT_OUT]


def _solve(dev, lay, variant, abandon=None):
    key = ("s3", variant, abandon)
    if key not in _SOLVED:
        probs = [PS.sweep_problem(n, 2.0) for n in _solve_nxy()]
        opt = _term_ctx(dev, lay, variant, SOLVE_TERM, params=PS.SOLVE_PARAMS)
        if abandon is not None:
            opt.set_trial_abandon(abandon)
        opt.set_rho(1.0)
        _upload(opt, probs, variant)
        opt.solve()
        first, stats = opt.download(), opt.stats()
        opt.set_rho(1.0)
        second = opt.optimize_batch(probs)
        _SOLVED[key] = (first, second, stats)
    return _SOLVED[key]


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_s3_capped_solves_with_the_term(dev, lay, oracle, oracle_grid, variant):
    """S3, MODE 2: SOLVE_PARAMS, rho = 1, the solve list at ratio 2 with the term: ret, lbfgs_iters and evals equal the oracle's, x and the cost within 1e-5
    (where the oracle's own cost lies on a jump of f -- after a failed line search, measured by piece_sweep.cost_jumps -- within 1e-5 of either side of it), the batch solved again is bit-identical, and the automatic selection (512 lanes
    for 22 problems) is bit for bit the forced 512-lane variant"""
    cases = [(n, 2.0) for n in _solve_nxy()]
    ref = PS.oracle_solves_term(oracle, oracle_grid, cases, lay["D"], SOLVE_TERM)
    first, second, _ = _solve(dev, lay, variant)
    bad = []
    for c, o in zip(cases, first):
        ro, where = ref[c], PS.pieces(PS.sweep_problem(*c))
        if (o["ret"], o["lbfgs_iters"], o["evals"]) != (ro["ret"], ro["lbfgs_iters"], ro["evals"]):
            bad.append((variant[0], variant[1]) + where + ("ret / lbfgs_iters / evals", (o["ret"], o["lbfgs_iters"], o["evals"]), (ro["ret"], ro["lbfgs_iters"], ro["evals"])))
    assert not bad, bad
    jump = PS.cost_jumps(oracle, oracle_grid, cases, lay["D"], SOLVE_TERM)
    got = [dict(x=PS.rel(ref[c]["x"], o["x"]), cost=PS.cost_error(ref[c]["cost"], o["cost"], jump[c])) for c, o in zip(cases, first)]
    raw = {PS.pieces(PS.sweep_problem(*c)): dict(cost_raw=PS.rel1(ref[c]["cost"], o["cost"]), oracle_jump=jump[c]) for c, o in zip(cases, first)}
    PS.record("s3_capped_solves_cost_raw", _vid(variant), raw)
    PS.COST_RAW[("s3_capped_solves", _vid(variant))] = raw
    _check("s3_capped_solves", variant, cases, got, lambda q, nxy: 1e-5)
    again = [PS.pieces(PS.sweep_problem(*c)) for c, a, b in zip(cases, first, second) if not (np.array_equal(a["x"], b["x"]) and a["cost"] == b["cost"] and a["evals"] == b["evals"])]
    assert not again, ("the second solve of the same batch differs", variant, again)
    if variant == AUTO:
        assert len(cases) <= 256
        forced = _solve(dev, lay, (512, 0))[0]
        diff = [PS.pieces(PS.sweep_problem(*c)) for c, a, b in zip(cases, first, forced) if not (np.array_equal(a["x"], b["x"]) and a["cost"] == b["cost"] and a["evals"] == b["evals"])]
        assert not diff, diff


@pytest.mark.parametrize("lanes", LANES)
def test_s3_trial_abandonment_with_the_term(dev, lay, lanes):
    """set_trial_abandon(True) and (False) give the same x, cost and ret at each lane count, with at least one trial abandoned (the added cost is never negative:
    lb_dual stays a bound)"""
    on, _, st_on = _solve(dev, lay, (lanes, 0), True)
    off, _, st_off = _solve(dev, lay, (lanes, 0), False)
    print("S3 abandon, %d lanes: on %s" % (lanes, {k: st_on[k] for k in ("ls_rejected", "ls_guarded", "ls_abandoned", "chunks_skipped", "adjoints_skipped")}))
    assert st_on["ls_abandoned"] >= 1 and st_off["ls_abandoned"] == 0 and st_off["adjoints_skipped"] == 0
    diff = [n for n, a, b in zip(_solve_nxy(), on, off) if not (np.array_equal(a["x"], b["x"]) and a["cost"] == b["cost"] and a["ret"] == b["ret"])]
    assert not diff, (lanes, diff)


# ---- S4 ---------------------------------------------------------------------------------------------------------------------------------
def test_s4_the_descriptor_belongs_to_the_context_and_is_read_at_every_launch(dev, lay, oracle, oracle_grid):
    """S4: two contexts on one map with different layers (another lattice, rmax = 5), d_safe and weight: their asynchronous solves, in flight together, equal
    their blocking solves bit for bit.  On one context two penalty calls with weight w and then 2 w each match the oracle at 1e-9."""
    body2, layer2, D2 = _layer(dev, (5, 13, 3, 241), 5)
    other = dict(body=body2, layer=layer2, D=D2)
    terms = ((lay, SOLVE_TERM), (other, (5, 0.2, 3.0e8)))
    nxys = [3, 9, 17, 33]
    probs = [PS.sweep_problem(n, 2.0) for n in nxys]
    blocking, ctx = [], []
    for L, term in terms:
        opt = _term_ctx(dev, L, (256, 0), term, params=PS.SOLVE_PARAMS)
        opt.set_rho(1.0)
        blocking.append(opt.optimize_batch(probs))
        ctx.append(opt)
    assert any(not np.array_equal(a["x"], b["x"]) for a, b in zip(*blocking))            # (the two terms are different problems)
    for opt in ctx:
        opt.set_rho(1.0)
        opt.upload(probs)
    for opt in ctx:
        opt.solve_async()
    for opt in ctx:
        opt.wait()
    for opt, ref in zip(ctx, blocking):
        for n, a, b in zip(nxys, opt.download(), ref):
            assert np.array_equal(a["x"], b["x"]) and a["cost"] == b["cost"] and a["evals"] == b["evals"], n
    # one context, the weight changed between two launches
    cases = [(n, 2.0) for n in (1, 2, 7, 8, 31, 64, 128)]
    variant = (256, 0)
    opt = _term_ctx(dev, other, variant, (5, 0.2, 3.0e8))
    _evaluate(opt, [PS.sweep_problem(*c) for c in cases], [PS.case_state(*c) for c in cases], variant)
    for k, w in enumerate((3.0e8, 6.0e8)):
        opt.set_clearance_term(layer2, 0.2, w)
        ref = PS.oracle_evals_term(oracle, oracle_grid, cases, D2, (5, 0.2, w))
        pen = opt.penalty_batch(repeat=1, store_residuals=True)
        out = opt.download()
        _check("s4_penalty_weight_%d" % (k + 1), variant, cases, [PS.penalty_errors(ref[c], d, o["hx"], o["gx"]) for c, d, o in zip(cases, pen, out)], lambda q, nxy: 1e-9)
    for o in ctx + [opt]:
        o.set_clearance_term(None)
    layer2.close()
    body2.close()


# ---- S5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", (256, 512))
def test_s5_edges_inside_an_evaluation(dev, lay, oracle, oracle_grid, lanes):
    """S5: test_gpu_edge::test_trajectory_leaving_the_map's problem with the term (samples beyond the border: the field's corner indices clamp on both sides), a
    one-piece and a two-piece problem, against the oracle at the S1 bars"""
    from uneven_planner_amd import resample
    variant = (lanes, 0)
    probs = [resample.make_problem((4.2, 4.2, 0.2), (5.6, 4.8, 0.3))]
    for length in (0.25, 0.45):                   # one piece, two pieces: the first start of a fixed list whose samples feel the term (by the oracle)
        for k in range(40):
            s = (-1.3 + 0.173 * k, 0.7 - 0.091 * k, -0.4 + 0.05 * k)
            p = resample.make_problem(s, (s[0] + length * np.cos(s[2]), s[1] + length * np.sin(s[2]), s[2] + 0.15))
            st = PS.sweep_state(p, 7700 + len(probs))
            if PS.oracle_eval_one(oracle, oracle_grid, p, st, lay["D"], TERM)["f"] > 1.05 * PS.oracle_eval_one(oracle, oracle_grid, p, st)["f"]:
                probs.append(p)
                break
    assert [PS.pieces(p)[0] for p in probs[1:]] == [1, 2]
    states = [PS.sweep_state(p, 7700 + i) for i, p in enumerate(probs)]
    ref = [PS.oracle_eval_one(oracle, oracle_grid, p, st, lay["D"], TERM) for p, st in zip(probs, states)]
    off = [PS.oracle_eval_one(oracle, oracle_grid, p, st) for p, st in zip(probs, states)]
    assert all(r["f"] > 1.05 * o["f"] for r, o in zip(ref, off))                           # (the term is in every one of them)
    # the leaving problem: by the mirror, samples beyond the border -- where the field's corner indices clamp -- lie below d_safe and pay
    from uneven_planner_amd.clearance import clearance_term_rows
    rows = clearance_term_rows(lay["D"], PS.CLR_GEOM, TERM[0], TERM[1], TERM[2], off[0]["c_xy"], off[0]["c_yaw"], off[0]["T_xy"], off[0]["T_yaw"], 16, states[0]["scale_fx"])
    pose = PS.sample_poses(off[0]["c_xy"], off[0]["c_yaw"], off[0]["T_xy"], off[0]["T_yaw"])
    outside = (np.abs(pose[..., 0]) > 5.0) | (np.abs(pose[..., 1]) > 5.0)
    assert (outside & rows["below"]).sum() >= 3, (outside.sum(), rows["below"].sum())
    got = _evaluate(_term_ctx(dev, lay, variant, TERM), probs, states, variant)
    errs, bad = {}, []
    for p, r, g in zip(probs, ref, got):
        e = PS.eval_errors(r, g)
        errs[PS.pieces(p)] = e
        bad += [(lanes, PS.pieces(p), q, v) for q, v in e.items() if not v < _eval_bar(q, PS.pieces(p)[0])]
    print("s5_edges %d: worst" % lanes, PS.record("s5_edges", _vid(variant), errs))
    assert not bad, bad


# ---- S6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", (256, 512))
@pytest.mark.parametrize("grid", ("tall", "fine"))
def test_s6_other_geometries(oracle, grid, lanes):
    """S6: one evaluation and the penalty alone with the term on grid_cases' tall (42 x 76 x 38) and fine (60 x 80 x 127) grids, their own problems and a lattice
    layer of their dimensions, at the S1 and S2 bars: a swapped stride or a bin count of 64 baked in shows up only here"""
    import uneven_planner_amd as U
    variant = (lanes, 0)
    m = U.UnevenMap(GC.map_params(grid))
    m.set_cells(GC.cells(grid))
    GC.check_dims(grid, m.voxel_num)
    lattice, rmax = (3, 5, 2, 61), 6
    body, layer, D = _layer(m, lattice, rmax)
    res = GC.GRIDS[grid]["xy_res"]
    term = (rmax, 4 * res, 1.0e9)
    og = GC.oracle_grid(oracle, grid)
    probs = GC.optimiser_problems(grid)
    states = [GC.state_for(p, 8800 + i) for i, p in enumerate(probs)]
    ref = [PS.oracle_eval_one(oracle, og, p, st, D, term) for p, st in zip(probs, states)]
    off = [PS.oracle_eval_one(oracle, og, p, st) for p, st in zip(probs, states)]
    assert sum(r["f"] > 1.05 * o["f"] for r, o in zip(ref, off)) >= 6
    opt = _ctx(m, variant)
    opt.set_clearance_term(layer, term[1], term[2])
    got = _evaluate(opt, probs, states, variant)
    pen = opt.penalty_batch(repeat=2, store_residuals=True)
    out = opt.download()
    errs, bad = {}, []
    for i, (p, r, g, d, o) in enumerate(zip(probs, ref, got, pen, out)):
        e = PS.eval_errors(r, g)
        bad += [(grid, lanes, i, q, v) for q, v in e.items() if not v < _eval_bar(q, PS.pieces(p)[0])]
        pe = PS.penalty_errors(r, d, o["hx"], o["gx"])
        bad += [(grid, lanes, i, "pen_" + q, v) for q, v in pe.items() if not v < 1e-9]
        e.update({"pen_" + q: v for q, v in pe.items()})
        errs[PS.pieces(p) + (i,)] = e
    print("s6 %s %d: worst" % (grid, lanes), PS.record("s6_geometry_" + grid, _vid(variant), errs))
    opt.set_clearance_term(None)
    layer.close()
    body.close()
    assert not bad, bad
