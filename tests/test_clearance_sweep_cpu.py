"""CPU tier of the clearance term over the piece-count sweep (tests/piece_sweep.py).  The oracle's optional clearance term pinned against
the two references that were written independently of it (the numpy mirror clearance_term_rows and oracle.minco_grad); the conditions that make the sweep's
layer and weight a test of the term itself; the workgroup program instantiated WITH the term in the CPU emulator (tests/emu/emu_clearance.cpp) against the
oracle, for one evaluation at every piece count and for the capped solves; the statement order of the 512-lane device kernels (ClearLoadsLate) on the CPU;
and which solve cases are fit to test.  The device runs the same references in tests/test_gpu_clearance_sweep.py."""
import numpy as np
import pytest

import clearance_emu as CE
import piece_sweep as PS

EMU_LANES = (64, 128, 256)
TERM = (PS.CLR_RMAX, PS.CLR_D_SAFE, PS.CLR_WEIGHT)
SOLVE_TERM = (PS.CLR_RMAX, PS.CLR_D_SAFE, PS.CLR_SOLVE_WEIGHT)
EPS = 2.0 ** -53


def _cases():
    """ratio 2 at every Nxy, then the ragged ratio 1.7 at every Nxy: the 256 cases of the generator conditions"""
    return [c for c in PS.all_cases() if c[1] == 2.0] + [c for c in PS.all_cases() if c[1] == 1.7]


def _eval_cases():
    """ratio 2 at every Nxy and ratio 1.7 at the solve list: what the emulator evaluates"""
    return [c for c in PS.all_cases() if c[1] == 2.0] + [(n, 1.7) for n in PS.SOLVE_NXY]


def _tau_grad(tau):
    return tau + 1.0 if tau > 0 else (1.0 - tau) / ((0.5 * tau - 1.0) * tau + 1.0) ** 2


def _bound(added, total):
    """1e-12 of the largest added entry, and the rounding of the two totals that cancel: 8 * 2^-53 of the largest total"""
    return 1e-12 * float(np.abs(added).max()) + 8.0 * EPS * float(np.abs(total).max())


def test_no_term_set_is_the_oracle_as_it_was(oracle, oracle_grid):
    """a term set and cleared again leaves an object that evaluates and solves bit for bit like one that never had a term (the golden vectors and
    test_oracle_cpu hold the plain oracle itself)"""
    D = PS.clearance_layer()
    for c in ((3, 2.0), (17, 1.7)):
        p, st = PS.sweep_problem(*c), PS.case_state(*c)
        out = []
        for had in (False, True):
            a = oracle.OracleALM(oracle_grid)
            x0 = a.setup(p)
            if had:
                a.set_clearance_term(D, *TERM)
                a.set_clearance_term(None)
            a.set_state(lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], scale_fx=st["scale_fx"])
            a.set_rho(st["rho"])
            out.append(a.eval(x0)[:2] + a.constrain(x0))
        for u, v in zip(*out):
            assert np.array_equal(u, v)
    a, b = oracle.OracleALM(oracle_grid, PS.SOLVE_PARAMS), oracle.OracleALM(oracle_grid, PS.SOLVE_PARAMS)
    b.set_clearance_term(D, *SOLVE_TERM)
    b.set_clearance_term(None)
    ra, rb = a.optimize(PS.sweep_problem(9, 2.0)), b.optimize(PS.sweep_problem(9, 2.0))
    assert np.array_equal(ra["x"], rb["x"]) and ra["cost"] == rb["cost"] and ra["evals"] == rb["evals"]


def test_oracle_term_is_the_mirrors_rows(oracle, oracle_grid):
    """The oracle with the term minus the oracle without it, against clearance_term_rows at the oracle's own coefficients, on all 256 cases of ratios 2 and
    1.7: the cost of one evaluation; gdCxy and the sum of gdTxy of calConstrainCostGrad (the yaw arrays do not change by a bit: no yaw gradient); and the
    gradient, against oracle.minco_grad applied to the rows, followed by the time map sum gdT / Nxy * dT/dtau.  Each difference within
    1e-12 max|added| + 8 * 2^-53 max|total|."""
    cases = _cases()
    D = PS.clearance_layer()
    off, on = PS.oracle_evals(oracle, oracle_grid, cases), PS.oracle_evals_term(oracle, oracle_grid, cases, D, TERM)
    rows = PS.term_rows(oracle, oracle_grid, cases, D, TERM, PS.CLR_GEOM)
    worst = dict(cost=0.0, gdCxy=0.0, gdT=0.0, grad=0.0)
    bad = []
    for c in cases:
        p, a, b, r = PS.sweep_problem(*c), off[c], on[c], rows[c]["rows"]
        nxy = c[0]
        assert np.array_equal(a["c_xy"], b["c_xy"]) and np.array_equal(a["c_yaw"], b["c_yaw"]) and a["T_xy"] == b["T_xy"]
        assert np.array_equal(a["hx"], b["hx"]) and np.array_equal(a["gx"], b["gx"])                       # no residual
        assert np.array_equal(a["gdCyaw"], b["gdCyaw"]) and np.array_equal(a["gdTyaw"], b["gdTyaw"])       # no yaw gradient
        q = {}
        q["cost"] = abs((b["f"] - a["f"]) - r["cost"]) / _bound(r["cost"], b["f"])
        assert abs((b["pen_cost"] - a["pen_cost"]) - r["cost"]) <= _bound(r["cost"], b["pen_cost"])
        q["gdCxy"] = np.abs((b["gdCxy"] - a["gdCxy"]) - r["gdCxy"]).max() / _bound(r["gdCxy"], b["gdCxy"])
        # the sum of the added time gradients: the totals that cancel are the entries of gdTxy
        q["gdT"] = abs((b["gdTxy"] - a["gdTxy"]).sum() - r["gdT"]) / (1e-12 * abs(r["gdT"]) + 8.0 * EPS * nxy * np.abs(b["gdTxy"]).max())
        T = np.full(nxy, a["T_xy"])
        gP, gT = oracle.minco_grad(nxy, 2, p["inner_xy"], T, p["init_xy"], p["end_xy"], r["gdCxy"], np.zeros(nxy))
        want = np.zeros_like(a["g"])
        want[1:1 + 2 * (nxy - 1)] = gP.T.ravel()
        want[0] = (gT.sum() + r["gdT"]) / nxy * _tau_grad(a["x0"][0])
        q["grad"] = np.abs((b["g"] - a["g"]) - want).max() / _bound(want, b["g"])
        assert np.array_equal(b["g"][1 + 2 * (nxy - 1):], a["g"][1 + 2 * (nxy - 1):])                      # the yaw way-points' gradient: not a bit
        for k, v in q.items():
            worst[k] = max(worst[k], float(v))
            if not v <= 1.0:
                bad.append((c, k, float(v)))
    print("oracle term against the mirror, worst error in units of the bound:", worst)
    assert not bad, bad[:8]


def test_generator_conditions(oracle, oracle_grid):
    """what makes the 1e-9 bars on the totals bind the term itself, and what keeps two correct implementations on the same side of every kink -- from the
    oracle and the mirror alone, on all 256 cases of ratios 2 and 1.7"""
    cases = _cases()
    assert len(cases) == 256
    body = PS.lattice_body()
    assert any(not np.array_equal(body[:, :, 0], body[:, :, k]) for k in (4, 8, 32))                       # the bytes differ between yaw slices
    D = PS.clearance_layer()
    assert D.shape == PS.CLR_DIMS and (D == 0).any() and D.max() <= 65535
    off = PS.oracle_evals(oracle, oracle_grid, cases)
    rows = PS.term_rows(oracle, oracle_grid, cases, D, TERM, PS.CLR_GEOM)
    o, res, yres = PS.CLR_GEOM
    # The yaw of a sample is the sweep's curve's, which no lattice moves: the tangent of the curve turns round 1e-7 rad from the edge between slices 16 and 17.
    # The edges that count are those across which the layer differs -- between two slices with the same values no implementation can land on a wrong side.
    # The lattice is laid so that the edges the curve's yaw lingers at (17 and 46) lie inside a group of four equal slices.
    differs = np.array([True] + [not np.array_equal(D[:, :, k - 1], D[:, :, k]) for k in range(1, PS.CLR_DIMS[2])] + [True])
    assert differs.sum() == 2 + PS.CLR_DIMS[2] // 4 - 1 and not differs[17] and not differs[46]
    fig = dict(share=[], cost=[], gd=[], border=[], slice=[], any_edge=[], g=[])
    near_edges = set()                             # the slice edges some sample lies within 1e-6 rad of
    for c in cases:
        r, pose = rows[c]["rows"], rows[c]["poses"].reshape(-1, 3)
        fig["share"].append(r["below"].mean())
        fig["cost"].append(r["cost"] / abs(off[c]["f"]))
        fig["gd"].append(np.abs(r["gdCxy"]).max() / np.abs(off[c]["gdCxy"]).max())
        u = np.concatenate([(pose[:, 0] - o[0]) / res - 0.5, (pose[:, 1] - o[1]) / res - 0.5])
        fig["border"].append(np.abs(u - np.round(u)).min())                                                  # in cells, to a line through cell centres
        w = (pose[:, 2] - o[2]) / yres
        k = np.round(w).astype(np.int64)
        dist = np.abs(w - k) * yres                                                                          # in rad, to the nearest slice edge
        fig["any_edge"].append(dist.min())
        near_edges |= set(int(v) for v in k[dist < 1e-6])
        fig["slice"].append(np.where(differs[np.clip(k, 0, PS.CLR_DIMS[2])], dist, np.inf).min())
        fig["g"].append(np.abs(PS.CLR_D_SAFE - r["c"]).min())
    print("share of samples below d_safe %.3f .. %.3f; added cost / |f(off)| >= %.3g; added / plain gdCxy >= %.3g; nearest patch border %.3g cell, nearest slice edge across which the "
          "layer differs %.3g rad (any edge: %.3g rad), smallest |g| %.3g m" % (min(fig["share"]), max(fig["share"]), min(fig["cost"]), min(fig["gd"]), min(fig["border"]),
                                                                                   min(fig["slice"]), min(fig["any_edge"]), min(fig["g"])))
    assert min(fig["share"]) >= 0.1 and max(fig["share"]) <= 0.9
    assert min(fig["cost"]) >= 0.1
    assert min(fig["gd"]) >= 0.1
    assert min(fig["border"]) >= 1e-6
    assert min(fig["slice"]) >= 1e-6
    assert near_edges <= {17, 46}, near_edges      # a near-edge sample anywhere else is new: look at it
    assert min(fig["g"]) >= 1e-9


def _emu(oracle, analytic_cells, lanes, params=None, late=False):
    return CE.ClearanceEmu(analytic_cells, oracle.map_params_vec(), oracle.params_vec(params), lanes=lanes, late=late)


@pytest.mark.parametrize("lanes", EMU_LANES)
def test_emu_single_evaluation_with_the_term(oracle, oracle_grid, analytic_cells, lanes):
    """f, grad f, hx, gx and the coefficients of one evaluation WITH the term against the oracle with the term: ratio 2 at every Nxy and ratio 1.7 at the solve
    list, random duals, rho = 3, scale_fx = 0.37, at test_pieces_cpu's bar of 1e-10"""
    cases = _eval_cases()
    PS.assert_chunk_coverage([n for n, r in cases if r == 2.0], lanes)
    D = PS.clearance_layer()
    ref = PS.oracle_evals_term(oracle, oracle_grid, cases, D, TERM)
    emu = _emu(oracle, analytic_cells, lanes)
    bad, errs = [], {}
    for c in cases:
        p, st = PS.sweep_problem(*c), PS.case_state(*c)
        r = emu.run_term(0, p, ref[c]["x0"], (D,) + TERM, lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], rho=st["rho"], scale_fx=st["scale_fx"])
        e = PS.eval_errors(ref[c], r)
        errs[PS.pieces(p) + (c[1],)] = e
        bad += [(lanes, PS.pieces(p), q, v) for q, v in e.items() if not v < 1e-10]
    print("emulator with the term, %d lanes: worst" % lanes, PS.record("cpu_term_single_evaluation", lanes, errs))
    assert not bad, bad[:8]


def _fit_nxy():
    return [n for n in PS.SOLVE_NXY if n not in PS.CLR_SOLVE_LEFT_OUT]


@pytest.mark.parametrize("lanes", EMU_LANES)
def test_emu_capped_solves_with_the_term(oracle, oracle_grid, analytic_cells, lanes):
    """Solver<HostWG, double, true> in the solve mode: SOLVE_PARAMS, rho 1, the solve list at ratio 2: return code, iteration and evaluation counts equal the
    oracle's with the term, x and cost within test_emu_capped_solves' 1e-7 in every case.  After a failed line search the oracle's returned cost is f at the last
    rejected trial, which lies on a jump of f between two yaw slices; piece_sweep.cost_jumps measures that jump with the oracle alone (8 of the 22 cases,
    2.7 to 6.3 % of the cost) and the cost may lie on either side of it (piece_sweep.cost_error) -- within 1e-7 of one of the two values."""
    cases = [(n, 2.0) for n in _fit_nxy()]
    D = PS.clearance_layer()
    ref, ev = PS.oracle_solves_term(oracle, oracle_grid, cases, D, SOLVE_TERM), PS.oracle_evals(oracle, oracle_grid, cases)
    emu = _emu(oracle, analytic_cells, lanes, PS.SOLVE_PARAMS)
    jump = PS.cost_jumps(oracle, oracle_grid, cases, D, SOLVE_TERM)
    bad, errs, raw = [], {}, {}
    for c in cases:
        p, ro = PS.sweep_problem(*c), ref[c]
        r = emu.run_term(2, p, ev[c]["x0"], (D,) + SOLVE_TERM)
        if (r["ret"], r["lbfgs_iters"], r["evals"]) != (ro["ret"], ro["lbfgs_iters"], ro["evals"]):
            bad.append((lanes, PS.pieces(p), "counters", (r["ret"], r["lbfgs_iters"], r["evals"]), (ro["ret"], ro["lbfgs_iters"], ro["evals"])))
        e = dict(x=PS.rel(ro["x"], r["x"]), cost=PS.cost_error(ro["cost"], r["f"], jump[c]))
        errs[PS.pieces(p)] = e
        bad += [(lanes, PS.pieces(p), q, v) for q, v in e.items() if not v < 1e-7]
        raw[PS.pieces(p)] = dict(cost_raw=PS.rel1(ro["cost"], r["f"]), oracle_jump=jump[c])
    PS.record("cpu_term_capped_solves_cost_raw", lanes, raw)
    PS.COST_RAW[("cpu_term_capped_solves", str(lanes))] = raw
    print("emulator capped solves with the term, %d lanes: worst" % lanes, PS.record("cpu_term_capped_solves", lanes, errs))
    assert not bad, bad[:8]


def test_late_loads_give_the_same_bits(oracle, oracle_grid, analytic_cells):
    """The 512-lane device kernels issue the field's loads behind the penalties and take the geometry from the solver's grid argument (ClearLoadsLate).  The
    emulator built with that order evaluates f and grad f bit for bit as the early build does, at Nxy 1, 7, 8 and 31: the field is a function of the pose alone."""
    D = PS.clearance_layer()
    cases = [(n, 2.0) for n in (1, 7, 8, 31)]
    ev = PS.oracle_evals(oracle, oracle_grid, cases)
    early, late = _emu(oracle, analytic_cells, 128), _emu(oracle, analytic_cells, 128, late=True)
    assert early.L.emu_clear_loads_late() == 0 and late.L.emu_clear_loads_late() == 1
    for c in cases:
        p, st = PS.sweep_problem(*c), PS.case_state(*c)
        kw = dict(lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], rho=st["rho"], scale_fx=st["scale_fx"])
        a, b = early.run_term(0, p, ev[c]["x0"], (D,) + TERM, **kw), late.run_term(0, p, ev[c]["x0"], (D,) + TERM, **kw)
        off = early.eval(p, ev[c]["x0"], **kw)
        assert a["f"] == b["f"] and np.array_equal(a["g"], b["g"]), c
        assert a["f"] > 1.1 * off["f"]                              # (and the term is in both)


def test_solve_cases_fit_to_test(oracle, oracle_grid, analytic_cells):
    """Each solve case solved by the oracle four times: with and without the term, in the default build and the -DORACLE_EIGEN_REDUX=1 build.  With the term the
    two builds agree in ret, lbfgs_iters and evals and their x differ by no more than ten times what they show without the term (or 1e-7); a case that fails is
    left out of the solve tests on both tiers (piece_sweep.CLR_SOLVE_LEFT_OUT): at most 2 of the 22, never both members of a pair 16|17, 32|33, 64|65.  The
    solve with the term moves x by more than 1e-3 relative at every Nxy >= 2: 100 times the device's bar.

    Measured at weight 1e9: all 22 cases fit; the builds' x differ by at most 3.1e-10 with the term (Nxy 33; 6.8e-11 without) and the term moves x by 0.025
    (Nxy 3) to 0.13 (Nxy 26).  The builds' returned costs differ by 3.1 to 6.3 % at Nxy 8, 9, 16, 17, 27 and 44: each time by
    the jump cost_jumps measures there (Nxy 18 and 64 have a jump as well, and both builds on one side of it)."""
    fit = PS.solve_fitness(oracle, oracle_grid, analytic_cells, PS.clearance_layer(), SOLVE_TERM)
    for n, r in fit.items():
        print("Nxy %3d: counters agree on / off %s / %s, builds' x apart on %.2e off %.2e, term moves x by %.3g%s" % (n, r["counters_on"], r["counters_off"], r["dx_on"],
                                                                                                                    r["dx_off"], r["moved"], "" if r["fit"] else "  LEFT OUT"))
    PS.MEASURED[("cpu_term_two_builds", "default/eigen")] = {k: max((float(r[k]), (n,)) for n, r in fit.items()) for k in ("dx_on", "dx_off", "dcost_on", "dcost_off")}
    # the two builds' costs part only where the oracle's own cost lies on a measured jump, and then by that jump; nowhere else, and never without the term
    for n, r in fit.items():
        assert min(r["dcost_on"], abs(r["dcost_on"] - r["cost_jump"])) <= max(10.0 * r["dcost_off"], 1e-7), (n, r)
    assert sum(r["cost_jump"] == 0.0 for r in fit.values()) >= 12 and all(r["cost_jump"] == 0.0 or r["cost_jump"] > 1e-3 for r in fit.values())
    off_jump = PS.cost_jumps(oracle, oracle_grid, [(n, 2.0) for n in fit], PS.clearance_layer(), None)
    assert not any(off_jump.values())
    left = tuple(n for n, r in fit.items() if not r["fit"])
    assert left == tuple(PS.CLR_SOLVE_LEFT_OUT), left
    assert len(left) <= 2 and not any(a in left and b in left for a, b in ((16, 17), (32, 33), (64, 65)))
    assert all(r["moved"] > 1e-3 for n, r in fit.items() if n >= 2), {n: r["moved"] for n, r in fit.items()}
