"""The wave-uniform chains of an evaluation formed aside the knot solve, host path: the emulator runs
Solver::generate's aside lambda through the default asideKnotSolve (a plain loop before the solve), reads the published LDS words where the
device reads them, and has the sample-time tables filled in generate() instead of expand().  Every entry that reaches the moved code -- one
evaluation at x0 (with the residual refresh behind it), initScaling (its explicit refill after adjoint), a residual refresh FOLLOWED by an
evaluation (a solve of two passes of one iteration), the capped solve -- is held to the oracle at the bars tests/test_pieces_cpu.py applies to
the same quantities, at the piece counts where the tables and the solve degenerate (Nxy = 1: no interior knot; Nxy + 1 below and above the
K + 1 in-piece times of the shared loop) for int_K = 16 and 8; a second run must be bit-identical."""
import numpy as np
import pytest

import emu_bridge as E
import piece_sweep as PS

LANES = (64, 128, 256)
NXYS = (1, 2, 3, 7, 8, 43)
CASES = [(n, r) for r in (1.0, 2.0) for n in NXYS]
REFRESH_PARAMS = dict(inner_max_iter=1.0, max_iter=1.0)       # pass 1: x0 + one search, refresh, dual update; pass 2 starts with an evaluation
ARRAYS = ("x", "g", "hx", "gx", "lam", "mu", "scale_cx", "c_xy", "c_yaw")
SCALARS = ("f", "jerk_cost", "T_xy", "T_yaw", "rho", "scale_fx", "ret", "alm_iters", "lbfgs_iters", "evals", "last_lbfgs_ret")


def _params(int_K, extra=None):
    p = dict(extra or {})
    if int_K != 16:
        p["int_K"] = float(int_K)
    return p or None


def _same(a, b, what):
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    for k in SCALARS:
        assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (what, k, a[k], b[k])


def _oracle_scalings(O, og, int_K):
    def make(case):
        a = O.OracleALM(og, _params(int_K))
        a.init_scaling(a.setup(PS.sweep_problem(*case)))
        s = a.get_state()
        return dict(scale_fx=s["scale_fx"], scale_cx=s["scale_cx"])
    return PS._fill("aside_scaling", int(int_K), CASES, make)


def _oracle_solves(O, og, int_K, name, params):
    def make(case):
        return O.OracleALM(og, _params(int_K, params)).optimize(PS.sweep_problem(*case))
    return PS._fill("aside_solve_" + name, int(int_K), CASES, make)


def test_cases_reach_both_orders_of_the_shared_table_loop():
    """the aside loop runs max(Nxy, K) + 1 steps for both tables: piece counts below, at and above the in-piece sample count must occur"""
    for K in (16, 8):
        assert any(n < K for n in NXYS) and any(n > K for n in NXYS)
    assert 7 in NXYS and 8 in NXYS                                   # int_K = 8: the two tables one entry apart and equally long
    assert 1 in NXYS and all(PS.pieces(PS.sweep_problem(n, 2.0))[1] > n for n in NXYS if n > 1)


@pytest.mark.parametrize("int_K", (16, 8))
@pytest.mark.parametrize("lanes", LANES)
def test_emu_evaluation_and_scaling(oracle, oracle_grid, analytic_cells, lanes, int_K):
    """f, grad f, hx, gx (the refresh behind the evaluation), coefficients and T at 1e-10; initScaling's scale_fx / scale_cx at 1e-10"""
    ref = PS.oracle_evals(oracle, oracle_grid, CASES, int_K=int_K)
    refs = _oracle_scalings(oracle, oracle_grid, int_K)
    emu = E.Emu(analytic_cells, oracle.map_params_vec(), oracle.params_vec(_params(int_K)))
    E.lib().emu_set_lanes(lanes)
    bad = []
    try:
        for c in CASES:
            p, st = PS.sweep_problem(*c), PS.case_state(c[0], c[1], int_K)
            kw = dict(lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], rho=st["rho"], scale_fx=st["scale_fx"])
            r = emu.run(0, p, ref[c]["x0"], **kw)
            e = PS.eval_errors(ref[c], r)
            print("eval  lanes %d K %d %s %s" % (lanes, int_K, PS.pieces(p), {k: "%.1e" % v for k, v in e.items()}))
            bad += [(lanes, int_K, PS.pieces(p), q, v) for q, v in e.items() if not v < 1e-10]
            _same(r, emu.run(0, p, ref[c]["x0"], **kw), ("eval", lanes, int_K, c))
            s = emu.run(1, p, ref[c]["x0"])
            e = dict(scale_fx=PS.rel1(refs[c]["scale_fx"], s["scale_fx"]), scale_cx=PS.rel(refs[c]["scale_cx"], s["scale_cx"]))
            print("scale lanes %d K %d %s %s" % (lanes, int_K, PS.pieces(p), {k: "%.1e" % v for k, v in e.items()}))
            bad += [(lanes, int_K, PS.pieces(p), q, v) for q, v in e.items() if not v < 1e-10]
            _same(s, emu.run(1, p, ref[c]["x0"]), ("scaling", lanes, int_K, c))
    finally:
        E.lib().emu_set_lanes(256)
    assert not bad, bad[:8]


@pytest.mark.parametrize("name,params", [("refresh", REFRESH_PARAMS), ("capped", PS.SOLVE_PARAMS)], ids=["refresh_then_evaluation", "capped_solve"])
@pytest.mark.parametrize("int_K", (16, 8))
@pytest.mark.parametrize("lanes", LANES)
def test_emu_solves(oracle, oracle_grid, analytic_cells, lanes, int_K, name, params):
    """two ALM passes of at most 1 / at most 12 L-BFGS iterations: the oracle's decisions (return code, iteration and evaluation counts equal), x and
    the cost within 1e-7 (test_pieces_cpu::test_emu_capped_solves), the second run bit-identical"""
    ref = _oracle_solves(oracle, oracle_grid, int_K, name, params)
    ev = PS.oracle_evals(oracle, oracle_grid, CASES, int_K=int_K)
    emu = E.Emu(analytic_cells, oracle.map_params_vec(), oracle.params_vec(_params(int_K, params)))
    E.lib().emu_set_lanes(lanes)
    bad, second_pass = [], 0
    try:
        for c in CASES:
            p, ro = PS.sweep_problem(*c), ref[c]
            r = emu.run(2, p, ev[c]["x0"])
            if (r["ret"], r["lbfgs_iters"], r["evals"]) != (ro["ret"], ro["lbfgs_iters"], ro["evals"]):
                bad.append((lanes, int_K, PS.pieces(p), "counters", (r["ret"], r["lbfgs_iters"], r["evals"]), (ro["ret"], ro["lbfgs_iters"], ro["evals"])))
            e = dict(x=PS.rel(ro["x"], r["x"]), cost=PS.rel1(ro["cost"], r["f"]))
            print("%s lanes %d K %d %s evals %d %s" % (name, lanes, int_K, PS.pieces(p), r["evals"], {k: "%.1e" % v for k, v in e.items()}))
            bad += [(lanes, int_K, PS.pieces(p), q, v) for q, v in e.items() if not v < 1e-7]
            _same(r, emu.run(2, p, ev[c]["x0"]), (name, lanes, int_K, c))
            second_pass += r["alm_iters"] >= 1 and r["evals"] >= 3      # an evaluation followed a refresh (a trajectory may also converge in its first pass)
    finally:
        E.lib().emu_set_lanes(256)
    assert not bad, bad[:8]
    assert 2 * second_pass >= len(CASES), second_pass


@pytest.mark.parametrize("lanes", LANES)
def test_emu_equals_the_build_with_the_chains_in_place(oracle, oracle_grid, analytic_cells, lanes):
    """-DUPH_ASIDE_PREP=0 forms every value where it is used, as before the move: the same operations on the same operands, so one evaluation,
    initScaling and the capped solve of the two builds agree bit for bit"""
    ev = PS.oracle_evals(oracle, oracle_grid, CASES)
    mp, op = oracle.map_params_vec(), oracle.params_vec(PS.SOLVE_PARAMS)
    new, old = E.Emu(analytic_cells, mp, op), E.Emu(analytic_cells, mp, op, flags=("-DUPH_ASIDE_PREP=0",))
    try:
        for L in (new.L, old.L):
            L.emu_set_lanes(lanes)
        for c in CASES:
            p, st = PS.sweep_problem(*c), PS.case_state(*c)
            kw = dict(lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], rho=st["rho"], scale_fx=st["scale_fx"])
            _same(new.run(0, p, ev[c]["x0"], **kw), old.run(0, p, ev[c]["x0"], **kw), ("eval", lanes, c))
            _same(new.run(1, p, ev[c]["x0"]), old.run(1, p, ev[c]["x0"]), ("scaling", lanes, c))
            _same(new.run(2, p, ev[c]["x0"]), old.run(2, p, ev[c]["x0"]), ("solve", lanes, c))
    finally:
        for L in (new.L, old.L):
            L.emu_set_lanes(256)
