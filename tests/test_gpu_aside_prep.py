"""The wave-uniform chains of an evaluation formed aside the knot solve on the device: one wave publishes 1 / Txy, 1 / Tyaw,
Txy / K, expC2(tau), getTtoTauGrad(tau) and the sample-time tables through LDS while the other carries the solve.  The smallest shapes at which
that hand-over can go wrong, at every lane count: Nxy = 1 (no interior knot: the solve is empty, the words must still arrive), Nxy = 2, and
Nxy = 64 | 65 at two yaw pieces per position piece (all chains on wave 0 and wave 1 aside | a chain on every wave and the second residency
class), plus one fp32-sample-mode case.  Bars: tests/test_gpu_pieces.py's and tests/test_gpu_abandon.py's for the same quantities."""
import numpy as np
import pytest

import piece_sweep as PS

pytestmark = pytest.mark.gpu

LANES = [64, 128, 256, 512, 0]                    # 0 = automatic
CASES = [(1, 2.0), (2, 2.0), (64, 2.0), (65, 2.0)]
STEP_PARAMS = dict(inner_max_iter=1.0, max_iter=1.0)          # per pass: the evaluation at x0 / after the refresh, then line-search trials only
ARRAYS = ("x", "c_xy", "c_yaw", "hx", "gx", "lam", "mu", "scale_cx")
SCALARS = ("ret", "alm_iters", "lbfgs_iters", "evals", "last_lbfgs_ret", "cost", "jerk_cost", "T_xy", "T_yaw", "rho_final", "scale_fx")


@pytest.fixture(scope="module")
def dev(analytic_cells):
    import uneven_planner_amd as U
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    return m


def _opt(dev, lanes, params=None, bits=64, abandon=True):
    import uneven_planner_amd as U
    opt = U.ALMTrajOpt(dev, params=params)
    opt.set_lanes(lanes)
    if bits != 64:
        opt.set_sample_precision(bits)
    opt.set_trial_abandon(abandon)
    return opt


def _probs():
    return [PS.sweep_problem(*c) for c in CASES]


def _same(a, b, what, keys=ARRAYS + SCALARS):
    for i, (ra, rb) in enumerate(zip(a, b)):
        for k in keys:
            if k in ra:
                assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k]), equal_nan=True), (what, CASES[i], k)


def _load(opt, probs):
    st = [PS.case_state(*c) for c in CASES]
    opt.upload(probs)
    opt.set_state(lam=[s["lam"] for s in st], mu=[s["mu"] for s in st], scale_cx=[s["scale_cx"] for s in st],
                  scale_fx=np.array([s["scale_fx"] for s in st]), rho=np.array([s["rho"] for s in st]))


def _evaluate(opt, probs):
    _load(opt, probs)
    f, gs = opt.eval_batch(opt.x0_packed(probs))
    out = opt.download()
    return [dict(out[i], f=f[i], g=gs[i]) for i in range(len(probs))]


def _eval_bar(q, nxy):
    if q == "T":
        return 1e-13
    return 1e-8 if (q == "grad" and nxy >= 64) else 1e-9


def _assert_below(errs, bar, what):
    bad = [(what, c, q, v) for c, e in zip(CASES, errs) for q, v in e.items() if not v < bar(q, c[0])]
    print(what, [{q: "%.1e" % v for q, v in e.items()} for e in errs])
    assert not bad, bad


def test_cases_sit_on_both_sides_of_the_chain_placement():
    """Nyaw - 1 <= 127 and Nxy - 1 <= 63 puts the three chains on one wave (DevWG::thomasT): 64 pieces are the last that do, 65 the first that do not"""
    pc = [PS.pieces(p) for p in _probs()]
    assert pc[0] == (1, 1) or pc[0][0] == 1
    assert pc[2][0] == 64 and pc[2][1] <= 128 and pc[3][0] == 65 and pc[3][1] > 128


@pytest.mark.parametrize("lanes", LANES)
def test_evaluation_scaling_and_penalty(dev, oracle, oracle_grid, lanes):
    """one evaluation at x0 (f, grad f, hx, gx, coefficients, T), uph_init_scaling_batch and uph_penalty_batch against the oracle at the sweep's bars;
    every result bit-identical between two consecutive calls"""
    probs = _probs()
    ref = PS.oracle_evals(oracle, oracle_grid, CASES)
    refs = PS.oracle_scalings(oracle, oracle_grid, CASES)
    opt = _opt(dev, lanes)
    got = _evaluate(opt, probs)
    _assert_below([PS.eval_errors(ref[c], g) for c, g in zip(CASES, got)], _eval_bar, "evaluation, lanes %d" % lanes)
    pen = opt.penalty_batch(repeat=2, store_residuals=True)
    out = opt.download()
    _assert_below([PS.penalty_errors(ref[c], d, o["hx"], o["gx"]) for c, d, o in zip(CASES, pen, out)], lambda q, n: 1e-9, "penalty, lanes %d" % lanes)
    pen2 = opt.penalty_batch(repeat=2, store_residuals=True)
    _same(pen, pen2, "penalty twice", ("cost", "gdCxy", "gdCyaw", "gdTxy_sum", "gdTyaw_sum"))
    _same(got, _evaluate(opt, probs), "evaluation twice", ARRAYS + SCALARS + ("f", "g"))
    scal = []
    for _ in range(2):
        opt.upload(probs)
        opt.init_scaling_batch()
        scal.append(opt.download())
    _assert_below([dict(scale_fx=PS.rel1(refs[c]["scale_fx"], o["scale_fx"]), scale_cx=PS.rel(refs[c]["scale_cx"], o["scale_cx"])) for c, o in zip(CASES, scal[0])],
                  lambda q, n: 1e-9, "initScaling, lanes %d" % lanes)
    _same(scal[0], scal[1], "initScaling twice")


def _oracle_step_solves(O, og):
    def make(case):
        return O.OracleALM(og, STEP_PARAMS).optimize(PS.sweep_problem(*case))
    return PS._fill("aside_step_solve", "f64", CASES, make)


@pytest.mark.parametrize("name", ["line_search_step", "capped"])
@pytest.mark.parametrize("lanes", LANES)
def test_solves_take_the_oracles_decisions(dev, oracle, oracle_grid, lanes, name):
    """two ALM passes of at most 1 (the evaluations at line-search steps, compared through the search's decisions and its cost) / at most 12 L-BFGS
    iterations: return code, iteration and evaluation counts equal the oracle's, x and the cost within 1e-5; the second solve bit-identical; the solve
    with trial abandonment on equal to the one with it off, bit for bit"""
    probs = _probs()
    params = STEP_PARAMS if name == "line_search_step" else PS.SOLVE_PARAMS
    ref = _oracle_step_solves(oracle, oracle_grid) if name == "line_search_step" else PS.oracle_solves(oracle, oracle_grid, CASES)
    runs = []
    for on in (True, True, False):
        opt = _opt(dev, lanes, params=params, abandon=on)
        opt.set_rho(1.0)
        runs.append(opt.optimize_batch(probs))
    bad = []
    for c, o in zip(CASES, runs[0]):
        ro = ref[c]
        if (o["ret"], o["lbfgs_iters"], o["evals"]) != (ro["ret"], ro["lbfgs_iters"], ro["evals"]):
            bad.append((lanes, c, (o["ret"], o["lbfgs_iters"], o["evals"]), (ro["ret"], ro["lbfgs_iters"], ro["evals"])))
    assert not bad, bad
    _assert_below([dict(x=PS.rel(ref[c]["x"], o["x"]), cost=PS.rel1(ref[c]["cost"], o["cost"])) for c, o in zip(CASES, runs[0])], lambda q, n: 1e-5,
                  "%s solve, lanes %d" % (name, lanes))
    _same(runs[0], runs[1], "second solve")
    _same(runs[0], runs[2], "abandonment on against off")
    assert sum(o["evals"] - o["lbfgs_iters"] for o in runs[0]) > len(CASES)          # line-search trials beyond the accepted ones ran


def test_fp32_sample_mode(dev):
    """the fp32 sample phase reads the same published words (ec_iTyaw, the step, the tables): against this library's fp64 path at test_gpu_km2's bars
    (f 1e-6, grad f 1e-4), twice bit-identical, and a capped solve twice bit-identical"""
    probs = _probs()
    e64, e32 = _evaluate(_opt(dev, 128), probs), _evaluate(_opt(dev, 128, bits=32), probs)
    _assert_below([dict(f=PS.rel1(a["f"], b["f"]), grad=PS.rel(a["g"], b["g"])) for a, b in zip(e64, e32)], lambda q, n: 1e-6 if q == "f" else 1e-4, "fp32 samples")
    _same(e32, _evaluate(_opt(dev, 128, bits=32), probs), "fp32 evaluation twice", ARRAYS + SCALARS + ("f", "g"))
    runs = []
    for _ in range(2):
        opt = _opt(dev, 128, params=PS.SOLVE_PARAMS, bits=32)
        opt.set_rho(1.0)
        runs.append(opt.optimize_batch(probs))
    _same(runs[0], runs[1], "fp32 capped solve twice")
    assert all(np.isfinite(o["cost"]) and o["evals"] > 2 for o in runs[0])
