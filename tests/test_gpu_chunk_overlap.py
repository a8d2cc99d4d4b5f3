"""The chunk loop of Solver::eval on the device: a chunk's scatter has no barrier of its own, the wave that finishes its half
first runs the next chunk's sample arithmetic and meets the other one in front of the record stores (DevWG::accChunkSplit).  The smallest shapes at
which a misplaced barrier can show, at every lane count -- at 128 and 64 lanes Nxy = 7 (one chunk at 128: no barrier between compute and commit, the
scatter ordered by accEnd alone), 8 (aligned chunks of 119 + 17 samples: the second wave has no sample in the last chunk), 15 (plain chunks, a piece
straddles them), 22 (three chunks, one of them touching nine pieces: two MFMA tiles, one per wave), 43 (six chunks); at 256 lanes 30 and 31 pieces
(the last count with two aligned chunks of 15 pieces and the first with three; 7, 8 and 15 pieces are the single chunks there; at 512 lanes 30 | 31
are one chunk | two) -- plus one int_K = 8 case (the vector scatter) and one fp32-sample-mode case.  A race shows as a difference between two runs
of the same call: every call is made twice and compared bit for bit.  Bars: tests/test_gpu_pieces.py's and tests/test_gpu_aside_prep.py's for the same
quantities (one evaluation and the penalty call 1e-9, T 1e-13 absolute; the capped solves: the oracle's counters, x and the cost within 1e-5)."""
import numpy as np
import pytest

import piece_sweep as PS

pytestmark = pytest.mark.gpu

LANES = [64, 128, 256, 512, 0]                    # 0 = automatic
NXYS = (7, 8, 15, 22, 30, 31, 43)
CASES = [(n, 2.0) for n in NXYS]
ARRAYS = ("x", "c_xy", "c_yaw", "hx", "gx", "lam", "mu", "scale_cx")
SCALARS = ("ret", "alm_iters", "lbfgs_iters", "evals", "last_lbfgs_ret", "cost", "jerk_cost", "T_xy", "T_yaw", "rho_final", "scale_fx")
PEN = ("cost", "gdCxy", "gdCyaw", "gdTxy_sum", "gdTyaw_sum")


@pytest.fixture(scope="module")
def dev(analytic_cells):
    import uneven_planner_amd as U
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    return m


def _opt(dev, lanes, params=None, bits=64, abandon=True, wps=0):
    import uneven_planner_amd as U
    opt = U.ALMTrajOpt(dev, params=params)
    opt.set_lanes(lanes)
    if wps:
        opt.set_wps(wps)
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


def _evaluate(opt, probs, int_K=16):
    st = [PS.case_state(c[0], c[1], int_K) for c in CASES]
    opt.upload(probs)
    opt.set_state(lam=[s["lam"] for s in st], mu=[s["mu"] for s in st], scale_cx=[s["scale_cx"] for s in st],
                  scale_fx=np.array([s["scale_fx"] for s in st]), rho=np.array([s["rho"] for s in st]))
    f, gs = opt.eval_batch(opt.x0_packed(probs))
    out = opt.download()
    return [dict(out[i], f=f[i], g=gs[i]) for i in range(len(probs))]


def _assert_below(errs, bar, what):
    bad = [(what, c, q, v) for c, e in zip(CASES, errs) for q, v in e.items() if not v < bar(q)]
    print(what, [{q: "%.1e" % v for q, v in e.items()} for e in errs])
    assert not bad, bad


def _eval_bar(q):
    return 1e-13 if q == "T" else 1e-9            # (every case has fewer than 64 pieces: test_gpu_pieces' bar for grad f is 1e-9 there)


def test_cases_reach_every_shape_of_the_chunk_loop():
    """(aligned, chunks, pieces touched by one chunk, MFMA tiles of one chunk) of the cases, from the restated constructor"""
    cc = PS.chunk_class
    assert cc(7, 128)[1] == 1                                               # one chunk: no barrier A, accEnd alone orders the scatter
    assert cc(8, 128)[:2] == (True, 2) and 8 * 17 - 119 <= 64              # aligned 119 + 17: no sample on the second wave in the last chunk
    assert cc(15, 128)[0] is False and cc(15, 128)[1] == 2 and 128 % 17 != 0   # plain chunks: piece 7 straddles them
    assert cc(22, 128)[0] is False and cc(22, 128)[1] == 3 and cc(22, 128)[2] == 9 and cc(22, 128)[3] == 2
    assert cc(43, 128)[1] == 6
    assert {cc(n, 64)[0] for n in NXYS} == {True, False} and cc(7, 64)[1] >= 2
    assert cc(15, 256)[1] == 1 and cc(30, 256)[:2] == (True, 2) and cc(31, 256)[:2] == (True, 3)      # 15 pieces per chunk of 255 samples
    assert cc(30, 512)[1] == 1 and cc(31, 512)[1] == 2 and cc(30, 512)[3] == 4                          # one chunk | two, four tiles on eight waves
    assert all(n < 64 for n in NXYS)


@pytest.mark.parametrize("lanes", LANES)
def test_evaluation_and_penalty(dev, oracle, oracle_grid, lanes):
    """one evaluation at x0 (f, grad f, hx, gx, coefficients, T) and uph_penalty_batch against the oracle; both twice, bit-identical"""
    probs = _probs()
    ref = PS.oracle_evals(oracle, oracle_grid, CASES)
    opt = _opt(dev, lanes)
    got = _evaluate(opt, probs)
    _assert_below([PS.eval_errors(ref[c], g) for c, g in zip(CASES, got)], _eval_bar, "evaluation, lanes %d" % lanes)
    pen = opt.penalty_batch(repeat=2, store_residuals=True)
    out = opt.download()
    _assert_below([PS.penalty_errors(ref[c], d, o["hx"], o["gx"]) for c, d, o in zip(CASES, pen, out)], lambda q: 1e-9, "penalty, lanes %d" % lanes)
    _same(pen, opt.penalty_batch(repeat=2, store_residuals=True), "penalty twice", PEN)
    _same(got, _evaluate(opt, probs), "evaluation twice", ARRAYS + SCALARS + ("f", "g"))


@pytest.mark.parametrize("lanes", LANES)
def test_capped_solves_take_the_oracles_decisions(dev, oracle, oracle_grid, lanes):
    """two ALM passes of at most 12 L-BFGS iterations: return code, iteration and evaluation counts equal the oracle's, x and the cost within 1e-5;
    the second solve bit-identical; trial abandonment on equal to off, bit for bit (an abandoned trial returns behind accEnd's barrier)"""
    probs = _probs()
    ref = PS.oracle_solves(oracle, oracle_grid, CASES)
    runs = []
    for on in (True, True, False):
        opt = _opt(dev, lanes, params=PS.SOLVE_PARAMS, abandon=on)
        opt.set_rho(1.0)
        runs.append(opt.optimize_batch(probs))
    bad = []
    for c, o in zip(CASES, runs[0]):
        ro = ref[c]
        if (o["ret"], o["lbfgs_iters"], o["evals"]) != (ro["ret"], ro["lbfgs_iters"], ro["evals"]):
            bad.append((lanes, c, (o["ret"], o["lbfgs_iters"], o["evals"]), (ro["ret"], ro["lbfgs_iters"], ro["evals"])))
    assert not bad, bad
    _assert_below([dict(x=PS.rel(ref[c]["x"], o["x"]), cost=PS.rel1(ref[c]["cost"], o["cost"])) for c, o in zip(CASES, runs[0])], lambda q: 1e-5,
                  "capped solve, lanes %d" % lanes)
    _same(runs[0], runs[1], "second solve")
    _same(runs[0], runs[2], "abandonment on against off")


@pytest.mark.parametrize("lanes", [64, 128, 256])
def test_capped_solves_do_not_depend_on_the_occupancy_variant(dev, lanes):
    """wps = 1 and wps = 2 of one lane count: the same program under another register budget, bit-identical"""
    probs = _probs()
    runs = []
    for wps in (1, 2):
        opt = _opt(dev, lanes, params=PS.SOLVE_PARAMS, wps=wps)
        opt.set_rho(1.0)
        runs.append(opt.optimize_batch(probs))
    _same(runs[0], runs[1], "wps 1 against 2, lanes %d" % lanes)


def test_vector_scatter_int_K_8(dev, oracle, oracle_grid):
    """int_K = 8 takes the vector scatter (its barrier-free form in the chunk loop): one evaluation against the oracle built with the same
    parameter at test_gpu_pieces' bar, twice bit-identical, at 128 lanes (one to four chunks)"""
    probs = _probs()
    assert {PS.chunk_class(n, 128, 8)[1] for n in NXYS} >= {1, 2, 3, 4}
    ref = PS.oracle_evals(oracle, oracle_grid, CASES, int_K=8)
    opt = _opt(dev, 128, params=dict(int_K=8))
    got = _evaluate(opt, probs, int_K=8)
    _assert_below([PS.eval_errors(ref[c], g) for c, g in zip(CASES, got)], _eval_bar, "int_K 8")
    _same(got, _evaluate(opt, probs, int_K=8), "int_K 8 twice", ARRAYS + SCALARS + ("f", "g"))


def test_fp32_sample_mode(dev):
    """the fp32 sample phase hands the same record over: against this library's fp64 path at test_gpu_km2's bars (f 1e-6, grad f 1e-4), twice
    bit-identical, and a capped solve twice bit-identical"""
    probs = _probs()
    e64, e32 = _evaluate(_opt(dev, 128), probs), _evaluate(_opt(dev, 128, bits=32), probs)
    _assert_below([dict(f=PS.rel1(a["f"], b["f"]), grad=PS.rel(a["g"], b["g"])) for a, b in zip(e64, e32)], lambda q: 1e-6 if q == "f" else 1e-4, "fp32 samples")
    _same(e32, _evaluate(_opt(dev, 128, bits=32), probs), "fp32 evaluation twice", ARRAYS + SCALARS + ("f", "g"))
    runs = []
    for _ in range(2):
        opt = _opt(dev, 128, params=PS.SOLVE_PARAMS, bits=32)
        opt.set_rho(1.0)
        runs.append(opt.optimize_batch(probs))
    _same(runs[0], runs[1], "fp32 capped solve twice")
    assert all(np.isfinite(o["cost"]) and o["evals"] > 2 for o in runs[0])
