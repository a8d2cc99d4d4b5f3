"""Every position piece count 1..128 x yaw ratios {1, 1.7, 2, 3} through every lane / occupancy variant of the solve, scaling and penalty
kernels, against the oracle (run with -m gpu on an MI355X; everything goes through the C-ABI).

The kernels are one workgroup program whose control flow depends on (Nxy, lanes): aligned or plain sample chunks, pieces straddling two
chunks, one to four MFMA scatter tiles with a partly empty last one, the vector scatter for int_K != 16, the two-loop's register classes.
tests/piece_sweep.py generates the problems, says which class a pair falls in (coverage assertions only) and holds the oracle's answers,
computed once per process.  Each case uploads its whole problem list as ONE heterogeneous batch (1 to 128 pieces side by side: the
residency classes of oversize trajectories are exercised as well) -- a few hundred small problems per launch.

The worst error of every (test, variant) is kept in piece_sweep.MEASURED; tools/piece_sweep_report.py runs this file and writes them, next
to the oracle's own FMA floor, to profiles/.
"""
import numpy as np
import pytest

import piece_sweep as PS
from test_gpu_lanes import VARIANTS

pytestmark = pytest.mark.gpu

AUTO = (0, 0)                                     # automatic kernel selection
ALL_VARIANTS = list(VARIANTS) + [AUTO]
_vid = lambda v: "auto" if v == AUTO else "%dx%d" % v
_SOLVED = {}                                      # (lanes, wps) -> results of the capped solves (first and second run), computed once


@pytest.fixture(scope="module")
def dev(analytic_cells):
    import uneven_planner_amd as U
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    return m


def _ctx(dev, variant, params=None):
    import uneven_planner_amd as U
    opt = U.ALMTrajOpt(dev, params=params)
    if variant != AUTO:
        opt.set_lanes(variant[0])
        if variant[1]:
            opt.set_wps(variant[1])
    return opt


def _upload(opt, probs, variant):
    """one upload of the whole list.  A refusal is a failure: 128 pieces at 512 lanes need about 128 KB of LDS, below the 160 KiB of a workgroup,
    and include/uneven_hip.h documents no limit other than UPH_MAX_PIECE_XY / _YAW, inside which every problem of the sweep lies.  The message
    names the refused problems."""
    import uneven_planner_amd as U
    try:
        opt.upload(probs)
    except U._lib.UnevenHipError as e:
        refused = []
        for p in probs:
            try:
                opt.upload([p])
            except U._lib.UnevenHipError:
                refused.append(PS.pieces(p))
        pytest.fail("upload refused at variant %s: %s; refused alone (Nxy, Nyaw): %s" % (_vid(variant), e, refused[:16]))


def _evaluate(opt, cases, variant, int_K=16):
    probs = [PS.sweep_problem(*c) for c in cases]
    st = [PS.case_state(c[0], c[1], int_K) for c in cases]
    _upload(opt, probs, variant)
    opt.set_state(lam=[s["lam"] for s in st], mu=[s["mu"] for s in st], scale_cx=[s["scale_cx"] for s in st],
                  scale_fx=np.array([s["scale_fx"] for s in st]), rho=np.array([s["rho"] for s in st]))
    f, gs = opt.eval_batch(opt.x0_packed(probs))
    out = opt.download()
    return probs, [dict(out[i], f=f[i], g=gs[i]) for i in range(len(probs))]


def _check(test, variant, cases, got, bar):
    """got[i]: dict quantity -> error of case i; bar(quantity, nxy) -> bound.  Records the worst error, fails with (lanes, wps, Nxy, Nyaw, quantity, error)"""
    errs, bad = {}, []
    for c, e in zip(cases, got):
        where = PS.pieces(PS.sweep_problem(*c))
        errs[where if len({r for _, r in cases}) == 1 else where + (c[1],)] = e
        bad += [(variant[0], variant[1], where[0], where[1], q, v) for q, v in e.items() if not v < bar(q, where[0])]
    print("%s %s: worst" % (test, _vid(variant)), PS.record(test, _vid(variant), errs))
    assert not bad, "%d above the bar, (lanes, wps, Nxy, Nyaw, quantity, error): %s" % (len(bad), bad[:12])


def _eval_bar(q, nxy):
    """the project's bar for one evaluation (test_gpu_parity, test_gpu_lanes): 1e-9; 1e-8 for grad f from 64 pieces on
    (test_gpu_edge::test_largest_supported_problem); the piece durations to 1e-13 absolute (test_gpu_parity)"""
    if q == "T":
        return 1e-13
    return 1e-8 if (q == "grad" and nxy >= 64) else 1e-9


# ---- a. single evaluation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ALL_VARIANTS, ids=_vid)
def test_single_evaluation_every_piece_count_and_ratio(dev, oracle, oracle_grid, variant):
    """f, grad f, hx, gx, c_xy, c_yaw and T for every Nxy in 1..128 x four yaw ratios in one batch"""
    cases = PS.all_cases()
    for lanes in ([variant[0]] if variant != AUTO else PS.LANE_COUNTS):
        for r in PS.RATIOS:                        # per ratio (ratio 3 ends at Nxy = 85): every chunking and tile count this lane count has
            PS.assert_chunk_coverage([n for n, rr in cases if rr == r], lanes)
    ref = PS.oracle_evals(oracle, oracle_grid, cases)
    probs, got = _evaluate(_ctx(dev, variant), cases, variant)
    _check("a_single_evaluation", variant, cases, [PS.eval_errors(ref[c], g) for c, g in zip(cases, got)], _eval_bar)


# ---- b. initScaling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ALL_VARIANTS, ids=_vid)
def test_init_scaling_every_piece_count(dev, oracle, oracle_grid, variant):
    """scale_fx and scale_cx of uph_init_scaling_batch, ratio 2, every Nxy, at 1e-9"""
    cases = [c for c in PS.all_cases() if c[1] == 2.0]
    assert [c[0] for c in cases] == PS.NXY_ALL
    ref = PS.oracle_scalings(oracle, oracle_grid, cases)
    opt = _ctx(dev, variant)
    _upload(opt, [PS.sweep_problem(*c) for c in cases], variant)
    opt.init_scaling_batch()
    out = opt.download()
    got = [dict(scale_fx=PS.rel1(ref[c]["scale_fx"], o["scale_fx"]), scale_cx=PS.rel(ref[c]["scale_cx"], o["scale_cx"])) for c, o in zip(cases, out)]
    _check("b_init_scaling", variant, cases, got, lambda q, nxy: 1e-9)


# ---- c. the penalty kernel alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", PS.LANE_COUNTS)
def test_penalty_kernel_every_piece_count(dev, oracle, oracle_grid, lanes):
    """uph_penalty_batch(repeat = 2, store_residuals) in each of its four instantiations, ratio 2, every Nxy: cost, gdCxy, gdCyaw, the two gdT
    sums, hx, gx at 1e-9 -- the quantities and the bar of test_gpu_lanes::test_penalty_kernel_alone_for_every_lane_count"""
    variant = (lanes, 0)
    cases = [c for c in PS.all_cases() if c[1] == 2.0]
    ref = PS.oracle_evals(oracle, oracle_grid, cases)
    opt = _ctx(dev, variant)
    probs, _ = _evaluate(opt, cases, variant)
    pen = opt.penalty_batch(repeat=2, store_residuals=True)
    out = opt.download()
    got = [PS.penalty_errors(ref[c], d, o["hx"], o["gx"]) for c, d, o in zip(cases, pen, out)]
    _check("c_penalty", variant, cases, got, lambda q, nxy: 1e-9)


# ---- d. capped solves -------------------------------------------------------------------------------------------------------------------
def _solve(dev, variant):
    if variant not in _SOLVED:
        probs = [PS.sweep_problem(n, 2.0) for n in PS.SOLVE_NXY]
        opt = _ctx(dev, variant, params=PS.SOLVE_PARAMS)
        opt.set_rho(1.0)
        _upload(opt, probs, variant)
        opt.solve()
        first = opt.download()
        opt.set_rho(1.0)
        second = opt.optimize_batch(probs)
        _SOLVED[variant] = (first, second)
    return _SOLVED[variant]


@pytest.mark.parametrize("variant", ALL_VARIANTS, ids=_vid)
def test_capped_solves(dev, oracle, oracle_grid, variant):
    """two ALM passes of at most 12 L-BFGS iterations (inner_max_iter = 12, max_iter = 1, rho = 1) at piece_sweep.SOLVE_NXY, ratio 2 -- n crosses
    the two-loop's register classes at 64, 128 and 256: return code, iteration and evaluation counts equal the oracle's, x and the cost within
    1e-5 (test_largest_supported_problem's bar for 40 iterations), and the same batch solved again gives bit-identical x"""
    cases = [(n, 2.0) for n in PS.SOLVE_NXY]
    ref = PS.oracle_solves(oracle, oracle_grid, cases)
    first, second = _solve(dev, variant)
    bad = []
    for c, o in zip(cases, first):
        ro, where = ref[c], PS.pieces(PS.sweep_problem(*c))
        if (o["ret"], o["lbfgs_iters"], o["evals"]) != (ro["ret"], ro["lbfgs_iters"], ro["evals"]):
            bad.append((variant[0], variant[1]) + where + ("ret / lbfgs_iters / evals", (o["ret"], o["lbfgs_iters"], o["evals"]), (ro["ret"], ro["lbfgs_iters"], ro["evals"])))
    assert not bad, bad
    got = [dict(x=PS.rel(ref[c]["x"], o["x"]), cost=PS.rel1(ref[c]["cost"], o["cost"])) for c, o in zip(cases, first)]
    _check("d_capped_solves", variant, cases, got, lambda q, nxy: 1e-5)
    again = [PS.pieces(PS.sweep_problem(*c)) for c, a, b in zip(cases, first, second) if not (np.array_equal(a["x"], b["x"]) and a["evals"] == b["evals"])]
    assert not again, ("the second solve of the same batch differs", variant, again)


@pytest.mark.parametrize("lanes", [64, 256])
def test_capped_solves_do_not_depend_on_the_occupancy_variant(dev, lanes):
    """wps = 1 and wps = 2 of one lane count are the same program under another register budget: bit-identical x, cost and counters"""
    a, b = _solve(dev, (lanes, 1))[0], _solve(dev, (lanes, 2))[0]
    diff = [PS.pieces(PS.sweep_problem(n, 2.0)) for n, p, q in zip(PS.SOLVE_NXY, a, b)
            if not (np.array_equal(p["x"], q["x"]) and p["cost"] == q["cost"] and p["evals"] == q["evals"])]
    assert not diff, (lanes, diff)


# ---- e. the vector scatter on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [128, 512])
def test_vector_scatter_int_K_8_every_piece_count(dev, oracle, oracle_grid, lanes):
    """int_K = 8 (nine samples per piece) takes the vector xyTask path instead of the matrix cores: ratio 2, every Nxy, one evaluation at 1e-9
    against the oracle built with the same parameter"""
    variant = (lanes, 0)
    cases = [c for c in PS.all_cases() if c[1] == 2.0]
    assert {PS.chunk_class(c[0], lanes, 8)[0] for c in cases} == {True, False}
    ref = PS.oracle_evals(oracle, oracle_grid, cases, int_K=8)
    probs, got = _evaluate(_ctx(dev, variant, params=dict(int_K=8)), cases, variant, int_K=8)
    _check("e_vector_scatter_int_K_8", variant, cases, [PS.eval_errors(ref[c], g) for c, g in zip(cases, got)],
           lambda q, nxy: 1e-13 if q == "T" else 1e-9)


# ---- f. fp32 cell storage ---------------------------------------------------------------------------------------------------------------
def test_f32_cell_storage_every_piece_count(oracle, analytic_cells):
    """UnevenMap(storage = "f32") at <128, 2>: cells stored as floats, widened on load, fp64 arithmetic -- so one evaluation equals the oracle's on
    the float-rounded grid at test_emu_f32_cell_storage_equals_oracle_on_rounded_cells's bar (f 1e-11, grad f 1e-10; the other quantities at
    1e-9 as everywhere), ratio 2, every Nxy.  (The fp32 SAMPLE mode is test_gpu_km2's.)"""
    import uneven_planner_amd as U
    variant = (128, 2)
    rounded = analytic_cells.astype(np.float32).astype(np.float64)
    og = oracle.OracleGrid()
    og.set_cells(rounded)
    m = U.UnevenMap(storage="f32")
    m.set_cells(analytic_cells)
    cases = [c for c in PS.all_cases() if c[1] == 2.0]
    ref = PS.oracle_evals(oracle, og, cases, tag="f32-rounded")
    probs, got = _evaluate(_ctx(m, variant), cases, variant)
    _check("f_f32_cell_storage", variant, cases, [PS.eval_errors(ref[c], g) for c, g in zip(cases, got)],
           lambda q, nxy: {"f": 1e-11, "grad": 1e-10, "T": 1e-13}.get(q, 1e-9))
