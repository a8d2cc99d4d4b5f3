"""Trial abandonment of the line search on the device: with the switch on (the default) a trial whose rejection by the Armijo
test is certain stops before its samples or before its adjoint; every result must equal the switch-off solve bit for bit, and the counters must show
that trials really were abandoned."""
import numpy as np
import pytest

import forced_cases as F

pytestmark = pytest.mark.gpu

RESULT_SCALARS = ("ret", "alm_iters", "lbfgs_iters", "evals", "last_lbfgs_ret", "cost", "jerk_cost", "T_xy", "T_yaw", "rho_final", "scale_fx")
ARRAYS = ("x", "c_xy", "c_yaw", "hx", "gx", "lam", "mu")
COUNTERS = ("ls_rejected", "ls_guarded", "ls_abandoned", "chunks_skipped", "adjoints_skipped")


@pytest.fixture(scope="module")
def devmap(analytic_cells):
    import uneven_planner_amd as U
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    return m


@pytest.fixture(scope="module")
def batch():
    from uneven_planner_amd import scenes
    return scenes.random_problems(40, seed0=1000)


@pytest.fixture(scope="module")
def forced_probs():
    from uneven_planner_amd import scenes
    return [scenes.hill_problem()] + scenes.random_problems(3, seed0=1000)


def _opt(devmap, params, lanes, on):
    import uneven_planner_amd as U
    opt = U.ALMTrajOpt(devmap, params)
    opt.set_lanes(lanes)
    opt.set_trial_abandon(on)
    return opt


def _assert_same(a, b, what, keys=ARRAYS + RESULT_SCALARS):
    for i, (ra, rb) in enumerate(zip(a, b)):
        for k in keys:
            assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k]), equal_nan=True), (what, i, k)


def _solve(devmap, probs, lanes, on, trace=2048):
    opt = _opt(devmap, None, lanes, on)
    opt.set_trace(trace)
    opt.set_rho(1.0)
    out = opt.optimize_batch(probs)
    return out, opt.get_trace(), opt.stats()


@pytest.mark.parametrize("lanes", [64, 128, 256, 512, 0])
def test_batch_is_bit_identical_on_and_off_and_trials_are_abandoned(devmap, batch, lanes):
    r_on, t_on, s_on = _solve(devmap, batch, lanes, True)
    r_off, t_off, s_off = _solve(devmap, batch, lanes, False)
    print("lanes %d on: %s   off: %s" % (lanes, {k: s_on[k] for k in COUNTERS + ("evals", "sample_evals")}, {k: s_off[k] for k in COUNTERS + ("evals", "sample_evals")}))
    _assert_same(r_on, r_off, "lanes %d" % lanes)
    assert np.array_equal(t_on, t_off, equal_nan=True)
    assert s_on["evals"] == s_off["evals"] and s_on["lbfgs_iters"] == s_off["lbfgs_iters"]
    # not vacuous: the CPU oracle proves 51 % of the Armijo rejections of exactly these problems before the first sample; half of that is the floor
    assert s_on["ls_rejected"] > 0 and 4 * s_on["ls_abandoned"] >= s_on["ls_rejected"]
    assert s_on["adjoints_skipped"] >= s_on["ls_rejected"] - s_on["ls_guarded"]
    assert s_on["chunks_skipped"] >= s_on["ls_abandoned"]
    assert all(s_off[k] == 0 for k in COUNTERS), s_off
    # sample_evals counts the samples that ran: off = every evaluation's, on = fewer by the abandoned trials'
    S = [(p["inner_xy"].shape[1] + 1) * 17 for p in batch]
    assert s_off["sample_evals"] == sum(r["evals"] * s for r, s in zip(r_off, S)) and s_on["sample_evals"] < s_off["sample_evals"]


def _load(opt, probs, states):
    opt.upload(probs)
    opt.set_state(lam=[s["lam"] for s in states], mu=[s["mu"] for s in states], scale_cx=[s["scale_cx"] for s in states],
                  scale_fx=[s["scale_fx"] for s in states], rho=[s["rho"] for s in states])
    opt.set_lbfgs_state(states)


def test_exhausted_search_restores_the_same_state_and_evaluates_its_last_trial_in_full(devmap, oracle_grid, forced_probs):
    prm = dict(mem_size=8)
    rng = np.random.default_rng(4)
    states = [F.doctor(F.capture(oracle_grid, p, prm, 1, 3), "ls_fail", rng, p) for p in forced_probs]
    got, stats = {}, {}
    for on in (True, False):
        opt = _opt(devmap, prm, 128, on)
        _load(opt, forced_probs, states)
        opt.lbfgs_resume(5, finish_pass=True)
        got[on] = opt.get_lbfgs_state()
        stats[on] = opt.stats()
    for a, b, s in zip(got[True], got[False], states):
        assert a["code"] == b["code"] == F.LBFGSERR_MAXIMUMLINESEARCH
        assert np.array_equal(a["x"], s["x"]) and np.array_equal(a["g"], s["g"])                     # restored (lbfgs.hpp:575-582)
        for k in ("x", "g", "fx", "step", "k", "accepted", "converged", "hx", "gx", "lam", "mu", "rho"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k                          # st.f, the residuals of the last trial (Q1), the dual update
    # 64 rejected trials per search; an exit can follow the one at the cap, so that one -- and no other -- ran its adjoint
    n = len(forced_probs)
    assert stats[True]["ls_rejected"] == 64 * n and stats[True]["ls_guarded"] == n and stats[True]["adjoints_skipped"] == 63 * n
    assert all(stats[False][k] == 0 for k in COUNTERS)


def test_later_alm_pass_with_duals_is_bit_identical_and_abandons(devmap, oracle_grid, forced_probs):
    """ALM passes >= 2 replayed from the oracle's own (x, lambda, mu, rho): the dual bound is not zero there"""
    prm = dict(mem_size=64)
    opts = {on: _opt(devmap, prm, 128, on) for on in (True, False)}
    abandoned = done = 0
    for p in forced_probs[:2]:
        st = F.capture(oracle_grid, p, prm, 0, 1)
        for i, ps in enumerate(st["passes"]):
            if i == 0 or ps["k"] > 30:
                continue
            assert np.abs(ps["lam_in"]).max() > 0 or np.abs(ps["mu_in"]).max() > 0
            res = {}
            for on, opt in opts.items():
                opt.upload([p])
                opt.set_state(lam=[ps["lam_in"]], mu=[ps["mu_in"]], scale_cx=[st["scale_cx"]], scale_fx=[st["scale_fx"]], rho=[ps["rho_in"]])
                opt.set_x([ps["x_in"]])
                opt.alm_passes(1)
                res[on] = opt.download()
                if on:
                    abandoned += opt.stats()["ls_abandoned"]
            _assert_same(res[True], res[False], "pass %d" % i)
            done += 1
    assert done >= 4 and abandoned > 0


def test_nan_cell_under_the_first_piece_gives_the_same_result_on_and_off(analytic_cells, batch):
    """a non-finite partial sum never abandons: the return code and every output equal the switch-off solve"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    probs = batch[:4]
    nx, ny, nyaw = scenes.grid_dims(10.0, 10.0, 0.05, 0.1)
    cells = analytic_cells.copy().reshape(nx, ny, nyaw, 4)
    for p in probs:                                   # the cell half way from the start to the first way-point of the initial guess, every yaw bin
        q = 0.5 * (p["init_xy"][:, 0] + p["inner_xy"][:, 0])
        cells[int((q[0] + 5.0) / 0.05), int((q[1] + 5.0) / 0.05), :, :] = np.nan
    m = U.UnevenMap()
    m.set_cells(cells.reshape(-1, 4))
    r_on, t_on, s_on = _solve(m, probs, 128, True, trace=256)
    r_off, t_off, s_off = _solve(m, probs, 128, False, trace=256)
    _assert_same(r_on, r_off, "nan cell")
    assert np.array_equal(t_on, t_off, equal_nan=True)
    assert [r["ret"] for r in r_on] == [r["ret"] for r in r_off] and s_on["evals"] == s_off["evals"]
