"""Trial abandonment of the line search, CPU tier: the dual bound every abandonment rests on, the rule that says when a
rejected trial cannot be followed by an exit of the search, and the workgroup program in the CPU emulator with the switch on against off."""
import numpy as np
import pytest

import abandon_emu as A
import forced_cases as F

EPS = 2.0 ** -52
RUN_KEYS = ("x", "g", "lam", "mu", "hx", "gx", "c_xy", "c_yaw", "f", "jerk_cost", "T_xy", "T_yaw", "rho", "scale_fx", "ret", "alm_iters", "lbfgs_iters", "evals",
            "last_lbfgs_ret", "hist_reads")


def _terms(h, g, lam, mu, rho):
    """penalty cost of one sample as Solver::sampleEval forms it (alm_traj_opt.h:153-163): the equality term and six PHR inequality terms.
    h, lam, rho: (n,)   g, mu: (n, 6)   ->   terms (n, 7), active (n, 6)"""
    r = rho[:, None]
    eq = h * (lam + 0.5 * rho * h)
    act = r * g + mu > 0
    ineq = np.where(act, g * (mu + 0.5 * r * g), -0.5 * mu * mu / r)
    return np.concatenate([eq[:, None], ineq], axis=1), act


@pytest.mark.parametrize("zero_duals", [False, True])
def test_every_penalty_term_is_at_or_above_its_dual_bound(zero_duals):
    rng = np.random.default_rng(11)
    n = 20000
    rho = 10.0 ** rng.uniform(-3, 3, size=n)
    scale = 10.0 ** rng.uniform(-4, 4, size=n)
    h = rng.normal(size=n) * scale
    g = rng.normal(size=(n, 6)) * scale[:, None]
    lam = rng.normal(size=n) * 10.0 ** rng.uniform(-4, 4, size=n)
    mu = np.abs(rng.normal(size=(n, 6))) * 10.0 ** rng.uniform(-4, 4, size=(n, 1))
    mu[rng.random(size=(n, 6)) < 0.1] = 0.0                               # inactive multipliers, as most are in a real solve
    if zero_duals:                                                        # the first ALM pass
        lam[:] = 0.0
        mu[:] = 0.0
    # the first 2000 samples sit at the PHR branch point rho g + mu = 0, or a hair to either side of it, and at the minimiser of the equality term
    k = 2000
    g[:k] = -mu[:k] / rho[:k, None] * rng.choice([1.0, 1.0 - 1e-12, 1.0 + 1e-12], size=(k, 6))
    h[:k] = -lam[:k] / rho[:k]
    t, act = _terms(h, g, lam, mu, rho)
    assert act.any() and (~act).any()                                     # both PHR branches are drawn
    dual = np.concatenate([lam[:, None], mu], axis=1)
    vals = np.concatenate([h[:, None], g], axis=1)
    bound = -dual * dual / (2.0 * rho[:, None])
    # a computed term may lie below its exact value by a few roundings of the products it is made of
    slack = 8 * EPS * (np.abs(vals * dual) + 0.5 * rho[:, None] * vals * vals + np.abs(bound))
    assert (t >= bound - slack).all(), float((bound - t).max())
    lb_dual = (dual * dual / (2.0 * rho[:, None])).sum()
    assert t.sum() >= -lb_dual - 7 * n * EPS * np.abs(t).sum()
    if zero_duals:
        assert lb_dual == 0.0 and (t >= 0.0).all()


def _exit_follows_rejection(count, stp, mu, stpmin, stpmax, max_linesearch, machine_prec):
    """lbfgs.hpp:349-387 restated literally for a trial that has just failed the Armijo test at :332-336 (count = trials before this one)"""
    count += 1                                                            # :317
    nu, brackt, touched = stp, True, False                                # :334-335
    if max_linesearch <= count:                                           # :349-353
        return True
    if brackt and (nu - mu) < machine_prec * nu:                          # :355-358
        return True
    if brackt:                                                            # :360-364
        stp = 0.5 * (mu + nu)
    else:
        stp *= 2.0
    if stp < stpmin:                                                      # :365-368
        return True
    if stp > stpmax:                                                      # :369-378
        if touched:
            return True
        touched, stp = True, stpmax
    return False


def test_may_abandon_is_true_only_where_no_exit_follows_a_rejection():
    L = A.lib()
    rng = np.random.default_rng(5)
    cases = []
    for _ in range(20000):
        max_ls = int(rng.integers(1, 70))
        count = int(rng.integers(0, max_ls))
        stp = 10.0 ** rng.uniform(-22, 3)
        mu = stp * rng.choice([0.0, 0.5, 1.0 - 1e-16, 1.0 - 2e-16, 1.0 - 1e-15, 1.0 - 1e-12])
        if rng.random() < 0.7:
            stpmin = 10.0 ** rng.choice([-20.0, -3.0])
        else:                                                             # the next step lands on, just above or just below the minimum step
            stpmin = 0.5 * (mu + stp) * rng.choice([1.0, 1.0 + 1e-15, 1.0 - 1e-15])
        cases.append((count, stp, mu, stpmin, 1e20, max_ls, 1e-16))
    # the reference's own parameters: the last trial before the cap, the one before it, the first trial of a search
    cases += [(63, 1e-3, 0.0, 1e-20, 1e20, 64, 1e-16), (62, 1e-3, 0.0, 1e-20, 1e20, 64, 1e-16), (0, 1.0, 0.0, 1e-20, 1e20, 64, 1e-16)]
    seen = {True: 0, False: 0}
    for c in cases:
        may = bool(L.emu_may_abandon(*c))
        assert may == (not _exit_follows_rejection(*c)), c
        seen[may] += 1
    assert seen[True] > 1000 and seen[False] > 1000
    assert not L.emu_may_abandon(*cases[-3]) and L.emu_may_abandon(*cases[-2]) and L.emu_may_abandon(*cases[-1])


def _pair(oracle, cells, params, lanes=128):
    mk = lambda: A.AbandonEmu(cells, oracle.map_params_vec(), oracle.params_vec(params), lanes)
    return mk(), mk().set_trial_abandon(False)


def _same(a, b, keys=RUN_KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("lanes", [128, 256])
def test_emulated_full_solves_are_bit_identical_on_and_off(oracle, oracle_grid, analytic_cells, small_problems, lanes):
    on, off = _pair(oracle, analytic_cells, {}, lanes)
    tot = dict.fromkeys(A.COUNTERS, 0)
    for p in small_problems:
        x0 = oracle.OracleALM(oracle_grid).setup(p)
        r_on = on.run(2, p, x0)
        c_on = on.counters()
        r_off = off.run(2, p, x0)
        c_off = off.counters()
        _same(r_on, r_off)
        assert all(v == 0 for v in c_off.values()), c_off
        for k in tot:
            tot[k] += c_on[k]
    print("emulated solves, lanes %d: %s" % (lanes, tot))
    assert tot["ls_rejected"] > 0 and tot["ls_abandoned"] > 0 and tot["chunks_skipped"] >= tot["ls_abandoned"]
    assert tot["adjoints_skipped"] >= tot["ls_rejected"] - tot["ls_guarded"]


def test_emulated_later_alm_pass_with_duals_is_bit_identical_and_abandons(oracle, oracle_grid, analytic_cells):
    """a later ALM pass of the oracle's solve replayed from the oracle's own (x, lambda, mu, rho): lb_dual is not zero there"""
    from uneven_planner_amd import scenes
    prob = scenes.random_problems(1, seed0=1000)[0]
    prm = dict(mem_size=64)
    st = F.capture(oracle_grid, prob, prm, 0, 1)
    on, off = _pair(oracle, analytic_cells, prm)
    abandoned = done = 0
    for i, ps in enumerate(st["passes"]):
        if i == 0 or ps["k"] > 30:
            continue
        assert np.abs(ps["lam_in"]).max() > 0 or np.abs(ps["mu_in"]).max() > 0
        kw = dict(lam=ps["lam_in"], mu=ps["mu_in"], scale_cx=st["scale_cx"], rho=ps["rho_in"], scale_fx=st["scale_fx"])
        r_on = on.alm_passes(prob, ps["x_in"], 1, **kw)
        abandoned += on.counters()["ls_abandoned"]
        _same(r_on, off.alm_passes(prob, ps["x_in"], 1, **kw))
        done += 1
    assert done >= 3 and abandoned > 0


def test_emulated_exhausted_search_evaluates_its_last_trial_in_full(oracle, oracle_grid, analytic_cells):
    from uneven_planner_amd import scenes
    prob = scenes.random_problems(1, seed0=1000)[0]
    prm = dict(mem_size=8)
    st = F.doctor(F.capture(oracle_grid, prob, prm, 1, 3), "ls_fail", np.random.default_rng(4), prob)
    kw = dict(lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], rho=st["rho"], scale_fx=st["scale_fx"])
    on, off = _pair(oracle, analytic_cells, prm)
    r_on, s_on = on.lbfgs_resume(prob, st, 5, finish=True, **kw)
    c = on.counters()
    r_off, s_off = off.lbfgs_resume(prob, st, 5, finish=True, **kw)
    assert s_on["code"] == s_off["code"] == F.LBFGSERR_MAXIMUMLINESEARCH
    _same(r_on, r_off)
    for k in ("x", "g", "fx", "step", "hx", "gx", "lam", "mu", "rho", "accepted", "converged", "k"):
        assert np.array_equal(np.asarray(s_on[k]), np.asarray(s_off[k])), k
    # 64 rejected trials; the one at the cap may be followed by the exit, so it -- and only it -- is evaluated in full
    assert c["ls_rejected"] == 64 and c["ls_guarded"] == 1 and c["adjoints_skipped"] == 63
