"""CPU tier of the piece-count sweep (tests/piece_sweep.py): the generator's properties, the coverage of the chunk / tile classes, and the
workgroup program through the host emulator (tests/emu: the vector scatter at 64, 128 and 256 lanes) against the oracle for every position
piece count 1..128 at the yaw ratios 1, 1.7, 2 and 3.  The device's matrix-core scatter and its 512-lane kernel have no CPU stand-in: they
are swept by tests/test_gpu_pieces.py against the same cached oracle results."""
import numpy as np
import pytest

import emu_bridge as E
import piece_sweep as PS

EMU_LANES = (64, 128, 256)


def _emu(oracle, analytic_cells, params=None):
    return E.Emu(analytic_cells, oracle.map_params_vec(), oracle.params_vec(params))


def test_generator_is_exact_and_stays_inside_the_map():
    """every requested Nxy comes out as requested for every ratio, Nyaw lies in [Nxy, 256] for every kept pair, only the ratio-3 tail is left
    out, and every point of every path and problem lies inside the 10 m x 10 m map"""
    cases = PS.all_cases()                                            # (asserts exactness and >= MIN_CASES pairs)
    assert len(cases) >= PS.MIN_CASES
    kept = set(cases)
    for r in PS.RATIOS:
        for nxy in PS.NXY_ALL:
            p = PS.sweep_problem(nxy, r)
            got, nyaw = PS.pieces(p)
            assert got == nxy
            if (nxy, r) in kept:
                assert nxy <= nyaw <= PS.MAX_PIECE_YAW
            else:
                assert r == 3.0 and nyaw > PS.MAX_PIECE_YAW, (nxy, r, nyaw)
            pts = np.concatenate([p["init_xy"][:, :1], p["end_xy"][:, :1], p["inner_xy"].reshape(2, -1)], axis=1)
            assert np.abs(pts).max() < 4.7
    for nxy in PS.NXY_ALL:
        path = PS.sweep_path(nxy)
        assert np.abs(path[:, :2]).max() < 4.7 and np.isfinite(path).all()
        assert np.abs(np.hypot(*np.diff(path[:, :2], axis=0).T) - PS.PATH_STEP).max() < 0.01 or nxy == 1
    # the ratios give what they are meant to: 1:1, ragged, two and three yaw pieces per position piece
    assert PS.pieces(PS.sweep_problem(60, 1.0)) == (60, 60) and PS.pieces(PS.sweep_problem(60, 2.0))[1] in (119, 120)
    assert PS.pieces(PS.sweep_problem(60, 3.0))[1] in (178, 179, 180) and 100 <= PS.pieces(PS.sweep_problem(60, 1.7))[1] <= 103
    # deterministic state with both PHR branches
    st, st2 = PS.sweep_state(PS.sweep_problem(20, 2.0), 5), PS.sweep_state(PS.sweep_problem(20, 2.0), 5)
    assert all(np.array_equal(st[k], st2[k]) for k in ("lam", "mu", "scale_cx"))
    assert 0.2 < (st["mu"] == 0.0).mean() < 0.4 and (st["mu"] >= 0.0).all()


@pytest.mark.parametrize("lanes", PS.LANE_COUNTS)
def test_chunk_class_coverage(lanes):
    """guards the sweep against becoming vacuous if the constants move: among Nxy = 1..128 -- and among the subsets the GPU tests use -- every
    chunking that exists at this lane count occurs (aligned AND plain at 64 and 128 lanes; at 256 and 512 lanes no trajectory within the
    compiled limit of 128 pieces has plain chunks, piece_sweep.chunkings_possible), with a straddling piece and a partial last chunk, every
    tile count of the MFMA scatter, and a partly empty last tile"""
    PS.assert_chunk_coverage(PS.NXY_ALL, lanes)
    PS.assert_chunk_coverage([n for n, r in PS.all_cases() if r == 3.0], lanes)          # (the shortest of the four ratio lists: Nxy <= 85)
    assert PS.chunkings_possible(64) == {True, False} and PS.chunkings_possible(128) == {True, False}
    assert PS.tiles_possible(64) == {1} and PS.tiles_possible(128) == {1, 2} and PS.tiles_possible(256) == {1, 2} and PS.tiles_possible(512) == {1, 2, 3, 4}
    # the examples of the constructor's comment: 39 pieces at 128 lanes are 6 chunks either way (aligned), 22 pieces keep the plain chunks (3 against 4)
    assert PS.chunk_class(39, 128)[:2] == (True, 6) and PS.chunk_class(22, 128)[:2] == (False, 3)
    # the vector path's other sample count (int_K = 8) has both chunkings at the two lane counts the GPU tier runs it with
    if lanes in (128, 512):
        assert {PS.chunk_class(n, lanes, 8)[0] for n in PS.NXY_ALL} == {True, False}
    # capped solves: n = 2 (Nxy - 1) + (Nyaw - 1) + 1 of the solve list crosses the register classes of the two-loop at 64, 128 and 256
    ns = sorted(2 * (a - 1) + b for a, b in (PS.pieces(PS.sweep_problem(n, 2.0)) for n in PS.SOLVE_NXY))
    for edge in (64, 128, 256):
        assert any(n <= edge for n in ns) and any(n > edge for n in ns) and max(n for n in ns if n <= edge) > edge - 8 and min(n for n in ns if n > edge) <= edge + 8
    assert ns[-1] > 500


@pytest.mark.parametrize("lanes", EMU_LANES)
def test_emu_single_evaluation_every_piece_count(oracle, oracle_grid, analytic_cells, lanes):
    """f, grad f, hx, gx, coefficients against the oracle for all Nxy x four ratios, random duals (30 % zero mu), scales, rho = 3, scale_fx = 0.37,
    at test_emu_terrain_eval_scaling's bar of 1e-10"""
    cases = PS.all_cases()
    ref = PS.oracle_evals(oracle, oracle_grid, cases)
    emu = _emu(oracle, analytic_cells)
    E.lib().emu_set_lanes(lanes)
    bad, errs = [], {}
    for c in cases:
        p, st = PS.sweep_problem(*c), PS.case_state(*c)
        r = emu.run(0, p, ref[c]["x0"], lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], rho=st["rho"], scale_fx=st["scale_fx"])
        e = PS.eval_errors(ref[c], r)
        errs[PS.pieces(p)] = e
        bad += [(lanes, PS.pieces(p), q, v) for q, v in e.items() if not v < 1e-10]
    E.lib().emu_set_lanes(256)
    print("emulator, %d lanes: worst" % lanes, PS.record("cpu_single_evaluation", lanes, errs))
    assert not bad, bad[:8]


@pytest.mark.parametrize("lanes", (128, 256))
def test_emu_single_evaluation_int_K_8(oracle, oracle_grid, analytic_cells, lanes):
    """nine samples per piece instead of 17 (other chunk classes: piece_sweep.chunk_class(n, lanes, 8)), ratio 2, every Nxy, at 1e-10"""
    cases = [c for c in PS.all_cases() if c[1] == 2.0]
    ref = PS.oracle_evals(oracle, oracle_grid, cases, int_K=8)
    emu = _emu(oracle, analytic_cells, dict(int_K=8.0))
    E.lib().emu_set_lanes(lanes)
    bad, errs = [], {}
    for c in cases:
        p, st = PS.sweep_problem(*c), PS.case_state(c[0], c[1], 8)
        r = emu.run(0, p, ref[c]["x0"], lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], rho=st["rho"], scale_fx=st["scale_fx"])
        e = PS.eval_errors(ref[c], r)
        errs[PS.pieces(p)] = e
        bad += [(lanes, PS.pieces(p), q, v) for q, v in e.items() if not v < 1e-10]
    E.lib().emu_set_lanes(256)
    print("emulator int_K = 8, %d lanes: worst" % lanes, PS.record("cpu_int_K_8", lanes, errs))
    assert not bad, bad[:8]


def test_emu_init_scaling_over_the_piece_counts(oracle, oracle_grid, analytic_cells):
    """initScaling, ratio 2, every fourth Nxy plus the solve list (the oracle's scaling is the slow part), lanes in turn, at 1e-10"""
    nxys = sorted(set(PS.NXY_ALL[::4]) | set(PS.SOLVE_NXY))
    cases = [(n, 2.0) for n in nxys]
    ref, ev = PS.oracle_scalings(oracle, oracle_grid, cases), PS.oracle_evals(oracle, oracle_grid, cases)
    emu = _emu(oracle, analytic_cells)
    bad, errs = [], {}
    for i, c in enumerate(cases):
        lanes = EMU_LANES[i % 3] if c[0] not in PS.SOLVE_NXY else None
        for ln in ([lanes] if lanes else EMU_LANES):
            E.lib().emu_set_lanes(ln)
            p = PS.sweep_problem(*c)
            r = emu.run(1, p, ev[c]["x0"])
            e = dict(scale_fx=PS.rel1(ref[c]["scale_fx"], r["scale_fx"]), scale_cx=PS.rel(ref[c]["scale_cx"], r["scale_cx"]))
            errs[PS.pieces(p) + (ln,)] = e
            bad += [(ln, PS.pieces(p), q, v) for q, v in e.items() if not v < 1e-10]
    E.lib().emu_set_lanes(256)
    print("emulator initScaling: worst", PS.record("cpu_init_scaling", "64/128/256", errs))
    assert not bad, bad[:8]


@pytest.mark.parametrize("lanes", EMU_LANES)
def test_emu_capped_solves(oracle, oracle_grid, analytic_cells, lanes):
    """two ALM passes of at most 12 L-BFGS iterations (inner_max_iter = 12, max_iter = 1) at the solve list, ratio 2: the state machine takes the
    oracle's decisions (return code, iteration and evaluation counts equal) and ends within 1e-7 of its x and cost"""
    cases = [(n, 2.0) for n in PS.SOLVE_NXY]
    ref, ev = PS.oracle_solves(oracle, oracle_grid, cases), PS.oracle_evals(oracle, oracle_grid, cases)
    emu = _emu(oracle, analytic_cells, PS.SOLVE_PARAMS)
    E.lib().emu_set_lanes(lanes)
    bad, errs = [], {}
    for c in cases:
        p, ro = PS.sweep_problem(*c), ref[c]
        r = emu.run(2, p, ev[c]["x0"])
        if (r["ret"], r["lbfgs_iters"], r["evals"]) != (ro["ret"], ro["lbfgs_iters"], ro["evals"]):
            bad.append((lanes, PS.pieces(p), "counters", (r["ret"], r["lbfgs_iters"], r["evals"]), (ro["ret"], ro["lbfgs_iters"], ro["evals"])))
        e = dict(x=PS.rel(ro["x"], r["x"]), cost=PS.rel1(ro["cost"], r["f"]))
        errs[PS.pieces(p)] = e
        bad += [(lanes, PS.pieces(p), q, v) for q, v in e.items() if not v < 1e-7]
    E.lib().emu_set_lanes(256)
    print("emulator capped solves, %d lanes: worst" % lanes, PS.record("cpu_capped_solves", lanes, errs))
    assert not bad, bad[:8]


@pytest.mark.parametrize("lanes", EMU_LANES)
def test_emu_report_every_piece_count(oracle, oracle_grid, analytic_cells, lanes):
    """Solver::report (the sample count by wg.sum, about 70 samples per piece reduced by wg.sumMax) after ONE evaluation at x0, ratio 2 at every Nxy
    plus the ragged ratio 1.7 at the solve list: the emulator's seven values against the oracle's report on the emulator's own coefficients, at the
    device's bar (test_gpu_parity::test_report_matches_oracle_on_same_trajectory: columns 0-5 rtol 1e-9 / atol 1e-12, column 6 1e-9 max(1, ref))"""
    cases = [c for c in PS.all_cases() if c[1] == 2.0] + [(n, 1.7) for n in PS.SOLVE_NXY]
    assert [c[0] for c in cases[:len(PS.NXY_ALL)]] == PS.NXY_ALL and set(cases) <= set(PS.all_cases())
    ev = PS.oracle_evals(oracle, oracle_grid, cases)
    emu = _emu(oracle, analytic_cells)
    E.lib().emu_set_lanes(lanes)
    got = {}
    for c in cases:
        st = PS.case_state(*c)
        got[c] = emu.eval_report(PS.sweep_problem(*c), ev[c]["x0"], lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], rho=st["rho"], scale_fx=st["scale_fx"])
    E.lib().emu_set_lanes(256)
    ref = PS.oracle_reports(oracle, oracle_grid, got, "emu%d" % lanes)
    bad, errs = [], {}
    for c in cases:
        where = PS.pieces(PS.sweep_problem(*c)) + (c[1],)
        assert np.isfinite(got[c]["report"]).all() and got[c]["report"][0] > 0.0 and got[c]["report"][6] > 0.0, (lanes, where, got[c]["report"])
        e = PS.report_errors(ref[c], got[c]["report"])
        errs[where] = e
        bad += [(lanes, where, q, v) for q, v in e.items() if not v < 1e-9]
    print("emulator report, %d lanes: worst" % lanes, PS.record("cpu_report", lanes, errs))
    assert not bad, bad[:8]
