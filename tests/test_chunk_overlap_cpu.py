"""The chunk loop of Solver::eval with the sample pass in two parts, host path: the emulator's workgroup object has no
sampleChunk of its own, so it runs the default of solver_program.hpp -- compute and commit back to back per task, then accChunk's end -- and the
barrier-free scatter through the default pforOpen.  The default build and the build with -DUPH_CHUNK_OVERLAP=0 (the loop as it was: sampleEval,
scatterChunk) run the same operations on the same operands: one evaluation, initScaling, a residual refresh followed by an evaluation and the
capped solve of tests/test_pieces_cpu.py agree bit for bit, at 64, 128 and 256 lanes, for int_K = 16 and 8 (the vector scatter), at piece counts
with one chunk, aligned and plain chunks, a straddling piece and up to six chunks.  The capped solve is also held to the oracle at
test_pieces_cpu::test_emu_capped_solves' bars (the oracle's counters, x and the cost within 1e-7)."""
import numpy as np
import pytest

import emu_bridge as E
import piece_sweep as PS

LANES = (64, 128, 256)
NXYS = (1, 7, 8, 15, 22, 43)
CASES = [(n, r) for r in (1.0, 2.0) for n in NXYS]
REFRESH_PARAMS = dict(inner_max_iter=1.0, max_iter=1.0)       # pass 1: x0 + one search, refresh, dual update; pass 2 starts with an evaluation
ARRAYS = ("x", "g", "hx", "gx", "lam", "mu", "scale_cx", "c_xy", "c_yaw")
SCALARS = ("f", "jerk_cost", "T_xy", "T_yaw", "rho", "scale_fx", "ret", "alm_iters", "lbfgs_iters", "evals", "last_lbfgs_ret")
OFF = ("-DUPH_CHUNK_OVERLAP=0",)


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


def test_cases_reach_every_shape_of_the_chunk_loop():
    """one chunk (no barrier between compute and commit), several chunks, aligned and plain chunkings, a chunk that touches more pieces than fit
    whole (a straddling piece), for both sample counts per piece"""
    for K in (16, 8):
        for lanes in LANES:
            cls = [PS.chunk_class(n, lanes, K) for n in NXYS]
            assert any(c[1] == 1 for c in cls) and any(c[1] >= 2 for c in cls), (K, lanes)
    for lanes in (64, 128):                          # (int_K = 8 and 256 lanes have aligned chunks at every one of these piece counts)
        cls = [PS.chunk_class(n, lanes) for n in NXYS]
        assert {c[0] for c in cls} == {True, False}, lanes
        assert any(not c[0] and c[1] > 1 and c[2] > lanes // 17 + 1 for c in cls), lanes      # a plain chunk that begins and ends inside a piece
    assert PS.chunk_class(43, 128)[1] == 6 and PS.chunk_class(22, 128)[2:] == (9, 2)


@pytest.mark.parametrize("int_K", (16, 8))
@pytest.mark.parametrize("lanes", LANES)
def test_emu_equals_the_build_with_the_loop_as_it_was(oracle, oracle_grid, analytic_cells, lanes, int_K):
    """default against -DUPH_CHUNK_OVERLAP=0, bit for bit: one evaluation, initScaling, refresh then evaluation, the capped solve; and the capped
    solve takes the oracle's decisions with x and the cost within 1e-7"""
    ev = PS.oracle_evals(oracle, oracle_grid, CASES, int_K=int_K)
    ref = PS._fill("chunk_overlap_solve", int(int_K), CASES,
                   lambda case: oracle.OracleALM(oracle_grid, _params(int_K, PS.SOLVE_PARAMS)).optimize(PS.sweep_problem(*case)))
    mp = oracle.map_params_vec()
    bad = []
    for name, params in (("capped", PS.SOLVE_PARAMS), ("refresh", REFRESH_PARAMS)):
        op = oracle.params_vec(_params(int_K, params))
        new, old = E.Emu(analytic_cells, mp, op), E.Emu(analytic_cells, mp, op, flags=OFF)
        try:
            for L in (new.L, old.L):
                L.emu_set_lanes(lanes)
            for c in CASES:
                p, st = PS.sweep_problem(*c), PS.case_state(c[0], c[1], int_K)
                x0 = ev[c]["x0"]
                r = new.run(2, p, x0)
                _same(r, old.run(2, p, x0), (name, lanes, int_K, c))
                if name != "capped":
                    continue
                kw = dict(lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], rho=st["rho"], scale_fx=st["scale_fx"])
                _same(new.run(0, p, x0, **kw), old.run(0, p, x0, **kw), ("eval", lanes, int_K, c))
                _same(new.run(1, p, x0), old.run(1, p, x0), ("scaling", lanes, int_K, c))
                ro = ref[c]
                if (r["ret"], r["lbfgs_iters"], r["evals"]) != (ro["ret"], ro["lbfgs_iters"], ro["evals"]):
                    bad.append((lanes, int_K, PS.pieces(p), "counters", (r["ret"], r["lbfgs_iters"], r["evals"]), (ro["ret"], ro["lbfgs_iters"], ro["evals"])))
                e = dict(x=PS.rel(ro["x"], r["x"]), cost=PS.rel1(ro["cost"], r["f"]))
                print("capped lanes %d K %d %s evals %d %s" % (lanes, int_K, PS.pieces(p), r["evals"], {k: "%.1e" % v for k, v in e.items()}))
                bad += [(lanes, int_K, PS.pieces(p), q, v) for q, v in e.items() if not v < 1e-7]
        finally:
            for L in (new.L, old.L):
                L.emu_set_lanes(256)
    assert not bad, bad[:8]
