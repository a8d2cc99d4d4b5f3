"""Sweep over every position piece count and yaw ratio for the solve / scaling / penalty kernels (TEST INFRASTRUCTURE).

The workgroup program (uneven_planner_amd/csrc/solver_program.hpp) branches on the pair (position pieces Nxy, lanes per trajectory CH):
aligned or plain sample chunks, one to four MFMA scatter tiles with a partly empty last one, pieces straddling two chunks, the L-BFGS
register classes at n = 64, 128, 256.  This module generates one problem for EVERY Nxy in 1..128 at the yaw ratios 1, 1.7, 2 and 3 (a slice
of one winding curve), deterministic duals / scales for them, and the oracle's answers -- computed once per process and shared by
tests/test_pieces_cpu.py (the emulator) and tests/test_gpu_pieces.py (the device through the C-ABI), like tests/forced_cases.py is shared
by the forced-state tests.  No fixtures here: the callers hand in the `oracle` module and its grid.

For the kernels that read a finished trajectory back (report, rollout, states at given times, check, refine staging: tests/test_gpu_resident_sweep.py
and the emulator's report in tests/test_pieces_cpu.py) it also holds the references: the oracle's report on handed-in coefficients
(oracle_reports) and plain numpy restatements of the trajectory evaluation and of the report's rule (ref_states, ref_terms, report_from_terms).
"""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

NXY_ALL = list(range(1, 129))                   # 1 .. UPH_MAX_PIECE_XY
RATIOS = (1.0, 1.7, 2.0, 3.0)                   # yaw pieces per position piece: 1:1, ragged, PlanManager's 2, the test node's 3
MAX_PIECE_YAW = 256                             # UPH_MAX_PIECE_YAW
# capped solves: every small count, the neighbours of the chunk / tile / knot-table (THOMAS_J = 26) boundaries, and -- at ratio 2, n = 4 Nxy - 3 --
# n crossing 64 (Nxy 16 | 17), 128 (32 | 33), 256 (64 | 65) and the largest n = 509
SOLVE_NXY = [1, 2, 3, 4, 8, 9, 16, 17, 18, 26, 27, 28, 32, 33, 43, 44, 64, 65, 86, 87, 127, 128]
SOLVE_PARAMS = dict(inner_max_iter=12.0, max_iter=1.0)
RHO, SCALE_FX = 3.0, 0.37                       # of the single evaluation and the penalty call
PIECE_LEN, PATH_STEP = 0.3, 0.06
MIN_CASES = 440

_LOCK = threading.Lock()
_CACHE = {}
COST_RAW = {}                                   # (test, variant) -> {(Nxy, Nyaw): dict(cost_raw, oracle_jump)}: the capped solves' cost of every case as measured
MEASURED = {}                                   # (test, variant) -> {quantity: (worst error, where)}: filled by record(), written by write_report()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(a).max()))


def rel1(ref, got):
    return float(abs(got - ref) / max(1e-300, abs(ref)))


# ---- generator ----------------------------------------------------------------------------------------------------------------------------
def _curve():
    """y = -0.5 + 3.2 sin(3.3 x), x in [-4.6, 4.6], as a fine polyline with its running arc length (61.98 m in all)"""
    if "curve" not in _CACHE:
        x = np.linspace(-4.6, 4.6, 40001)
        y = -0.5 + 3.2 * np.sin(3.3 * x)
        arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
        _CACHE["curve"] = (x, y, arc)
    return _CACHE["curve"]


def sweep_path(nxy):
    """the first 0.3 (nxy - 0.5) metres of the curve sampled every 0.06 m like a front-end path; yaw = unwrapped tangent"""
    x, y, arc = _curve()
    length = PIECE_LEN * (nxy - 0.5)
    assert length < arc[-1]
    sq = np.linspace(0.0, length, max(2, int(round(length / PATH_STEP)) + 1))
    xs, ys = np.interp(sq, arc, x), np.interp(sq, arc, y)
    yaw = np.unwrap(np.arctan2(np.gradient(ys), np.gradient(xs)))
    return np.column_stack([xs, ys, yaw])


def sweep_problem(nxy, ratio, int_K=16):
    """the optimizeSE2Traj arguments of the sweep's problem with `nxy` position pieces and `ratio` yaw pieces per position piece
    (int_K does not enter the resampling stage; it is accepted so that callers can pass one key everywhere)"""
    key = ("prob", int(nxy), float(ratio))
    if key not in _CACHE:
        from uneven_planner_amd import resample
        _CACHE[key] = resample.resample_path(sweep_path(nxy), piece_len=PIECE_LEN, yaw_piece_times=float(ratio))
    return _CACHE[key]


def pieces(prob):
    return prob["inner_xy"].shape[1] + 1, prob["inner_yaw"].shape[0] + 1


def sweep_cases(ratios=RATIOS, nxys=NXY_ALL):
    """the (nxy, ratio) pairs of the sweep.  A pair is left out only when its problem lies outside the compiled limits: Nyaw > 256 (ratio 3
    above Nxy = 85) or Nyaw < Nxy.  Everything else must be there, and the generator must be exact."""
    out = []
    for r in ratios:
        for nxy in nxys:
            got, nyaw = pieces(sweep_problem(nxy, r))
            assert got == nxy, ("the generator missed the requested piece count", nxy, r, got)
            if nyaw > MAX_PIECE_YAW or nyaw < nxy:
                continue
            out.append((nxy, r))
    return out


def all_cases():
    if "cases" not in _CACHE:
        c = sweep_cases()
        assert len(c) >= MIN_CASES, len(c)
        _CACHE["cases"] = c
    return _CACHE["cases"]


def sweep_state(problem, seed, int_K=16):
    """deterministic duals and scales for one problem: lambda ~ 0.1 N(0, 1); mu >= 0 with about 30 % exact zeros (both branches of the PHR
    penalty occur); constraint scales in [0.2, 1]"""
    rng = np.random.default_rng(int(seed))
    S = pieces(problem)[0] * (int(int_K) + 1)
    lam = rng.normal(size=S) * 0.1
    mu = np.abs(rng.normal(size=6 * S)) * 0.1 * (rng.uniform(size=6 * S) < 0.7)
    sc = rng.uniform(0.2, 1.0, size=7 * S)
    return dict(lam=lam, mu=mu, scale_cx=sc, scale_fx=SCALE_FX, rho=RHO)


def case_seed(nxy, ratio):
    return 100000 + 1000 * int(round(10 * ratio)) + int(nxy)


def case_state(nxy, ratio, int_K=16):
    key = ("state", int(nxy), float(ratio), int(int_K))
    if key not in _CACHE:
        _CACHE[key] = sweep_state(sweep_problem(nxy, ratio), case_seed(nxy, ratio), int_K)
    return _CACHE[key]


# ---- which code path a (piece count, lane count) pair takes -------------------------------------------------------------------------------
LANE_COUNTS = (64, 128, 256, 512)


def chunk_class(nxy, lanes, K=16):
    """Restates the constructor of Solver (solver_program.hpp, "Chunks of whole pieces where that costs no extra chunk") and the tile count of
    DevWG::scatterXY17: returns (aligned, n_chunks, max pieces touched by one chunk, max 16-column MFMA tiles of one chunk).  For COVERAGE
    assertions only -- never an expected value of a result."""
    K1 = K + 1
    S = nxy * K1
    ppc = lanes // K1
    aligned = ppc >= 1 and (nxy + ppc - 1) // ppc == (S + lanes - 1) // lanes
    chs = ppc * K1 if aligned else lanes
    n_chunks, pmax = 0, 0
    for s0 in range(0, S, chs):
        cnt = min(S - s0, chs)
        pmax = max(pmax, (s0 + cnt - 1) // K1 - s0 // K1 + 1)
        n_chunks += 1
    return bool(aligned), n_chunks, pmax, (2 * pmax + 15) // 16


def tiles_possible(lanes, K=16):
    """every tile count a chunk of `lanes` record slots can need: a window of CH consecutive samples touches at most floor((CH - 2) / (K + 1)) + 2
    pieces of K + 1 samples (5 at 64 lanes, 9 at 128, 16 at 256, 32 at 512), fewer for short trajectories"""
    pmax = (lanes - 2) // (K + 1) + 2
    return {(2 * p + 15) // 16 for p in range(1, pmax + 1)}


def chunkings_possible(lanes, K=16):
    """which chunkings exist at all within the compiled limit of 128 pieces.  The plain chunking needs ceil(Nxy / ppc) > ceil(Nxy (K + 1) / CH),
    ppc = floor(CH / (K + 1)): for K = 16 that happens at 64 lanes (ppc 3 against 3.76 pieces per chunk) and at 128 lanes (7 against 7.53), but
    never at 256 (15 against 15.06) or 512 lanes (30 against 30.12) below Nxy = 241 -- there every trajectory the library accepts has aligned chunks."""
    return {chunk_class(n, lanes, K)[0] for n in NXY_ALL}


def assert_chunk_coverage(nxys, lanes, K=16):
    """the piece counts `nxys` reach, at this lane count, every chunking that exists (with a piece straddling two chunks and a partial last chunk
    where the plain one does), every tile count, and a partly empty last tile"""
    cls = [chunk_class(n, lanes, K) for n in nxys]
    assert {c[0] for c in cls} == chunkings_possible(lanes, K), ("chunkings", lanes, K)
    assert {c[3] for c in cls} == tiles_possible(lanes, K), ("tile counts", lanes, sorted({c[3] for c in cls}), sorted(tiles_possible(lanes, K)))
    assert any((2 * c[2]) % 16 != 0 for c in cls), ("no partly empty last tile", lanes)
    if False in chunkings_possible(lanes, K):
        K1 = K + 1
        plain = [n for n, c in zip(nxys, cls) if not c[0] and c[1] > 1]
        # plain chunks start at multiples of the lane count, which is no multiple of K + 1: the second chunk begins inside a piece
        assert plain and lanes % K1 != 0, ("no multi-chunk plain chunking: no piece straddles two chunks", lanes)
        assert any((n * K1) % lanes != 0 for n in plain), ("no partial last chunk", lanes)


# ---- the oracle's answers, once per process -----------------------------------------------------------------------------------------------
def _threads():
    return max(1, min(8, os.cpu_count() or 1))


def _fill(kind, tag, keys, make):
    """compute the missing entries (kind, tag, key) of the cache with make(key) on a few host threads (the oracle's C entry points release the
    GIL; every evaluation has its own OracleALM, the grid is only read); entries are never recomputed and never modified afterwards"""
    with _LOCK:
        todo = [k for k in keys if (kind, tag, k) not in _CACHE]
        if todo:
            for k in todo:                       # the resampler's output is cached from one thread only
                sweep_problem(*k)
            with ThreadPoolExecutor(max_workers=_threads()) as ex:
                for k, v in zip(todo, ex.map(make, todo)):
                    _CACHE[(kind, tag, k)] = v
    return {k: _CACHE[(kind, tag, k)] for k in keys}


def _params(int_K, extra=None):
    p = dict(extra or {})
    if int_K != 16:
        p["int_K"] = float(int_K)
    return p or None


def oracle_evals(O, og, cases, int_K=16, tag="f64"):
    """one innerCallback evaluation at x0 with case_state() per case, and calConstrainCostGrad alone at the same point: dict case ->
    dict(x0, f, g, hx, gx, c_xy, c_yaw, T_xy, T_yaw, pen_cost, gdCxy, gdCyaw, gdTxy, gdTyaw, pen_hx, pen_gx).  `tag` names the grid `og` in the cache."""
    def make(case):
        p, st = sweep_problem(*case), case_state(case[0], case[1], int_K)
        a = O.OracleALM(og, _params(int_K))
        x0 = a.setup(p)
        a.set_state(lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], scale_fx=st["scale_fx"])
        a.set_rho(st["rho"])
        f, g, _ = a.eval(x0)
        s = a.get_state()
        cxy, cyaw, txy, tyaw, _ = a.coeffs()
        cost, gcx, gtx, gcy, gty = a.constrain(x0)
        s2 = a.get_state()
        return dict(x0=x0, f=f, g=g, hx=s["hx"], gx=s["gx"], c_xy=cxy, c_yaw=cyaw, T_xy=txy, T_yaw=tyaw, pen_cost=cost, gdCxy=gcx, gdCyaw=gcy,
                    gdTxy=gtx, gdTyaw=gty, pen_hx=s2["hx"], pen_gx=s2["gx"])
    return _fill("eval", (tag, int(int_K)), list(cases), make)


def oracle_scalings(O, og, cases, tag="f64"):
    """initScaling at x0 per case: dict case -> dict(scale_fx, scale_cx)"""
    def make(case):
        a = O.OracleALM(og)
        a.init_scaling(a.setup(sweep_problem(*case)))
        s = a.get_state()
        return dict(scale_fx=s["scale_fx"], scale_cx=s["scale_cx"])
    return _fill("scaling", tag, list(cases), make)


def oracle_solves(O, og, cases, tag="f64"):
    """the capped solve (SOLVE_PARAMS: two ALM passes of at most 12 L-BFGS iterations each, rho = 1) per case: dict case -> OracleALM.optimize's dict"""
    def make(case):
        return O.OracleALM(og, SOLVE_PARAMS).optimize(sweep_problem(*case))
    return _fill("solve", tag, list(cases), make)


def oracle_reports(O, og, coeffs_by_case, tag):
    """getMaxVxAxAyCurAttSig + the non-holonomic error of the oracle on HANDED-IN trajectories: coeffs_by_case = {case: dict with c_xy, c_yaw,
    T_xy, T_yaw} (a device's or the emulator's downloaded ones, as test_gpu_parity::test_report_matches_oracle_on_same_trajectory hands them
    over); dict case -> the seven values.  `tag` names whose coefficients these are (the kernel variant): they differ at rounding level
    between variants, so every variant has its own cache entries."""
    def make(case):
        d = coeffs_by_case[case]
        a = O.OracleALM(og)
        a.setup(sweep_problem(*case))
        a.set_coeffs(d["c_xy"], d["c_yaw"], d["T_xy"], d["T_yaw"])
        return a.report()
    return _fill("report", str(tag), list(coeffs_by_case), make)


# ---- the clearance term over the sweep (tests/test_clearance_sweep_cpu.py, tests/test_gpu_clearance_sweep.py) -----------------------------
# The layer: hand-set body bytes on the sweep's 200 x 200 x 64 grid, a lattice that shifts every fourth yaw slice (reading the wrong slice changes the
# answer), its distance transform truncated at CLR_RMAX cells.  CLR_WEIGHT: the sweep's objective at x0 is jerk-dominated (f 1e5 .. 6e7); the weight is
# the one at which the term is a tenth or more of every case's f and of its largest gdCxy entry (asserted by the CPU tier from the oracle and the mirror).
CLR_DIMS = (200, 200, 64)
CLR_LATTICE = (7, 11, 5, 251)
CLR_RMAX, CLR_D_SAFE, CLR_WEIGHT = 12, 0.3, 1.0e9
CLR_SOLVE_WEIGHT = 1.0e9                        # of the capped solves (scale_fx is initScaling's there; the term carries it like the jerk cost does)
CLR_SOLVE_LEFT_OUT = ()                         # solve cases unfit to test (solve_fitness; test_clearance_sweep_cpu asserts this is what it finds): none
CLR_GEOM = (np.array([-5.0, -5.0, -(2.0 * np.pi + 5e-2) / 2.0]), 0.05, 0.1)      # (origin, res, yaw_res) of the sweep's 10 m x 10 m grid: clearance.layer_geometry's form


def _key_of(D):
    """cache key of a layer's values: shape and a digest of the bytes (two arrays with the same values share their answers; no stale entry for a new array)"""
    import hashlib
    D = np.ascontiguousarray(D)
    return (D.shape, hashlib.sha1(D.tobytes()).hexdigest())


def lattice_body(dims=CLR_DIMS, lattice=CLR_LATTICE):
    """body bytes [nx][ny][nyaw]: 1 where (a ix + b iy + c (iw // 4)) % m == 0"""
    a, b, c, m = lattice
    ix, iy, iw = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), np.arange(dims[2]), indexing="ij")
    return (((a * ix + b * iy + c * (iw // 4)) % m) == 0).astype(np.uint8)


def clearance_layer(dims=CLR_DIMS, lattice=CLR_LATTICE, rmax=CLR_RMAX):
    """the layer's values D [nx][ny][nyaw] by the host mirror of the distance transform (the device's layer.get() must equal it: the GPU tier asserts that)"""
    key = ("clr_layer", tuple(dims), tuple(lattice), int(rmax))
    with _LOCK:
        if key not in _CACHE:
            from uneven_planner_amd.clearance import clearance_rows
            D = np.ascontiguousarray(clearance_rows(lattice_body(dims, lattice), rmax), dtype=np.uint16)
            D.setflags(write=False)
            _CACHE[key] = D
    return _CACHE[key]


def sample_poses(c_xy, c_yaw, T_xy, T_yaw, K=16):
    """x, y and the normalised yaw at the quadrature samples of a trajectory given by its coefficients, at the reference's sample times (running sums
    s1 += T_xy / K, base += T_xy; yaw piece min(int((s1 + base) / T_yaw), Nyaw - 1)): (Nxy, K + 1, 3).  For the generator conditions only."""
    cx = np.asarray(c_xy, dtype=np.float64).reshape(-1, 6, 2)
    cw = np.asarray(c_yaw, dtype=np.float64).reshape(-1, 6)
    Nxy, Nyaw = cx.shape[0], cw.shape[0]
    s1 = np.array([running_sum(T_xy / K, j) for j in range(K + 1)])
    base = np.array([running_sum(T_xy, i) for i in range(Nxy)])
    pw = np.stack([s1 ** k for k in range(6)], axis=1)
    pos = np.einsum("jk,ikd->ijd", pw, cx)
    now = s1[None, :] + base[:, None]
    yi = np.clip((now / T_yaw).astype(np.int64), 0, Nyaw - 1)
    u = now - yi * T_yaw
    yaw = sum(cw[yi][..., k] * u ** k for k in range(6))
    return np.concatenate([pos, norm_so2(yaw).reshape(Nxy, K + 1, 1)], axis=2)


def term_rows(O, og, cases, D, term, geometry, int_K=16, tag="f64"):
    """the mirror's rows (uneven_planner_amd.clearance.clearance_term_rows) of the term at the oracle's own coefficients at x0, per case, and the poses
    of the samples: dict case -> dict(rows, poses).  term = (rmax, d_safe, weight); geometry = (origin, res, yaw_res)"""
    from uneven_planner_amd.clearance import clearance_term_rows
    ev = oracle_evals(O, og, cases, int_K, tag)
    rmax, d_safe, weight = term

    def make(case):
        e, st = ev[case], case_state(case[0], case[1], int_K)
        rows = clearance_term_rows(D, geometry, rmax, d_safe, weight, e["c_xy"], e["c_yaw"], e["T_xy"], e["T_yaw"], int_K, st["scale_fx"])
        return dict(rows=rows, poses=sample_poses(e["c_xy"], e["c_yaw"], e["T_xy"], e["T_yaw"], int_K))
    return _fill("clr_rows", (tag, int(int_K), _key_of(D), tuple(term)), list(cases), make)


def oracle_eval_one(O, og, p, st, D=None, term=None, int_K=16):
    """oracle_evals' answers for ONE problem p with the state st (sweep_state's dict), with the clearance term (D, term = (rmax, d_safe, weight)) or without"""
    a = O.OracleALM(og, _params(int_K))
    x0 = a.setup(p)
    if term is not None:
        a.set_clearance_term(D, *term)
    a.set_state(lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], scale_fx=st["scale_fx"])
    a.set_rho(st["rho"])
    f, g, _ = a.eval(x0)
    s = a.get_state()
    cxy, cyaw, txy, tyaw, _ = a.coeffs()
    cost, gcx, gtx, gcy, gty = a.constrain(x0)
    s2 = a.get_state()
    return dict(x0=x0, f=f, g=g, hx=s["hx"], gx=s["gx"], c_xy=cxy, c_yaw=cyaw, T_xy=txy, T_yaw=tyaw, pen_cost=cost, gdCxy=gcx, gdCyaw=gcy,
                gdTxy=gtx, gdTyaw=gty, pen_hx=s2["hx"], pen_gx=s2["gx"])


def oracle_evals_term(O, og, cases, D, term, int_K=16, tag="f64"):
    """oracle_evals with the clearance term set: term = (rmax, d_safe, weight), D the layer's values (the caller keeps the array: the cache is keyed by it)"""
    def make(case):
        return oracle_eval_one(O, og, sweep_problem(*case), case_state(case[0], case[1], int_K), D, term, int_K)
    return _fill("eval_term", (tag, int(int_K), _key_of(D), tuple(term)), list(cases), make)


def solve_fitness(O, og, cells, D, term, nxys=None):
    """Each solve case (ratio 2) solved by the oracle four times: with and without the term, in the default build and in the -DORACLE_EIGEN_REDUX=1 build.
    dict nxy -> dict(counters_on, counters_off: the two builds agree in ret / lbfgs_iters / evals; dx_on, dx_off: their x apart (relative, infinity norm);
    dcost_on, dcost_off: their returned costs apart; cost_jump: cost_jumps' figure of the default build; moved: x(on) against x(off) in the default build; fit: counters_on and dx_on <= max(10 dx_off, 1e-7))"""
    key = ("clr_fitness", _key_of(D), _key_of(cells), tuple(term), tuple(nxys or SOLVE_NXY))
    if key not in _CACHE:
        cases = [(n, 2.0) for n in (nxys or SOLVE_NXY)]
        on, off = oracle_solves_term(O, og, cases, D, term), oracle_solves_term(O, og, cases, D, None)
        import sensitivity
        with sensitivity.fma_session(*sensitivity.fma_session.EIGEN_ORDER) as F:
            fg = F.OracleGrid()
            fg.set_cells(cells)
            eon, eoff = oracle_solves_term(F, fg, cases, D, term, tag="eig"), oracle_solves_term(F, fg, cases, D, None, tag="eig")
        same = lambda a, b: all(a[k] == b[k] for k in ("ret", "lbfgs_iters", "evals"))
        jump = cost_jumps(O, og, cases, D, term)
        out = {}
        for c in cases:
            r = dict(counters_on=same(on[c], eon[c]), counters_off=same(off[c], eoff[c]), dx_on=rel(on[c]["x"], eon[c]["x"]), dx_off=rel(off[c]["x"], eoff[c]["x"]),
                     moved=rel(off[c]["x"], on[c]["x"]), dcost_on=rel1(on[c]["cost"], eon[c]["cost"]), dcost_off=rel1(off[c]["cost"], eoff[c]["cost"]),
                     cost_jump=jump[c])
            r["fit"] = bool(r["counters_on"] and r["dx_on"] <= max(10.0 * r["dx_off"], 1e-7))
            out[c[0]] = r
        _CACHE[key] = out
    return _CACHE[key]


def cost_jumps(O, og, cases, D, term, tag="f64"):
    """How far the oracle's own returned cost is from being a function of the returned x, per solve case: dict case -> relative jump (0.0 where the last
    L-BFGS pass did not end in a failed line search).

    After a failed line search (LBFGSERR_MAXIMUMLINESEARCH and its kin) lbfgs_optimize restores x and returns f at the search's last REJECTED trial
    xp + stp d.  With the term, f is discontinuous -- the field is piecewise constant in yaw, f jumps where a sample's yaw crosses a slice edge across which
    the layer differs -- and a search that bisects 64 times without meeting the Armijo test has converged onto such a jump: the side the last trial falls on
    is rounding.  The jump is MEASURED here with the oracle alone: the failing iteration's state is captured (set_capture), its line search is replayed with
    the oracle's evaluation (lbfgs.hpp:276-389 restated; the replay's last f must BE the solve's returned cost, bit for bit), and f is evaluated at
    xp + stp (1 -+ 2^-30) d.  For a continuous f the two differ by about 2^-29 stp |g . d|; the measured relative difference is the reference's own error
    of that cost, and the solve tests add it to their bar for the cost of that case (x and the counters keep their bars everywhere)."""
    def make(case):
        p = sweep_problem(*case)

        def fresh():
            a = O.OracleALM(og, SOLVE_PARAMS)
            if term is not None:
                a.set_clearance_term(D, *term)
            return a
        a = fresh()
        a.set_capture(-1, -1, True)
        r = a.optimize(p)
        if not (r["last_lbfgs_ret"] < 0 and r["last_lbfgs_ret"] != -1008):
            return 0.0
        log = a.iter_log()
        assert log[-1][2] == r["last_lbfgs_ret"]
        b = fresh()
        b.set_capture(int(log[-1][0]), int(log[-1][1]), True)
        b.optimize(p)
        st = b.capture()
        assert st is not None
        c = fresh()
        c.init_scaling(c.setup(p))
        c.set_state(lam=st["lam"], mu=st["mu"])
        c.set_rho(st["rho"])
        prm = dict(zip(O.PARAM_ORDER, c.pv))
        xp, d, stp, finit = st["x"], st["d"], st["step"], st["fx"]
        dginit = float(np.dot(st["g"], d))
        dgtest, dstest = 1e-4 * dginit, 0.9 * dginit
        mu_, nu, brackt, f = 0.0, 1e20, False, None
        for count in range(1, 65):
            f, g, _ = c.eval(xp + stp * d)
            assert not (prm["past"] > 0 and abs(finit - f) / (abs(finit) + 1.0) < prm["delta"] / prm["past"])
            if f > finit + stp * dgtest:
                nu, brackt = stp, True
            else:
                assert float(np.dot(g, d)) < dstest
                mu_ = stp
            if count == 64:
                break
            stp = 0.5 * (mu_ + nu) if brackt else stp * 2.0
        assert f == r["cost"], ("the replayed line search does not end where the solve did", case, f, r["cost"])
        h = 2.0 ** -30
        lo, hi = c.eval(xp + stp * (1.0 - h) * d)[0], c.eval(xp + stp * (1.0 + h) * d)[0]
        return float(abs(hi - lo) / abs(r["cost"]))
    return _fill("clr_cost_jump", (tag, _key_of(D), None if term is None else tuple(term)), list(cases), make)


def cost_error(ref_cost, got_cost, jump):
    """the relative error of a solve's returned cost, allowing for the reference's own jump (cost_jumps): the cost may lie on either side of it, so the error is
    the smaller of |d| and | |d| - jump |.  With jump = 0 it is rel1."""
    e = rel1(ref_cost, got_cost)
    return float(min(e, abs(e - jump)))


def oracle_solves_term(O, og, cases, D, term, tag="f64"):
    """oracle_solves with the clearance term set (term = (rmax, d_safe, weight); None: the plain solve through the same entry)"""
    def make(case):
        a = O.OracleALM(og, SOLVE_PARAMS)
        if term is not None:
            a.set_clearance_term(D, *term)
        return a.optimize(sweep_problem(*case))
    return _fill("solve_term", (tag, _key_of(D), None if term is None else tuple(term)), list(cases), make)


# ---- plain references of the kernels that read a resident trajectory back ------------------------------------------------------------------
STATE_COLS = ("x", "y", "dx", "dy", "ddx", "ddy", "yaw_norm", "dyaw", "ddyaw", "yaw")      # uph_traj_states' columns
ROW_OF_STATE = [0, 1, 6, 2, 3, 4, 5, 7]         # ref_states' columns in the order of a rollout row's x y yaw dx dy ddx ddy dyaw


def running_sum(step, n):
    """the value after n additions of `step` to 0.0, one rounding per addition (how the reference and the library form durations)"""
    t = 0.0
    for _ in range(int(n)):
        t += step
    return t


def total_duration(T_xy, T_yaw, Nxy, Nyaw):
    """SE2Trajectory::getTotalDuration as the library documents it: the two running sums of the piece durations, the smaller one"""
    dx, dy = running_sum(float(T_xy), Nxy), running_sum(float(T_yaw), Nyaw)
    return dx if dx < dy else dy


def time_table(dt, total):
    """t_q of `for (t = 0; t < total; t += dt)`: every t_q < total and the first one at or beyond it (the running sum, never q * dt)"""
    out, t = [0.0], 0.0
    while t < total:
        t += dt
        out.append(t)
    return np.array(out)


def _locate(T, N, t):
    """PolyTrajectory::locatePieceIdx (se2traj.hpp:343-361) with uniform durations, in double, by repeated subtraction, with the i == N fall-back --
    over an array of times.  The decision is discrete: it is restated, not improved."""
    T = float(T)
    tl = np.array(t, dtype=np.float64).reshape(-1).copy()
    idx = np.zeros(tl.shape[0], dtype=np.int64)
    act = np.nonzero(tl > T)[0] if N > 0 else np.zeros(0, dtype=np.int64)
    for _ in range(int(N)):
        if act.size == 0:
            break
        tl[act] -= T
        idx[act] += 1
        act = act[tl[act] > T]
    end = idx == N
    idx[end] -= 1
    tl[end] += T
    return idx, tl


def _quintic(c6, tl):
    """value, first and second derivative of sum_k c6[:, k] tl^k by Horner in np.longdouble, rounded to double once at the end"""
    c = np.asarray(c6, dtype=np.longdouble)
    x = np.asarray(tl, dtype=np.longdouble)
    v = c[:, 5]
    for k in (4, 3, 2, 1, 0):
        v = v * x + c[:, k]
    d = 5 * c[:, 5]
    for k in (4, 3, 2, 1):
        d = d * x + k * c[:, k]
    a = 20 * c[:, 5]
    for k in (4, 3, 2):
        a = a * x + (k * (k - 1)) * c[:, k]
    return v.astype(np.float64), d.astype(np.float64), a.astype(np.float64)


def norm_so2(y):
    """UnevenMap::normSO2 (uneven_map.cpp:63-70) over an array: whole turns added, then removed, one at a time"""
    y = np.array(y, dtype=np.float64).reshape(-1).copy()
    for _ in range(4096):
        m = y < -np.pi
        if not m.any():
            break
        y[m] += 2 * np.pi
    for _ in range(4096):
        m = y > np.pi
        if not m.any():
            break
        y[m] -= 2 * np.pi
    return y


def ref_states(c_xy, c_yaw, T_xy, T_yaw, Nxy, Nyaw, t):
    """SE2Trajectory's getNormSE2Pos / getVel / getAcc (se2traj.hpp:106-140, 343-361) of ONE trajectory given by its coefficients (c_xy (6 Nxy, 2),
    c_yaw (6 Nyaw,), ascending powers per piece) at the times t (any shape, used as given: the caller clamps): (n, 10) rows in STATE_COLS --
    x, y, dx, dy, ddx, ddy, normSO2(yaw), dyaw, ddyaw, raw yaw.  Written from the reference's rule, with no product code: numpy only."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    cx = np.asarray(c_xy, dtype=np.float64).reshape(int(Nxy), 6, 2)
    cw = np.asarray(c_yaw, dtype=np.float64).reshape(int(Nyaw), 6)
    ix, tl = _locate(T_xy, Nxy, t)
    iw, tw = _locate(T_yaw, Nyaw, t)
    px, vx, ax = _quintic(cx[ix, :, 0], tl)
    py, vy, ay = _quintic(cx[ix, :, 1], tl)
    w, dw, ddw = _quintic(cw[iw], tw)
    return np.column_stack([px, py, vx, vy, ax, ay, norm_so2(w), dw, ddw, w])


def ref_terms(og, state, gravity):
    """the seven report terms (alm_traj_opt.h:170-229, se2traj.hpp:551-561) assembled in numpy from the oracle's terrain variables; state (n, 8):
    x, y, normSO2(yaw), dx, dy, ddx, ddy, dyaw -- the STATE columns of a rollout row after its time"""
    x, y, w, dx, dy, ddx, ddy, dw = state.T
    tv = og.terrain_variables(np.column_stack([x, y, w]))
    c, s = np.cos(w), np.sin(w)
    vx = np.hypot(dx, dy) * tv[:, 0]
    lon, lat = ddx * c + ddy * s, -ddx * s + ddy * c
    return np.column_stack([vx, lon * tv[:, 0] + gravity * tv[:, 1], lat * tv[:, 2] + gravity * tv[:, 3], dw * tv[:, 5] / np.sqrt(vx * vx + 0.01),
                            -1.0 / tv[:, 5], tv[:, 6], np.abs(dx * s - dy * c)])


def report_from_terms(terms):
    """the rule of getMaxVxAxAyCurAttSig (alm_traj_opt.h:170-229) on the (n, 7) terms of a trajectory's samples: vx, ax, ay, cur as the signed value
    of largest magnitude with both maxima started from 0, att started from -1, sigma from 0, and the sum of the non-holonomic error"""
    T = np.asarray(terms, dtype=np.float64).reshape(-1, 7)
    smax = lambda v: max(0.0, v.max()) if max(0.0, v.max()) >= max(0.0, (-v).max()) else -max(0.0, (-v).max())   # signed largest magnitude, maxima from 0
    return np.array([smax(T[:, 0]), smax(T[:, 1]), smax(T[:, 2]), smax(T[:, 3]), max(0.0, (T[:, 4] + 1.0).max()) - 1.0, max(0.0, T[:, 5].max()),
                     T[:, 6].sum()])


def report_errors(ref, got):
    """the project's bar for the report (test_gpu_parity::test_report_matches_oracle_on_same_trajectory) as two numbers to hold below 1e-9:
    columns 0-5 |d| <= 1e-12 + 1e-9 |ref| is |d| / (|ref| + 1e-3) <= 1e-9; column 6 |d| / max(1, ref)"""
    ref, got = np.asarray(ref, dtype=np.float64), np.asarray(got, dtype=np.float64)
    return dict(maxima=float((np.abs(got[:6] - ref[:6]) / (np.abs(ref[:6]) + 1e-3)).max()), nonhol=float(abs(got[6] - ref[6]) / max(1.0, ref[6])))


# ---- comparisons shared by the two tiers --------------------------------------------------------------------------------------------------
def eval_errors(ref, got):
    """relative errors of one evaluation: got has f, g, hx, gx, c_xy, c_yaw, T_xy, T_yaw (T: absolute, as test_gpu_parity compares it)"""
    return dict(f=rel1(ref["f"], got["f"]), grad=rel(ref["g"], got["g"]), hx=rel(ref["hx"], got["hx"]), gx=rel(ref["gx"], got["gx"]),
                c_xy=rel(ref["c_xy"], got["c_xy"]), c_yaw=rel(ref["c_yaw"], got["c_yaw"]),
                T=max(abs(got["T_xy"] - ref["T_xy"]), abs(got["T_yaw"] - ref["T_yaw"])))


def penalty_errors(ref, got, hx, gx):
    """the quantities of test_gpu_lanes::test_penalty_kernel_alone_for_every_lane_count"""
    gtx, gty = ref["gdTxy"], ref["gdTyaw"]
    return dict(cost=rel1(ref["pen_cost"], got["cost"]), gdCxy=rel(ref["gdCxy"], got["gdCxy"]), gdCyaw=rel(ref["gdCyaw"], got["gdCyaw"]),
                gdTxy_sum=abs(got["gdTxy_sum"] - gtx.sum()) / max(1e-300, np.abs(gtx).sum()),
                gdTyaw_sum=abs(got["gdTyaw_sum"] - gty.sum()) / max(1e-300, np.abs(gty).sum()),
                hx=rel(ref["pen_hx"], hx), gx=rel(ref["pen_gx"], gx))


def record(test, variant, errs_by_case):
    """keep the worst error of a (test, variant), overall and per quantity, and where it occurred; errs_by_case: {(nxy, nyaw): {quantity: error}}.
    Returns the overall worst (error, (where, quantity))."""
    MEASURED[(test, str(variant))] = _worst_each(errs_by_case)
    return _worst(errs_by_case)


def _line(test, variant, per_q):
    q, (e, where) = max(per_q.items(), key=lambda kv: kv[1][0])
    rest = "  ".join("%s %.1e @%s" % (k, v[0], v[1]) for k, v in sorted(per_q.items()))
    return "%-32s %-11s %-10.3e %s %s\n%46s%s\n" % (test, variant, e, where, q, "", rest)


def write_report(path, floor=None, header="", only=None):
    """the worst error of every (variant, test) recorded in this process -- overall, then per quantity with the (Nxy, Nyaw) it occurred at -- and,
    when given, the oracle's own floor (oracle against its FMA build) in the same form; only(test name) selects the recorded tests"""
    with open(path, "w") as fh:
        if header:
            fh.write(header.rstrip("\n") + "\n")
        fh.write("%-32s %-11s %-10s %s\n" % ("test", "variant", "worst", "at (Nxy, Nyaw[, ratio]), quantity; then every quantity's worst"))
        for (test, variant), per_q in sorted(MEASURED.items()):
            if only is not None and not only(test):
                continue
            fh.write(_line(test, variant, per_q))
        if floor:
            fh.write("\noracle against the oracle rebuilt with -march=native -ffp-contract=fast, same problems (its own rounding floor)\n")
            for test, per_q in sorted(floor.items()):
                fh.write(_line(test, "oracle/fma", per_q))


def fma_floor(O, og, cells):
    """worst difference between the oracle and its FMA rebuild over the sweep: single evaluation (all cases), initScaling and the capped solves
    (ratio 2).  Uses the cached plain results."""
    import sensitivity
    cases = all_cases()
    r2 = [c for c in cases if c[1] == 2.0]
    sol = [(n, 2.0) for n in SOLVE_NXY]
    plain_e, plain_s, plain_o = oracle_evals(O, og, cases), oracle_scalings(O, og, r2), oracle_solves(O, og, sol)
    with sensitivity.fma_session() as F:
        fg = F.OracleGrid()
        fg.set_cells(cells)
        fe, fs, fo = oracle_evals(F, fg, cases, tag="fma"), oracle_scalings(F, fg, r2, tag="fma"), oracle_solves(F, fg, sol, tag="fma")
    out = {}
    w = {pieces(sweep_problem(*c)): eval_errors(plain_e[c], fe[c]) for c in cases if c[1] == 2.0}
    out["single_evaluation (ratio 2)"] = _worst_each(w)
    w = {pieces(sweep_problem(*c)) + (c[1],): eval_errors(plain_e[c], fe[c]) for c in cases}
    out["single_evaluation (all ratios)"] = _worst_each(w)
    w = {pieces(sweep_problem(*c)): penalty_errors(plain_e[c], dict(cost=fe[c]["pen_cost"], gdCxy=fe[c]["gdCxy"], gdCyaw=fe[c]["gdCyaw"],
                                                                      gdTxy_sum=fe[c]["gdTxy"].sum(), gdTyaw_sum=fe[c]["gdTyaw"].sum()),
                                                   fe[c]["pen_hx"], fe[c]["pen_gx"]) for c in r2}
    out["penalty (ratio 2)"] = _worst_each(w)
    w = {pieces(sweep_problem(*c)): dict(scale_fx=rel1(plain_s[c]["scale_fx"], fs[c]["scale_fx"]), scale_cx=rel(plain_s[c]["scale_cx"], fs[c]["scale_cx"])) for c in r2}
    out["init_scaling (ratio 2)"] = _worst_each(w)
    w = {pieces(sweep_problem(*c)): dict(x=rel(plain_o[c]["x"], fo[c]["x"]), cost=rel1(plain_o[c]["cost"], fo[c]["cost"]),
                                          counters=float(any(plain_o[c][k] != fo[c][k] for k in ("ret", "lbfgs_iters", "evals")))) for c in sol}
    out["capped_solves (ratio 2)"] = _worst_each(w)
    return out


def report_floor(O, og, cells):
    """the oracle's report against its FMA rebuild's on the same coefficients -- the oracle's own at x0 -- for every case of the sweep, in
    report_errors' two numbers (ratio 2, and all ratios)"""
    import sensitivity
    cases = all_cases()
    ev = oracle_evals(O, og, cases)
    plain = oracle_reports(O, og, {c: ev[c] for c in cases}, "oracle-x0")
    with sensitivity.fma_session() as F:
        fg = F.OracleGrid()
        fg.set_cells(cells)
        fma = oracle_reports(F, fg, {c: ev[c] for c in cases}, "oracle-x0/fma")
    out = {}
    out["report (ratio 2)"] = _worst_each({pieces(sweep_problem(*c)): report_errors(plain[c], fma[c]) for c in cases if c[1] == 2.0})
    out["report (all ratios)"] = _worst_each({pieces(sweep_problem(*c)) + (c[1],): report_errors(plain[c], fma[c]) for c in cases})
    return out


def _worst(errs_by_case):
    worst = (-1.0, None)
    for where, errs in errs_by_case.items():
        for q, e in errs.items():
            if e > worst[0]:
                worst = (float(e), (where, q))
    return worst


def _worst_each(errs_by_case):
    out = {}
    for where, errs in errs_by_case.items():
        for q, e in errs.items():
            if q not in out or e > out[q][0]:
                out[q] = (float(e), where)
    return out
