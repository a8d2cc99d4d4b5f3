"""Every position piece count 1..128 x the yaw ratios of tests/piece_sweep.py through the queries that read resident trajectories back on a window or a common
clock: uph_locate_kernel / uph_within_kernel, uph_extent_kernel, uph_separation_kernel / uph_footprint_kernel, uph_delay_sweep_kernel / uph_delay_extent_kernel
and the fleet calls built on them (run with -m gpu on an MI355X; everything goes through the C-ABI).

No solve anywhere: the resident batch is test_gpu_resident_sweep._auto's -- all 469 cases evaluated at x0 under the automatic variant, one upload for both files.
The queries are tests/query_sweep.py's (W1: long windows from before both starts to after both arrivals, the 256-lane kernels; W2: 192 samples around an
arrival, the one-wave kernels; W3: W2's windows at W1's dt), whose conditions tests/test_query_sweep_cpu.py proves on the oracle's coefficients.

(a) ties the device's states at the clock's sample times u = tau - t0 to query_sweep.ref_clock_states (numpy, long double Horner, the reference's piece location,
clamped in numpy).  Everything after it is held bit for bit (footprints: by test_gpu_footprint.py's classes) to the numpy mirrors fed with those states, by the
helpers of the hill tests.  The worst error of (a), and two figures that are recorded and not asserted, are kept in piece_sweep.MEASURED under names starting with
"q_"; tools/query_sweep_report.py writes them to profiles/.

A call takes ONE dt.  W1 (0.05 s) and W2 (0.01 s) therefore go in two calls, and the launch that mixes both widths and arrives sorted is W1 + W3.
"""
import time

import numpy as np
import pytest

import piece_sweep as PS
import query_sweep as QS
from test_gpu_delay import _extent_held, _held, _schedule_held
from test_gpu_footprint import Tally, _fleet_held, _hold_row
from test_gpu_locate import LKEYS, WKEYS, _expect_locate, _expect_within, _poses_near, _properties, _rects_near
from test_gpu_locate import _same as _same_rows
from test_gpu_pieces import AUTO, _check, dev      # noqa: F401  (dev: the module-scoped map fixture)
from test_gpu_resident_sweep import PO, ST, TR, _auto, _range, _rollout, _scaled
from test_gpu_separation import EKEYS, SKEYS, _fleet_brute, _fleet_listed, _same
from uneven_planner_amd.alm_traj_opt import delay_times, extent_rows, separation_rows, separation_times

pytestmark = pytest.mark.gpu
INF = float("inf")
CHUNK = 1 << 18                                  # rows of one traj_states call
FKEYS = ("min_c2", "min_t", "first_t", "last_t", "counts")
_S = {}


def _states(opt, tr, u):
    out = np.empty((u.shape[0], 10))
    for a in range(0, u.shape[0], CHUNK):
        out[a:a + CHUNK] = opt.traj_states(tr[a:a + CHUNK], u[a:a + CHUNK])
    return out


@pytest.fixture(scope="module")
def sweep(dev):
    """once per module: the resident batch, query_sweep.build on ITS downloaded coefficients (the windows, the long-double reference states of both sides of
    every query) and the device's states traj_states(traj, tau - t0) at the same times; read only"""
    if "S" not in _S:
        R = _auto(dev)
        t = time.time()
        Q = QS.build(R["out"])
        t_ref = time.time() - t
        for name in QS.SETS:
            w = Q[name]
            sizes = w["K"]
            cut = np.cumsum(sizes)[:-1]
            for side, tr, t0 in (("dev_a", w["ta"], w["t0a"]), ("dev_b", w["tb"], w["t0b"])):
                u = np.concatenate([tau - s for tau, s in zip(w["taus"], t0)])
                st = _states(R["opt"], np.repeat(tr, sizes).astype(np.int32), u)
                st.setflags(write=False)
                w[side] = np.split(st, cut)
        print("query sweep: %d reference states in %.1f s" % (2 * sum(int(Q[n]["K"].sum()) for n in QS.SETS), t_ref))
        _S["S"] = dict(R=R, Q=Q)
    return _S["S"]


def _calls(Q):
    """the two calls that cover the three sets: (tag, dt, the sets' names, their queries one after the other, per query its set's row)"""
    keys = ("ta", "tb", "t0a", "t0b", "tf", "tt", "radius", "sa", "sb", "m", "K")
    out = []
    for tag, names in (("W1+W3", ("W1", "W3")), ("W2", ("W2",))):
        rows = [(n, q) for n in names for q in range(Q[n]["K"].size)]
        out.append((tag, Q[names[0]]["dt"], QS.concat(Q, names, keys), rows))
    return out


# ---- a. the states the clock kernels sample ------------------------------------------------------------------------------------------------
def test_clock_states_every_piece_count(sweep):
    """uph_traj_states at u = tau_k - t0 for both vehicles of every query of W1, W2 and W3 -- 1.3 M rows: away from knots, through the clamp at both ends, at every
    piece count and ratio -- against ref_clock_states at 1e-12 in close's scaling, the bar r_traj_states holds.  Every output finite; W1's first sample finds
    both vehicles in their start states and its last in their goal states, bit for bit."""
    R, Q = sweep["R"], sweep["Q"]
    opt, cases, total = R["opt"], R["cases"], Q["total"]
    B = len(cases)
    got = [dict() for _ in range(B)]
    for name in QS.SETS:
        w = Q[name]
        for side, tr in (("a", w["ta"]), ("b", w["tb"])):
            for q in range(B):
                d, r = w["dev_" + side][q], w["ref_" + side][q]
                assert d.shape == r.shape == (w["K"][q], 10) and np.isfinite(d).all(), (name, side, q)
                assert np.array_equal(PS.norm_so2(d[:, 9]), d[:, 6]), (name, side, q)
                e = got[tr[q]]
                for key, err in (("%s_%s" % (name, side), _scaled(d[:, :9], r[:, :9])), ("%s_%s_raw_yaw" % (name, side), _scaled(d[:, 9:], r[:, 9:]))):
                    e[key] = max(e.get(key, 0.0), err)
    assert all(len(e) >= 10 for e in got)                           # every trajectory was side a of every set, and side b of some
    _check("q_clock_states", AUTO, cases, got, lambda q, nxy: 1e-12)
    w = Q["W1"]
    every = np.arange(B, dtype=np.int32)
    start, goal = opt.traj_states(every, np.zeros(B)), opt.traj_states(every, total + 9.0)
    for q in range(B):
        a, b = w["ta"][q], w["tb"][q]
        assert np.array_equal(w["dev_a"][q][0], start[a]) and np.array_equal(w["dev_b"][q][0], start[b]), q
        assert np.array_equal(w["dev_a"][q][-1], goal[a]) and np.array_equal(w["dev_b"][q][-1], goal[b]), q
        assert not np.array_equal(start[a][:2], goal[a][:2])
    # W2: side a moves at the first sample and stands at its goal at the last
    w = Q["W2"]
    assert all(np.array_equal(w["dev_a"][q][-1], goal[w["ta"][q]]) and not np.array_equal(w["dev_a"][q][0], goal[w["ta"][q]]) for q in range(B))


# ---- b. separation and extent ----------------------------------------------------------------------------------------------------------------
def test_separation_and_extent_every_piece_count(sweep):
    """separation() and extent() over W1 + W3 in one call each (both launch widths in one launch, sorted by length) and over W2: every output equals
    separation_rows / extent_rows on the states of (a), bit for bit.  Recorded, not asserted: |sqrt(min_d2) - sqrt(ref)| against ref_clock_states alone."""
    R, Q = sweep["R"], sweep["Q"]
    opt, cases = R["opt"], R["cases"]
    rec = [dict() for _ in cases]
    for tag, dt, c, rows in _calls(Q):
        got = opt.separation(c["ta"], c["tb"], c["tf"], c["tt"], c["radius"], t0_a=c["t0a"], t0_b=c["t0b"], dt=dt)
        ext = opt.extent(c["ta"], c["tf"], c["tt"], t0=c["t0a"], dt=dt)
        ext_b = opt.extent(c["tb"], c["tf"], c["tt"], t0=c["t0b"], dt=dt)
        per, pe, pb = [], [], []
        for name, q in rows:
            w = Q[name]
            per.append(separation_rows(w["taus"][q], w["dev_a"][q][:, :2], w["dev_b"][q][:, :2], w["radius"][q]))
            pe.append(extent_rows(w["dev_a"][q][:, :2])), pb.append(extent_rows(w["dev_b"][q][:, :2]))
        _same(got, {k: np.array([p[k] for p in per]) for k in SKEYS}, SKEYS, tag)
        _same(ext, {k: np.array([p[k] for p in pe]) for k in EKEYS}, EKEYS, tag + " extent")
        _same(ext_b, {k: np.array([p[k] for p in pb]) for k in EKEYS}, EKEYS, tag + " extent of b")
        K, below = got["counts"][:, 0], got["counts"][:, 1]
        assert np.array_equal(K, c["K"]) and np.array_equal(ext["counts"], np.stack([K, 0 * K], axis=1))
        assert np.array_equal(K, [separation_times(f, t, dt).shape[0] for f, t in zip(c["tf"], c["tt"])])
        assert np.isfinite(got["min_d2"]).all() and np.isfinite(got["min_t"]).all() and np.isfinite(ext["box"]).all() and np.isfinite(ext_b["box"]).all()
        # coverage: the widths, and rows with none, some and all samples below
        if tag == "W2":
            assert (K <= 192).all() and (K == 192).all()
        else:
            assert (K[:len(cases)] > 192).all() and (K[len(cases):] <= 192).all()
        none, some, full = (below == 0).sum(), ((below > 0) & (below < K)).sum(), (below == K).sum()
        print("%s: rows with no sample below %d, some %d, all %d" % (tag, none, some, full))
        assert none >= 50 and full >= 40 and some >= 300
        assert (np.isnan(got["first_t"]) == (below == 0)).all()
        for (name, q), m2 in zip(rows, got["min_d2"]):
            w = Q[name]
            d2 = ((w["ref_a"][q][:, :2] - w["ref_b"][q][:, :2]) ** 2).sum(axis=1).min()
            for b in (w["ta"][q], w["tb"][q]):
                rec[b][name] = max(rec[b].get(name, 0.0), abs(np.sqrt(m2) - np.sqrt(d2)))
    _check("q_separation", AUTO, cases, rec, lambda q, nxy: INF)


# ---- c. the delay kernels ----------------------------------------------------------------------------------------------------------------------
def test_delay_sweep_and_extent_every_piece_count(sweep):
    """row j of delay_sweep() equals separation() at t0_b + delta_j bit for bit, and delay_extent() the hull of extent()'s boxes (the rules test_gpu_delay.py
    holds), with delays 0.37 s apart so that a delayed start moves samples across pieces: W1 at ratio 2 with D = 70 (256 lanes, two lanes per delay), W1
    at piece_sweep.SOLVE_NXY of every ratio with D = 300 (two passes, rows spilled), and the first 64 samples of every W2 window with D = 3 (K D = 192:
    one wave, 16 lanes per delay)"""
    R, Q = sweep["R"], sweep["Q"]
    opt, cases = R["opt"], R["cases"]
    w1, w2 = Q["W1"], Q["W2"]
    b0, b1 = _range(cases, 2.0)
    solve = np.array([q for q, c in enumerate(cases) if c[0] in PS.SOLVE_NXY])
    assert solve.size == 3 * len(PS.SOLVE_NXY) + sum(n <= 85 for n in PS.SOLVE_NXY) == 84          # (ratio 3 ends at 85 pieces)
    first64 = w2["tf"] + 63 * w2["dt"]
    for tag, w, sel, tt, D, wide in (("W1 ratio 2, D = 70", w1, np.arange(b0, b1), w1["tt"], 70, True), ("W1 solve counts, D = 300", w1, solve, w1["tt"], 300, True),
                                     ("W2 64 samples, D = 3", w2, np.arange(len(cases)), first64, 3, False)):
        a = dict(t0_a=w["t0a"][sel], t0_b=w["t0b"][sel], dt=w["dt"])
        got = _held(opt, w["ta"][sel], w["tb"][sel], w["tf"][sel], tt[sel], w["radius"][sel], -0.5, 0.37, D, tag=tag, **a)
        K = got["counts"]
        assert ((K * D > 192).all() and (K > 600).all()) if wide else (K == 64).all(), tag
        assert np.isfinite(got["min_d2"]).all() and np.isfinite(got["min_t"]).all() and got["below"].shape == (sel.size, D), tag
        if wide:
            assert (got["below"].max(axis=1) > got["below"].min(axis=1)).sum() >= sel.size // 4, tag     # the delay matters
        for side, tr, t0 in (("a", w["ta"], w["t0a"]), ("b", w["tb"], w["t0b"])):
            e, _ = _extent_held(opt, tr[sel], w["tf"][sel], tt[sel], -0.5, 0.37, D, t0[sel], w["dt"], "%s, side %s" % (tag, side))
            assert np.array_equal(e["counts"], np.stack([K, 0 * K], axis=1)) and np.isfinite(e["box"]).all(), tag
    assert delay_times(-0.5, 0.37, 300)[-1] > 100.0                 # the last delays of D = 300 park b at its start for the whole window
    assert opt.delay_kernel_ms() > 0.0


# ---- d. footprints -------------------------------------------------------------------------------------------------------------------------------
def test_footprints_every_piece_count(sweep):
    """footprint_separation() over W1 + W3 and over W2 with the generator's shapes and margins, held by test_gpu_footprint.py's F1 classes (TOL = 1e-9 m^2,
    undecided <= 0.1 %) on the device poses of the fixture, which (a) ties to the reference"""
    R, Q = sweep["R"], sweep["Q"]
    opt = R["opt"]
    B = len(R["cases"])
    for tag, dt, c, rows in _calls(Q):
        got = opt.footprint_separation(c["ta"], c["tb"], c["tf"], c["tt"], c["sa"], c["sb"], c["m"], t0_a=c["t0a"], t0_b=c["t0b"], dt=dt)
        tally = Tally()
        assert np.array_equal(got["counts"][:, 0], c["K"]) and np.isfinite(got["min_c2"]).all() and np.isfinite(got["min_t"]).all(), tag
        for r, (name, q) in enumerate(rows):
            w = Q[name]
            row = (got["min_c2"][r], got["min_t"][r], got["first_t"][r], got["last_t"][r], int(got["counts"][r, 1]), int(got["counts"][r, 2]))
            _hold_row(row, w["taus"][q], w["dev_a"][q][:, [0, 1, 9]], w["dev_b"][q][:, [0, 1, 9]], w["sa"][q], w["sb"][q], w["m"][q], tally, (tag, name, q))
        tally.close("footprints " + tag)
        K, below, over = got["counts"][:, 0], got["counts"][:, 1], got["counts"][:, 2]
        mix, wider = ((over > 0) & (over < K)), below > over
        print("%s: rows overlapping at some samples %d, at none %d, more below than overlapping %d" % (tag, mix.sum(), (over == 0).sum(), wider.sum()))
        # coverage as in F1, with test_query_sweep_cpu.py's figures for the reference poses
        if tag == "W2":
            # (on the reference poses: 83 rows mix, 34 hold samples below and not below, 58 more below than overlapping, 4 never overlap)
            assert mix.sum() >= 30 and ((below > 0) & (below < K)).sum() >= 10 and wider.sum() >= 3 and (over == 0).sum() >= 1
        else:
            assert mix[:B].sum() >= 400 and wider[:B].sum() >= 250 and (over[B:] == 0).sum() >= 1
    assert opt.footprint_kernel_ms() > 0.0


# ---- e. locate and within ----------------------------------------------------------------------------------------------------------------------
def test_locate_and_within_every_piece_count(sweep):
    """locate() and within() on the sweep's rollout at 0.05 s with the end row, all ratios, two queries per trajectory: the full window (one wave up to 192 rows,
    256 lanes beyond) and a window of at most 192 rows that ends in the end row.  P1, P2 and P5 of test_gpu_locate.py as its own tests hold them.  P3, the
    Newton residual bar, was established on solved trajectories; x0 is none (it turns with up to 44 1/m), so the largest |g| / G is recorded as q_locate and not
    asserted."""
    R = sweep["R"]
    opt, cases = R["opt"], R["cases"]
    B = len(cases)
    ref = _rollout(R, 0.05, ST | TR | PO, 0, B)
    offs, rows = ref
    n_rows = np.diff(offs)
    rng = np.random.default_rng(4691)
    every = np.arange(B, dtype=np.int32)
    tail = np.minimum(n_rows, 192)
    tf_tail = rows[offs[1:] - tail, 0]
    traj = np.concatenate([every, every])
    tf = np.concatenate([np.zeros(B), tf_tail])
    poses = np.concatenate([_poses_near(ref, every, rng), rows[offs[1:] - 1 - rng.integers(0, tail), 1:4] + rng.normal(0.0, 0.05, (B, 3))])
    rects = np.concatenate([_rects_near(ref, every, rng), _rects_near(ref, every, rng)])
    got = opt.locate(traj, poses, tf, None, dt=0.05, with_end=1)
    want = _expect_locate(ref, traj, poses, tf, None)
    _same_rows(got, want, LKEYS, "sweep")
    ratio = _properties(opt, got, want, traj, poses, "sweep", assert_p3=False)
    w = opt.within(traj, rects, tf, None, dt=0.05, with_end=1)
    _same_rows(w, _expect_within(ref, traj, rects, tf, None), WKEYS, "sweep")
    # coverage: both widths, windows that end in the end row, refined and kept candidates, rects crossed and missed
    assert np.array_equal(got["count"], np.concatenate([n_rows, tail])) and np.array_equal(w["counts"][:, 0], got["count"])
    assert (n_rows > 192).sum() >= 300 and (n_rows <= 192).sum() >= 20 and (tail == 192).sum() >= 300 and n_rows.min() < 16 and n_rows.max() > 1800
    assert (got["refined"] == 1).sum() >= B // 2 and np.isfinite(got["state"]).all() and np.isfinite(got["err"]).all() and np.isfinite(got["d2"]).all()
    assert (w["counts"][:, 1] > 0).sum() >= B and (w["counts"][:, 1] < w["counts"][:, 0]).sum() >= B // 2 and (w["counts"][B:, 1] == 0).any()
    inner = np.isfinite(ratio)
    assert inner.sum() >= B // 2
    rec = [dict() for _ in cases]
    for q in np.nonzero(inner)[0]:
        key = "full" if q < B else "tail"
        rec[traj[q]][key] = ratio[q]
    print("P3 on the sweep, not asserted: %d interior, |g| / G above 1 in %d" % (inner.sum(), (ratio[inner] > 1.0).sum()))
    have = [b for b in range(B) if rec[b]]
    _check("q_locate", AUTO, [cases[b] for b in have], [rec[b] for b in have], lambda q, nxy: INF)
    assert opt.locate_kernel_ms() > 0.0


# ---- f. the fleet calls ------------------------------------------------------------------------------------------------------------------------
def test_fleet_calls_on_the_sweep(sweep):
    """conflicts(), footprint_conflicts() and delays() over the 44 vehicles of piece_sweep.SOLVE_NXY at ratios 2 and 1.7 (946 pairs), starts staggered around
    1000 s, dt 0.05 -- held as test_gpu_separation::test_the_fleet, test_gpu_footprint::test_the_fleet and
    test_gpu_delay::test_the_schedule_is_the_sequential_greedy hold them on the hill fleet: the brute force of the mirrors over all pairs, and delay_schedule
    driven by separation().  All sweep trajectories leave one pose along one curve, so the window opens after the last start (before it every pair stands at
    distance 0 exactly) and the longest trajectory comes first: a shorter one then waits until the longer ones have passed its goal."""
    R, Q = sweep["R"], sweep["Q"]
    opt, cases, total = R["opt"], R["cases"], Q["total"]
    tr = np.array([q for r in (2.0, 1.7) for q, c in enumerate(cases) if c[1] == r and c[0] in PS.SOLVE_NXY], dtype=np.int32)
    tr = tr[np.argsort(-total[tr], kind="stable")]                  # the longest first: it has the right of way
    n, dt = tr.size, 0.05
    assert n == 44
    rng = np.random.default_rng(4692)
    t0 = 1000.0 + 0.4 * np.arange(n)
    tf, tt = float(t0.max()) + 0.3, float((t0 + total[tr]).max()) + 1.0
    # discs
    want = _fleet_brute(opt, tr, t0, tf, tt, dt)
    assert want["n_pairs"] == 946 and want["radius"][0] > 0.0
    radius = want["radius"]
    got = opt.conflicts(tr, radius, tf, tt, t0=t0, dt=dt)
    print("sweep fleet: K = %d, radius = %.4g, conflicts %d, candidates %d of 946" % (want["tau"].shape[0], radius[0], got["n_conflicts"], got["n_candidates"]))
    _fleet_listed(got, want)
    # (the radius is half the median of the pairs' smallest distances: about half of the pairs conflict)
    assert 100 <= got["n_conflicts"] <= 846 and got["n_candidates"] >= got["n_conflicts"] and np.isfinite(got["rows"][:, :2]).all()
    # rectangles
    shape = np.stack([rng.uniform(0.4, 0.5, n), rng.uniform(0.1, 0.2, n), rng.uniform(0.12, 0.18, n)], axis=1)
    margin = rng.uniform(0.0, 0.1, n) * (np.arange(n) % 3 != 0)
    fgot, listed, sure, maybe, _ = _fleet_held(opt, tr, t0, tf, tt, dt, shape, margin, tag="sweep fleet")
    print("sweep fleet: rectangles report %d pairs (%d undecided), candidates %d" % (len(listed), len(maybe), fgot["n_candidates"]))
    assert len(sure) >= 1 and np.isfinite(fgot["rows"][:, :2]).all()
    # the schedule, with every delay of the table and with per-vehicle limits.  The goals lie 0.3 m apart along the curve and every piece count is there at both
    # ratios with one path: discs of 0.1 m let a vehicle wait until those ahead have left (the twin of the other ratio, which ends in the same goal, it cannot clear)
    D, step = 16, 0.5
    small = np.full(n, 0.1)
    for nd in (None, 1 + (np.arange(n) * 5) % D):
        sched = opt.delays(tr, small, tf, tt, 0.0, step, D, t0=t0, n_delays=nd, dt=dt)
        print("sweep fleet: choice %s rounds %d candidates %d unresolved %d" % (sched["choice"].tolist(), sched["n_rounds"], sched["n_candidates"], sched["n_unresolved"]))
        _schedule_held(opt, sched, tr, t0, small, tf, tt, 0.0, step, D, dt, n_delays=nd, tag="sweep fleet delays")
        assert sched["choice"][0] == 0 and ((sched["blocker"] >= 0) == (sched["choice"] < 0)).all() and np.isfinite(sched["start"]).all()
        if nd is None:
            assert (sched["choice"] > 0).sum() >= 3 and sched["n_unresolved"] >= 1 and sched["n_rounds"] >= 2
    assert opt.separation_kernel_ms() > 0.0 and opt.delay_kernel_ms() > 0.0
