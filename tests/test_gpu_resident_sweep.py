"""Every position piece count 1..128 x the yaw ratios of tests/piece_sweep.py through the code that reads a FINISHED trajectory back: the post-solve
report (Solver::report, compiled once per lane / occupancy variant), the rollout, the check, uph_traj_states and the staging of uph_refine_upload
(run with -m gpu on an MI355X; everything goes through the C-ABI).

No solve anywhere: upload + set_state + one evaluation at x0 (test_gpu_pieces._evaluate) leaves the trajectory of x0 resident, and every call
here accepts that.  One heterogeneous batch per context -- 1 and 128 pieces side by side, so the per-trajectory offsets of the coefficient arrays
matter -- with trajectories of up to 92 s (9 172 samples at 0.01 s).  References: the oracle's report on the downloaded coefficients, and
piece_sweep.ref_states / ref_terms / report_from_terms (numpy, long double Horner, the reference's discrete piece location).  The check is held
bit for bit against the numpy mirror check_rows on the rollout's rows, which (b) ties to those references.

The worst error of every test is kept in piece_sweep.MEASURED under names starting with "r_"; tools/piece_sweep_report.py writes them to profiles/.
"""
import numpy as np
import pytest

import piece_sweep as PS
from test_gpu_check import _same
from test_gpu_pieces import ALL_VARIANTS, AUTO, _check, _ctx, _evaluate, _vid, dev      # noqa: F401  (dev: the module-scoped map fixture)
from test_refine_cpu import refine_counts

pytestmark = pytest.mark.gpu
ST, TR, PO = 1, 2, 4
INF = float("inf")
ROW_COLS_OF_STATE = [1, 2, 4, 5, 6, 7, 3, 8]     # rollout STATE columns (t x y yaw dx dy ddx ddy dyaw) of uph_traj_states' columns 0..7
# (d) the second set of limits is check_limits() times this.  The issue's half does not split the sweep: x0 is no solved trajectory, it peaks at
# 0.66 m/s against max_vel = 0.5 (and turns with up to 44 1/m against max_kap = 2.1), so at half the limits 99.3 % of the 1 024 queries violate
# (every window but a few single samples next to the start).  With the reference terms (ref_states + ref_terms on the oracle's coefficients,
# on the CPU): factor 0.9 -> 51 % violate (all full windows, 15 % of the single samples, 44 % / 45 % of the 256- / 257-sample windows) and
# 49 % do not; 0.8 -> 97 %; check_limits() itself -> 47 %.  No factor above 1.2 is usable: the attitude limit -min_cxi is negative, scaled
# up it lies below every sample.
CHECK_FACTOR = 0.9
_RES = {}


def _resident(dev, cases):
    """the automatic variant's context with `cases` evaluated at x0 as one batch (once per module): opt, the cases, their downloads"""
    key = tuple(cases)
    if key not in _RES:
        opt = _ctx(dev, AUTO)
        probs, out = _evaluate(opt, cases, AUTO)
        assert all(o["ret"] != 4 for o in out)
        _RES[key] = dict(opt=opt, cases=list(cases), probs=probs, out=out, roll={})
    return _RES[key]


def _auto(dev):
    return _resident(dev, PS.all_cases())


def _range(cases, ratio):
    idx = [i for i, c in enumerate(cases) if c[1] == ratio]
    assert idx and idx == list(range(idx[0], idx[-1] + 1))                # all_cases() is ratio-major: one ratio is one range [b0, b1)
    return idx[0], idx[-1] + 1


def _rollout(R, dt, channels, b0, b1):
    """rollout with the end row of trajectories [b0, b1), kept for the module: (offsets relative to b0, rows); read only"""
    key = (dt, channels, b0, b1)
    if key not in R["roll"]:
        offs, rows = R["opt"].rollout(dt, channels, with_end=True, b0=b0, b1=b1)
        assert rows.nbytes < 256 << 20, rows.nbytes
        rows.setflags(write=False)
        R["roll"][key] = (offs, rows)
    return R["roll"][key]


def _pieces(o):
    return o["c_xy"].shape[0] // 6, o["c_yaw"].shape[0] // 6


def _total(o):
    return PS.total_duration(o["T_xy"], o["T_yaw"], *_pieces(o))


def _ref_states(o, t):
    nx, ny = _pieces(o)
    return PS.ref_states(o["c_xy"], o["c_yaw"], o["T_xy"], o["T_yaw"], nx, ny, t)


def _scaled(a, b, scale=None):
    """test_gpu_rollout.close's error: |a - b| over max(1, the column's largest |b|), the largest entry"""
    a, b = np.asarray(a), np.asarray(b)
    scale = np.maximum(1.0, np.abs(b).max(axis=0)) if scale is None else scale
    return float((np.abs(a - b) / scale).max())


# ---- a. the report, every variant ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ALL_VARIANTS, ids=_vid)
def test_report_every_piece_count(dev, oracle, oracle_grid, variant):
    """getMaxVxAxAyCurAttSig after one evaluation of one heterogeneous batch -- all four ratios under the automatic variant, the shipped ratio 2 and
    the ragged 1.7 (Nyaw != k Nxy, min(durx, dury) decided in the last bits) under each forced one -- against the oracle's report on that variant's
    downloaded coefficients at test_gpu_parity::test_report_matches_oracle_on_same_trajectory's bar.  Automatic variant: the first six columns
    also equal report_from_terms of the context's own rollout(0.01, TERRAIN) bit for bit, column 6 to 1e-12 (what
    test_gpu_rollout::test_report_follows_from_terrain_columns claims for ten short trajectories); for a forced variant that equality is only
    recorded (report_ne_rollout 0 / 1): instantiations may contract differently, their bar is the oracle."""
    cases = PS.all_cases() if variant == AUTO else [c for c in PS.all_cases() if c[1] in (2.0, 1.7)]
    if variant == AUTO:
        R = _auto(dev)
        opt, out = R["opt"], R["out"]
    else:
        opt = _ctx(dev, variant)
        _, out = _evaluate(opt, cases, variant)
    rep = opt.getMaxVxAxAyCurAttSig()
    assert rep.shape == (len(cases), 7) and all(o["ret"] != 4 for o in out)                    # no refusal (_upload fails on one), no unsupported slot
    # no placeholder: every row is a real reduction of a moving trajectory (vx > 0, att >= -1, a positive non-holonomic error sum)
    assert np.isfinite(rep).all() and (rep[:, 0] > 0.0).all() and (rep[:, 4] >= -1.0).all() and (rep[:, 5] >= 0.0).all() and (rep[:, 6] > 0.0).all()
    ref = PS.oracle_reports(oracle, oracle_grid, dict(zip(cases, out)), _vid(variant))
    got = [PS.report_errors(ref[c], rep[i]) for i, c in enumerate(cases)]
    # the report against the rollout's TERRAIN columns of the same context
    eq = []
    for r in sorted({c[1] for c in cases}):
        b0, b1 = _range(cases, r)
        offs, rows = opt.rollout(0.01, TR, b0=b0, b1=b1)
        assert rows.nbytes < 256 << 20
        for b in range(b0, b1):
            want = PS.report_from_terms(rows[offs[b - b0]:offs[b + 1 - b0]])
            eq.append((bool(np.array_equal(rep[b, :6], want[:6])), abs(rep[b, 6] - want[6]) / abs(want[6])))
    if variant == AUTO:
        bad = [(PS.pieces(PS.sweep_problem(*c)), c[1], e) for c, e in zip(cases, eq) if not (e[0] and e[1] <= 1e-12)]
        assert not bad, ("the report differs from its own rollout's terms", len(bad), bad[:8])
    for g, e in zip(got, eq):
        g["rollout_sum"] = e[1]                           # column 6 against the rollout's sum (another order of summation)
    bar = lambda q, nxy: {"rollout_sum": 1e-12 if variant == AUTO else INF}.get(q, 1e-9)
    try:
        _check("r_report", variant, cases, got, bar)
    finally:
        flags = {PS.pieces(PS.sweep_problem(*c)) + (c[1],): dict(report_ne_rollout=0.0 if e[0] else 1.0) for c, e in zip(cases, eq)}
        PS.record("r_report_vs_rollout_bits", _vid(variant), flags)


# ---- b. the rollout -----------------------------------------------------------------------------------------------------------------------
def _rollout_case(dev, oracle_grid, R, dt, channels, b0, b1, tag):
    """one rollout call with the end row of trajectories [b0, b1) against the references; returns the per-trajectory row counts"""
    from uneven_planner_amd import alm_traj_opt as A
    opt, out, cases = R["opt"], R["out"], R["cases"]
    offs, rows = _rollout(R, dt, channels, b0, b1)
    sub = out[b0:b1]
    want = A.rollout_sizes([_pieces(o)[0] for o in out], [o["T_xy"] for o in out], [_pieces(o)[1] for o in out], [o["T_yaw"] for o in out], dt, True)
    assert np.array_equal(opt.rollout_plan(dt, True), want)
    assert np.array_equal(offs, want[b0:b1 + 1] - want[b0]) and rows.shape == (offs[-1], 9 + 7 + (12 if channels & PO else 0))
    tab = PS.time_table(dt, max(_total(o) for o in sub))
    gravity = dev.params["gravity"]
    terms = PS.ref_terms(oracle_grid, rows[:, 1:9], gravity)
    t_scale = np.maximum(1.0, np.abs(terms).max(axis=0))                  # (close() over the whole call, as test_terrain_terms_match_oracle)
    if channels & PO:
        Rm, p = dev.getTerrainPosBatch(rows[:, 1:4])
        poses = np.concatenate([Rm.transpose(0, 2, 1).reshape(-1, 9), p], axis=1)
        p_scale = np.maximum(1.0, np.abs(poses).max(axis=0))
        assert np.array_equal(rows[:, 25:27], rows[:, 1:3])               # p = the sample's own (x, y)
    got = []
    for k, o in enumerate(sub):
        a, e = int(offs[k]), int(offs[k + 1])
        blk, total = rows[a:e], _total(o)
        cnt = e - a - 1
        # the time column: the running sum bit for bit (its length the first t_q at or beyond the total, counted here and not by the library), then the total
        assert cnt == int(np.searchsorted(tab, total, "left")) and cnt >= 1, (tag, k, cnt)
        assert np.array_equal(blk[:cnt, 0], tab[:cnt]) and blk[cnt, 0] == total, (tag, k)
        err = dict(states=_scaled(blk[:, 1:9], _ref_states(o, blk[:, 0])[:, PS.ROW_OF_STATE]), terms=_scaled(blk[:, 9:16], terms[a:e], t_scale))
        if channels & PO:
            err["poses"] = _scaled(blk[:, 16:28], poses[a:e], p_scale)
        end = np.asarray(R["probs"][b0 + k]["end_xy"])[:, 0]
        err["end_xy"] = float(np.abs(blk[-1, 1:3] - end).max())
        assert np.isfinite(blk).all(), (tag, k)
        got.append(err)
    _check(tag, AUTO, cases[b0:b1], got, lambda q, nxy: {"poses": 1e-15, "end_xy": 1e-9}.get(q, 1e-12))
    return np.diff(offs)


def test_rollout_every_piece_count(dev, oracle_grid):
    """uph_rollout_batch over the resident sweep with the end row: ratio 2 at dt 0.01 (STATE | TERRAIN, 589 392 rows, up to 36 chunks of 256 rows per
    trajectory) and all four ratios at dt 0.05 (all channels).  Offsets = uph_rollout_sizes on the downloaded durations; the time column is the running
    sum bit for bit and the total in the end row; states against ref_states and terms against ref_terms at 1e-12 (test_gpu_rollout.close's scaling),
    poses against uph_terrain_pose_query at 1e-15, the last row's (x, y) the problem's end point to 1e-9; a call split by b0 / b1 equals the whole."""
    R = _auto(dev)
    B = len(R["cases"])
    b0, b1 = _range(R["cases"], 2.0)
    n1 = _rollout_case(dev, oracle_grid, R, 0.01, ST | TR, b0, b1, "r_rollout_dt0.01")
    n2 = _rollout_case(dev, oracle_grid, R, 0.05, ST | TR | PO, 0, B, "r_rollout_dt0.05")
    # coverage, never an expected value: the row counts of the two calls leave every residue a 64-lane wave can trip over -- a full last wave,
    # one row over, one row short -- and the longest trajectory spans dozens of row chunks (blockIdx.y).  (On the CPU, from uph_rollout_sizes
    # on the oracle's durations: residues 0 / 1 / 63 occur 13 / 7 / 7 times in these two calls; no third dt is needed.)
    res = set((np.concatenate([n1, n2]) % 64).tolist())
    assert {0, 1, 63} <= res, sorted(res)
    assert n1.max() > 9000 and n1.min() < 128 and n2.max() > 1800, (n1.max(), n1.min(), n2.max())
    # parts equal the whole bit for bit
    offs, whole = _rollout(R, 0.05, ST | TR | PO, 0, B)
    cut = [0, 1, 130, 131, 300, B]
    parts = [R["opt"].rollout(0.05, ST | TR | PO, with_end=True, b0=a, b1=e) for a, e in zip(cut[:-1], cut[1:])]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole)
    assert all(np.array_equal(p[0], offs[a:e + 1] - offs[a]) for p, a, e in zip(parts, cut[:-1], cut[1:]))


# ---- c. states at given times -------------------------------------------------------------------------------------------------------------
def _knot_times(T, N):
    """per knot k = 0 .. N of N uniform pieces of T: k T as a product and as the k-fold running sum, the neighbouring doubles of both on either side,
    and (k < N) the middle of piece k"""
    ts, run = [], 0.0
    for k in range(N + 1):
        for v in (k * T, run):
            ts += [v, np.nextafter(v, -INF), np.nextafter(v, INF)]
        if k < N:
            ts.append(run + 0.5 * T)
        run += T
    return ts


def test_traj_states_every_piece(dev):
    """uph_traj_states at every knot of every trajectory of the sweep (all four ratios): k T as a product, as the running sum, one double to either
    side, mid-piece, for the xy and the yaw pieces; per trajectory also 0, -0.25, the total, the double before it and total + 3.  Against ref_states
    at the clamped time (total = the smaller running sum) at 1e-12 (close's scaling); normSO2(column 9) = column 6 exactly; at the rollout's times
    bit-equal to the rollout's rows.  x, v, a are continuous across knots, so a wrong piece AT a knot is invisible in them: the knot queries are there
    for the index range -- the last piece, the ix == Nxy fall-back, the neighbouring trajectory's coefficients -- hence also: every output finite, and
    no row's xy or yaw part equal to what the next trajectory of the batch gives at the same time."""
    R = _auto(dev)
    opt, out, cases = R["opt"], R["out"], R["cases"]
    B = len(cases)
    tr, ts, first = [], [], [0]
    for b, o in enumerate(out):
        nx, ny = _pieces(o)
        total = _total(o)
        t = [0.0, -0.25, total, np.nextafter(total, 0.0), total + 3.0] + _knot_times(o["T_xy"], nx) + _knot_times(o["T_yaw"], ny)
        tr.append(np.full(len(t), b, dtype=np.int32)), ts.append(np.array(t)), first.append(first[-1] + len(t))
    tr, ts = np.concatenate(tr), np.concatenate(ts)
    assert ts.size > 500000
    st = opt.traj_states(tr, ts)
    assert st.shape == (ts.size, 10) and np.isfinite(st).all()
    assert np.array_equal(PS.norm_so2(st[:, 9]), st[:, 6])
    nb = opt.traj_states(np.where(tr + 1 < B, tr + 1, tr - 1).astype(np.int32), ts)          # the neighbour in the batch at the same time
    # (at the start neighbours legitimately agree: every problem of the sweep starts at rest in the same pose of the same curve)
    later = ts > 1e-6                                     # (so also not at the doubles next to 0)
    same_xy, same_yaw = (st[:, :6] == nb[:, :6]).all(axis=1) & later, (st[:, 7:] == nb[:, 7:]).all(axis=1) & later
    assert not same_xy.any() and not same_yaw.any(), (int(same_xy.sum()), int(same_yaw.sum()), tr[same_xy | same_yaw][:8], ts[same_xy | same_yaw][:8])
    got = []
    for b, o in enumerate(out):
        a, e = first[b], first[b + 1]
        total = _total(o)
        tc = np.where(ts[a:e] <= 0.0, 0.0, np.where(ts[a:e] >= total, total, ts[a:e]))
        ref = _ref_states(o, tc)
        got.append(dict(states=_scaled(st[a:e, :9], ref[:, :9]), raw_yaw=_scaled(st[a:e, 9:], ref[:, 9:])))
        # the clamped queries are the end / start states themselves
        assert np.array_equal(st[a + 4], st[a + 2]) and np.array_equal(st[a + 1], st[a]), b
    _check("r_traj_states", AUTO, cases, got, lambda q, nxy: 1e-12)
    # at the rollout's own times: bit-equal to its rows
    offs, rows = _rollout(R, 0.05, ST | TR | PO, 0, B)
    rt = np.repeat(np.arange(B, dtype=np.int32), np.diff(offs))
    z = opt.traj_states(rt, rows[:, 0])
    assert np.array_equal(z[:, :8], rows[:, ROW_COLS_OF_STATE])


# ---- d. the check -------------------------------------------------------------------------------------------------------------------------
def check_queries(b, tab, cnt, total):
    """the four windows of trajectory b, whose rollout at 0.01 s with the end row has rows 0 .. cnt (row cnt the end row at t = total): the whole
    trajectory, one sample, exactly 256 samples (one trip of the check's 256 lanes), 257 (one sample into the second trip) -- the latter clipped to
    the trajectory where it is shorter; every fourth trajectory's 257-window ends in the end row.  Returns (t_from, t_to, samples) per window."""
    rows = cnt + 1
    at = lambda i: total if i == cnt else float(tab[i])
    out = [(0.0, INF, rows)]
    for n in (1, 256, 257):
        n = min(n, rows)
        i = rows - n if (n == 257 and b % 4 == 0) else (37 * b + 11 * n) % (rows - n + 1)
        out.append((at(i), at(i + n - 1), n))
    return out


def test_check_every_piece_count(dev):
    """uph_check_batch (dt 0.01, with the end row) over ratio 2 and 1.7 of the resident sweep: per trajectory its full window -- up to 9 173 samples, 36
    trips of the kernel's `j += 256` walk -- and windows of 1, 256 and 257 samples placed through uph_check_window, under check_limits() and under
    CHECK_FACTOR times it.  Every output equals check_rows on the rollout's rows (tied to the references by test_rollout_every_piece_count) and
    uph_frontend_query's occupancy at them, bit for bit."""
    from uneven_planner_amd.alm_traj_opt import check_rows, check_window
    R = _auto(dev)
    opt, out, cases = R["opt"], R["out"], R["cases"]
    tr, tf, tt, want_n, src = [], [], [], [], {}
    for ratio in (2.0, 1.7):
        b0, b1 = _range(cases, ratio)
        offs, rows = _rollout(R, 0.01, ST | TR, b0, b1)
        occ = dev.frontend_query(rows[:, 1:4])[1]
        tab = PS.time_table(0.01, max(_total(o) for o in out[b0:b1]))
        for b in range(b0, b1):
            a, e = int(offs[b - b0]), int(offs[b + 1 - b0])
            src[b] = (rows[a:e, 0], rows[a:e, 9:16], occ[a:e])
            total = _total(out[b])
            for t0, t1, n in check_queries(b, tab, e - a - 1, total):
                lo, hi, end = check_window(0.01, True, total, t0, t1)
                assert hi - lo + int(end) == n, (b, t0, t1, n, lo, hi, end)
                tr.append(b), tf.append(t0), tt.append(t1), want_n.append(n)
    tr, tf, tt, want_n = np.array(tr, dtype=np.int32), np.array(tf), np.array(tt), np.array(want_n)
    # coverage: the three window sizes exist for all but the shortest trajectories (up to four pieces last less than 2.57 s), some end in the end row
    assert (want_n == 1).sum() >= 256 and (want_n == 256).sum() >= 240 and (want_n == 257).sum() >= 240 and want_n.max() > 9000
    assert sum(1 for q in range(tr.size) if want_n[q] == 257 and tt[q] == _total(out[tr[q]])) >= 60
    base = opt.check_limits()
    for name, lim in (("limits", base), ("limits x %g" % CHECK_FACTOR, base * CHECK_FACTOR)):
        got = opt.check(tr, tf, tt, dt=0.01, with_end=True, limits=lim)
        per = [check_rows(*src[b], lim, t0, t1) for b, t0, t1 in zip(tr, tf, tt)]
        _same(got, {k: np.array([p[k] for p in per]) for k in per[0]}, name)
        assert np.array_equal(got["counts"][:, 0], want_n), name
        viol = got["first_mask"] != 0
        print("check, %s: %d of %d queries violate" % (name, viol.sum(), viol.size))
        if lim is not base:
            assert 4 * viol.sum() >= viol.size and 4 * (~viol).sum() >= viol.size, (name, int(viol.sum()), viol.size)


# ---- e. the staging of uph_refine_upload --------------------------------------------------------------------------------------------------
def test_refine_staging_every_piece_count(dev):
    """uph_refine_upload from the resident sweep without a solve, at t_switch = 0 and at one mid-piece time per trajectory: ratio 2 at every Nxy plus
    the 128-piece trajectories of the other ratios.  At t = 0 the tail of (128, 255) needs 127 position way-points -- all the staging holds -- and 254
    yaw way-points, one below its 255: the sweep has no problem of 256 yaw pieces (ratio 2 ends at 255, ratio 3 is cut at 85 x 255).  They must
    be accepted, not refused.  dst.plan_staged() against the problems assembled on the host: counts and way-point times from the count
    rule (test_refine_cpu.refine_counts), way-point and start states from ref_states at 1e-12, the sweep problem's own end boundary and the
    remaining time exactly; statuses, traj_of, origin() and the counts exactly."""
    import uneven_planner_amd as U
    R = _auto(dev)
    src, out, cases, probs = R["opt"], R["out"], R["cases"], R["probs"]
    b0, b1 = _range(cases, 2.0)
    sel = sorted(set(range(b0, b1)) | {b for b, o in enumerate(out) if _pieces(o)[0] == 128})
    assert max(_pieces(out[b])[1] for b in sel) == PS.MAX_PIECE_YAW - 1 and len(sel) > b1 - b0
    tr = np.array(sel, dtype=np.int32)
    mid = np.array([out[b]["T_xy"] * ((7 * b) % _pieces(out[b])[0] + 0.5) for b in sel])
    close = lambda got, want: float((np.abs(np.asarray(got) - np.asarray(want)) / np.maximum(1.0, np.abs(want))).max()) if np.size(want) else 0.0
    for tag, ts in (("r_refine_staging_t0", np.zeros(tr.size)), ("r_refine_staging_mid", mid)):
        dst = U.ALMTrajOpt(src.uneven_map)              # the source's map object: the resident batch is shared with test_gpu_query_sweep.py, whichever ran first made it
        plan = dst.refine_upload(src, tr, ts)
        staged = dst.plan_staged()
        assert (plan["status"] == 0).all() and np.array_equal(plan["traj_of"], np.arange(tr.size)) and np.array_equal(dst.origin(), np.arange(tr.size)), tag
        assert len(staged) == tr.size
        got = []
        for q, b in enumerate(sel):
            o, p, s = out[b], probs[b], staged[q]
            c = refine_counts(o["T_xy"], _pieces(o)[0], o["T_yaw"], _pieces(o)[1], ts[q])
            assert (plan["n_inner_xy"][q], plan["n_inner_yaw"][q]) == (c["n_xy"] - 1, c["n_yaw"] - 1) == (s["n_inner_xy"], s["n_inner_yaw"]), (tag, b)
            assert s["complete"] and s["inner_xy"].shape == (2, c["n_xy"] - 1) and s["inner_yaw"].shape == (c["n_yaw"] - 1,), (tag, b)
            assert s["total_time"] == c["R"] and np.array_equal(s["end_xy"], p["end_xy"]) and np.array_equal(s["end_yaw"], np.asarray(p["end_yaw"]).ravel()), (tag, b)
            z = _ref_states(o, [c["tc"]])[0]
            wx, wy = _ref_states(o, c["t_xy"]), _ref_states(o, c["t_yaw"])
            got.append(dict(init_xy=close(s["init_xy"], [[z[0], z[2], z[4]], [z[1], z[3], z[5]]]), init_yaw=close(s["init_yaw"], [z[9], z[7], z[8]]),
                            inner_xy=close(s["inner_xy"], wx[:, :2].T), inner_yaw=close(s["inner_yaw"], wy[:, 9]),
                            switch_states=close(plan["switch_states"][q], z)))
        _check(tag, AUTO, [cases[b] for b in sel], got, lambda q, nxy: 1e-12)
        if tag.endswith("t0"):               # the source's own counts: 127 and 254 way-points among them
            assert np.array_equal(plan["n_inner_xy"], [_pieces(out[b])[0] - 1 for b in sel]) and np.array_equal(plan["n_inner_yaw"], [_pieces(out[b])[1] - 1 for b in sel])
            assert plan["n_inner_xy"].max() == 127 and plan["n_inner_yaw"].max() == 254
