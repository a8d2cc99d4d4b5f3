"""GPU tier of re-planning from states on resident trajectories, uph_replan_upload: the switch state of each query evaluated on the device from the
source's coefficients, the search from it, PlanManager's resampling stage and the upload of problems whose start boundary is that state.

Bars: the switch state equals the rollout's row at the same t BIT FOR BIT; the device chain equals the composed host chain (switch states ->
KinoAstar.plan_batch -> resample_batch with the start boundary patched -> upload on a fresh context) bit for bit; the new trajectories start in the
switch state (MINCO's fixed start boundary) to 1e-12; the moving-start problems evaluate as the oracle does at 1e-9 and solve without drifting from
it.  Source: 512 hill goals planned and solved by plan_goals."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES_KEYS = ("x", "c_xy", "c_yaw", "hx", "gx", "lam", "mu", "scale_cx")
SCALAR_KEYS = ("ret", "alm_iters", "lbfgs_iters", "evals", "last_lbfgs_ret", "cost", "jerk_cost", "T_xy", "T_yaw", "rho_final", "scale_fx")
PROB_KEYS = ("init_xy", "end_xy", "inner_xy", "init_yaw", "end_yaw", "inner_yaw")
ROW_OF_STATE = [1, 2, 4, 5, 6, 7, 3, 8]          # rollout STATE columns (t x y yaw dx dy ddx ddy dyaw) of switch columns 0..7


def _queries(m, n, seed0, **kw):
    from uneven_planner_amd import scenes
    nx, ny = int(m.voxel_num[0]), int(m.voxel_num[1])
    return scenes.random_queries(n, seed0=seed0, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]), **kw)


def _hill_map(cloud=None):
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m = U.UnevenMap()
    m.build(scenes.make_hill_cloud() if cloud is None else cloud)
    return m


def _source(m, ka, S, G):
    import uneven_planner_amd as U
    src = U.ALMTrajOpt(m)
    src.set_rho(1.0)
    out = src.plan_goals(ka, S, G)
    return src, [out[b] for b in np.nonzero(src.last_plan["traj_of"] >= 0)[0]]


def _switch_times(src, res, n, seed):
    """n queries over the resident trajectories: kinds 0 start, 1 before the start, 2 a rollout row (dt 0.05), 3 a piece boundary, 4 the end row
    (t = duration), 5 beyond the end, 6 anywhere.  Returns traj, t, kind, the rollout (offsets, rows) and the row each kind 0-2, 4, 5 equals."""
    rng = np.random.default_rng(seed)
    offs, rows = src.rollout(0.05, channels=1, with_end=True)
    ok = [j for j, r in enumerate(res) if r["ret"] != 4]
    tr, ts, kind, row = [], [], [], []
    for q in range(n):
        j = ok[q % len(ok)]
        k = q % 7
        r0, r1 = int(offs[j]), int(offs[j + 1])
        if k == 0:
            t, rr = 0.0, r0
        elif k == 1:
            t, rr = -0.25, r0
        elif k == 2:
            rr = int(rng.integers(r0, r1 - 1))
            t = float(rows[rr, 0])
        elif k == 3:
            t, rr = res[j]["T_xy"] * int(rng.integers(1, max(2, res[j]["c_xy"].shape[0] // 6))), -1
        elif k == 4:
            t, rr = float(rows[r1 - 1, 0]), r1 - 1
        elif k == 5:
            t, rr = float(rows[r1 - 1, 0]) + 3.0, r1 - 1
        else:
            t, rr = float(rng.uniform(0.0, rows[r1 - 1, 0])), -1
        tr.append(j), ts.append(t), kind.append(k), row.append(rr)
    return np.array(tr, dtype=np.int32), np.array(ts), np.array(kind), (offs, rows), np.array(row)


@pytest.fixture(scope="module")
def hill():
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 512, 12000)
    src, res = _source(m, ka, S, G)
    assert len(res) >= 400, len(res)
    tr, ts, kind, roll, row = _switch_times(src, res, 512, 5)
    _, G2 = _queries(m, 512, 13000)
    return dict(m=m, ka=ka, S=S, G=G, src=src, res=res, tr=tr, ts=ts, kind=kind, roll=roll, row=row, G2=G2)


def _end_goals(src, tr):
    """the goals of goals == NULL: each source problem's end position and normSO2 of its end yaw"""
    from uneven_planner_amd.alm_traj_opt import norm_so2
    st = src.plan_staged()
    return np.array([[st[j]["end_xy"][0, 0], st[j]["end_xy"][1, 0], norm_so2(st[j]["end_yaw"][0])] for j in tr])


def _composed(m, ka, sw, goals, **mk):
    """the host-chained form from the switch states: search (complete paths) -> uph_resample_batch -> the start boundary patched -> upload + solve on
    a fresh context"""
    import uneven_planner_amd as U
    from uneven_planner_amd import resample as R
    sr = ka.plan_batch(np.ascontiguousarray(sw[:, [0, 1, 6]]), goals, path_cap=1024, complete=True)
    found = [b for b, r in enumerate(sr) if r["status"] == 0]
    probs = R.resample_batch([sr[b]["path"] for b in found], cap_xy=4096, cap_yaw=4096, **mk)
    for b, p in zip(found, probs):
        p["init_xy"] = np.array(p["init_xy"], dtype=np.float64)
        p["init_xy"][:, 1] = sw[b, 2:4]
        p["init_xy"][:, 2] = sw[b, 4:6]
        p["init_yaw"] = np.array(p["init_yaw"], dtype=np.float64)
        p["init_yaw"][1], p["init_yaw"][2] = sw[b, 7], sw[b, 8]
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    opt.upload(probs)
    opt.solve()
    res = opt.download(full=True)
    return dict(status=np.array([r["status"] for r in sr]), found=np.array(found, dtype=np.int64), probs=probs, res=res, opt=opt)


def _same_results(a, b, tag=""):
    """bit for bit; NaN equals NaN (with goals == NULL a switch pose closer to the goal than one collision sample gives a zero-length path,
    total_time 0 and a NaN solve -- in both chains alike)"""
    assert len(a) == len(b), tag
    for j, (x, y) in enumerate(zip(a, b)):
        for k in SCALAR_KEYS:
            assert x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]), (tag, j, k, x[k], y[k])
        for k in RES_KEYS:
            if k in x or k in y:
                assert np.array_equal(x[k], y[k], equal_nan=True), (tag, j, k)


def _same_probs(staged, host, tag=""):
    assert len(staged) == len(host), tag
    for j, (x, y) in enumerate(zip(staged, host)):
        assert (x["n_inner_xy"], x["n_inner_yaw"]) == (y["inner_xy"].shape[1], y["inner_yaw"].shape[0]), (tag, j)
        for k in PROB_KEYS:
            a, b = np.asarray(x[k]), np.asarray(y[k])
            if not x["complete"]:
                b = b[..., :a.shape[-1]]
            assert np.array_equal(a, b, equal_nan=True), (tag, j, k)
        assert x["total_time"] == y["total_time"], (tag, j)


def _check_chain(opt, plan, comp, tag):
    found = comp["found"]
    assert np.array_equal(plan["status"], comp["status"]), tag
    assert np.array_equal(np.nonzero(plan["traj_of"] >= 0)[0], found) and np.array_equal(plan["traj_of"][found], np.arange(len(found))), tag
    assert np.array_equal(opt.origin(), found), tag
    assert np.array_equal(plan["n_inner_xy"][found], [p["inner_xy"].shape[1] for p in comp["probs"]]), tag
    assert np.array_equal(plan["n_inner_yaw"][found], [p["inner_yaw"].shape[0] for p in comp["probs"]]), tag
    assert (plan["n_inner_xy"][plan["traj_of"] < 0] == 0).all()


def _replan(h, goals, full=True, dst=None, **mk):
    import uneven_planner_amd as U
    if dst is None:
        dst = U.ALMTrajOpt(h["m"])
        dst.set_rho(1.0)
    out = dst.replan_goals(h["ka"], h["src"], h["tr"], h["ts"], goals=goals, full=full, **mk)
    return dst, out


def test_switch_state_equals_the_rollout_row(hill):
    """where t_switch is a rollout row's t (0, the dt grid, the duration) or clamps to one (before the start, beyond the end), the switch state is
    that row's x, y, yaw, dx, dy, ddx, ddy, dyaw bit for bit -- with the rollout's STATE-only and all-channel kernels; ddyaw and every other query
    equal the host mirror SE2Traj.getState on the downloaded coefficients to 1e-12"""
    from uneven_planner_amd.alm_traj_opt import SE2Traj
    dst, _ = _replan(hill, hill["G2"], full=False)
    sw = dst.last_plan["switch_states"]
    assert np.isfinite(sw).all()
    _, rows = hill["roll"]
    _, rows_all = hill["src"].rollout(0.05, channels=7, with_end=True)
    sel = hill["row"] >= 0
    assert sel.sum() >= 350 and set(hill["kind"][sel]) == {0, 1, 2, 4, 5}
    for q in np.nonzero(sel)[0]:
        r = hill["row"][q]
        assert np.array_equal(sw[q, :8], rows[r, ROW_OF_STATE]), (q, hill["kind"][q], sw[q], rows[r])
        assert np.array_equal(sw[q, :8], rows_all[r, ROW_OF_STATE]), q
    for q in range(sw.shape[0]):
        r = hill["res"][hill["tr"][q]]
        want = SE2Traj(r["c_xy"], r["c_yaw"], r["T_xy"], r["T_yaw"]).getState(hill["ts"][q])
        d = np.abs(sw[q] - want)
        d[6] = abs(math.remainder(sw[q, 6] - want[6], 2 * math.pi))
        assert (d <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (q, hill["kind"][q], d)
    moving = np.hypot(sw[:, 2], sw[:, 3])
    assert (moving > 0.2).sum() >= 200          # most switches happen at cruising speed: the starts PlanManager would form are 0.05 m/s


@pytest.mark.parametrize("goal_mode", ["new_goal", "same_goal"])
def test_device_chain_equals_composed_chain(hill, goal_mode):
    """uph_replan_upload + solve + download == the composed host chain from the switch states it returned, on the staged problems, the statuses,
    traj_of, the counts and every solved output; with goals == NULL the goals are the source problems' end poses"""
    goals = hill["G2"] if goal_mode == "new_goal" else None
    dst, out = _replan(hill, goals)
    plan = dst.last_plan
    sw = plan["switch_states"]
    g = hill["G2"] if goals is not None else _end_goals(hill["src"], hill["tr"])
    comp = _composed(hill["m"], hill["ka"], sw, g)
    _check_chain(dst, plan, comp, goal_mode)
    assert len(comp["found"]) >= 300, len(comp["found"])
    _same_probs(dst.plan_staged(), comp["probs"], goal_mode)
    _same_results([out[b] for b in comp["found"]], comp["res"], goal_mode)
    for b, r in enumerate(out):
        assert r["status"] == comp["status"][b]


def test_new_trajectories_start_in_the_switch_state(hill):
    """MINCO's start boundary is {P, V, A} and {yaw, dyaw, ddyaw}: row 0 of each new trajectory's rollout is the switch state -- position, velocity,
    acceleration and yaw rate to 1e-12, yaw modulo 2 pi -- and its yaw acceleration (host mirror) too.  goals == NULL: the new end pose is the
    source's end pose up to the search's last sample spacing (the path ends at the last collision sample of the one-shot, as the source's did)"""
    from uneven_planner_amd.alm_traj_opt import SE2Traj
    for goals in (hill["G2"], None):
        dst, out = _replan(hill, goals, full=False)
        sw = dst.last_plan["switch_states"]
        offs, rows = dst.rollout(0.05, channels=1, with_end=True)
        org = dst.origin()
        ends = _end_goals(hill["src"], hill["tr"])
        staged = dst.plan_staged()
        n = degenerate = 0
        for j, q in enumerate(org):
            r = out[q]
            if r["ret"] == 4:
                continue
            if not np.isfinite(r["c_xy"]).all():
                # (goals == NULL and the switch pose closer to the goal than one collision sample: the path is the start twice, the problem has no
                # length and total_time 0 -- as uph_plan_upload's problem for a start on its goal; the composed chain solves it the same way)
                assert goals is None and staged[j]["total_time"] == 0.0, (q, hill["kind"][q], staged[j]["total_time"])
                degenerate += 1
                continue
            n += 1
            row = rows[offs[j]]
            assert row[0] == 0.0
            for c in (0, 1, 2, 3, 4, 5, 7):
                assert abs(row[ROW_OF_STATE[c]] - sw[q, c]) <= 1e-12 * max(1.0, abs(sw[q, c])), (q, c, row, sw[q])
            assert abs(math.remainder(row[3] - sw[q, 6], 2 * math.pi)) <= 1e-12, q
            ddw = SE2Traj(r["c_xy"], r["c_yaw"], r["T_xy"], r["T_yaw"]).getState(0.0)[8]
            assert abs(ddw - sw[q, 8]) <= 1e-12 * max(1.0, abs(sw[q, 8])), q
            if goals is None:
                end = rows[offs[j + 1] - 1]
                assert math.hypot(end[1] - ends[q, 0], end[2] - ends[q, 1]) <= hill["ka"].collision_interval + 1e-9, q
        assert n >= (300 if goals is not None else 250), (n, degenerate)


def test_moving_starts_match_the_oracle(hill, oracle):
    """the moving-start problems as staged: initScaling and the first evaluation at the oracle's setup / init_scaling / eval to 1e-9; the solves of
    >= 256 of them drift no more one way from the oracle than the oracle's own FMA rebuild does"""
    import sensitivity
    m = hill["m"]
    dst, out = _replan(hill, hill["G2"], full=False)
    probs = dst.plan_staged()
    keep = [j for j, p in enumerate(probs) if p["complete"]]
    probs = [probs[j] for j in keep]
    assert len(probs) >= 300 and max(abs(p["init_xy"][0, 1]) + abs(p["init_xy"][1, 1]) for p in probs) > 0.2
    og = oracle.OracleGrid()
    og.set_cells(m.map_buffer)
    import uneven_planner_amd as U
    ev = U.ALMTrajOpt(m)
    ev.upload(probs)
    ev.init_scaling_batch()
    st = ev.download()
    f, g = ev.eval_batch(ev.x0_packed(probs))
    for i in range(0, len(probs), 6):
        a = oracle.OracleALM(og)
        x0 = a.setup(probs[i])
        a.init_scaling(x0)
        so = a.get_state()
        assert rel(so["scale_cx"], st[i]["scale_cx"]) < 1e-9 and abs(so["scale_fx"] - st[i]["scale_fx"]) <= 1e-9 * abs(so["scale_fx"]), i
        fo, go, _ = a.eval(x0)
        assert abs(f[i] - fo) <= 1e-9 * abs(fo) and rel(go, g[i]) < 1e-9, i
    sub = list(range(0, len(probs)))[:288]
    dev = [out[dst.origin()[keep[j]]] for j in sub]
    ps = [probs[j] for j in sub]
    ref = sensitivity.solve_many(lambda: oracle.OracleALM(og), ps, threads=16)
    fma = sensitivity.solve_with_fma_oracle(m.map_buffer, ps, threads=16)
    stt = sensitivity.drift_stats(ref, fma, dev)
    print("moving starts drift:", stt)
    sensitivity.assert_no_directional_drift(stt, "hill moving starts, %d solves" % len(ps))


def test_in_place_equals_separate_dst(hill):
    """dst == src: every state is taken before the batch is replaced -- the same switch states, plan and results as a separate dst"""
    import uneven_planner_amd as U
    sep = hill["src"]
    own, _ = _source(hill["m"], hill["ka"], hill["S"], hill["G"])         # the same source batch on a context of its own
    out_in = own.replan_goals(hill["ka"], own, hill["tr"], hill["ts"], goals=hill["G2"], full=True)
    dst = U.ALMTrajOpt(hill["m"])
    dst.set_rho(1.0)
    out_sep = dst.replan_goals(hill["ka"], sep, hill["tr"], hill["ts"], goals=hill["G2"], full=True)
    ref_plan = dst.last_plan
    for k in ("status", "traj_of", "n_inner_xy", "n_inner_yaw", "switch_states"):
        assert np.array_equal(own.last_plan[k], ref_plan[k]), k
    assert np.array_equal(own.origin(), dst.origin())
    found = np.nonzero(ref_plan["traj_of"] >= 0)[0]
    _same_results([out_in[b] for b in found], [out_sep[b] for b in found], "in place")


def test_local_frames_chain_equals_composed():
    """a 70 m grid: the source and the new problems are solved in local frames.  Switch states come back in map coordinates (equal to the rollout's
    rows, which add the frame shift) and the device chain equals the composed one bit for bit"""
    import uneven_planner_amd as U
    m = U.UnevenMap(dict(map_size_x=70.0, map_size_y=70.0, xy_resolution=0.1)).fill_fbm(dict(amplitude=3.0, max_slope_deg=12.0, rough_threshold=0.95))
    ka = U.KinoAstar(m)
    S, G = _queries(m, 48, 9800, half=33.0, dmin=2.0, dmax=5.0)
    src, res = _source(m, ka, S, G)
    assert len(res) >= 12
    offs, rows = src.rollout(0.05, channels=1, with_end=True)
    ok = [j for j, r in enumerate(res) if r["ret"] != 4]
    tr = np.array(ok, dtype=np.int32)
    ri = np.array([int(offs[j]) + (int(offs[j + 1]) - int(offs[j])) // 2 for j in ok])
    ts = rows[ri, 0].copy()
    assert np.abs(rows[ri, 1:3]).max() > 20.0
    h = dict(m=m, ka=ka, src=src, tr=tr, ts=ts)
    _, G2 = _queries(m, len(ok), 9900, half=33.0, dmin=2.0, dmax=5.0)
    G2[:, :2] = rows[ri, 1:3] + np.array([2.0, 1.5])      # a new goal near each vehicle
    dst, out = _replan(h, G2)
    sw = dst.last_plan["switch_states"]
    assert np.array_equal(sw[:, :8], rows[ri][:, ROW_OF_STATE])
    comp = _composed(m, ka, sw, G2)
    assert len(comp["found"]) >= 6, comp["status"]
    _check_chain(dst, dst.last_plan, comp, "frames")
    _same_probs(dst.plan_staged(), comp["probs"], "frames")
    _same_results([out[b] for b in comp["found"]], comp["res"], "frames")


def _raw(opt, ka, src, tr, ts, goals=None, B=None):
    from uneven_planner_amd import _lib
    from uneven_planner_amd import resample as R
    mp = _lib.ManagerParams(**R.MANAGER_PARAMS)
    tr = np.ascontiguousarray(tr, dtype=np.int32)
    ts = np.ascontiguousarray(ts, dtype=np.float64)
    B = tr.shape[0] if B is None else B
    st, to, nx, ny = (np.full(B, -9, dtype=np.int32) for _ in range(4))
    sw = np.full((B, 9), -9.0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(_lib.DP)
    g = None if goals is None else np.ascontiguousarray(goals, dtype=np.float64)
    rc = opt.L.uph_replan_upload(ka.h, src.h, opt.h, C.byref(mp), B, ip(tr), dp(ts), None if g is None else dp(g), 0, dp(sw), ip(st), ip(to), ip(nx), ip(ny))
    return rc, dict(status=st, traj_of=to, n_inner_xy=nx, n_inner_yaw=ny, switch_states=sw)


def _untouched(o):
    return all((o[k] == -9).all() for k in o)


def test_refusals_and_edges(hill):
    """refused with UPH_ERR_INVALID, every output untouched and dst's batch as it was: source not resident, an index out of range, an unsupported
    source slot, a NaN / infinite time, contexts on different maps, a pending asynchronous solve.  No query with a path: UPH_ERR_INVALID with the
    outputs written and no batch"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m, ka, src = hill["m"], hill["ka"], hill["src"]
    F = src.L.uph_batch_count(src.h)
    dst = U.ALMTrajOpt(m)
    dst.set_rho(1.0)
    dst.plan_goals(ka, hill["S"][:16], hill["G"][:16])
    nb = dst.L.uph_batch_count(dst.h)
    before = dst.rollout(0.1, channels=1)[1]
    tr, ts = hill["tr"][:4], hill["ts"][:4]

    def refused(rc, o, what):
        assert rc == -1 and _untouched(o), (what, rc)
        assert dst.L.uph_batch_count(dst.h) == nb and np.array_equal(dst.rollout(0.1, channels=1)[1], before), what

    fresh = U.ALMTrajOpt(m)
    fresh.plan_goals_upload(ka, hill["S"][:8], hill["G"][:8])                 # uploaded, not solved: no resident trajectory
    rc, o = _raw(dst, ka, fresh, [0], [0.5])
    refused(rc, o, "not resident")
    assert b"resident" in dst.L.uph_last_error()
    for bad in ([F], [-1], [0, F + 7]):
        rc, o = _raw(dst, ka, src, bad, [0.5] * len(bad))
        refused(rc, o, ("index", bad))
    for t in (float("nan"), float("inf"), -float("inf")):
        rc, o = _raw(dst, ka, src, tr, [0.1, t, 0.2, 0.3])
        refused(rc, o, ("time", t))
    # an UPH_RET_UNSUPPORTED slot: a problem beyond UPH_MAX_PIECE_XY next to ordinary ones
    probs = scenes.random_problems(3, seed0=2100)
    big = dict(probs[0])
    big["inner_xy"] = np.linspace([0.0, 0.0], [3.0, 0.5], 140).T.copy()
    big["inner_yaw"] = np.zeros(140)
    uns = U.ALMTrajOpt(m)
    uns.set_rho(1.0)
    r_uns = uns.optimize_batch(probs + [big])
    assert r_uns[3]["ret"] == 4
    rc, o = _raw(dst, ka, uns, [0, 3], [0.5, 0.5])
    refused(rc, o, "unsupported slot")
    assert b"UNSUPPORTED" in dst.L.uph_last_error()
    # contexts bound to another map
    other_map = _hill_map()
    other = U.ALMTrajOpt(other_map)
    rc, o = _raw(other, ka, src, tr, ts)
    assert rc == -1 and _untouched(o) and b"different maps" in other.L.uph_last_error()
    rc, o = _raw(dst, ka, other, [0], [0.5])
    refused(rc, o, "src on another map")
    # an asynchronous solve pending on the source, then on dst
    src2, _ = _source(m, ka, hill["S"][:32], hill["G"][:32])
    src2.solve_async()
    rc, o = _raw(dst, ka, src2, [0], [0.5])
    src2.wait()
    refused(rc, o, "pending src")
    dst.solve_async()
    rc, o = _raw(dst, ka, src2, [0], [0.5])
    dst.wait()
    assert rc == -1 and _untouched(o) and b"in flight" in dst.L.uph_last_error()
    # no query with a path: every goal outside the map
    far = np.tile([[40.0, 0.0, 0.0]], (4, 1))
    rc, o = _raw(dst, ka, src, tr, ts, goals=far)
    assert rc == -1 and b"no goal" in dst.L.uph_last_error()
    assert ((o["status"] >= 1) & (o["status"] <= 6)).all() and (o["traj_of"] == -1).all() and (o["n_inner_xy"] == 0).all()
    assert np.isfinite(o["switch_states"]).all()                               # written together with the statuses
    assert dst.L.uph_batch_count(dst.h) == 0


def test_occupied_switch_pose_fails_that_query_only():
    """the map changed under the vehicle: the cells around one trajectory's switch pose are rebuilt tilted beyond min_cnormal, so that pose is
    occupied.  Re-planned in place to the same goals, that query comes back UPH_KINO_START_OCCUPIED; the others keep the statuses a search from
    their switch states gets"""
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = [j for j, r in enumerate(res) if r["ret"] == 0]
    offs, rows = src.rollout(0.05, channels=1, with_end=True)
    mid = [int(offs[j]) + (int(offs[j + 1]) - int(offs[j])) // 2 for j in ok]
    p0 = rows[mid[0], 1:3]
    far = [i for i in range(1, len(ok)) if np.hypot(*(rows[mid[i], 1:3] - p0)) > 2.5][:15]
    assert len(far) >= 8
    pick = [0] + far
    tr = np.array([ok[i] for i in pick], dtype=np.int32)
    ts = np.array([rows[mid[i], 0] for i in pick])
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    cells = np.array(m.map_buffer, dtype=np.float64).reshape(nx, ny, nyaw, 4)
    xs = (np.arange(nx) + 0.5) * m.xy_resolution + m.map_origin[0]
    ys = (np.arange(ny) + 0.5) * m.xy_resolution + m.map_origin[1]
    near = np.hypot(xs[:, None] - p0[0], ys[None, :] - p0[1]) < 0.4
    cells[near, :, 2], cells[near, :, 3] = 0.8, 0.0                          # normal tilted: c_normal 0.6 < min_cnormal 0.8
    m.set_cells(cells.reshape(-1, 4))
    out = src.replan_goals(ka, src, tr, ts)
    st = np.array([r["status"] for r in out])
    sw = src.last_plan["switch_states"]
    assert st[0] == 1, st
    ref = ka.plan_batch(np.ascontiguousarray(sw[:, [0, 1, 6]]), np.ones_like(sw[:, :3]), path_cap=4)
    assert all((ref[q]["status"] == 1) == (st[q] == 1) for q in range(len(pick))), (st, [r["status"] for r in ref])
    assert (st[1:] == 0).sum() >= 4
