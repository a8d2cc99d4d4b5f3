"""GPU tier of the goals -> resident trajectories chain, uph_plan_upload (PlanManager::rcvWpsCallBack, plan_manager.cpp:43-134, with every stage on
the device): the search into device memory, PlanManager's resampling stage as a device kernel, the upload from the staged problems.

Bar: BIT FOR BIT against the composed host chain -- KinoAstar.plan_batch(complete=True) -> resample_batch (uph_resample_batch, host C++) ->
optimize_batch on a second, fresh context with the same parameters and rho.  tests/test_gpu_resample.py ties the host stage to the oracle, so the
chain is closed."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RES_KEYS = ("x", "c_xy", "c_yaw", "hx", "gx", "lam", "mu", "scale_cx")
SCALAR_KEYS = ("ret", "alm_iters", "lbfgs_iters", "evals", "last_lbfgs_ret", "cost", "jerk_cost", "T_xy", "T_yaw", "rho_final", "scale_fx")
PROB_KEYS = ("init_xy", "end_xy", "inner_xy", "init_yaw", "end_yaw", "inner_yaw")


def _queries(m, n, seed0, free=True, **kw):
    from uneven_planner_amd import scenes
    nx, ny = int(m.voxel_num[0]), int(m.voxel_num[1])
    if not free:
        return scenes.random_queries(n, seed0=seed0, **kw)
    return scenes.random_queries(n, seed0=seed0, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]), **kw)


def _map_from_cloud(name, params=None):
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m = U.UnevenMap(params)
    m.build(scenes.make_hill_cloud() if name == "hill" else np.load(os.path.join(GOLD, name + "_xyz.npz"))["xyz"])
    return m


@pytest.fixture(scope="module")
def hill():
    import uneven_planner_amd as U
    m = _map_from_cloud("hill")
    return m, U.KinoAstar(m)


def _composed(m, ka, S, G, full=True, **mk):
    """the host-chained form: search (complete paths) -> uph_resample_batch -> optimize_batch on a fresh context"""
    import uneven_planner_amd as U
    from uneven_planner_amd import resample as R
    sr = ka.plan_batch(S, G, path_cap=1024, complete=True)
    found = [b for b, r in enumerate(sr) if r["status"] == 0]
    probs = R.resample_batch([sr[b]["path"] for b in found], cap_xy=4096, cap_yaw=4096, **mk)
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    opt.upload(probs)
    opt.solve()
    res = opt.download(full=full)
    return dict(status=np.array([r["status"] for r in sr]), found=np.array(found, dtype=np.int64), probs=probs, res=res, opt=opt)


def _same_results(a, b, tag=""):
    assert len(a) == len(b), tag
    for j, (x, y) in enumerate(zip(a, b)):
        for k in SCALAR_KEYS:
            assert x[k] == y[k], (tag, j, k, x[k], y[k])
        for k in RES_KEYS:
            if k in x or k in y:
                assert np.array_equal(x[k], y[k]), (tag, j, k)


def _same_probs(staged, host, tag=""):
    """staged (plan_staged) against the host stage; NaN way-points compare equal (the test node's `if` comb leaves the remainder carried, so a
    repeated pose right after a node divides by a zero segment length -- in the reference as here).  A problem beyond the staging's capacity
    has its counts, boundary states, total_time and its first way-points compared"""
    assert len(staged) == len(host), tag
    n_cut = 0
    for j, (x, y) in enumerate(zip(staged, host)):
        assert (x["n_inner_xy"], x["n_inner_yaw"]) == (y["inner_xy"].shape[1], y["inner_yaw"].shape[0]), (tag, j)
        for k in PROB_KEYS:
            a, b = np.asarray(x[k]), np.asarray(y[k])
            if not x["complete"]:
                b = b[..., :a.shape[-1]]
                n_cut += k == "inner_xy"
            assert np.array_equal(a, b, equal_nan=True), (tag, j, k)
        assert x["total_time"] == y["total_time"], (tag, j)
    return n_cut


@pytest.mark.parametrize("scene", ["hill", "desert", "vocano"])
def test_staged_problems_equal_the_host_stage(scene):
    """uph_plan_staged (the device's resampling of the paths the search left in HBM, boundary velocities formed on the host) equals
    uph_resample_batch on the same complete paths: counts, way-points, boundary states and total_time, bit for bit -- PlanManager's stage with
    the run_hill values and with another parameter set, and the test node's variant"""
    import uneven_planner_amd as U
    m = _map_from_cloud(scene, dict(max_rho=0.08) if scene == "vocano" else None)
    ka = U.KinoAstar(m)
    S, G = _queries(m, 96, 9100)
    from uneven_planner_amd import resample as R
    sr = ka.plan_batch(S, G, path_cap=1024, complete=True)
    found = [b for b, r in enumerate(sr) if r["status"] == 0]
    assert len(found) >= 24, (scene, len(found))
    paths = [sr[b]["path"] for b in found]
    opt = U.ALMTrajOpt(m)
    for mk in (dict(), dict(piece_len=0.2, yaw_piece_times=3.0, mean_vel=0.7, init_time_times=1.4, init_sig_vel=0.08), dict(test_mode=1, test_max_vel=0.5)):
        plan = opt.plan_goals_upload(ka, S, G, **mk)
        assert np.array_equal(plan["status"], [r["status"] for r in sr])
        assert np.array_equal(np.nonzero(plan["traj_of"] >= 0)[0], found) and np.array_equal(opt.origin(), found)
        host = R.resample_batch(paths, cap_xy=4096, cap_yaw=4096, **mk)
        assert np.array_equal(plan["n_inner_xy"][found], [h["inner_xy"].shape[1] for h in host])
        assert np.array_equal(plan["n_inner_yaw"][found], [h["inner_yaw"].shape[0] for h in host])
        _same_probs(opt.plan_staged(), host, (scene, mk))


@pytest.fixture(scope="module")
def hill512(hill):
    """512 hill goals: 500 drawn without looking at the occupancy (some starts / goals occupied), 12 with a start or goal outside the map"""
    m, ka = hill
    S, G = _queries(m, 500, 9300, free=False)
    S = np.concatenate([S, [[4.0, -4.0, 0.0]] * 6, [[30.0, 1.0, 0.0]] * 6])
    G = np.concatenate([G, [[-60.0, 0.0, 1.0]] * 6, [[1.0, 1.0, 0.0]] * 6])
    comp = _composed(m, ka, S, G)
    return S, G, comp


def _check_chain(opt, plan, comp, tag):
    found = comp["found"]
    assert np.array_equal(plan["status"], comp["status"]), tag
    assert np.array_equal(np.nonzero(plan["traj_of"] >= 0)[0], found) and np.array_equal(plan["traj_of"][found], np.arange(len(found))), tag
    assert (plan["traj_of"][comp["status"] != 0] == -1).all()
    assert np.array_equal(opt.origin(), found), tag


def test_chain_equals_the_composed_chain(hill, hill512):
    """uph_plan_upload + uph_batch_solve + uph_batch_download == plan_batch(complete) -> resample_batch -> optimize_batch, every output of every goal;
    goals without a path carry the search status and traj_of = -1"""
    import uneven_planner_amd as U
    m, ka = hill
    S, G, comp = hill512
    assert (comp["status"] != 0).sum() >= 12 and len(comp["found"]) >= 300
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    out = opt.plan_goals(ka, S, G, full=True)
    plan = opt.last_plan
    _check_chain(opt, plan, comp, "chain")
    for b, r in enumerate(out):
        assert r["status"] == comp["status"][b]
    _same_results([out[b] for b in comp["found"]], comp["res"], "chain")


def test_clipped_paths_are_searched_again(hill, hill512):
    """path_cap = 8 clips every path of the first search: all of them come from the second search, and the results are those of test 2"""
    import uneven_planner_amd as U
    m, ka = hill
    S, G, comp = hill512
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    out = opt.plan_goals(ka, S, G, full=True, path_cap=8)
    _check_chain(opt, opt.last_plan, comp, "cap 8")
    _same_results([out[b] for b in comp["found"]], comp["res"], "cap 8")


def test_existing_calls_work_on_the_planned_batch(hill, hill512):
    """uph_batch_origin = the found goals; uph_report_batch and uph_rollout_batch equal the composed context's bit for bit; the split form with
    solve_async / wait equals the blocking one"""
    import uneven_planner_amd as U
    m, ka = hill
    S, G, comp = hill512
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    plan = opt.plan_goals_upload(ka, S, G)
    opt.solve_async()
    opt.wait()
    res = opt.download(full=True)
    _check_chain(opt, plan, comp, "async")
    _same_results(res, comp["res"], "async")
    assert np.array_equal(opt.getMaxVxAxAyCurAttSig(), comp["opt"].getMaxVxAxAyCurAttSig())
    for ch, dt in ((7, 0.05), (4, 0.03)):
        o1, r1 = opt.rollout(dt, channels=ch, with_end=True)
        o2, r2 = comp["opt"].rollout(dt, channels=ch, with_end=True)
        assert np.array_equal(o1, o2) and np.array_equal(r1, r2)


def test_unsupported_problems_keep_their_slot(hill):
    """piece_len 0.05 on goals more than 6.4 m apart needs more than UPH_MAX_PIECE_XY position pieces: those slots come back UPH_RET_UNSUPPORTED
    (their way-points never fitted the staging), their neighbours equal the composed chain's results"""
    import uneven_planner_amd as U
    m, ka = hill
    S1, G1 = _queries(m, 24, 9500, dmin=6.6, dmax=9.0)
    S2, G2 = _queries(m, 24, 9600, dmin=1.0, dmax=2.5)
    S, G = np.concatenate([S1, S2]), np.concatenate([G1, G2])
    mk = dict(piece_len=0.05)
    comp = _composed(m, ka, S, G, **mk)
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    out = opt.plan_goals(ka, S, G, full=True, **mk)
    _check_chain(opt, opt.last_plan, comp, "unsupported")
    got = [out[b] for b in comp["found"]]
    uns = [j for j, r in enumerate(comp["res"]) if r["ret"] == 4]
    assert len(uns) >= 8 and len(uns) < len(got)
    assert all(got[j]["ret"] == 4 and got[j]["last_lbfgs_ret"] == -4 for j in uns)
    _same_results(got, comp["res"], "unsupported")


def test_nothing_found_leaves_no_batch(hill):
    """no goal with a path: UPH_ERR_INVALID, the statuses are written, the context holds no batch and a rollout is refused"""
    import uneven_planner_amd as U
    from uneven_planner_amd import _lib
    from uneven_planner_amd import resample as R
    m, ka = hill
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    S, G = _queries(m, 8, 9700)
    opt.plan_goals(ka, S, G)
    assert opt.L.uph_batch_count(opt.h) > 0
    S = np.array([[40.0, 0.0, 0.0]] * 3 + [[1.0, 1.0, 0.0]] * 2)
    G = np.array([[1.0, 1.0, 0.0]] * 3 + [[-45.0, 2.0, 0.0]] * 2)
    mp = _lib.ManagerParams(**R.MANAGER_PARAMS)
    st, to, nx, ny = (np.full(5, 9, dtype=np.int32) for _ in range(4))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: np.ascontiguousarray(a).ctypes.data_as(_lib.DP)
    rc = opt.L.uph_plan_upload(ka.h, opt.h, C.byref(mp), 5, dp(S), dp(G), 0, ip(st), ip(to), ip(nx), ip(ny))
    assert rc == -1 and b"no goal" in opt.L.uph_last_error()
    assert ((st >= 1) & (st <= 6)).all() and (to == -1).all() and (nx == 0).all()          # (every search refused or failed, statuses written)
    assert opt.L.uph_batch_count(opt.h) == 0
    with pytest.raises(_lib.UnevenHipError):
        opt.rollout(0.05)
    out = opt.plan_goals(ka, S, G)                     # the Python door: one status per goal, no raise
    assert [r["status"] for r in out] == st.tolist() and opt._B == 0
    # a context bound to another map is refused
    other = U.ALMTrajOpt(_map_from_cloud("hill"))
    st[:] = -1
    assert other.L.uph_plan_upload(ka.h, other.h, C.byref(mp), 5, dp(S), dp(G), 0, ip(st), ip(to), ip(nx), ip(ny)) == -1
    assert b"different maps" in other.L.uph_last_error() and (st == -1).all()      # (refused before the search: outputs untouched)


def test_local_frames_chain_equals_composed():
    """a grid reaching beyond FRAME_EXTENT (32 m) from its origin: every problem is solved in its own local frame, so the x0 scatter subtracts the
    frame shift from the staged way-points -- the results equal the composed chain bit for bit"""
    import uneven_planner_amd as U
    m = U.UnevenMap(dict(map_size_x=70.0, map_size_y=70.0, xy_resolution=0.1)).fill_fbm(dict(amplitude=3.0, max_slope_deg=12.0, rough_threshold=0.95))
    ka = U.KinoAstar(m)
    S, G = _queries(m, 48, 9800, half=33.0, dmin=2.0, dmax=5.0)
    comp = _composed(m, ka, S, G)
    assert len(comp["found"]) >= 12, comp["status"]
    mids = [0.5 * (p["init_xy"][:, 0] + p["end_xy"][:, 0]) for p in comp["probs"]]
    assert max(np.abs(v).max() for v in mids) > 20.0       # problems whose frames are shifted far from the origin
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    out = opt.plan_goals(ka, S, G, full=True)
    _check_chain(opt, opt.last_plan, comp, "frames")
    _same_results([out[b] for b in comp["found"]], comp["res"], "frames")
    o1, r1 = opt.rollout(0.05, with_end=True)
    o2, r2 = comp["opt"].rollout(0.05, with_end=True)
    assert np.array_equal(o1, o2) and np.array_equal(r1, r2)


CPP = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
#include <cstdio>
using namespace uneven_hip;
int main(int argc, char** argv) {
    FILE* f = std::fopen(argv[1], "rb");
    long long hdr[2];
    if (!f || fread(hdr, 8, 2, f) != 2) return 2;
    std::vector<double> cells((size_t)hdr[0] * 4), sg((size_t)hdr[1] * 6);
    if (fread(cells.data(), 8, cells.size(), f) != cells.size() || fread(sg.data(), 8, sg.size(), f) != sg.size()) return 2;
    std::fclose(f);
    uph_map_params mp = {2, 10.0, 10.0, 0.2, 0.1, 0.1, 0.05, 0.1, 0.8, 0.05, 9.81};
    UnevenMapHandle map(mp, 0);
    map.setCells(cells.data());
    KinoAstar kino;
    kino.setEnvironment(&map);
    ALMTrajOpt opt;
    opt.setEnvironment(&map);
    std::vector<std::array<double, 3>> starts((size_t)hdr[1]), goals((size_t)hdr[1]);
    for (long long b = 0; b < hdr[1]; b++) for (int k = 0; k < 3; k++) { starts[b][k] = sg[6 * b + k]; goals[b][k] = sg[6 * b + 3 + k]; }
    uph_manager_params mgr{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5};
    ALMTrajOpt::GoalPlan p = opt.planSE2TrajBatch(kino, starts, goals, mgr);
    // per goal: status, traj_of, ret, jerk_cost, total_time, nxy, nyaw, then per piece duration + coeff[d][0..5] (highest order first)
    FILE* o = std::fopen(argv[2], "wb");
    for (size_t b = 0; b < starts.size(); b++) {
        const SE2Trajectory& t = p.traj[b];
        double h[7] = {(double)p.status[b], (double)p.traj_of[b], (double)p.ret[b], p.jerk_cost[b], p.total_time[b], (double)t.pos_traj.getPieceNum(),
                       (double)t.yaw_traj.getPieceNum()};
        fwrite(h, 8, 7, o);
        for (int i = 0; i < t.pos_traj.getPieceNum(); i++) { double d = t.pos_traj[i].getDuration(); fwrite(&d, 8, 1, o); fwrite(t.pos_traj[i].coeff, 8, 12, o); }
        for (int i = 0; i < t.yaw_traj.getPieceNum(); i++) { double d = t.yaw_traj[i].getDuration(); fwrite(&d, 8, 1, o); fwrite(t.yaw_traj[i].coeff, 8, 6, o); }
    }
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_matches_ctypes_bit_for_bit(tmp_path, analytic_cells):
    """ALMTrajOpt::planSE2TrajBatch from a compiled C++ consumer against plan_goals through ctypes: statuses, return codes, jerk costs and every
    coefficient of every goal's trajectory; goals without a path come back empty with ret -1"""
    import uneven_planner_amd as U
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    ka = U.KinoAstar(m)
    S, G = _queries(m, 30, 9900, free=False)
    S = np.concatenate([S, [[40.0, 0.0, 0.0]]])
    G = np.concatenate([G, [[1.0, 1.0, 0.0]]])
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    out = opt.plan_goals(ka, S, G)
    src = tmp_path / "goals.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "goals")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    cells = np.ascontiguousarray(analytic_cells, dtype=np.float64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2q", cells.shape[0], S.shape[0]))
        f.write(cells.tobytes())
        f.write(np.ascontiguousarray(np.concatenate([S, G], axis=1), dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, dtype=np.float64)
    at, n_found = 0, 0
    for b, r in enumerate(out):
        h = raw[at:at + 7]
        at += 7
        assert int(h[0]) == r["status"], b
        if r["status"] != 0:
            assert int(h[1]) == -1 and int(h[2]) == -1 and h[5] == 0 and h[6] == 0
            continue
        n_found += 1
        assert int(h[1]) == r["traj_of"] and int(h[2]) == r["ret"] and h[3] == r["jerk_cost"]
        nxy, nyaw = int(h[5]), int(h[6])
        assert nxy == r["c_xy"].shape[0] // 6 and nyaw == r["c_yaw"].shape[0] // 6 and h[4] == nxy * r["T_xy"]
        for i in range(nxy):
            blk = raw[at:at + 13]
            at += 13
            assert blk[0] == r["T_xy"]
            cx = blk[1:].reshape(2, 6)[:, ::-1]            # coeff[d][5 - k] = c_xy row 6 i + k, column d
            assert np.array_equal(cx.T, r["c_xy"][6 * i:6 * i + 6])
        for i in range(nyaw):
            blk = raw[at:at + 7]
            at += 7
            assert blk[0] == r["T_yaw"] and np.array_equal(blk[1:][::-1], r["c_yaw"][6 * i:6 * i + 6])
    assert at == raw.size and n_found >= 15
