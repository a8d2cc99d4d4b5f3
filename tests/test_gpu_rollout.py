"""Device rollout of solved trajectories (include/uneven_hip.h uph_rollout_*): the resident batch sampled every dt on the device -- states,
the per-sample terms behind the report, and visSE3Traj's SE(3) path (alm_traj_opt.cpp:1102-1135) -- checked against host evaluations of
the downloaded coefficients, the oracle's terrain lookups, uph_terrain_pose_query, the device report, and each other's call forms."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from piece_sweep import ref_terms, report_from_terms

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST, TR, PO = 1, 2, 4


def _norm_so2(y):                           # UnevenMap::normSO2 (uneven_map.cpp:63-70)
    while y > math.pi:
        y -= 2.0 * math.pi
    while y < -math.pi:
        y += 2.0 * math.pi
    return y


def _piece(T, N, t):                        # locatePieceIdx (se2traj.hpp:343-361), uniform durations
    i = 0
    while i < N and t > T:
        t -= T
        i += 1
    if i == N:
        i -= 1
        t += T
    return i, t


def _poly(c, t):                            # value, first, second derivative; c ascending powers
    v = sum(c[k] * t ** k for k in range(6))
    d = sum(k * c[k] * t ** (k - 1) for k in range(1, 6))
    a = sum(k * (k - 1) * c[k] * t ** (k - 2) for k in range(2, 6))
    return v, d, a


def host_state(r, t):
    """(x, y, normSO2 yaw, dx, dy, ddx, ddy, dyaw) of a downloaded result at t (SE2Trajectory getValue / getVel / getAcc)"""
    cxy, cyaw = np.asarray(r["c_xy"]), np.asarray(r["c_yaw"])
    nxy, nyaw = cxy.shape[0] // 6, cyaw.shape[0] // 6
    i, tl = _piece(r["T_xy"], nxy, t)
    px = _poly(cxy[6 * i:6 * i + 6, 0], tl)
    py = _poly(cxy[6 * i:6 * i + 6, 1], tl)
    j, tw = _piece(r["T_yaw"], nyaw, t)
    pw = _poly(cyaw[6 * j:6 * j + 6], tw)
    return np.array([px[0], py[0], _norm_so2(pw[0]), px[1], py[1], px[2], py[2], pw[1]])


def total_duration(r):
    dx = 0.0
    for _ in range(np.asarray(r["c_xy"]).shape[0] // 6):
        dx += r["T_xy"]
    dy = 0.0
    for _ in range(np.asarray(r["c_yaw"]).shape[0] // 6):
        dy += r["T_yaw"]
    return dx if dx < dy else dy


def running_times(total, dt):
    t, out = 0.0, []
    while t < total:
        out.append(t)
        t += dt
    return np.array(out)


def close(a, b, tol=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    scale = np.maximum(1.0, np.abs(b).max(axis=0))
    err = (np.abs(a - b) / scale).max()
    assert err <= tol, err


@pytest.fixture(scope="module")
def hill(analytic_cells):
    import uneven_planner_amd as U
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    return m


@pytest.fixture(scope="module")
def solved(hill):
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    probs = scenes.random_problems(10, seed0=4100, dmin=2.0, dmax=6.0)
    opt = U.ALMTrajOpt(hill)
    opt.set_rho(1.0)
    out = opt.optimize_batch(probs)
    return opt, probs, out


def test_sizes_and_times(solved):
    from uneven_planner_amd import alm_traj_opt as A
    opt, probs, out = solved
    for dt, we in ((0.01, False), (0.03, True), (0.07, False)):
        offs = opt.rollout_plan(dt, we)
        ref = A.rollout_sizes([o["c_xy"].shape[0] // 6 for o in out], [o["T_xy"] for o in out], [o["c_yaw"].shape[0] // 6 for o in out],
                              [o["T_yaw"] for o in out], dt, we)
        assert np.array_equal(offs, ref)
        o2, rows = opt.rollout(dt, ST, we)
        assert np.array_equal(o2, offs)
        for b, r in enumerate(out):
            t = rows[offs[b]:offs[b + 1], 0]
            tt = running_times(total_duration(r), dt)
            if we:
                tt = np.append(tt, total_duration(r))
            assert np.array_equal(t, tt), b                # the running sum, bit for bit


def test_states_match_host_evaluation(solved):
    opt, probs, out = solved
    offs, rows = opt.rollout(0.03, ST, with_end=True)
    for b, r in enumerate(out):
        blk = rows[offs[b]:offs[b + 1]]
        ref = np.array([host_state(r, t) for t in blk[:, 0]])
        close(blk[:, 1:], ref)


def test_terrain_terms_match_oracle(solved, oracle_grid, hill):
    opt, probs, out = solved
    offs, rows = opt.rollout(0.01, ST | TR)
    ref = ref_terms(oracle_grid, rows[:, 1:9], hill.params["gravity"])
    close(rows[:, 9:16], ref)


def test_poses_match_pose_query(solved, hill):
    """the same source (locate, terrainValues, terrainPoseFrom) as uph_terrain_pose_query; the two kernels are contracted into FMAs by the
    compiler each in its own way, so the last bit of an interpolated normal may differ"""
    opt, probs, out = solved
    offs, rows = opt.rollout(0.01, ST | PO, with_end=True)
    R, p = hill.getTerrainPosBatch(rows[:, 1:4])
    q = np.concatenate([R.transpose(0, 2, 1).reshape(-1, 9), p], axis=1)
    close(rows[:, 9:21], q, 1e-15)
    assert np.array_equal(rows[:, 18:20], rows[:, 1:3])                 # p = the sample's own (x, y)


def test_report_follows_from_terrain_columns(solved):
    opt, probs, out = solved
    rep = opt.getMaxVxAxAyCurAttSig()
    offs, rows = opt.rollout(0.01, TR)
    for b in range(len(out)):
        want = report_from_terms(rows[offs[b]:offs[b + 1]])          # (piece_sweep: signed largest magnitude with maxima from 0, att from -1, sigma from 0)
        for k in range(6):
            assert rep[b, k] == want[k], (b, k)
        assert abs(rep[b, 6] - want[6]) <= 1e-12 * abs(rep[b, 6])


def test_vis_se3_grid_ends_at_the_end_pose(solved, hill):
    opt, probs, out = solved
    offs, rows = opt.rollout(0.03, ST | PO, with_end=True)
    for b, r in enumerate(out):
        last = rows[offs[b + 1] - 1]
        assert last[0] == total_duration(r)
        assert np.abs(last[1:3] - np.asarray(probs[b]["end_xy"])[:, 0]).max() < 1e-9
        R, p = hill.getTerrainPosBatch(last[None, 1:4])
        close(last[None, 9:], np.concatenate([R[0].T.ravel(), p[0]])[None], 1e-15)
        assert offs[b + 1] - offs[b] == len(running_times(total_duration(r), 0.03)) + 1


def test_far_from_origin_rows_in_map_coordinates():
    """a grid reaching beyond FRAME_EXTENT: every trajectory is solved in its own local frame (uph_common.hpp TrajFrame); its rows come back in
    map coordinates"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    big = U.UnevenMap(dict(map_size_x=160.0, map_size_y=160.0, xy_resolution=0.25)).fill_fbm()
    nx, ny = int(big.voxel_num[0]), int(big.voxel_num[1])
    far, seed = [], 7300
    while len(far) < 6:
        p = scenes.local_problems(1, seed0=seed, half=75.0, dmin=4.0, dmax=9.0, occ_r2=big.occ_r2_buffer, grid=(nx, ny, big.xy_resolution, big.map_origin[0], big.map_origin[1]))[0]
        seed += 1
        if max(abs(p["init_xy"][0, 0]), abs(p["init_xy"][1, 0])) > 45.0:
            far.append(p)
    opt = U.ALMTrajOpt(big)
    opt.set_rho(1.0)
    out = opt.optimize_batch(far)
    offs, rows = opt.rollout(0.03, ST | PO, with_end=True)
    for b, r in enumerate(out):
        blk = rows[offs[b]:offs[b + 1]]
        assert np.abs(blk[0, 1:3] - np.asarray(far[b]["init_xy"])[:, 0]).max() < 1e-9
        close(blk[:, 1:9], np.array([host_state(r, t) for t in blk[:, 0]]))
    R, p = big.getTerrainPosBatch(rows[:, 1:4])
    close(rows[:, 9:21], np.concatenate([R.transpose(0, 2, 1).reshape(-1, 9), p], axis=1))


def test_fp32_cells_and_fp32_sample_context(oracle):
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m32 = U.UnevenMap(dict(map_size_x=32.0, map_size_y=32.0, xy_resolution=0.25), storage="f32").fill_fbm(dict(patch_lambda=5.0, rough_threshold=0.5))
    og = oracle.OracleGrid(size_x=32.0, size_y=32.0, xy_res=0.25)
    og.set_cells(m32.map_buffer)
    nx, ny = int(m32.voxel_num[0]), int(m32.voxel_num[1])
    probs = scenes.local_problems(6, seed0=5000, half=14.0, dmin=4.0, dmax=12.0, occ_r2=m32.occ_r2_buffer,
                                  grid=(nx, ny, m32.xy_resolution, m32.map_origin[0], m32.map_origin[1]))
    for bits in (64, 32):
        opt = U.ALMTrajOpt(m32)
        opt.set_sample_precision(bits)
        opt.set_rho(1.0)
        opt.optimize_batch(probs)
        offs, rows = opt.rollout(0.01, ST | TR)
        assert offs[-1] > 0
        close(rows[:, 9:16], ref_terms(og, rows[:, 1:9], m32.params["gravity"]))


def test_call_forms_agree_bit_for_bit(solved):
    import torch
    opt, probs, out = solved
    offs, full = opt.rollout(0.03, 7, with_end=True)
    B = len(out)
    parts = [opt.rollout(0.03, 7, with_end=True, b0=a, b1=min(B, a + 3))[1] for a in range(0, B, 3)]
    assert np.array_equal(np.concatenate(parts), full)
    o2, dev = opt.rollout(0.03, 7, with_end=True, device=True)
    assert isinstance(dev, torch.Tensor) and dev.dtype == torch.float64 and dev.is_cuda
    assert np.array_equal(o2, offs) and np.array_equal(dev.cpu().numpy(), full)
    cols = {ST: slice(0, 9), TR: slice(9, 16), PO: slice(16, 28)}
    for mask in (ST, TR, PO, ST | PO, TR | PO):
        _, sub = opt.rollout(0.03, mask, with_end=True)
        assert np.array_equal(sub, np.concatenate([full[:, cols[g]] for g in (ST, TR, PO) if mask & g], axis=1)), mask
    views = __import__("uneven_planner_amd.alm_traj_opt", fromlist=["split_rollout"]).split_rollout(offs, full)
    assert len(views) == B and all(v.shape[0] == offs[i + 1] - offs[i] for i, v in enumerate(views))


def test_multi_context_rollout_in_caller_order(solved, hill):
    import uneven_planner_amd as U
    opt, probs, out = solved
    _, single = opt.rollout(0.01, 7)
    offs1 = opt.rollout_plan(0.01)
    a, b = U.ALMTrajOpt(hill), U.ALMTrajOpt(hill)
    a.set_rho(1.0); b.set_rho(1.0)
    U.ALMTrajOpt.optimize_batch_multi([a, b], probs)
    assert 0 < a.L.uph_batch_count(a.h) < len(probs)
    offs, rows = U.ALMTrajOpt.rollout_multi([a, b], 0.01, 7)
    assert np.array_equal(offs, offs1) and np.array_equal(rows, single)


def test_unsupported_problem_has_no_rows(solved, hill):
    import uneven_planner_amd as U
    opt, probs, out = solved
    bad = dict(probs[1])
    bad["inner_xy"] = np.asarray(probs[1]["inner_xy"])
    bad["inner_yaw"] = np.asarray(probs[1]["inner_yaw"])[:max(0, np.asarray(probs[1]["inner_xy"]).shape[1] - 2)]     # fewer yaw than xy pieces
    o = U.ALMTrajOpt(hill)
    o.set_rho(1.0)
    res = o.optimize_batch([probs[0], bad, probs[2]])
    assert res[1]["ret"] == 4
    offs, rows = o.rollout(0.03, 7, with_end=True)
    assert offs[2] == offs[1]
    ref_offs, ref = opt.rollout(0.03, 7, with_end=True, b0=0, b1=3)
    assert np.array_equal(rows[offs[0]:offs[1]], ref[ref_offs[0]:ref_offs[1]])
    assert np.array_equal(rows[offs[2]:offs[3]], ref[ref_offs[2]:ref_offs[3]])


def test_refusals(hill, small_problems):
    import uneven_planner_amd as U
    o = U.ALMTrajOpt(hill)
    o.upload(small_problems)
    with pytest.raises(U._lib.UnevenHipError, match="resident"):
        o.rollout(0.01)
    L = o.L
    buf = np.zeros(16)
    dp = buf.ctypes.data_as(U._lib.DP)
    assert L.uph_rollout_batch(o.h, 0.01, 0, 7, 0, 1, dp) == -1
    o.set_rho(1.0)
    o.solve()
    offs = o.rollout_plan(0.01)
    assert offs[-1] > 0
    for dt in (0.0, -0.01, float("nan"), float("inf")):
        assert L.uph_rollout_batch(o.h, dt, 0, 7, 0, 1, dp) == -1
    for b0, b1 in ((-1, 1), (2, 1), (0, len(small_problems) + 1)):
        assert L.uph_rollout_batch(o.h, 0.01, 0, 7, b0, b1, dp) == -1
    assert L.uph_rollout_batch(o.h, 0.01, 0, 0, 0, 1, dp) == -1
    assert L.uph_rollout_batch(o.h, 0.01, 0, 8, 0, 1, dp) == -1
    assert L.uph_rollout_batch(o.h, 0.01, 0, 7, 0, 1, None) == -1
    assert L.uph_rollout_batch_dev(o.h, 0.01, 0, 7, 0, 1, None) == -1
    # an evaluation stores a trajectory as well; the next upload clears it again
    o.upload(small_problems)
    o.eval_batch(o.x0_packed(small_problems))
    assert o.rollout_plan(0.01)[-1] > 0
    o.upload(small_problems)
    with pytest.raises(U._lib.UnevenHipError):
        o.rollout_plan(0.01)


MAIN_SE3 = r"""
#include <cstdio>
#include <cstdlib>
static std::vector<double> readv(FILE* f, size_t n) { std::vector<double> v(n); if (fread(v.data(), 8, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(3); } return v; }
int main(int argc, char** argv) {
    // in:  header {ncell, n_inner_xy, n_inner_yaw}, cells[ncell*4], init_xy[6], end_xy[6], inner_xy[2*nxy], init_yaw[3], end_yaw[3], inner_yaw[nyaw], total_time
    FILE* f = std::fopen(argv[1], "rb");
    long long hdr[3];
    if (!f || fread(hdr, 8, 3, f) != 3) return 2;
    const long long ncell = hdr[0]; const int nxy = (int)hdr[1], nyaw = (int)hdr[2];
    std::vector<double> cells = readv(f, (size_t)ncell * 4);
    Mat init_xy(2, 3), end_xy(2, 3), inner_xy(2, nxy), init_yaw(3, 1), end_yaw(3, 1), inner_yaw(nyaw, 1);
    init_xy.v = readv(f, 6); end_xy.v = readv(f, 6); inner_xy.v = readv(f, 2 * (size_t)nxy);
    init_yaw.v = readv(f, 3); end_yaw.v = readv(f, 3); inner_yaw.v = readv(f, nyaw);
    const double total_time = readv(f, 1)[0];
    std::fclose(f);
    uph_map_params mp = {2, 10.0, 10.0, 0.2, 0.1, 0.1, 0.05, 0.1, 0.8, 0.05, 9.81};
    UnevenMapHandle map(mp, 0);
    map.setCells(cells.data());
    FakeNodeHandle nh;
    ALMTrajOpt traj_opt;
    traj_opt.init(nh);
    traj_opt.setEnvironment(&map);
    const int rc = traj_opt.optimizeSE2Traj(init_xy, end_xy, inner_xy, init_yaw, end_yaw, inner_yaw, total_time);
    SE2Trajectory back_end_traj = traj_opt.getTraj();
    traj_opt.visSE3Traj(back_end_traj);
    const std::vector<SE3Pose> path = traj_opt.getSE3Path();
    FILE* o = std::fopen(argv[2], "wb");
    double head[2] = {(double)rc, (double)path.size()};
    fwrite(head, 8, 2, o);
    for (const SE3Pose& p : path) { fwrite(p.R, 8, 9, o); fwrite(p.p, 8, 3, o); }
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_se3_path_matches_ctypes(tmp_path, analytic_cells, hill_problem, hill):
    import uneven_planner_amd as U
    from test_abi_cpu import CONSUMER
    src = tmp_path / "se3.cpp"
    src.write_text(CONSUMER + MAIN_SE3)
    exe = str(tmp_path / "se3")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", libdir,
                           "-lunevenhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    pr = hill_problem
    cells = np.ascontiguousarray(analytic_cells, dtype=np.float64)
    ixy = np.asarray(pr["inner_xy"], dtype=np.float64)
    iyw = np.asarray(pr["inner_yaw"], dtype=np.float64).ravel()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3q", cells.shape[0], ixy.shape[1], iyw.shape[0]))
        f.write(cells.tobytes())
        f.write(np.asarray(pr["init_xy"], dtype=np.float64).T.tobytes())
        f.write(np.asarray(pr["end_xy"], dtype=np.float64).T.tobytes())
        f.write(ixy.T.tobytes())
        f.write(np.asarray(pr["init_yaw"], dtype=np.float64).ravel().tobytes())
        f.write(np.asarray(pr["end_yaw"], dtype=np.float64).ravel().tobytes())
        f.write(iyw.tobytes())
        f.write(struct.pack("<d", float(pr["total_time"])))
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, dtype=np.float64)
    rc, n = int(raw[0]), int(raw[1])
    poses = raw[2:].reshape(n, 12)
    opt = U.ALMTrajOpt(hill)
    opt.set_rho(1.0)
    out = opt.optimize_batch([pr])
    assert rc == out[0]["ret"]
    offs, rows = opt.rollout(0.03, PO, with_end=True)
    assert n == offs[1] > 1 and np.array_equal(poses, rows)
