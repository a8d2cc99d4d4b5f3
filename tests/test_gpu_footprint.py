"""GPU tier of the oriented-rectangle footprints between resident trajectories (uph_footprint_separation_batch, uph_footprint_conflicts_batch;
uph_footprint_kernel).

The mirror's inputs are traj_states rows fetched from the device -- columns 0, 1 and 9 at tau - t0 --, so position and yaw are the same numbers on both
sides.  What remains between footprint_rows / footprint_clearance2 and the kernel are the sine and cosine (each under 0.8 ulp) and a few dozen roundings on
lengths of at most 15 m: about 1e-12 m^2 in c2.  TOL = 1e-9 m^2, the figure test_gpu_locate.py P5 uses for the same kind of quantity.  A mirror sample is
  surely below   overlapping with g < -TOL, or c2 < M2 - TOL,
  surely clear   g > TOL and c2 > M2 + TOL,
  undecided      anything else;
the undecided samples of a test may be at most 0.1 % of its samples.

F1: one call that mixes K = 0 .. 1000 at both widths, held to the mirror through these classes.
F2: known answers -- a trajectory against itself, a window after both have arrived, all-zero shapes against separation(), the disc bounds.
F3: two contexts -- refined trajectories (a second object, also in local frames and on fp32 cells) against their sources.
F4: footprint_conflicts() over a fleet against the brute force of the mirror over all pairs, and against conflicts() with the circumscribed discs.
F5: determinism -- a permutation of the queries, a query alone, a repeated call: bit for bit.
F6: refusals.  F7: the C++ adapter against the ctypes path, bit for bit.
Source: 64 hill goals planned and solved by plan_goals (the fixture of test_gpu_separation.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_replan import _hill_map, _queries, _source
from test_gpu_separation import _totals, _valid
from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import conflict_candidates, footprint_clearance2, footprint_radii, separation_times

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
TOL = 1e-9
FKEYS = ("min_c2", "min_t", "first_t", "last_t", "counts")


def _bc(v, n, width=None):
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (n,) if width is None else (n, width))


def _poses(opt, traj, t0, taus):
    """per query the (K, 3) poses x, y, raw yaw of vehicle (traj[q], t0[q]) at taus[q]: one traj_states call for all of them"""
    sizes = [t.shape[0] for t in taus]
    if sum(sizes) == 0:
        return [np.zeros((0, 3)) for _ in taus]
    tr = np.concatenate([np.full(k, b, dtype=np.int32) for k, b in zip(sizes, traj)])
    u = np.concatenate([t - s for t, s in zip(taus, t0)])
    st = opt.traj_states(tr, u)[:, [0, 1, 9]]
    return np.split(st, np.cumsum(sizes)[:-1])


class Tally:
    """samples and undecided samples of a test, the largest |min_c2 - mirror| it saw"""

    def __init__(self):
        self.samples = self.undecided = 0
        self.diff = 0.0

    def close(self, tag):
        print("%s: %d samples, %d undecided, largest |min_c2 - mirror| = %.3g m^2" % (tag, self.samples, self.undecided, self.diff))
        assert self.undecided <= 1e-3 * self.samples, (tag, self.undecided, self.samples)


def _hold_row(row, tau, pa, pb, sa, sb, M, tally, tag):
    """one device row (min_c2, min_t, first_t, last_t, below, overlapping or None) against the mirror on the poses pa, pb (K, 3), by F1's rules"""
    min_c2, min_t, first_t, last_t, n_below, n_over = row
    K = tau.shape[0]
    if K == 0:
        assert min_c2 == INF and np.isnan(min_t) and np.isnan(first_t) and np.isnan(last_t) and n_below == 0 and n_over in (0, None), tag
        return
    c2, over, g = footprint_clearance2(pa[:, :2], pa[:, 2], sa, pb[:, :2], pb[:, 2], sb, gap=True)
    assert np.isfinite(c2).all(), tag
    M2 = M * M
    sure_over, maybe_over = g < -TOL, np.abs(g) <= TOL
    sure_below = sure_over | (c2 < M2 - TOL)
    sure_clear = (g > TOL) & (c2 > M2 + TOL)
    undecided = ~sure_below & ~sure_clear
    tally.samples += K
    tally.undecided += int(undecided.sum())
    # the minimum
    diff = abs(min_c2 - c2.min())
    tally.diff = max(tally.diff, diff)
    assert diff <= TOL, (tag, min_c2, c2.min())
    k = np.nonzero(tau == min_t)[0]
    assert k.size == 1 and c2[k[0]] <= c2.min() + 2.0 * TOL, (tag, min_t)
    # the counts
    assert sure_below.sum() <= n_below <= sure_below.sum() + undecided.sum(), (tag, n_below, int(sure_below.sum()), int(undecided.sum()))
    if n_over is not None:
        assert sure_over.sum() <= n_over <= sure_over.sum() + maybe_over.sum(), (tag, n_over, int(sure_over.sum()))
        assert n_over <= n_below
    # the first and the last sample below
    if n_below == 0:
        assert np.isnan(first_t) and np.isnan(last_t) and not sure_below.any(), tag
    else:
        kf, kl = np.nonzero(tau == first_t)[0], np.nonzero(tau == last_t)[0]
        assert kf.size == 1 and kl.size == 1 and kf[0] <= kl[0] and kl[0] - kf[0] + 1 >= n_below, tag
        assert not sure_clear[kf[0]] and not sure_clear[kl[0]], tag
        if sure_below.any():
            sb_ = np.nonzero(sure_below)[0]
            assert kf[0] <= sb_[0] and kl[0] >= sb_[-1], (tag, kf[0], sb_[0], kl[0], sb_[-1])
    if not sure_below.any() and not undecided.any():
        assert n_below == 0, tag


def _hold(got, A, B, ta, tb, tf, tt, sa, sb, margin, t0_a, t0_b, dt, tally, tag):
    """the rows of a footprint_separation() call against the mirror; returns the windows' sample times"""
    n = len(ta)
    tf, tt, margin, t0_a, t0_b = (_bc(v, n) for v in (tf, tt, margin, t0_a, t0_b))
    sa, sb = _bc(sa, n, 3), _bc(sb, n, 3)
    taus = [separation_times(tf[q], tt[q], dt) for q in range(n)]
    pa, pb = _poses(A, ta, t0_a, taus), _poses(B, tb, t0_b, taus)
    assert np.array_equal(got["counts"][:, 0], [t.shape[0] for t in taus]), tag
    for q in range(n):
        row = (got["min_c2"][q], got["min_t"][q], got["first_t"][q], got["last_t"][q], int(got["counts"][q, 1]), int(got["counts"][q, 2]))
        _hold_row(row, taus[q], pa[q], pb[q], sa[q], sb[q], margin[q], tally, (tag, q))
    return taus


def _random_shapes(rng, n):
    """the shape range of a small car, with rear = 0, half_width = 0 and all-zero shapes among them"""
    s = np.stack([rng.uniform(0.1, 0.5, n), rng.uniform(0.0, 0.3, n), rng.uniform(0.05, 0.25, n)], axis=1)
    s[1::7, 1] = 0.0
    s[2::7, 2] = 0.0
    s[3::11] = 0.0
    return s


@pytest.fixture(scope="module")
def hill():
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array(_valid(res), dtype=np.int32)
    assert len(ok) >= 40, len(ok)
    total = _totals(src)
    assert (total[ok] > 3.0).all()
    return dict(m=m, ka=ka, S=S, G=G, src=src, res=res, ok=ok, total=total)


F1_K = (0, 1, 2, 63, 64, 65, 191, 192, 193, 255, 256, 257, 1000)


def _f1_queries(hill, seed=41):
    """three queries of every K of F1_K at dt = 0.05 on a clock around 1000 s: a vehicle against another one, or against the same trajectory started a
    little later (nose to tail: overlapping while both stand at the start, clear in between, overlapping again at the goal)"""
    ok, total = hill["ok"], hill["total"]
    rng = np.random.default_rng(seed)
    dt = 0.05
    q = dict(ta=[], tb=[], t0a=[], t0b=[], tf=[], tt=[], K=[])
    for k, K in enumerate(F1_K * 3):
        a = int(ok[(5 * k) % ok.size])
        b = a if k % 2 == 0 else int(ok[(5 * k + 9) % ok.size])
        s0 = 1000.0 + rng.uniform(0.0, 2.0)
        s1 = s0 + rng.uniform(0.5, 2.5) if b == a else 1000.0 + rng.uniform(0.0, 2.0)
        if K >= 191:
            f = min(s0, s1) - rng.uniform(0.1, 0.5)                 # from before both starts
        else:
            f = (min(s0, s1) - 0.5 * K * dt, max(s0, s1) + 1.0, max(s0 + total[a], s1 + total[b]) - 0.5 * K * dt)[k % 3] + rng.uniform(0.0, 0.2)
        q["ta"].append(a), q["tb"].append(b), q["t0a"].append(s0), q["t0b"].append(s1), q["tf"].append(f), q["K"].append(K)
        q["tt"].append(f + (K - 1) * dt if K else f - 0.5)          # exactly on the last sample
    q = {k: np.array(v, dtype=np.int32 if k in ("ta", "tb", "K") else np.float64) for k, v in q.items()}
    n = q["K"].size
    q["sa"], q["sb"] = _random_shapes(rng, n), _random_shapes(rng, n)[::-1].copy()
    q["m"] = rng.uniform(0.0, 0.3, n) * (np.arange(n) % 4 != 0)     # zeros among the margins
    same = q["ta"] == q["tb"]                                       # (two vehicles in ONE pose touch exactly when a shape has a zero: that is F2's case, g = 0 is undecided here)
    q["sa"][same], q["sb"][same] = np.maximum(q["sa"][same], 0.05), np.maximum(q["sb"][same], 0.05)
    long = q["K"] == 1000
    assert (q["tt"][long] > np.maximum(q["t0a"] + total[q["ta"]], q["t0b"] + total[q["tb"]])[long]).all()       # ... to after both have arrived
    return q, dt


def _f1_call(src, q, dt, idx=slice(None)):
    return src.footprint_separation(q["ta"][idx], q["tb"][idx], q["tf"][idx], q["tt"][idx], q["sa"][idx], q["sb"][idx], q["m"][idx], t0_a=q["t0a"][idx], t0_b=q["t0b"][idx],
                                    dt=dt)


def test_the_rows_follow_the_mirror_at_every_length(hill):
    """F1"""
    src = hill["src"]
    q, dt = _f1_queries(hill)
    got = _f1_call(src, q, dt)
    tally = Tally()
    _hold(got, src, src, q["ta"], q["tb"], q["tf"], q["tt"], q["sa"], q["sb"], q["m"], q["t0a"], q["t0b"], dt, tally, "F1")
    tally.close("F1")
    assert np.array_equal(got["counts"][:, 0], q["K"])
    below, over, K = got["counts"][:, 1], got["counts"][:, 2], got["counts"][:, 0]
    # what keeps this honest: rows with samples below and not below, overlapping and not, below without overlapping
    assert ((below > 0) & (below < K)).sum() >= 5 and ((over > 0) & (over < K)).sum() >= 5 and (below > over).sum() >= 3 and (below == 0).sum() >= 3
    assert src.footprint_kernel_ms() > 0.0


def test_known_answers(hill):
    """F2"""
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    n = ok.size
    rng = np.random.default_rng(43)
    shapes = _random_shapes(rng, n)
    # a trajectory against itself with the same start: every sample overlaps (also two points in one place), the first is the minimum
    tf, tt = 999.5, 1000.0 + total[ok] + 0.5
    for margin in (0.0, 0.2):
        r = src.footprint_separation(ok, ok, tf, tt, shapes, shapes, margin, t0_a=1000.0, t0_b=1000.0, dt=0.05)
        K = r["counts"][:, 0]
        assert (K > 60).all() and (r["min_c2"] == 0.0).all() and (r["min_t"] == tf).all() and (r["first_t"] == tf).all()
        assert np.array_equal(r["counts"][:, 1], K) and np.array_equal(r["counts"][:, 2], K) and np.array_equal(r["last_t"], tf + (K - 1) * 0.05)
    # a window wholly after both have arrived: every sample has the c2 of the end poses
    tb = np.roll(ok, 5)
    sb = np.roll(shapes, 3, axis=0)
    t0_a, t0_b = 50.0 + 0.1 * np.arange(n), 52.0 - 0.05 * np.arange(n)
    f = np.maximum(t0_a + total[ok], t0_b + total[tb]) + 0.125
    ea, eb = src.traj_states(ok, total[ok])[:, [0, 1, 9]], src.traj_states(tb, total[tb])[:, [0, 1, 9]]
    want = np.array([footprint_clearance2(ea[q:q + 1, :2], ea[q:q + 1, 2], shapes[q], eb[q:q + 1, :2], eb[q:q + 1, 2], sb[q], gap=True) for q in range(n)])[:, :, 0]
    c2, g = want[:, 0], want[:, 2]
    r = src.footprint_separation(ok, tb, f, f + 3.0, shapes, sb, 0.25, t0_a=t0_a, t0_b=t0_b, dt=0.01)
    K = r["counts"][:, 0]
    print("after arrival: largest |min_c2 - mirror| = %.3g m^2" % np.abs(r["min_c2"] - c2).max())
    assert (K >= 300).all() and (np.abs(r["min_c2"] - c2) <= TOL).all() and np.array_equal(r["min_t"], f)
    clear_cut = (np.abs(g) > TOL) & (np.abs(c2 - 0.25 ** 2) > TOL)
    assert clear_cut.sum() >= n - 2
    for q in np.nonzero(clear_cut)[0]:
        below, over = g[q] < 0.0 or c2[q] < 0.25 ** 2, g[q] < 0.0
        assert r["counts"][q].tolist() == [K[q], K[q] if below else 0, K[q] if over else 0], q
        assert (r["first_t"][q] == f[q] and r["last_t"][q] == f[q] + (K[q] - 1) * 0.01) if below else (np.isnan(r["first_t"][q]) and np.isnan(r["last_t"][q])), q
    # all-zero shapes: two points, the disc query's d2
    tfw, ttw = 999.0, 1000.0 + np.maximum(total[ok], total[tb]) + 2.0
    s0a, s0b = 1000.0 + rng.uniform(0.0, 2.0, n), 1000.0 + rng.uniform(0.0, 2.0, n)
    disc = src.separation(ok, tb, tfw, ttw, 0.0, t0_a=s0a, t0_b=s0b, dt=0.05)
    pts = src.footprint_separation(ok, tb, tfw, ttw, np.zeros(3), np.zeros(3), 0.0, t0_a=s0a, t0_b=s0b, dt=0.05)
    assert (disc["min_d2"] > 0.0).all() and (np.abs(pts["min_c2"] - disc["min_d2"]) <= 1e-12 * disc["min_d2"]).all() and (pts["counts"][:, 1:] == 0).all()
    taus = [separation_times(tfw, ttw[q], 0.05) for q in range(n)]
    pa, pb = _poses(src, ok, s0a, taus), _poses(src, tb, s0b, taus)
    leads = 0
    for q in range(n):
        d2 = np.sort(((pa[q][:, :2] - pb[q][:, :2]) ** 2).sum(axis=1))
        if d2[1] - d2[0] > 4e-12 * d2[0]:
            leads += 1
            assert pts["min_t"][q] == disc["min_t"][q], q
    assert leads >= n // 2
    # any shape: the rectangles are no further apart than the points, and no closer than the circumscribed discs
    rho_a, rho_b = np.hypot(np.maximum(shapes[:, 0], shapes[:, 1]), shapes[:, 2]), np.hypot(np.maximum(sb[:, 0], sb[:, 1]), sb[:, 2])
    r = src.footprint_separation(ok, tb, tfw, ttw, shapes, sb, 0.1, t0_a=s0a, t0_b=s0b, dt=0.05)
    floor = np.maximum(np.sqrt(disc["min_d2"]) - rho_a - rho_b, 0.0) ** 2
    assert (r["min_c2"] <= disc["min_d2"] * (1.0 + 1e-12)).all() and (r["min_c2"] >= floor * (1.0 - 1e-12)).all()
    assert (floor > 0.0).sum() >= 5 and (r["min_c2"] < disc["min_d2"]).sum() >= n // 2


def _refined_against_source(src, m, tr, total, tag, t0_b, tally):
    """refine trajectories tr of src from 0.3 of their duration into a second object; each refined trajectory against its source on the common clock"""
    import uneven_planner_amd as U
    tr = np.asarray(tr, dtype=np.int32)
    t_sw = 0.3 * total[tr]
    dst = U.ALMTrajOpt(m)
    dst.set_rho(1.0)
    out = dst.refine(src, tr, t_sw)
    use = [q for q, r in enumerate(out) if r["status"] == 0 and r.get("ret", 4) != 4 and np.isfinite(r["c_xy"]).all()]
    assert len(use) >= max(3, len(tr) // 2), (tag, len(use))
    ta = np.array([out[q]["traj_of"] for q in use], dtype=np.int32)
    tb, t_sw = tr[use], t_sw[use]
    t0_b = _bc(t0_b, len(tr))[use]
    t0_a = t0_b + t_sw
    tt = np.maximum(t0_a + _totals(dst)[ta], t0_b + total[tb]) + 0.5
    rng = np.random.default_rng(47)
    sa, sb = _random_shapes(rng, ta.size), np.tile([0.3, 0.1, 0.1], (ta.size, 1))
    margin = 0.02 * (np.arange(ta.size) % 3)
    got = dst.footprint_separation(ta, tb, t0_b - 0.5, tt, sa, sb, margin, t0_a=t0_a, t0_b=t0_b, other=src, dt=0.05)
    _hold(got, dst, src, ta, tb, t0_b - 0.5, tt, sa, sb, margin, t0_a, t0_b, 0.05, tally, tag)
    assert (got["counts"][:, 0] > 60).all()
    # the order of the contexts: the same pair seen from the source, each side with its own context's frame shift
    back = src.footprint_separation(tb, ta, t0_b - 0.5, tt, sb, sa, margin, t0_a=t0_b, t0_b=t0_a, other=dst, dt=0.05)
    _hold(back, src, dst, tb, ta, t0_b - 0.5, tt, sb, sa, margin, t0_b, t0_a, 0.05, tally, tag + " back")
    assert np.array_equal(back["counts"][:, 0], got["counts"][:, 0]) and (np.abs(back["min_c2"] - got["min_c2"]) <= TOL).all()
    return dst


def test_two_contexts_refined_against_their_sources(hill):
    """F3 on the hill map"""
    tally = Tally()
    _refined_against_source(hill["src"], hill["m"], hill["ok"][:12], hill["total"], "F3 hill", 1000.0 + 0.25 * np.arange(12), tally)
    tally.close("F3 hill")


def test_two_contexts_in_local_frames_and_on_fp32_cells():
    """F3 on a grid beyond FRAME_EXTENT (every trajectory in its own local frame) and on an fp32-cell map, built as S3 of test_gpu_separation.py builds them"""
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
    m32 = U.UnevenMap(dict(map_size_x=32.0, map_size_y=32.0, xy_resolution=0.25), storage="f32").fill_fbm(dict(patch_lambda=5.0, rough_threshold=0.5))
    nx, ny = int(m32.voxel_num[0]), int(m32.voxel_num[1])
    p32 = scenes.local_problems(6, seed0=5000, half=14.0, dmin=4.0, dmax=12.0, occ_r2=m32.occ_r2_buffer,
                                grid=(nx, ny, m32.xy_resolution, m32.map_origin[0], m32.map_origin[1]))
    for tag, m, probs in (("F3 frames", big, far), ("F3 f32", m32, p32)):
        opt = U.ALMTrajOpt(m)
        opt.set_rho(1.0)
        opt.optimize_batch(probs)
        tr = np.arange(len(probs), dtype=np.int32)
        total = _totals(opt)
        if tag == "F3 frames":
            assert np.abs(opt.traj_states(tr, np.zeros(tr.size))[:, :2]).max() > 45.0
        tally = Tally()
        _refined_against_source(opt, m, tr, total, tag, 12.5, tally)
        # vehicles of one context against each other, in map coordinates
        t0 = 0.5 * np.arange(tr.size)
        got = opt.footprint_separation(tr, np.roll(tr, 1), 0.0, total.max() + 2.0, [0.4, 0.2, 0.15], [0.3, 0.0, 0.2], 3.0, t0_a=t0, t0_b=1.0, dt=0.05)
        _hold(got, opt, opt, tr, np.roll(tr, 1), 0.0, total.max() + 2.0, [0.4, 0.2, 0.15], [0.3, 0.0, 0.2], 3.0, t0, 1.0, 0.05, tally, tag + " own")
        tally.close(tag)


def _fleet_held(src, tr, t0, tf, tt, dt, shape, margin, tag="F4"):
    """F4: footprint_conflicts() over a fleet against the brute force of the mirror over all pairs, by F1's classes, and its broad phase against the mirror's on
    the extents the device computed.  Returns the call's result, its pairs as a dict pair -> row, and the pairs the mirror is sure / not sure of."""
    n = len(tr)
    tau = separation_times(tf, tt, dt)
    pose = _poses(src, tr, t0, [tau] * n)
    got = src.footprint_conflicts(tr, shape, margin, tf, tt, t0=t0, dt=dt)
    listed = {tuple(p): k for k, p in enumerate(got["pairs"].tolist())}
    assert got["n_conflicts"] == len(listed) == got["pairs"].shape[0] and got["pairs"].tolist() == sorted(got["pairs"].tolist())
    tally = Tally()
    sure, maybe = [], []
    for i in range(n):
        for j in range(i + 1, n):
            M = margin[i] + margin[j]
            c2, over, g = footprint_clearance2(pose[i][:, :2], pose[i][:, 2], shape[i], pose[j][:, :2], pose[j][:, 2], shape[j], gap=True)
            sure_below = (g < -TOL) | (c2 < M * M - TOL)
            sure_clear = (g > TOL) & (c2 > M * M + TOL)
            if sure_below.any():
                sure.append((i, j))
            elif not sure_clear.all():
                maybe.append((i, j))
            if (i, j) in listed:
                k = listed[(i, j)]
                _hold_row((got["rows"][k, 0], got["rows"][k, 1], got["rows"][k, 2], got["rows"][k, 3], int(got["below"][k]), None), tau, pose[i], pose[j], shape[i],
                          shape[j], M, tally, (tag, i, j))
            else:
                tally.samples += tau.shape[0]
                tally.undecided += int((~sure_below & ~sure_clear).sum())
    tally.close(tag)
    assert set(sure) <= set(listed) <= set(sure) | set(maybe), (sorted(set(sure) - set(listed)), sorted(set(listed) - set(sure) - set(maybe)))
    # the broad phase is the mirror's on the extents the device computed, with the radii of uph_footprint_radii
    ext = src.extent(tr, tf, tt, t0=t0, dt=dt)
    cand = conflict_candidates(ext["box"], footprint_radii(shape, margin))
    assert cand.shape[0] == got["n_candidates"] and set(listed) <= set(map(tuple, cand.tolist()))
    return got, listed, sure, maybe, tau


def test_the_fleet(hill):
    """F4: 24 cars of 0.6 m x 0.3 m (their sizes vary a little) that start 0.4 s apart"""
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    n, dt = 24, 0.05
    tr = ok[:n]
    rng = np.random.default_rng(53)
    t0 = 1000.0 + 0.4 * np.arange(n)
    tf, tt = 999.0, float((t0 + total[tr]).max()) + 1.0
    shape = np.stack([rng.uniform(0.4, 0.5, n), rng.uniform(0.1, 0.2, n), rng.uniform(0.12, 0.18, n)], axis=1)
    margin = rng.uniform(0.0, 0.1, n) * (np.arange(n) % 3 != 0)
    got, listed, sure, maybe, tau = _fleet_held(src, tr, t0, tf, tt, dt, shape, margin)
    # the circumscribed discs report every pair the rectangles report, and pairs the rectangles do not: vehicles that pass side by side or nose to tail
    rho = np.hypot(np.maximum(shape[:, 0], shape[:, 1]), shape[:, 2])
    disc = src.conflicts(tr, rho + margin, tf, tt, t0=t0, dt=dt)
    discs = set(map(tuple, disc["pairs"].tolist()))
    print("fleet: K = %d, rectangles report %d pairs (%d undecided), discs %d, candidates %d of %d" % (tau.shape[0], len(listed), len(maybe), len(discs), got["n_candidates"],
                                                                                                      n * (n - 1) // 2))
    assert set(listed) <= discs and len(discs - set(listed) - set(maybe)) >= 1 and len(sure) >= 1
    assert got["n_candidates"] < n * (n - 1) // 2 and got["n_candidates"] > got["n_conflicts"] and src.footprint_kernel_ms() > 0.0
    # a cap below the number of conflicts: the first of them, the full count
    cap = len(listed) // 2
    assert cap >= 1
    few = src.footprint_conflicts(tr, shape, margin, tf, tt, t0=t0, dt=dt, cap=cap)
    assert few["n_conflicts"] == len(listed) and few["n_candidates"] == got["n_candidates"] and np.array_equal(few["pairs"], got["pairs"][:cap])
    assert np.array_equal(few["rows"], got["rows"][:cap], equal_nan=True) and np.array_equal(few["below"], got["below"][:cap])
    # a row of the fleet call is the pair call's row, bit for bit
    pi, pj = got["pairs"][:, 0], got["pairs"][:, 1]
    one = src.footprint_separation(tr[pi], tr[pj], tf, tt, shape[pi], shape[pj], margin[pi] + margin[pj], t0_a=t0[pi], t0_b=t0[pj], dt=dt)
    assert np.array_equal(np.stack([one[k] for k in FKEYS[:4]], axis=1), got["rows"], equal_nan=True) and np.array_equal(one["counts"][:, 1], got["below"])


def test_the_answer_does_not_depend_on_the_launch(hill):
    """F5: a permutation of the queries permutes the rows, a query alone gives its row of the batch, a repeated call is identical -- bit for bit"""
    src = hill["src"]
    q, dt = _f1_queries(hill)
    got = _f1_call(src, q, dt)
    again = _f1_call(src, q, dt)
    perm = np.random.default_rng(59).permutation(q["K"].size)
    shuffled = _f1_call(src, q, dt, perm)
    for k in FKEYS:
        assert np.array_equal(again[k], got[k], equal_nan=True), k
        assert np.array_equal(shuffled[k], got[k][perm], equal_nan=True), k
    for K in (1000, 257, 193, 192, 64, 1):                          # alone: a launch of one width only, the query first in it
        r = int(np.nonzero(q["K"] == K)[0][1])
        one = _f1_call(src, q, dt, slice(r, r + 1))
        for k in FKEYS:
            assert np.array_equal(one[k][0], got[k][r], equal_nan=True), (K, k)
    # the same queries without the long ones: every workgroup is one wave, and the rows are still those of the mixed launch
    short = np.nonzero(q["K"] <= 192)[0]
    part = _f1_call(src, q, dt, short)
    for k in FKEYS:
        assert np.array_equal(part[k], got[k][short], equal_nan=True), k


def _raw_sep(a, b, ta, tb, t0a, t0b, tf, tt, sa, sb, mg, dt=0.01, n=None, null=()):
    ta, tb = np.ascontiguousarray(ta, dtype=np.int32), np.ascontiguousarray(tb, dtype=np.int32)
    t0a, t0b, tf, tt, sa, sb, mg = (np.ascontiguousarray(v, dtype=np.float64) for v in (t0a, t0b, tf, tt, sa, sb, mg))
    n = ta.size if n is None else n
    m = max(1, ta.size)
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda v: v.ctypes.data_as(_lib.DP)
    arg = lambda name, v: None if name in null else v
    o = dict(min_c2=np.full(m, -9.0), min_t=np.full(m, -9.0), first_t=np.full(m, -9.0), last_t=np.full(m, -9.0), counts=np.full((m, 3), -9, dtype=np.int32))
    rc = a.L.uph_footprint_separation_batch(arg("ctx", a.h), None if b is None else b.h, n, arg("traj_a", ip(ta)), arg("traj_b", ip(tb)), arg("t0_a", dp(t0a)),
                                            arg("t0_b", dp(t0b)), arg("t_from", dp(tf)), arg("t_to", dp(tt)), dt, arg("shape_a", dp(sa)), arg("shape_b", dp(sb)),
                                            arg("margin", dp(mg)), dp(o["min_c2"]), dp(o["min_t"]), dp(o["first_t"]), dp(o["last_t"]), ip(o["counts"]))
    return rc, o


def _raw_con(a, tr, t0, sh, mg, tf=0.0, tt=5.0, dt=0.05, n=None, null=(), cap=8):
    tr = np.ascontiguousarray(tr, dtype=np.int32)
    t0, sh, mg = (np.ascontiguousarray(v, dtype=np.float64) for v in (t0, sh, mg))
    n = tr.size if n is None else n
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda v: v.ctypes.data_as(_lib.DP)
    i64 = lambda v: v.ctypes.data_as(C.POINTER(C.c_int64))
    arg = lambda name, v: None if name in null else v
    o = dict(pairs=np.full((8, 2), -9, dtype=np.int32), rows=np.full((8, 4), -9.0), below=np.full(8, -9, dtype=np.int32), nc=np.full(1, -9, dtype=np.int64),
             nk=np.full(1, -9, dtype=np.int64))
    rc = a.L.uph_footprint_conflicts_batch(arg("ctx", a.h), n, arg("traj", ip(tr)), arg("t0", dp(t0)), arg("shape", dp(sh)), arg("margin", dp(mg)), tf, tt, dt, cap,
                                           ip(o["pairs"]), dp(o["rows"]), ip(o["below"]), i64(o["nc"]), i64(o["nk"]))
    return rc, o


def test_refusals(hill):
    """F6: the return code, the keyword in uph_last_error and every output as it was pre-filled"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m, ka, src, ok = hill["m"], hill["ka"], hill["src"], hill["ok"]
    F = src.L.uph_batch_count(src.h)
    untouched = lambda o: all((o[k] == -9).all() for k in o)
    tr = ok[:4]
    z4, w4, m4 = np.zeros(4), np.full(4, 5.0), np.full(4, 0.1)
    s4 = np.tile([0.4, 0.2, 0.15], (4, 1))
    fresh = U.ALMTrajOpt(m)
    fresh.plan_goals_upload(ka, hill["S"][:8], hill["G"][:8])                 # uploaded, not solved: no resident trajectory
    probs = scenes.random_problems(3, seed0=2100)                              # an UPH_RET_UNSUPPORTED slot next to ordinary ones
    big = dict(probs[0])
    big["inner_xy"] = np.linspace([0.0, 0.0], [3.0, 0.5], 140).T.copy()
    big["inner_yaw"] = np.zeros(140)
    uns = U.ALMTrajOpt(m)
    uns.set_rho(1.0)
    assert uns.optimize_batch(probs + [big])[3]["ret"] == 4
    src2, _ = _source(m, ka, hill["S"][:32], hill["G"][:32])

    def refused(res, what, word, code=_lib.UPH_ERR_INVALID):
        rc, o = res
        assert rc == code and untouched(o), (what, rc)
        assert word in src.L.uph_last_error(), (what, word, src.L.uph_last_error())

    sep = lambda a=src, t=tr, b=None, tb=None, t0a=z4, t0b=z4, tf=z4, tt=w4, sa=s4, sb=s4, mg=m4, **kw: _raw_sep(a, b, t, t if tb is None else tb, t0a, t0b, tf, tt, sa, sb, mg, **kw)
    con = lambda a=src, t=tr, t0=z4, sh=s4, mg=m4, **kw: _raw_con(a, t, t0, sh, mg, **kw)
    for call, name in ((sep, b"uph_footprint_separation_batch"), (con, b"uph_footprint_conflicts_batch")):
        for bad in (-1e-9, NAN, INF):
            for col in range(3):
                s = s4.copy()
                s[2, col] = bad
                refused(call(sa=s) if call is sep else call(sh=s), ("shape", bad, col), b"shape")
                assert name in src.L.uph_last_error()
            mg = m4.copy()
            mg[1] = bad
            refused(call(mg=mg), ("margin", bad), b"margin")
        refused(call(fresh), "not resident", b"resident")
        refused(call(uns, np.array([0, 3, 1, 2])), "unsupported slot", b"UNSUPPORTED")
        for bad in ([int(ok[0]), F, int(ok[1]), int(ok[2])], [-1, 0, 0, 0]):
            refused(call(src, bad), ("index", bad), b"names no trajectory")
        src2.solve_async()                                                      # an asynchronous solve pending
        res = call(src2, [0, 1, 2, 3])
        src2.wait()
        refused(res, "pending", b"in flight")
        refused(call(dt=1e-7), "too many samples", b"2^22", code=_lib.UPH_ERR_LIMIT)
        for n in (0, -3):
            refused(call(n=n), ("n", n), name)
        for dt in (0.0, -0.01, INF, NAN):
            refused(call(dt=dt), ("dt", dt), b"dt")
    s = s4.copy()
    s[3, 1] = -0.5
    refused(sep(sb=s), "shape_b", b"shape_b")
    for null in ("ctx", "traj_a", "traj_b", "t0_a", "t0_b", "t_from", "t_to", "shape_a", "shape_b", "margin"):
        refused(sep(null=(null,)), null, b"uph_footprint_separation_batch")
    for null in ("ctx", "traj", "t0", "shape", "margin"):
        refused(con(null=(null,)), null, b"uph_footprint_conflicts_batch")
    refused(con(cap=-1), "cap < 0", b"uph_footprint_conflicts_batch")
    for v in (NAN, INF):
        bad = np.array([0.0, v, 0.0, 0.0])
        for res in (sep(t0a=bad), sep(t0b=bad), sep(tf=bad), sep(tt=bad + 5.0), con(t0=bad), con(tf=v), con(tt=v)):
            refused(res, ("non-finite", v), b"finite")
    # side b is checked against ITS context
    refused(sep(src, tr, uns, np.array([0, 3, 1, 2])), "unsupported slot of b", b"UNSUPPORTED")
    refused(sep(src, tr, fresh), "b not resident", b"resident")
    # what is allowed: any output pointer NULL, a reversed window, a margin and shapes of 0
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda v: v.ctypes.data_as(_lib.DP)
    cnt = np.full((4, 3), -9, dtype=np.int32)
    z43 = np.zeros((4, 3))
    assert src.L.uph_footprint_separation_batch(src.h, None, 4, ip(tr), ip(tr), dp(z4), dp(z4), dp(z4), dp(w4), 0.01, dp(z43), dp(z43), dp(z4), None, None, None, None, ip(cnt)) == 0
    K = separation_times(0.0, 5.0, 0.01).shape[0]
    assert cnt.tolist() == [[K, K, K]] * 4                                      # a point on itself touches
    assert src.L.uph_footprint_separation_batch(src.h, None, 4, ip(tr), ip(tr), dp(z4), dp(z4), dp(w4), dp(z4), 0.01, dp(s4), dp(s4), dp(m4), None, None, None, None, ip(cnt)) == 0
    assert cnt.tolist() == [[0, 0, 0]] * 4
    assert src.L.uph_footprint_conflicts_batch(src.h, 4, ip(tr), dp(z4), dp(s4), dp(m4), 0.0, 5.0, 0.05, 0, None, None, None, None, None) == 0
    rc, o = con(mg=np.full(4, 50.0))
    assert rc == 0 and o["nc"][0] == 6 and o["nk"][0] == 6 and o["pairs"][:6].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]] and (o["pairs"][6:] == -9).all()
    assert (o["below"][:6] == separation_times(0.0, 5.0, 0.05).shape[0]).all() and (o["rows"][6:] == -9).all()


CPP = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
#include <cstdio>
using namespace uneven_hip;
int main(int argc, char** argv) {
    // in: {ncell, B}, cells, B x {start, goal, start time on the common clock, front, rear, half_width, margin}
    FILE* f = std::fopen(argv[1], "rb");
    long long hdr[2];
    if (!f || fread(hdr, 8, 2, f) != 2) return 2;
    std::vector<double> cells((size_t)hdr[0] * 4), sg((size_t)hdr[1] * 11);
    if (fread(cells.data(), 8, cells.size(), f) != cells.size() || fread(sg.data(), 8, sg.size(), f) != sg.size()) return 2;
    std::fclose(f);
    uph_map_params mp = {2, 10.0, 10.0, 0.2, 0.1, 0.1, 0.05, 0.1, 0.8, 0.05, 9.81};
    UnevenMapHandle map(mp, 0);
    map.setCells(cells.data());
    KinoAstar kino;
    kino.setEnvironment(&map);
    ALMTrajOpt opt, second;
    opt.setEnvironment(&map);
    second.setEnvironment(&map);
    std::vector<std::array<double, 3>> starts((size_t)hdr[1]), goals((size_t)hdr[1]);
    for (long long b = 0; b < hdr[1]; b++) for (int k = 0; k < 3; k++) { starts[b][k] = sg[11 * b + k]; goals[b][k] = sg[11 * b + 3 + k]; }
    uph_manager_params mgr{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5};
    ALMTrajOpt::GoalPlan p = opt.planSE2TrajBatch(kino, starts, goals, mgr);
    ALMTrajOpt::GoalPlan p2 = second.planSE2TrajBatch(kino, starts, goals, mgr);
    (void)p2;
    std::vector<int> traj, other;
    std::vector<double> t0, mg, tf, tt, t0b;
    std::vector<std::array<double, 3>> shape, shape_b;
    for (long long b = 0; b < hdr[1]; b++)
        if (p.traj_of[b] >= 0 && p.ret[b] != UPH_RET_UNSUPPORTED) {
            traj.push_back(p.traj_of[b]); t0.push_back(sg[11 * b + 6]); shape.push_back({sg[11 * b + 7], sg[11 * b + 8], sg[11 * b + 9]}); mg.push_back(sg[11 * b + 10]);
            tf.push_back(sg[11 * b + 6] - 0.5); tt.push_back(sg[11 * b + 6] + 12.0);
        }
    const size_t n = traj.size();
    for (size_t k = 0; k < n; k++) { other.push_back(traj[(k + 1) % n]); t0b.push_back(t0[(k + 1) % n]); shape_b.push_back(shape[(k + 1) % n]); }
    const ALMTrajOpt::TrajFootprintSeparation s = opt.footprintSeparationSE2TrajBatch(traj, other, t0, t0b, tf, tt, shape, shape_b, mg);
    const ALMTrajOpt::TrajFootprintSeparation x = opt.footprintSeparationSE2TrajBatch(traj, other, t0, t0b, tf, tt, shape, shape_b, mg, 0.05, &second);
    const ALMTrajOpt::TrajFootprintConflicts c = opt.footprintConflictsSE2TrajBatch(traj, t0, shape, mg, 99.0, 130.0);
    const ALMTrajOpt::TrajFootprintConflicts d = opt.footprintConflictsSE2TrajBatch(traj, t0, shape, mg, 99.0, 130.0, 0.1, 3);
    // out: n, per query traj; the two separations (7 per query), the two conflict lists (3 counts, then 7 per pair)
    FILE* o = std::fopen(argv[2], "wb");
    double nn = (double)n;
    fwrite(&nn, 8, 1, o);
    for (size_t k = 0; k < n; k++) { double q = (double)traj[k]; fwrite(&q, 8, 1, o); }
    for (const ALMTrajOpt::TrajFootprintSeparation* r : {&s, &x})
        for (size_t q = 0; q < n; q++) {
            double h[7] = {r->min_c2[q], r->min_t[q], r->first_t[q], r->last_t[q], (double)r->counts[3 * q], (double)r->counts[3 * q + 1], (double)r->counts[3 * q + 2]};
            fwrite(h, 8, 7, o);
        }
    for (const ALMTrajOpt::TrajFootprintConflicts* r : {&c, &d}) {
        double h[3] = {(double)r->n_conflicts, (double)r->n_candidates, (double)r->pairs.size()};
        fwrite(h, 8, 3, o);
        for (size_t k = 0; k < r->pairs.size(); k++) {
            double w[7] = {(double)r->pairs[k][0], (double)r->pairs[k][1], r->min_c2[k], r->min_t[k], r->first_t[k], r->last_t[k], (double)r->below[k]};
            fwrite(w, 8, 7, o);
        }
    }
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_matches_ctypes_bit_for_bit(tmp_path, analytic_cells):
    """F7: ALMTrajOpt::footprintSeparationSE2TrajBatch (one object and two) / footprintConflictsSE2TrajBatch from a compiled C++ consumer (after
    planSE2TrajBatch) against plan_goals + footprint_separation / footprint_conflicts through ctypes"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    ka = U.KinoAstar(m)
    S, G = scenes.random_queries(24, seed0=9900)
    B = S.shape[0]
    t0 = 100.0 + 0.5 * np.arange(B)
    shape = np.stack([0.3 + 0.05 * (np.arange(B) % 4), 0.1 * (np.arange(B) % 3), 0.1 + 0.02 * (np.arange(B) % 5)], axis=1)
    mg = 0.05 * (np.arange(B) % 3)
    mk = dict(piece_len=0.3, mean_vel=0.5, init_time_times=1.2, yaw_piece_times=2.0, init_sig_vel=0.05, test_mode=0, test_max_vel=0.5)
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    plan = opt.plan_goals(ka, S, G, **mk)
    second = U.ALMTrajOpt(m)
    second.set_rho(1.0)
    second.plan_goals(ka, S, G, **mk)
    src_ = tmp_path / "footprint.cpp"
    src_.write_text(CPP)
    exe = str(tmp_path / "footprint")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src_), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    cells = np.ascontiguousarray(analytic_cells, dtype=np.float64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2q", cells.shape[0], B))
        f.write(cells.tobytes())
        f.write(np.ascontiguousarray(np.concatenate([S, G, t0[:, None], shape, mg[:, None]], axis=1), dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, dtype=np.float64)
    n = int(raw[0])
    live = [b for b in range(B) if plan[b]["status"] == 0 and plan[b]["ret"] != 4]
    tr = np.array([plan[b]["traj_of"] for b in live], dtype=np.int32)
    assert n == len(tr) >= 10 and raw[1:1 + n].astype(int).tolist() == tr.tolist()
    t0, shape, mg = t0[live], shape[live], mg[live]
    tf, tt = t0 - 0.5, t0 + 12.0
    tb, t0b, sb = np.roll(tr, -1), np.roll(t0, -1), np.roll(shape, -1, axis=0)
    at = 1 + n
    sep = raw[at:at + 14 * n].reshape(2, n, 7)
    for got, want in ((sep[0], opt.footprint_separation(tr, tb, tf, tt, shape, sb, mg, t0_a=t0, t0_b=t0b)),
                      (sep[1], opt.footprint_separation(tr, tb, tf, tt, shape, sb, mg, t0_a=t0, t0_b=t0b, other=second, dt=0.05))):
        for k, key in enumerate(FKEYS[:4]):
            assert np.array_equal(got[:, k], want[key], equal_nan=True), key
        assert np.array_equal(got[:, 4:].astype(np.int32), want["counts"])
    assert (sep[0][:, 4] > 100).all() and np.isfinite(sep[0][:, 0]).all()
    at += 14 * n
    for want in (opt.footprint_conflicts(tr, shape, mg, 99.0, 130.0, t0=t0), opt.footprint_conflicts(tr, shape, mg, 99.0, 130.0, t0=t0, dt=0.1, cap=3)):
        nc, nk, m_ = (int(v) for v in raw[at:at + 3])
        rows = raw[at + 3:at + 3 + 7 * m_].reshape(m_, 7)
        at += 3 + 7 * m_
        assert nc == want["n_conflicts"] and nk == want["n_candidates"] and m_ == want["pairs"].shape[0]
        assert np.array_equal(rows[:, :2].astype(np.int32), want["pairs"]) and np.array_equal(rows[:, 2:6], want["rows"], equal_nan=True)
        assert np.array_equal(rows[:, 6].astype(np.int32), want["below"])
    assert at == raw.size
