"""GPU tier of the queries between resident trajectories on a common clock (uph_extent_batch, uph_separation_batch, uph_conflicts_batch;
uph_extent_kernel, uph_separation_kernel).

S1 (exact): every output of separation() and extent() EQUALS (np.array_equal, NaN = NaN) the numpy mirrors separation_rows / extent_rows fed with the
    sample times of separation_times and, for each side, the positions traj_states(traj, tau - t0) -- the clamp is traj_states' own.
S2: known answers -- a trajectory against itself, a window after both have arrived, positions equal to the rollout's STATE rows.
S3: two contexts -- refined trajectories (a second object, also in local frames and on fp32 cells) against their sources.  The refined trajectory
    starts where its source is at t_switch, so on the common clock t0_a = t0_b + t_switch, and the two coincide at tau = t0_a to 1e-9 m.
S4: conflicts() over a fleet EQUALS the brute force of separation_rows over all pairs, the radius taken from that brute force.
Source: 64 hill goals planned and solved by plan_goals (the fixture of test_gpu_locate.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_replan import _hill_map, _queries, _source
from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import conflict_candidates, extent_rows, separation_rows, separation_times

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
SKEYS = ("min_d2", "min_t", "first_t", "last_t", "counts")
EKEYS = ("box", "counts")


def _valid(res):
    return [j for j, r in enumerate(res) if r["ret"] != 4 and np.isfinite(r["c_xy"]).all() and np.isfinite([r["T_xy"], r["T_yaw"]]).all()]


def _totals(opt):
    offs, rows = opt.rollout(1.0, 1, with_end=True)
    return rows[offs[1:] - 1, 0]


def _bc(v, n):
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))


def _positions(opt, traj, t0, taus):
    """per query the (K, 2) positions of vehicle (traj[q], t0[q]) at taus[q]: one traj_states call for all of them"""
    sizes = [t.shape[0] for t in taus]
    if sum(sizes) == 0:
        return [np.zeros((0, 2)) for _ in taus]
    tr = np.concatenate([np.full(k, b, dtype=np.int32) for k, b in zip(sizes, traj)])
    u = np.concatenate([t - s for t, s in zip(taus, t0)])
    xy = opt.traj_states(tr, u)[:, :2]
    return np.split(xy, np.cumsum(sizes)[:-1])


def _expect(A, B, ta, tb, tf, tt, radius, t0_a, t0_b, dt):
    n = len(ta)
    tf, tt, radius, t0_a, t0_b = (_bc(v, n) for v in (tf, tt, radius, t0_a, t0_b))
    taus = [separation_times(tf[q], tt[q], dt) for q in range(n)]
    pa, pb = _positions(A, ta, t0_a, taus), _positions(B, tb, t0_b, taus)
    per = [separation_rows(taus[q], pa[q], pb[q], radius[q]) for q in range(n)]
    ext = [extent_rows(p) for p in pa]
    return ({k: np.array([p[k] for p in per]) for k in SKEYS}, {k: np.array([e[k] for e in ext]) for k in EKEYS}, taus, pa, pb)


def _same(got, want, keys, tag=""):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (tag, k, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            assert False, (tag, k, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _both(A, ta, tb, tf, tt, radius, t0_a=0.0, t0_b=0.0, other=None, dt=0.01, tag=""):
    """separation and extent (of side a) through the binding, held to S1"""
    B = A if other is None else other
    got = A.separation(ta, tb, tf, tt, radius, t0_a=t0_a, t0_b=t0_b, other=other, dt=dt)
    ext = A.extent(ta, tf, tt, t0=t0_a, dt=dt)
    want, want_ext, taus, pa, pb = _expect(A, B, ta, tb, tf, tt, radius, t0_a, t0_b, dt)
    _same(got, want, SKEYS, tag)
    _same(ext, want_ext, EKEYS, tag + " extent")
    return got, ext, taus, pa, pb


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


@pytest.mark.parametrize("dt", [0.01, 0.05])
def test_separation_and_extent_equal_the_mirrors_bit_for_bit(hill, dt):
    """windows from before both starts to after both ends, starts that differ and are not 0, a clock around 1000 s"""
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    rng = np.random.default_rng(31)
    ta = ok
    tb = np.roll(ok, 7)
    t0_a, t0_b = 1000.0 + rng.uniform(0.0, 5.0, ok.size), 1000.0 + rng.uniform(0.0, 5.0, ok.size)
    tf = np.minimum(t0_a, t0_b) - rng.uniform(0.2, 1.0, ok.size)
    tt = np.maximum(t0_a + total[ta], t0_b + total[tb]) + rng.uniform(0.2, 1.0, ok.size)
    radius = rng.uniform(0.2, 4.0, ok.size)
    got, ext, taus, pa, pb = _both(src, ta, tb, tf, tt, radius, t0_a, t0_b, dt=dt, tag="full %g" % dt)
    K = np.array([t.shape[0] for t in taus])
    assert np.array_equal(got["counts"][:, 0], K) and (K * dt > 4.0).all() and np.array_equal(ext["counts"], np.stack([K, 0 * K], axis=1))
    below = got["counts"][:, 1]
    assert (below > 0).any() and (below == 0).any() and ((below > 0) & (below < K)).any()
    assert np.isfinite(got["min_d2"]).all() and (got["min_t"] >= tf).all() and (got["min_t"] <= tt).all()
    # both ends of the clamp were used: the first sample finds both at their starts, the last at their goals
    st_a, st_b = src.traj_states(ta, np.zeros(ok.size))[:, :2], src.traj_states(tb, np.zeros(ok.size))[:, :2]
    en_a, en_b = src.traj_states(ta, total[ta] + 9.0)[:, :2], src.traj_states(tb, total[tb] + 9.0)[:, :2]
    for q in range(ok.size):
        assert np.array_equal(pa[q][0], st_a[q]) and np.array_equal(pb[q][0], st_b[q]) and np.array_equal(pa[q][-1], en_a[q]) and np.array_equal(pb[q][-1], en_b[q])
    assert src.separation_kernel_ms() > 0.0
    # the extent holds every position, and the broad phase keeps every pair that has a sample below
    for q in range(ok.size):
        b = ext["box"][q]
        assert (pa[q][:, 0] >= b[0]).all() and (pa[q][:, 0] <= b[1]).all() and (pa[q][:, 1] >= b[2]).all() and (pa[q][:, 1] <= b[3]).all()
    ext_b = src.extent(tb, tf, tt, t0=t0_b, dt=dt)
    for q in np.nonzero(below > 0)[0]:
        assert conflict_candidates([ext["box"][q], ext_b["box"][q]], [radius[q], 0.0]).tolist() == [[0, 1]]


def test_lane_and_wave_tails(hill):
    """K on both sides of a wave, of the length at which the launch is split and of 256 lanes, K = 0 and 1, in one launch that mixes both kernels, holds
    duplicates and comes in shuffled order; the radius sits at the median distance, so that first_t / last_t fall anywhere in the window"""
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    rng = np.random.default_rng(37)
    dt = 0.01
    ta, tb, tf, tt, t0a, t0b, want_K = [], [], [], [], [], [], []
    for k, K in enumerate((0, 1, 63, 64, 65, 192, 193, 256, 257, 1025) * 3):
        a, b = int(ok[(3 * k) % ok.size]), int(ok[(3 * k + 11) % ok.size])
        s0, s1 = 1000.0 + rng.uniform(0.0, 2.0), 1000.0 + rng.uniform(0.0, 2.0)
        f = max(s0, s1) + rng.uniform(-1.0, 1.5)
        ta.append(a), tb.append(b), t0a.append(s0), t0b.append(s1), tf.append(f), want_K.append(K)
        tt.append(f + (K - 1) * dt if K else f - 0.5)               # exactly on the last sample
    ta, tb = np.array(ta, dtype=np.int32), np.array(tb, dtype=np.int32)
    tf, tt, t0a, t0b, want_K = np.array(tf), np.array(tt), np.array(t0a), np.array(t0b), np.array(want_K)
    _, _, taus, pa, pb = _expect(src, src, ta, tb, tf, tt, 0.0, t0a, t0b, dt)
    radius = np.array([np.sqrt(np.median(((a - b) ** 2).sum(axis=1))) if a.shape[0] else 1.0 for a, b in zip(pa, pb)])
    dup = np.array([5, 5, 9, 29, 9, 0, 1], dtype=np.int64)
    idx = np.concatenate([np.arange(ta.size), dup])
    idx = idx[rng.permutation(idx.size)]
    got, ext, _, _, _ = _both(src, ta[idx], tb[idx], tf[idx], tt[idx], radius[idx], t0a[idx], t0b[idx], dt=dt, tag="tails")
    assert np.array_equal(got["counts"][:, 0], want_K[idx]) and np.array_equal(ext["counts"][:, 0], want_K[idx])
    empty = want_K[idx] == 0
    assert (got["min_d2"][empty] == INF).all() and np.isnan(got["min_t"][empty]).all() and np.isnan(got["first_t"][empty]).all() and np.isnan(got["last_t"][empty]).all()
    assert (ext["box"][empty] == [INF, -INF, INF, -INF]).all() and (got["counts"][empty] == 0).all()
    some = ~empty & (want_K[idx] > 1)
    assert ((got["counts"][some, 1] > 0) & (got["counts"][some, 1] < got["counts"][some, 0])).sum() >= some.sum() // 2
    # the same query answers the same wherever it stands in the launch, and alone (a launch of one kind of workgroup only)
    for q in np.unique(dup):
        rows = np.nonzero(idx == q)[0]
        assert rows.size >= 2
        for k in SKEYS:
            for r in rows[1:]:
                assert np.array_equal(got[k][r], got[k][rows[0]], equal_nan=True), (q, k)
    for r in (int(np.argmax(want_K[idx])), int(np.nonzero(want_K[idx] == 193)[0][0]), int(np.nonzero(want_K[idx] == 192)[0][0])):
        q = idx[r]
        one = src.separation([ta[q]], [tb[q]], tf[q], tt[q], radius[q], t0_a=t0a[q], t0_b=t0b[q], dt=dt)
        for k in SKEYS:
            assert np.array_equal(one[k][0], got[k][r], equal_nan=True), (q, k)


def test_known_answers(hill):
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    n = ok.size
    # a trajectory against itself with the same start: d2 = 0 at every sample, the first wins; every sample is below a positive radius, none below 0
    tf, tt = 999.5, 1000.0 + total[ok] + 0.5
    for radius, t0 in ((0.25, 1000.0), (1e-150, 1000.0), (0.0, 1000.0), (0.0, 7.5)):
        r = src.separation(ok, ok, tf, tt, radius, t0_a=t0, t0_b=t0, dt=0.05)
        K = r["counts"][:, 0]
        assert (K > 60).all() and (r["min_d2"] == 0.0).all() and (r["min_t"] == tf).all()
        if radius > 0.0:
            assert np.array_equal(r["counts"][:, 1], K) and (r["first_t"] == tf).all() and np.array_equal(r["last_t"], tf + (K - 1) * 0.05)
        else:
            assert (r["counts"][:, 1] == 0).all() and np.isnan(r["first_t"]).all() and np.isnan(r["last_t"]).all()
    # a window wholly after both have arrived: every d2 is the goals' distance
    tb = np.roll(ok, 5)
    t0_a, t0_b = 50.0 + 0.1 * np.arange(n), 52.0 - 0.05 * np.arange(n)
    f = np.maximum(t0_a + total[ok], t0_b + total[tb]) + 0.125
    ga, gb = src.traj_states(ok, total[ok])[:, :2], src.traj_states(tb, total[tb])[:, :2]
    ex, ey = ga[:, 0] - gb[:, 0], ga[:, 1] - gb[:, 1]
    d2 = ex * ex + ey * ey
    r = src.separation(ok, tb, f, f + 3.0, np.sqrt(d2) + 1.0, t0_a=t0_a, t0_b=t0_b, dt=0.01)
    assert np.array_equal(r["min_d2"], d2) and np.array_equal(r["min_t"], f) and np.array_equal(r["first_t"], f)
    assert (r["counts"][:, 0] >= 300).all() and np.array_equal(r["counts"][:, 1], r["counts"][:, 0]) and np.array_equal(r["last_t"], f + (r["counts"][:, 0] - 1) * 0.01)
    r = src.separation(ok, tb, f, f + 3.0, np.sqrt(d2) * 0.5, t0_a=t0_a, t0_b=t0_b, dt=0.01)
    assert np.array_equal(r["min_d2"], d2) and (r["counts"][:, 1] == 0).all() and np.isnan(r["first_t"]).all()
    e = src.extent(ok, f, f + 3.0, t0=t0_a, dt=0.01)
    assert np.array_equal(e["box"], np.stack([ga[:, 0], ga[:, 0], ga[:, 1], ga[:, 1]], axis=1))
    # ... and one wholly before both have left: the starts' distance
    sa, sb = src.traj_states(ok, np.zeros(n))[:, :2], src.traj_states(tb, np.zeros(n))[:, :2]
    ex, ey = sa[:, 0] - sb[:, 0], sa[:, 1] - sb[:, 1]
    r = src.separation(ok, tb, 40.0, 49.0, 0.0, t0_a=t0_a, t0_b=t0_b, dt=0.05)
    assert np.array_equal(r["min_d2"], ex * ex + ey * ey) and (r["min_t"] == 40.0).all() and (r["counts"][:, 0] == separation_times(40.0, 49.0, 0.05).shape[0]).all()
    # dt = 0.25 from 0 with t0 = 0: the samples are the rollout's (its running sum of 0.25 is exact), the positions its STATE rows
    offs, rows = src.rollout(0.25, 1)
    end = np.minimum(total[ok], total[tb]) - 0.3
    want, want_ext = [], []
    for q in range(n):
        ra, rb = rows[int(offs[ok[q]]):int(offs[ok[q] + 1])], rows[int(offs[tb[q]]):int(offs[tb[q] + 1])]
        K = int(np.count_nonzero(ra[:, 0] <= end[q]))
        assert K >= 8 and np.array_equal(ra[:K, 0], separation_times(0.0, end[q], 0.25)) and np.array_equal(rb[:K, 0], ra[:K, 0])
        want.append(separation_rows(ra[:K, 0], ra[:K, 1:3], rb[:K, 1:3], 1.0))
        want_ext.append(extent_rows(ra[:K, 1:3]))
    _same(src.separation(ok, tb, 0.0, end, 1.0, dt=0.25), {k: np.array([w[k] for w in want]) for k in SKEYS}, SKEYS, "rollout rows")
    _same(src.extent(ok, 0.0, end, dt=0.25), {k: np.array([w[k] for w in want_ext]) for k in EKEYS}, EKEYS, "rollout rows extent")


def _refined_against_source(src, m, tr, total, tag, t0_b):
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
    new_total = _totals(dst)[ta]
    tt = np.maximum(t0_a + new_total, t0_b + total[tb]) + 0.5
    for dt in (0.01, 0.05):
        got, _, taus, pa, pb = _both(dst, ta, tb, t0_b - 0.5, tt, 0.05, t0_a, t0_b, other=src, dt=dt, tag=tag)
        assert (got["counts"][:, 0] > 3.0 / dt).all()
    # at tau = t0_a the refined trajectory starts where its source is
    at = dst.separation(ta, tb, t0_a, t0_a, 1.0, t0_a=t0_a, t0_b=t0_b, other=src, dt=0.01)
    d = np.sqrt(at["min_d2"])
    print("%s: largest distance of a refined start from its source at tau = t0_a: %.3g m" % (tag, d.max()))
    assert (at["counts"] == 1).all() and np.array_equal(at["min_t"], t0_a) and (d <= 1e-9).all(), (tag, float(d.max()))
    # the order of the contexts: the same pair seen from the source
    back = src.separation(tb, ta, t0_b - 0.5, tt, 0.05, t0_a=t0_b, t0_b=t0_a, other=dst, dt=0.05)
    for k in SKEYS:
        assert np.array_equal(back[k], got[k], equal_nan=True), (tag, k)
    return dst


def test_two_contexts_refined_against_their_sources(hill):
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    _refined_against_source(src, hill["m"], ok[:16], total, "hill", 1000.0 + 0.25 * np.arange(16))


def test_two_contexts_in_local_frames_and_on_fp32_cells():
    """a grid beyond FRAME_EXTENT (every trajectory in its own local frame, each side with its own context's shift) and an fp32-cell map, built as
    test_gpu_locate.test_local_frames_and_fp32_cells builds them"""
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
    for tag, m, probs in (("frames", big, far), ("f32", m32, p32)):
        opt = U.ALMTrajOpt(m)
        opt.set_rho(1.0)
        opt.optimize_batch(probs)
        tr = np.arange(len(probs), dtype=np.int32)
        total = _totals(opt)
        if tag == "frames":
            assert np.abs(opt.traj_states(tr, np.zeros(tr.size))[:, :2]).max() > 45.0
        dst = _refined_against_source(opt, m, tr, total, tag, 12.5)
        # vehicles of one context against each other, and the extents, in map coordinates
        _both(opt, tr, np.roll(tr, 1), 0.0, total.max() + 2.0, 3.0, 0.5 * np.arange(tr.size), 1.0, dt=0.05, tag=tag + " own")
        assert dst.L.uph_batch_count(dst.h) > 0


def _fleet_brute(src, tr, t0, tf, tt, dt, radius=None):
    """S4's brute force: separation_rows over all pairs of the fleet on positions from traj_states.  radius None: every vehicle gets half the median of the
    pairs' smallest distances in that brute force.  Returns the sample times, the positions, the radii and what conflicts() must list."""
    n = len(tr)
    tau = separation_times(tf, tt, dt)
    pos = _positions(src, tr, t0, [tau] * n)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    if radius is None:
        least = np.array([np.sqrt(separation_rows(tau, pos[i], pos[j], 0.0)["min_d2"]) for i, j in pairs])
        radius = np.full(n, 0.5 * np.median(least))
    brute = [separation_rows(tau, pos[i], pos[j], radius[i] + radius[j]) for i, j in pairs]
    hits = [k for k, b in enumerate(brute) if b["counts"][1] > 0]
    return dict(tau=tau, pos=pos, radius=radius, n_pairs=len(pairs), hits=hits, pairs=np.array([pairs[k] for k in hits], dtype=np.int32).reshape(-1, 2),
                rows=np.array([[brute[k][c] for c in ("min_d2", "min_t", "first_t", "last_t")] for k in hits]).reshape(-1, 4),
                below=np.array([brute[k]["counts"][1] for k in hits], dtype=np.int32))


def _fleet_listed(got, want):
    """conflicts()' list EQUALS the brute force's"""
    assert got["n_conflicts"] == len(want["hits"]) and np.array_equal(got["pairs"], want["pairs"]) and np.array_equal(got["rows"], want["rows"], equal_nan=True)
    assert np.array_equal(got["below"], want["below"])


def test_the_fleet(hill):
    """S4: 24 vehicles that start 0.4 s apart.  The brute force is separation_rows over all 276 pairs on positions from traj_states; the radius of every
    vehicle is half the median of the pairs' smallest distances in that brute force, so about half of the pairs conflict"""
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    n, dt = 24, 0.05
    tr = ok[:n]
    t0 = 1000.0 + 0.4 * np.arange(n)
    tf, tt = 999.0, float((t0 + total[tr]).max()) + 1.0
    want = _fleet_brute(src, tr, t0, tf, tt, dt)
    assert want["n_pairs"] == 276
    tau, pos, radius, hits, want_pairs, want_rows, want_below = (want[k] for k in ("tau", "pos", "radius", "hits", "pairs", "rows", "below"))
    got = src.conflicts(tr, radius, tf, tt, t0=t0, dt=dt)
    print("fleet: K = %d, radius = %.4g, conflicts %d, candidates %d of 276" % (tau.shape[0], radius[0], got["n_conflicts"], got["n_candidates"]))
    _fleet_listed(got, want)
    # what keeps this honest: conflicts exist, the broad phase dropped pairs, and it kept pairs that are no conflict
    assert len(hits) >= 1 and got["n_candidates"] < 276 and got["n_candidates"] > got["n_conflicts"]
    # the broad phase is the mirror's on the extents the device computed
    ext = src.extent(tr, tf, tt, t0=t0, dt=dt)
    _same(ext, {k: np.array([extent_rows(p)[k] for p in pos]) for k in EKEYS}, EKEYS, "fleet extents")
    cand = conflict_candidates(ext["box"], radius)
    assert cand.shape[0] == got["n_candidates"] and set(map(tuple, want_pairs.tolist())) <= set(map(tuple, cand.tolist()))
    assert src.separation_kernel_ms() > 0.0
    # a cap below the number of conflicts: the first of them, the full count
    cap = len(hits) // 2
    assert cap >= 1
    few = src.conflicts(tr, radius, tf, tt, t0=t0, dt=dt, cap=cap)
    assert few["n_conflicts"] == len(hits) and few["n_candidates"] == got["n_candidates"] and np.array_equal(few["pairs"], want_pairs[:cap])
    assert np.array_equal(few["rows"], want_rows[:cap], equal_nan=True) and np.array_equal(few["below"], want_below[:cap])
    none = src.conflicts(tr, radius, tf, tt, t0=t0, dt=dt, cap=0)
    assert none["n_conflicts"] == len(hits) and none["pairs"].shape == (0, 2)
    # per-vehicle radii that differ, a vehicle named twice (it conflicts with itself), an order that is not the batch's
    perm = np.random.default_rng(5).permutation(n)
    tr2, t02 = np.concatenate([tr[perm], tr[perm[:1]]]), np.concatenate([t0[perm], t0[perm[:1]]])
    rad2 = np.concatenate([radius * (0.5 + np.arange(n) / n), [1e-3]])
    pos2 = [pos[k] for k in perm] + [pos[perm[0]]]
    got2 = src.conflicts(tr2, rad2, tf, tt, t0=t02, dt=dt)
    b2 = {(i, j): separation_rows(tau, pos2[i], pos2[j], rad2[i] + rad2[j]) for i in range(n + 1) for j in range(i + 1, n + 1)}
    want2 = [p for p in sorted(b2) if b2[p]["counts"][1] > 0]
    assert got2["pairs"].tolist() == [list(p) for p in want2] and (0, n) in want2
    assert np.array_equal(got2["rows"], np.array([[b2[p][c] for c in ("min_d2", "min_t", "first_t", "last_t")] for p in want2]), equal_nan=True)


def _raw_sep(a, b, ta, tb, t0a, t0b, tf, tt, rad, dt=0.01, n=None, null=()):
    ta, tb = np.ascontiguousarray(ta, dtype=np.int32), np.ascontiguousarray(tb, dtype=np.int32)
    t0a, t0b, tf, tt, rad = (np.ascontiguousarray(v, dtype=np.float64) for v in (t0a, t0b, tf, tt, rad))
    n = ta.size if n is None else n
    m = max(1, ta.size)
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda v: v.ctypes.data_as(_lib.DP)
    arg = lambda name, v: None if name in null else v
    o = dict(min_d2=np.full(m, -9.0), min_t=np.full(m, -9.0), first_t=np.full(m, -9.0), last_t=np.full(m, -9.0), counts=np.full((m, 2), -9, dtype=np.int32))
    rc = a.L.uph_separation_batch(arg("ctx", a.h), None if b is None else b.h, n, arg("traj_a", ip(ta)), arg("traj_b", ip(tb)), arg("t0_a", dp(t0a)), arg("t0_b", dp(t0b)),
                                  arg("t_from", dp(tf)), arg("t_to", dp(tt)), dt, arg("radius", dp(rad)), dp(o["min_d2"]), dp(o["min_t"]), dp(o["first_t"]), dp(o["last_t"]),
                                  ip(o["counts"]))
    return rc, o


def _raw_ext(a, tr, t0, tf, tt, dt=0.01, n=None, null=()):
    tr = np.ascontiguousarray(tr, dtype=np.int32)
    t0, tf, tt = (np.ascontiguousarray(v, dtype=np.float64) for v in (t0, tf, tt))
    n = tr.size if n is None else n
    m = max(1, tr.size)
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda v: v.ctypes.data_as(_lib.DP)
    arg = lambda name, v: None if name in null else v
    o = dict(box=np.full((m, 4), -9.0), counts=np.full((m, 2), -9, dtype=np.int32))
    rc = a.L.uph_extent_batch(arg("ctx", a.h), n, arg("traj", ip(tr)), arg("t0", dp(t0)), arg("t_from", dp(tf)), arg("t_to", dp(tt)), dt, dp(o["box"]), ip(o["counts"]))
    return rc, o


def _raw_con(a, tr, t0, rad, tf=0.0, tt=5.0, dt=0.05, n=None, null=(), cap=8):
    tr = np.ascontiguousarray(tr, dtype=np.int32)
    t0, rad = np.ascontiguousarray(t0, dtype=np.float64), np.ascontiguousarray(rad, dtype=np.float64)
    n = tr.size if n is None else n
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda v: v.ctypes.data_as(_lib.DP)
    arg = lambda name, v: None if name in null else v
    o = dict(pairs=np.full((8, 2), -9, dtype=np.int32), rows=np.full((8, 4), -9.0), below=np.full(8, -9, dtype=np.int32), nc=np.full(1, -9, dtype=np.int64),
             nk=np.full(1, -9, dtype=np.int64))
    i64 = lambda v: v.ctypes.data_as(C.POINTER(C.c_int64))
    rc = a.L.uph_conflicts_batch(arg("ctx", a.h), n, arg("traj", ip(tr)), arg("t0", dp(t0)), arg("radius", dp(rad)), tf, tt, dt, cap, ip(o["pairs"]), dp(o["rows"]),
                                 ip(o["below"]), i64(o["nc"]), i64(o["nk"]))
    return rc, o


def test_refusals(hill):
    """each refusal of include/uneven_hip.h: UPH_ERR_INVALID (UPH_ERR_LIMIT for too many samples) with every output as it was pre-filled"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m, ka, src, ok = hill["m"], hill["ka"], hill["src"], hill["ok"]
    F = src.L.uph_batch_count(src.h)
    untouched = lambda o: all((o[k] == -9).all() for k in o)
    tr = ok[:4]
    z4, w4, r4 = np.zeros(4), np.full(4, 5.0), np.full(4, 0.5)
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

    def refused(res, what, code=-1):
        rc, o = res
        assert rc == code and untouched(o), (what, rc)

    sep = lambda a=src, t=tr, b=None, tb=None, t0a=z4, t0b=z4, tf=z4, tt=w4, rad=r4, **kw: _raw_sep(a, b, t, t if tb is None else tb, t0a, t0b, tf, tt, rad, **kw)
    ext = lambda a=src, t=tr, t0=z4, tf=z4, tt=w4, **kw: _raw_ext(a, t, t0, tf, tt, **kw)
    con = lambda a=src, t=tr, t0=z4, rad=r4, **kw: _raw_con(a, t, t0, rad, **kw)
    for null in ("ctx", "traj_a", "traj_b", "t0_a", "t0_b", "t_from", "t_to", "radius"):
        refused(sep(null=(null,)), null)
        assert b"uph_separation_batch" in src.L.uph_last_error()
    for null in ("ctx", "traj", "t0", "t_from", "t_to"):
        refused(ext(null=(null,)), null)
        assert b"uph_extent_batch" in src.L.uph_last_error()
    for null in ("ctx", "traj", "t0", "radius"):
        refused(con(null=(null,)), null)
        assert b"uph_conflicts_batch" in src.L.uph_last_error()
    refused(con(cap=-1), "cap < 0")
    for call in (sep, ext, con):
        for n in (0, -3):
            refused(call(n=n), ("n", n))
        for dt in (0.0, -0.01, INF, NAN):
            refused(call(dt=dt), ("dt", dt))
        refused(call(dt=1e-7), "too many samples", code=_lib.UPH_ERR_LIMIT)
        refused(call(fresh), "not resident")
        assert b"resident" in src.L.uph_last_error()
        refused(call(U.ALMTrajOpt(m)), "no batch")
        refused(call(uns, np.array([0, 3, 1, 2])), "unsupported slot")
        assert b"UNSUPPORTED" in src.L.uph_last_error()
        for bad in ([int(ok[0]), F, int(ok[1]), int(ok[2])], [-1, 0, 0, 0]):
            refused(call(src, bad), ("index", bad))
        src2.solve_async()                                                      # an asynchronous solve pending
        res = call(src2, [0, 1, 2, 3])
        src2.wait()
        refused(res, "pending")
        assert b"in flight" in src.L.uph_last_error()
    for v in (NAN, INF, -INF):
        bad = np.array([0.0, v, 0.0, 0.0])
        for res in (sep(t0a=bad), sep(t0b=bad), sep(tf=bad), sep(tt=bad + 5.0), sep(rad=bad + 0.5), ext(t0=bad), ext(tf=bad), ext(tt=bad + 5.0), con(t0=bad),
                    con(rad=bad + 0.5), con(tf=v), con(tt=v)):
            refused(res, ("non-finite", v))
    refused(sep(rad=np.array([0.5, 0.5, -1e-9, 0.5])), "negative radius")
    refused(con(rad=np.array([0.5, 0.5, -1e-9, 0.5])), "negative radius")
    # side b is checked against ITS context, on either side of a two-context call
    refused(sep(src, tr, uns, np.array([0, 3, 1, 2])), "unsupported slot of b")
    refused(sep(src, tr, fresh), "b not resident")
    refused(sep(uns, np.array([0, 1, 2, 0]), src, np.array([int(ok[0]), int(ok[1]), int(ok[2]), F])), "index of b")
    assert sep(uns, np.array([0, 1, 2, 0]), src, tr)[0] == 0 and sep(src, tr, uns, np.array([0, 1, 2, 0]))[0] == 0
    src2.solve_async()
    res = sep(src, tr, src2, np.array([0, 1, 2, 3]))
    src2.wait()
    refused(res, "b pending")
    # what is allowed: any output pointer NULL, a reversed window, radius 0
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda v: v.ctypes.data_as(_lib.DP)
    cnt = np.full((4, 2), -9, dtype=np.int32)
    assert src.L.uph_separation_batch(src.h, None, 4, ip(tr), ip(tr), dp(z4), dp(z4), dp(z4), dp(w4), 0.01, dp(z4), None, None, None, None, ip(cnt)) == 0
    assert cnt.tolist() == [[separation_times(0.0, 5.0, 0.01).shape[0], 0]] * 4
    assert src.L.uph_extent_batch(src.h, 4, ip(tr), dp(z4), dp(w4), dp(z4), 0.01, None, ip(cnt)) == 0 and cnt.tolist() == [[0, 0]] * 4
    assert src.L.uph_extent_batch(src.h, 4, ip(tr), dp(z4), dp(z4), dp(w4), 0.01, None, None) == 0
    assert src.L.uph_conflicts_batch(src.h, 4, ip(tr), dp(z4), dp(r4), 0.0, 5.0, 0.05, 0, None, None, None, None, None) == 0
    rc, o = con(rad=np.full(4, 50.0))
    assert rc == 0 and o["nc"][0] == 6 and o["nk"][0] == 6 and o["pairs"][:6].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]] and (o["pairs"][6:] == -9).all()
    assert (o["below"][:6] == separation_times(0.0, 5.0, 0.05).shape[0]).all() and (o["rows"][6:] == -9).all()


CPP = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
#include <cstdio>
using namespace uneven_hip;
int main(int argc, char** argv) {
    // in: {ncell, B}, cells, B x {start, goal, start time on the common clock, radius}
    FILE* f = std::fopen(argv[1], "rb");
    long long hdr[2];
    if (!f || fread(hdr, 8, 2, f) != 2) return 2;
    std::vector<double> cells((size_t)hdr[0] * 4), sg((size_t)hdr[1] * 8);
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
    for (long long b = 0; b < hdr[1]; b++) for (int k = 0; k < 3; k++) { starts[b][k] = sg[8 * b + k]; goals[b][k] = sg[8 * b + 3 + k]; }
    uph_manager_params mgr{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5};
    ALMTrajOpt::GoalPlan p = opt.planSE2TrajBatch(kino, starts, goals, mgr);
    ALMTrajOpt::GoalPlan p2 = second.planSE2TrajBatch(kino, starts, goals, mgr);
    std::vector<int> traj, other;
    std::vector<double> t0, rad, tf, tt, t0b;
    for (long long b = 0; b < hdr[1]; b++)
        if (p.traj_of[b] >= 0 && p.ret[b] != UPH_RET_UNSUPPORTED) {
            traj.push_back(p.traj_of[b]); t0.push_back(sg[8 * b + 6]); rad.push_back(sg[8 * b + 7]);
            tf.push_back(sg[8 * b + 6] - 0.5); tt.push_back(sg[8 * b + 6] + 12.0);
        }
    const size_t n = traj.size();
    for (size_t k = 0; k < n; k++) { other.push_back(traj[(k + 1) % n]); t0b.push_back(t0[(k + 1) % n]); }
    (void)p2;
    const ALMTrajOpt::TrajExtent e = opt.extentSE2TrajBatch(traj, t0, tf, tt);
    const ALMTrajOpt::TrajSeparation s = opt.separationSE2TrajBatch(traj, other, t0, t0b, tf, tt, rad);
    const ALMTrajOpt::TrajSeparation x = opt.separationSE2TrajBatch(traj, other, t0, t0b, tf, tt, rad, 0.05, &second);
    const ALMTrajOpt::TrajConflicts c = opt.conflictsSE2TrajBatch(traj, t0, rad, 99.0, 130.0);
    const ALMTrajOpt::TrajConflicts d = opt.conflictsSE2TrajBatch(traj, t0, rad, 99.0, 130.0, 0.1, 3);
    // out: n, per query traj; extents (6 per query), the two separations (6 per query), the two conflict lists (2 counts, then 7 per pair)
    FILE* o = std::fopen(argv[2], "wb");
    double nn = (double)n;
    fwrite(&nn, 8, 1, o);
    for (size_t k = 0; k < n; k++) { double q = (double)traj[k]; fwrite(&q, 8, 1, o); }
    for (size_t q = 0; q < n; q++) { double h[6] = {e.box[4 * q], e.box[4 * q + 1], e.box[4 * q + 2], e.box[4 * q + 3], (double)e.counts[2 * q], (double)e.counts[2 * q + 1]}; fwrite(h, 8, 6, o); }
    for (const ALMTrajOpt::TrajSeparation* r : {&s, &x})
        for (size_t q = 0; q < n; q++) {
            double h[6] = {r->min_d2[q], r->min_t[q], r->first_t[q], r->last_t[q], (double)r->counts[2 * q], (double)r->counts[2 * q + 1]};
            fwrite(h, 8, 6, o);
        }
    for (const ALMTrajOpt::TrajConflicts* r : {&c, &d}) {
        double h[3] = {(double)r->n_conflicts, (double)r->n_candidates, (double)r->pairs.size()};
        fwrite(h, 8, 3, o);
        for (size_t k = 0; k < r->pairs.size(); k++) {
            double w[7] = {(double)r->pairs[k][0], (double)r->pairs[k][1], r->min_d2[k], r->min_t[k], r->first_t[k], r->last_t[k], (double)r->below[k]};
            fwrite(w, 8, 7, o);
        }
    }
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_matches_ctypes_bit_for_bit(tmp_path, analytic_cells):
    """ALMTrajOpt::extentSE2TrajBatch / separationSE2TrajBatch (one object and two) / conflictsSE2TrajBatch from a compiled C++ consumer (after
    planSE2TrajBatch) against plan_goals + extent / separation / conflicts through ctypes"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    ka = U.KinoAstar(m)
    S, G = scenes.random_queries(24, seed0=9900)
    t0 = 100.0 + 0.5 * np.arange(S.shape[0])
    rad = 0.2 + 0.05 * (np.arange(S.shape[0]) % 5)
    mk = dict(piece_len=0.3, mean_vel=0.5, init_time_times=1.2, yaw_piece_times=2.0, init_sig_vel=0.05, test_mode=0, test_max_vel=0.5)
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    plan = opt.plan_goals(ka, S, G, **mk)
    second = U.ALMTrajOpt(m)
    second.set_rho(1.0)
    second.plan_goals(ka, S, G, **mk)
    src_ = tmp_path / "separation.cpp"
    src_.write_text(CPP)
    exe = str(tmp_path / "separation")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src_), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    cells = np.ascontiguousarray(analytic_cells, dtype=np.float64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2q", cells.shape[0], S.shape[0]))
        f.write(cells.tobytes())
        f.write(np.ascontiguousarray(np.concatenate([S, G, t0[:, None], rad[:, None]], axis=1), dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, dtype=np.float64)
    n = int(raw[0])
    live = [b for b in range(S.shape[0]) if plan[b]["status"] == 0 and plan[b]["ret"] != 4]
    tr = np.array([plan[b]["traj_of"] for b in live], dtype=np.int32)
    assert n == len(tr) >= 10 and raw[1:1 + n].astype(int).tolist() == tr.tolist()
    t0, rad = t0[live], rad[live]
    tf, tt = t0 - 0.5, t0 + 12.0
    tb, t0b = np.roll(tr, -1), np.roll(t0, -1)
    at = 1 + n
    ext = raw[at:at + 6 * n].reshape(n, 6)
    _same(dict(box=ext[:, :4], counts=ext[:, 4:].astype(np.int32)), opt.extent(tr, tf, tt, t0=t0), EKEYS, "adapter extent")
    at += 6 * n
    sep = raw[at:at + 12 * n].reshape(2, n, 6)
    for got, want in ((sep[0], opt.separation(tr, tb, tf, tt, rad, t0_a=t0, t0_b=t0b)), (sep[1], opt.separation(tr, tb, tf, tt, rad, t0_a=t0, t0_b=t0b, other=second, dt=0.05))):
        _same(dict(min_d2=got[:, 0], min_t=got[:, 1], first_t=got[:, 2], last_t=got[:, 3], counts=got[:, 4:].astype(np.int32)), want, SKEYS, "adapter separation")
    assert (sep[0][:, 4] > 100).all() and np.isfinite(sep[0][:, 0]).all()
    at += 12 * n
    for want in (opt.conflicts(tr, rad, 99.0, 130.0, t0=t0), opt.conflicts(tr, rad, 99.0, 130.0, t0=t0, dt=0.1, cap=3)):
        nc, nk, m_ = (int(v) for v in raw[at:at + 3])
        rows = raw[at + 3:at + 3 + 7 * m_].reshape(m_, 7)
        at += 3 + 7 * m_
        assert nc == want["n_conflicts"] and nk == want["n_candidates"] and m_ == want["pairs"].shape[0]
        assert np.array_equal(rows[:, :2].astype(np.int32), want["pairs"]) and np.array_equal(rows[:, 2:6], want["rows"], equal_nan=True)
        assert np.array_equal(rows[:, 6].astype(np.int32), want["below"])
    assert at == raw.size
