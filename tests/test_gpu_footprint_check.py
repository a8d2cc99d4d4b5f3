"""GPU tier of the footprint check (uph_footprint_check_batch; uph_footprint_check_kernel): the vehicle's rectangle swept over the map's occupancy.

The mirror (footprint_check_rows) gets traj_states rows from the device -- columns 0, 1, 9 and 6 at the window's sample times -- and get_cells' occupancy, so
pose and map are the same numbers on both sides.  What remains between the mirror and the kernel are the sine and the cosine (each under 0.8 ulp) and a dozen
roundings on lengths of at most 15 m: about 1e-14 m in a centre's gap g.  TOL = 1e-9 m, the figure test_gpu_footprint.py uses for the same kind of quantity: a
column is surely covered when g < -TOL, surely not when g > TOL, undecided otherwise; a sample is undecided when its hit status rests on an undecided column.
Undecided samples may be at most 0.1 % of a test's samples (shapes come from continuous ranges, so edges do not sit on centres).

C1: an all-zero shape against check()'s occupancy count, bit for bit; also in local frames and on fp32 cells.
C2: one call mixes windows of K = 0 .. 1025 samples with boxes under 64 columns, over 64 and over 256, for each layers singleton and all layers: every
    output inside the mirror's surely / possibly sandwich.
C3: what the query exists for -- a patch beside a path that check() does not see and a 0.6 m wide body does.
C4: lane and wave tails.  C5: determinism, and hit samples non-decreasing in the margin.  C6: a fleet.  C7: refusals.  C8: the C++ adapter, bit for bit.
Source: 64 hill goals planned and solved by plan_goals (the fixture of test_gpu_footprint.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_footprint import _random_shapes
from test_gpu_replan import _hill_map, _queries, _source
from test_gpu_separation import _totals, _valid
from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import (FOOT_ALL, FOOT_OCC_XY, FOOT_OCC_YAW, FOOT_OUTSIDE, footprint_check_columns, footprint_check_rows, footprint_grid,
                                             footprint_radii)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
TOL = 1e-9
KEYS = ("first_t", "last_t", "first_mask", "first_cell", "counts", "cells")
CAR = (0.45, 0.15, 0.3)
DT = 0.002                      # 1025 samples fit the shortest trajectory of the fixture (3 s)


class Tally:
    """samples and undecided samples of a test"""

    def __init__(self):
        self.samples = self.undecided = self.hits = 0

    def close(self, tag):
        print("%s: %d samples, %d hit on the device, %d undecided" % (tag, self.samples, self.hits, self.undecided))
        assert self.undecided <= 1e-3 * self.samples, (tag, self.undecided, self.samples)


def _eq(got, want, tag=""):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (tag, k, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            assert False, (tag, k, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _tilt_discs(m, centres, radius):
    """the columns whose centre lies within radius of one of the centres rebuilt tilted beyond min_cnormal (as test_gpu_check._tilt does, in one upload)"""
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    cells = np.array(m.map_buffer, dtype=np.float64).reshape(nx, ny, nyaw, 4)
    xs = (np.arange(nx) + 0.5) * m.xy_resolution + m.map_origin[0]
    ys = (np.arange(ny) + 0.5) * m.xy_resolution + m.map_origin[1]
    near = np.zeros((nx, ny), dtype=bool)
    for p in centres:
        near |= np.hypot(xs[:, None] - p[0], ys[None, :] - p[1]) < radius
    cells[near, :, 2], cells[near, :, 3] = 0.8, 0.0
    m.set_cells(cells.reshape(-1, 4))
    return near


def _times(opt, dt=DT, with_end=True):
    """per resident trajectory the sample times of rollout(dt, with_end)"""
    offs, rows = opt.rollout(dt, 1, with_end=with_end)
    return [rows[int(offs[b]):int(offs[b + 1]), 0].copy() for b in range(len(offs) - 1)]


def _states(opt, traj, ts):
    """per query the (K, 10) traj_states rows of trajectory traj[q] at ts[q]: one call for all"""
    sizes = [t.shape[0] for t in ts]
    if sum(sizes) == 0:
        return [np.zeros((0, 10)) for _ in ts]
    tr = np.concatenate([np.full(k, b, dtype=np.int32) for k, b in zip(sizes, traj)])
    st = opt.traj_states(tr, np.concatenate(ts))
    return np.split(st, np.cumsum(sizes)[:-1])


def _hold_row(got, q, t, st, shape, margin, m, layers, tally, tag):
    """row q of a footprint_check() result against the mirror on the states st (K, 10) at the window's times t, by the sandwich of the module's docstring"""
    first_t, last_t, mask, cell = got["first_t"][q], got["last_t"][q], int(got["first_mask"][q]), got["first_cell"][q].tolist()
    counts, cells = got["counts"][q], got["cells"][q]
    run = lambda a, b: footprint_check_rows(t[a:b], st[a:b][:, [0, 1, 9]], st[a:b, 6], shape, margin, footprint_grid(m), m.occ_buffer, m.occ_r2_buffer, layers=layers, tol=TOL)
    r = run(0, t.shape[0])
    sure, poss = r["sure"], r["poss"]
    K = t.shape[0]
    assert counts[0] == K, (tag, counts[0], K)
    undecided = sure["hit"] != poss["hit"]
    tally.samples += K
    tally.undecided += int(undecided.sum())
    tally.hits += int(counts[1])
    for k in range(1, 5):
        assert sure["counts"][k] <= counts[k] <= poss["counts"][k], (tag, k, counts.tolist(), sure["counts"].tolist(), poss["counts"].tolist())
    for k in range(2):
        assert sure["cells"][k] <= cells[k] <= poss["cells"][k], (tag, k, cells.tolist(), sure["cells"].tolist(), poss["cells"].tolist())
    assert cells[1] <= cells[0] and counts[1] <= K
    if counts[1] == 0:
        assert np.isnan(first_t) and np.isnan(last_t) and mask == 0 and cell == [-1, -1] and not sure["hit"].any() and cells[1] == 0, tag
        return
    kf, kl = np.nonzero(t == first_t)[0], np.nonzero(t == last_t)[0]
    assert kf.size == 1 and kl.size == 1 and kf[0] <= kl[0] and kl[0] - kf[0] + 1 >= counts[1], tag
    kf, kl = int(kf[0]), int(kl[0])
    assert poss["hit"][kf] and poss["hit"][kl], tag                     # not surely clear
    if sure["hit"].any():
        s = np.nonzero(sure["hit"])[0]
        assert kf <= s[0] and kl >= s[-1], (tag, kf, s[0], kl, s[-1])
    # the first hit sample by itself: its mask between the surely and the possibly reading, its cell a possibly-hit column not above the smallest surely-hit one
    one = run(kf, kf + 1)
    s1, p1 = one["sure"], one["poss"]
    assert (s1["first_mask"] & ~mask) == 0 and (mask & ~p1["first_mask"]) == 0 and 0 < mask <= FOOT_ALL and (mask & ~layers) == 0, (tag, mask, s1["first_mask"], p1["first_mask"])
    ix, iy = one["cover"]["ix"][0], one["cover"]["iy"][0]
    may = set(zip(ix[p1["hitcol"][0]].tolist(), iy[p1["hitcol"][0]].tolist()))
    if not may:
        assert cell == [-1, -1] and not one["cover"]["ok"][0], tag
    else:
        assert tuple(cell) in may, (tag, cell)
        if s1["hitcol"][0].any():
            assert tuple(cell) <= tuple(s1["first_cell"].tolist()), (tag, cell, s1["first_cell"])


def _hold(got, opt, m, traj, ts, shape, margin, layers, tally, tag):
    n = len(traj)
    shape = np.broadcast_to(np.asarray(shape, dtype=np.float64), (n, 3))
    margin = np.broadcast_to(np.asarray(margin, dtype=np.float64), (n,))
    sts = _states(opt, traj, ts)
    for q in range(n):
        _hold_row(got, q, ts[q], sts[q], shape[q], margin[q], m, layers, tally, (tag, q))


def _window(t, i0, K):
    """[t_from, t_to] holding exactly samples i0 .. i0 + K - 1 of the table t (K = 0: a gap between two samples)"""
    if K == 0:
        return 0.75 * t[i0] + 0.25 * t[i0 + 1], 0.25 * t[i0] + 0.75 * t[i0 + 1]
    return t[i0], t[i0 + K - 1]


def _beside(st, side):
    """the point `side` metres to the left of the pose of a traj_states row"""
    return np.array([st[0] - side * np.sin(st[9]), st[1] + side * np.cos(st[9])])


@pytest.fixture(scope="module")
def hill():
    """the 64 hill goals solved on a map of their own, then discs of 0.1 m tilted 0.2 m beside (and a few on) several paths"""
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array(_valid(res), dtype=np.int32)
    assert len(ok) >= 40, len(ok)
    total = _totals(src)
    assert (total[ok] > 3.0).all()
    rng = np.random.default_rng(17)
    fr = rng.uniform(0.15, 0.85, (len(ok), 2))
    st = src.traj_states(np.repeat(ok, 2), (fr * total[ok][:, None]).ravel())
    side = np.where(np.arange(st.shape[0]) % 5 == 4, 0.0, np.where(np.arange(st.shape[0]) % 2 == 0, 0.2, -0.2))
    discs = np.array([_beside(s, d) for s, d in zip(st, side)])
    _tilt_discs(m, discs, 0.1)
    assert m.occ_r2_buffer.any() and m.occ_buffer.any()
    return dict(m=m, ka=ka, S=S, G=G, src=src, res=res, ok=ok, total=total, times=_times(src), discs=discs)


# ---- C1 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _c1(opt, m, traj, tag, dts=((0.01, 1), (0.03, 0))):
    seen = 0
    for dt, we in dts:
        chk = opt.check(traj, dt=dt, with_end=bool(we), limits=np.full(7, INF))
        got = opt.footprint_check(traj, (0.0, 0.0, 0.0), 0.0, dt=dt, with_end=bool(we), layers=FOOT_OCC_YAW | FOOT_OUTSIDE)
        assert np.array_equal(got["first_t"], chk["first_t"], equal_nan=True), tag
        assert np.array_equal(got["counts"][:, 1], chk["counts"][:, 2]) and np.array_equal(got["counts"][:, 0], chk["counts"][:, 0]), tag
        assert np.array_equal(got["cells"][:, 0], got["counts"][:, 0]) and np.array_equal(got["cells"][:, 1], got["counts"][:, 1]), tag     # one column per sample
        assert np.array_equal(got["counts"][:, 3] + got["counts"][:, 4], got["counts"][:, 1]), tag
        seen += int(got["counts"][:, 1].sum())
    print("C1 %s: %d occupied samples" % (tag, seen))
    return seen


def test_point_shape_equals_the_check_bit_for_bit(hill):
    """C1 on the hill map: no sine is involved, so first_t and the hit count ARE check()'s first_t and occupied count (its limits at +inf)"""
    assert _c1(hill["src"], hill["m"], hill["ok"], "hill") > 0
    tf, tt = 0.3 * hill["total"][hill["ok"]], 0.7 * hill["total"][hill["ok"]]
    chk = hill["src"].check(hill["ok"], tf, tt, limits=np.full(7, INF))
    got = hill["src"].footprint_check(hill["ok"], (0.0, 0.0, 0.0), 0.0, tf, tt, layers=FOOT_OCC_YAW | FOOT_OUTSIDE)
    assert np.array_equal(got["first_t"], chk["first_t"], equal_nan=True) and np.array_equal(got["counts"][:, 1], chk["counts"][:, 2])


def test_point_shape_in_local_frames_and_on_fp32_cells():
    """C1 on a grid beyond FRAME_EXTENT (every trajectory solved in its own frame, the occupancy looked up in map coordinates) and on an fp32-cell map"""
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
    p32 = scenes.local_problems(6, seed0=5000, half=14.0, dmin=4.0, dmax=12.0, occ_r2=m32.occ_r2_buffer, grid=(nx, ny, m32.xy_resolution, m32.map_origin[0], m32.map_origin[1]))
    for tag, m, probs in (("frames", big, far), ("f32", m32, p32)):
        opt = U.ALMTrajOpt(m)
        opt.set_rho(1.0)
        opt.optimize_batch(probs)
        tr = np.arange(len(probs), dtype=np.int32)
        _c1(opt, m, tr, tag)
        # and a body on these grids against the mirror: a 1.2 m x 0.8 m rectangle on 0.25 m columns
        tally = Tally()
        ts = _times(opt, 0.01, True)
        got = opt.footprint_check(tr, (0.8, 0.4, 0.4), 0.1)
        if m.occ_buffer is not None:
            _hold(got, opt, m, tr, ts, (0.8, 0.4, 0.4), 0.1, FOOT_ALL, tally, tag)
            tally.close("C1 body " + tag)
        assert (got["cells"][:, 0] > got["counts"][:, 0]).all(), tag


# ---- C2 ---------------------------------------------------------------------------------------------------------------------------------------------------
C2_K = (0, 1, 63, 64, 65, 192, 193, 256, 257, 1025)


def _c2_queries(hill, seed=23):
    """two queries of every K of C2_K for each of three box sizes, shuffled: windows placed around the trajectories' discs"""
    rng = np.random.default_rng(seed)
    ok, times = hill["ok"], hill["times"]
    tr, tf, tt, ts, shape, margin = [], [], [], [], [], []
    sizes = (lambda: (rng.uniform(0.0, 0.06), rng.uniform(0.0, 0.04), rng.uniform(0.0, 0.04), rng.uniform(0.0, 0.01)),        # a point up to boxes under 64 columns
             lambda: (rng.uniform(0.13, 0.17), rng.uniform(0.05, 0.09), rng.uniform(0.08, 0.1), rng.uniform(0.0, 0.02)),       # just over 64 columns: two trips
             lambda: (rng.uniform(0.4, 0.5), rng.uniform(0.1, 0.2), rng.uniform(0.27, 0.33), rng.uniform(0.03, 0.07)))         # over 256 columns
    for K in C2_K:
        for size in sizes:
            for _ in range(2):
                b = int(ok[rng.integers(len(ok))])
                t = times[b]
                i0 = int(rng.integers(0, t.shape[0] - max(K, 2)))
                a, e = _window(t, i0, K)
                f, r, h, mg = size()
                tr.append(b); tf.append(a); tt.append(e); ts.append(t[i0:i0 + K]); shape.append((f, r, h)); margin.append(mg)
    p = rng.permutation(len(tr))
    pick = lambda v: [v[i] for i in p]
    return np.array(pick(tr), dtype=np.int32), np.array(pick(tf)), np.array(pick(tt)), pick(ts), np.array(pick(shape)), np.array(pick(margin))


@pytest.mark.parametrize("layers", [FOOT_OCC_XY, FOOT_OCC_YAW, FOOT_OUTSIDE, FOOT_ALL])
def test_mixed_windows_and_boxes_against_the_mirror(hill, layers):
    """C2"""
    src, m = hill["src"], hill["m"]
    tr, tf, tt, ts, shape, margin = _c2_queries(hill)
    cols = np.array([footprint_check_columns(s, g, m.xy_resolution) for s, g in zip(shape, margin)])
    assert (cols < 64).any() and ((cols > 64) & (cols < 256)).any() and (cols > 256).any()
    got = src.footprint_check(tr, shape, margin, tf, tt, dt=DT, layers=layers)
    assert sorted(set(got["counts"][:, 0].tolist())) == sorted(C2_K)
    tally = Tally()
    _hold(got, src, m, tr, ts, shape, margin, layers, tally, "C2")
    tally.close("C2 layers %d" % layers)
    per = got["cells"][:, 0] / np.maximum(got["counts"][:, 0], 1)
    assert per.max() > 64 and (per[got["counts"][:, 0] > 0] >= 1).all()          # (covered columns per sample; the boxes are larger)
    if layers != FOOT_OUTSIDE:
        assert tally.hits > 0
    empty = got["counts"][:, 0] == 0
    assert empty.sum() == 6 and np.isnan(got["first_t"][empty]).all() and np.isnan(got["last_t"][empty]).all() and (got["first_mask"][empty] == 0).all()
    assert (got["first_cell"][empty] == -1).all() and (got["counts"][empty] == 0).all() and (got["cells"][empty] == 0).all()


# ---- C3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_patch_beside_the_path_is_seen_by_the_body_and_not_by_the_point():
    """C3: a disc of 0.1 m tilted 0.2 m to the side of one trajectory's mid pose.  check() reports nothing occupied for it; the 0.6 m wide car reports hits
    around that time with first_cell inside the disc; a 0.1 m wide one reports none; trajectories farther than the car's circumscribed radius answer as before
    the tilt, bit for bit.  Then the victim is refined from 0.5 s before first_t on a context of its own and checked again: reported, no pass mark."""
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array([j for j in _valid(res) if res[j]["ret"] == 0], dtype=np.int32)
    total = _totals(src)
    margin = 0.05
    before = src.footprint_check(ok, CAR, margin)
    clean = np.nonzero((before["counts"][:, 1] == 0) & (src.check(ok, limits=np.full(7, INF))["counts"][:, 2] == 0))[0]
    assert clean.size >= 1
    v = int(clean[0])
    t_mid = 0.5 * total[ok[v]]
    mid = src.traj_states([ok[v]], [t_mid])[0]
    p0 = _beside(mid, 0.2)
    offs, rows = src.rollout(0.01, 1, with_end=True)
    blk = lambda q: rows[int(offs[ok[q]]):int(offs[ok[q] + 1])]
    reach = footprint_radii(CAR, margin)[0] + 0.1 + m.xy_resolution
    far = [q for q in range(len(ok)) if q != v and np.hypot(*(blk(q)[:, 1:3] - p0).T).min() > reach]
    assert len(far) >= 8
    near = _tilt_discs(m, [p0], 0.1)
    assert near.sum() >= 8
    chk = src.check(ok, limits=np.full(7, INF))
    assert chk["counts"][v, 2] == 0 and np.isnan(chk["first_t"][v])
    after = src.footprint_check(ok, CAR, margin)
    assert after["counts"][v, 1] > 0 and after["first_t"][v] <= t_mid <= after["last_t"][v], (after["first_t"][v], t_mid, after["last_t"][v])
    assert after["first_mask"][v] & (FOOT_OCC_XY | FOOT_OCC_YAW) and after["counts"][v, 2] > 0 and after["counts"][v, 4] == 0
    ix, iy = (int(c) for c in after["first_cell"][v])
    assert near[ix, iy], (ix, iy)
    centre = np.array([(ix + 0.5) * m.xy_resolution + m.map_origin[0], (iy + 0.5) * m.xy_resolution + m.map_origin[1]])
    assert np.hypot(*(centre - p0)) < 0.1
    tally = Tally()
    _hold({k: after[k][[v]] for k in KEYS}, src, m, ok[[v]], [blk(v)[:, 0]], CAR, margin, FOOT_ALL, tally, "C3")
    tally.close("C3")
    slim = src.footprint_check(ok[[v]], (0.45, 0.15, 0.05), 0.0)
    assert slim["counts"][0, 1] == 0 and np.isnan(slim["first_t"][0]) and slim["first_cell"][0].tolist() == [-1, -1]
    for k in KEYS:
        assert np.array_equal(after[k][far], before[k][far], equal_nan=True), k
    dst = U.ALMTrajOpt(m)
    dst.set_rho(1.0)
    out = dst.refine(src, ok[[v]], [max(after["first_t"][v] - 0.5, 0.0)])
    if out[0]["status"] == 0 and out[0]["ret"] != 4:
        again = dst.footprint_check([out[0]["traj_of"]], CAR, margin)
        print("C3 refined from %.2f s: ret %d, %d of %d samples still hit, first at %s" % (max(after["first_t"][v] - 0.5, 0.0), out[0]["ret"], again["counts"][0, 1],
                                                                                          again["counts"][0, 0], again["first_t"][0]))
    else:
        print("C3 refine: status %d" % out[0]["status"])


# ---- C4 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_lane_and_wave_tails(hill):
    """C4: windows cut so that the first hit sample is the window's sample 0, 63, 64, 191, 192, 255, 256 and its last, at both launch widths"""
    src, m, ok, times = hill["src"], hill["m"], hill["ok"], hill["times"]
    margin = 0.05
    full = src.footprint_check(ok, CAR, margin, dt=DT)
    sts = _states(src, ok, [times[b] for b in ok])
    picks = []                          # (trajectory, index of its first hit sample, decided by the mirror)
    for q, b in enumerate(ok):
        t = times[b]
        if full["counts"][q, 1] == 0:
            continue
        f = int(np.nonzero(t == full["first_t"][q])[0][0])
        if f < 256 or f + 64 >= t.shape[0]:
            continue
        a = f - 256
        r = footprint_check_rows(t[a:f + 1], sts[q][a:f + 1][:, [0, 1, 9]], sts[q][a:f + 1, 6], CAR, margin, footprint_grid(m), m.occ_buffer, m.occ_r2_buffer, tol=TOL)
        if r["sure"]["hit"][-1] and not r["poss"]["hit"][:-1].any():
            picks.append((int(b), f))
    assert len(picks) >= 3, len(picks)
    done = 0
    tally = Tally()
    for p in (0, 63, 64, 191, 192, 255, 256):
        for n in sorted({p + 1, 192 if p < 192 else 300, 300}):
            b, f = picks[(p + n) % len(picks)]
            t = times[b]
            n = min(n, t.shape[0] - (f - p))
            tf, tt = _window(t, f - p, n)
            got = src.footprint_check([b], CAR, margin, tf, tt, dt=DT, with_end=False)
            assert got["counts"][0, 0] == n and got["first_t"][0] == t[f], (p, n, got["counts"][0].tolist(), got["first_t"][0], t[f])
            _hold(got, src, m, [b], [t[f - p:f - p + n]], CAR, margin, FOOT_ALL, tally, ("C4", p, n))
            if n == p + 1:
                assert got["counts"][0, 1] == 1 and got["last_t"][0] == t[f]
            done += 1
    assert done == 17
    tally.close("C4")


# ---- C5 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_determinism_and_monotone_in_the_margin(hill):
    """C5: a permutation of the queries, a query alone and a repeated call agree bit for bit; hit samples and covered columns do not decrease with the margin"""
    src = hill["src"]
    tr, tf, tt, _, shape, margin = _c2_queries(hill, seed=29)
    got = src.footprint_check(tr, shape, margin, tf, tt, dt=DT)
    _eq(src.footprint_check(tr, shape, margin, tf, tt, dt=DT), got, "repeat")
    p = np.random.default_rng(5).permutation(len(tr))
    perm = src.footprint_check(tr[p], shape[p], margin[p], tf[p], tt[p], dt=DT)
    _eq(perm, {k: got[k][p] for k in KEYS}, "permutation")
    for q in range(0, len(tr), 7):
        one = src.footprint_check(tr[q:q + 1], shape[q:q + 1], margin[q:q + 1], tf[q:q + 1], tt[q:q + 1], dt=DT)
        _eq(one, {k: got[k][q:q + 1] for k in KEYS}, ("alone", q))
    ok = hill["ok"]
    prev = None
    for mg in (0.0, 0.013, 0.05, 0.11, 0.2):
        now = src.footprint_check(ok, CAR, mg, dt=0.01)
        if prev is not None:
            assert (now["counts"][:, 1:] >= prev["counts"][:, 1:]).all() and (now["cells"] >= prev["cells"]).all(), mg
            hit = ~np.isnan(prev["first_t"])
            assert (now["first_t"][hit] <= prev["first_t"][hit]).all() and (now["last_t"][hit] >= prev["last_t"][hit]).all(), mg
        prev = now
    assert (prev["counts"][:, 1] > 0).any()
    assert src.footprint_check_kernel_ms() > 0.0


# ---- C6 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_fleet_answers_as_its_sources(hill):
    """C6: adopted slots answer as their sources, bit for bit; an empty slot is refused"""
    import uneven_planner_amd as U
    src, m, ok, total = hill["src"], hill["m"], hill["ok"], hill["total"]
    pick = ok[:12]
    fleet = U.TrajFleet(m, 16)
    slots = np.array([15, 0, 7, 3, 9, 1, 14, 2, 11, 5, 8, 4], dtype=np.int32)
    fleet.adopt(src, pick, slots)
    rng = np.random.default_rng(3)
    shape, margin = _random_shapes(rng, 12) + [0.2, 0.0, 0.1], rng.uniform(0.0, 0.06, 12)
    tf, tt = rng.uniform(0.0, 0.4, 12) * total[pick], rng.uniform(0.6, 1.1, 12) * total[pick]
    for layers in (FOOT_ALL, FOOT_OCC_XY):
        _eq(fleet.footprint_check(slots, shape, margin, tf, tt, layers=layers), src.footprint_check(pick, shape, margin, tf, tt, layers=layers), ("fleet", layers))
    assert (fleet.footprint_check(slots, CAR, 0.05)["counts"][:, 1] > 0).any()
    with pytest.raises(_lib.UnevenHipError, match="empty slot"):
        fleet.footprint_check([0, 6], CAR, 0.05)
    assert fleet.footprint_check_kernel_ms() > 0.0


# ---- C7 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _raw(c, tr, tf, tt=None, dt=0.01, with_end=1, shape=CAR, margin=0.05, layers=FOOT_ALL, n=None, null=()):
    tr = np.ascontiguousarray(tr, dtype=np.int32)
    tf = np.ascontiguousarray(tf, dtype=np.float64)
    tt = None if tt is None else np.ascontiguousarray(tt, dtype=np.float64)
    m = max(1, tr.size)
    sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shape, dtype=np.float64), (m, 3)))
    mg = None if margin is None else np.ascontiguousarray(np.broadcast_to(np.asarray(margin, dtype=np.float64), (m,)))
    n = tr.size if n is None else n
    o = dict(first_t=np.full(m, -9.0), last_t=np.full(m, -9.0), first_mask=np.full(m, -9, dtype=np.int32), first_cell=np.full((m, 2), -9, dtype=np.int32),
             counts=np.full((m, 5), -9, dtype=np.int32), cells=np.full((m, 2), -9, dtype=np.int64))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(_lib.DP)
    rc = c.L.uph_footprint_check_batch(c.h if "ctx" not in null else None, n, None if "traj" in null else ip(tr), None if "t_from" in null else dp(tf),
                                       None if tt is None else dp(tt), dt, with_end, None if "shape" in null else dp(sh), None if mg is None else dp(mg), layers,
                                       dp(o["first_t"]), dp(o["last_t"]), ip(o["first_mask"]), ip(o["first_cell"]), ip(o["counts"]),
                                       o["cells"].ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, o


def test_refusals(hill):
    """C7: each refusal of include/uneven_hip.h on live contexts: UPH_ERR_INVALID (UPH_ERR_LIMIT where the header says so) with every output as it was"""
    import uneven_planner_amd as U
    m, ka, src, ok = hill["m"], hill["ka"], hill["src"], hill["ok"]
    F = src.L.uph_batch_count(src.h)
    untouched = lambda o: all((o[k] == -9).all() for k in o)
    tr = ok[:4]
    err = src.L.uph_last_error

    def refused(rc, o, what, code=-1, text=b"uph_footprint_check_batch"):
        assert rc == code and untouched(o), (what, rc)
        assert text in err(), (what, err())

    for null in (("ctx",), ("traj",), ("t_from",), ("shape",)):
        refused(*_raw(src, tr, np.zeros(4), null=null), null)
    refused(*_raw(src, tr, np.zeros(4), n=0), "n = 0")
    refused(*_raw(src, tr, np.zeros(4), n=-3), "n < 0")
    for dt in (0.0, -0.01, INF, NAN):
        refused(*_raw(src, tr, np.zeros(4), dt=dt), ("dt", dt), text=b"dt")
    for layers in (0, 8, -1, 1 << 20):
        refused(*_raw(src, tr, np.zeros(4), layers=layers), ("layers", layers), text=b"layers")
    for bad in (-1e-9, NAN, INF, -INF):
        for col in range(3):
            sh = np.tile(CAR, (4, 1))
            sh[2, col] = bad
            refused(*_raw(src, tr, np.zeros(4), shape=sh), ("shape", bad, col), text=b"shape")
        refused(*_raw(src, tr, np.zeros(4), margin=[0.0, bad, 0.0, 0.0]), ("margin", bad), text=b"margin")
    # the box limit: a side of 129 columns at 0.05 m
    refused(*_raw(src, tr, np.zeros(4), shape=[CAR, CAR, (3.0, 3.0, 1.0), CAR], margin=0.0), "box", code=_lib.UPH_ERR_LIMIT, text=b"2^14")
    assert _raw(src, tr, np.zeros(4), shape=[CAR, CAR, (3.0, 3.0, 0.5), CAR], margin=0.0)[0] == 0
    fresh = U.ALMTrajOpt(m)
    fresh.plan_goals_upload(ka, hill["S"][:8], hill["G"][:8])                 # uploaded, not solved: no resident trajectory
    refused(*_raw(fresh, [0], [0.0]), "not resident", text=b"resident")
    refused(*_raw(U.ALMTrajOpt(m), [0], [0.0]), "no batch")
    for bad in ([F], [-1], [int(ok[0]), F + 7]):
        refused(*_raw(src, bad, [0.5] * len(bad)), ("index", bad))
    for t in (NAN, INF, -INF):
        refused(*_raw(src, tr, [0.1, t, 0.2, 0.3]), ("t_from", t))
    refused(*_raw(src, tr, np.zeros(4), [1.0, 2.0, NAN, 3.0]), "NaN t_to")
    for t in (INF, -INF):                                                       # an infinite t_to is a window
        rc, o = _raw(src, tr, np.zeros(4), [1.0, t, 2.0, 3.0])
        assert rc == 0 and not untouched(o) and (o["counts"][1, 0] == 0) == (t < 0)
    refused(*_raw(src, tr, np.zeros(4), dt=1e-6), "too many samples", code=_lib.UPH_ERR_LIMIT, text=b"samples")
    src2, _ = _source(m, ka, hill["S"][:32], hill["G"][:32])
    src2.solve_async()
    rc, o = _raw(src2, [0], [0.0])
    src2.wait()
    refused(rc, o, "pending", text=b"in flight")
    # margin == NULL is a margin of 0, and any output pointer may be NULL
    rc, o = _raw(src, tr, np.zeros(4), margin=None)
    want = src.footprint_check(tr, CAR, 0.0)
    assert rc == 0 and all(np.array_equal(o[k], want[k], equal_nan=True) for k in KEYS)
    cells = np.full((4, 2), -9, dtype=np.int64)
    sh, z = np.tile(CAR, (4, 1)), np.zeros(4)
    assert src.L.uph_footprint_check_batch(src.h, 4, tr.ctypes.data_as(C.POINTER(C.c_int32)), z.ctypes.data_as(_lib.DP), None, 0.01, 1, sh.ctypes.data_as(_lib.DP), None,
                                           FOOT_ALL, None, None, None, None, None, cells.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    assert np.array_equal(cells, want["cells"])
    with pytest.raises(_lib.UnevenHipError):
        src.footprint_check([], CAR)


# ---- C8 ---------------------------------------------------------------------------------------------------------------------------------------------------
CPP = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
#include <cstdio>
using namespace uneven_hip;
static void put(FILE* o, const ALMTrajOpt::TrajFootprintCheck& r) {
    for (size_t q = 0; q < r.first_t.size(); q++) {
        double h[12] = {r.first_t[q], r.last_t[q], (double)r.first_mask[q], (double)r.first_cell[q][0], (double)r.first_cell[q][1], (double)r.counts[5 * q],
                        (double)r.counts[5 * q + 1], (double)r.counts[5 * q + 2], (double)r.counts[5 * q + 3], (double)r.counts[5 * q + 4], (double)r.cells[2 * q],
                        (double)r.cells[2 * q + 1]};
        fwrite(h, 8, 12, o);
    }
}
int main(int argc, char** argv) {
    // in: {ncell, B}, cells, B x {start, goal, fractions of the planned duration the window starts and ends at, shape, margin}
    FILE* f = std::fopen(argv[1], "rb");
    long long hdr[2];
    if (!f || fread(hdr, 8, 2, f) != 2) return 2;
    std::vector<double> cells((size_t)hdr[0] * 4), sg((size_t)hdr[1] * 12);
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
    for (long long b = 0; b < hdr[1]; b++) for (int k = 0; k < 3; k++) { starts[b][k] = sg[12 * b + k]; goals[b][k] = sg[12 * b + 3 + k]; }
    uph_manager_params mgr{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5};
    ALMTrajOpt::GoalPlan p = opt.planSE2TrajBatch(kino, starts, goals, mgr);
    std::vector<int> traj;
    std::vector<double> tf, tt, margin;
    std::vector<std::array<double, 3>> shape;
    for (long long b = 0; b < hdr[1]; b++)
        if (p.traj_of[b] >= 0 && p.ret[b] != UPH_RET_UNSUPPORTED) {
            traj.push_back(p.traj_of[b]); tf.push_back(sg[12 * b + 6] * p.total_time[b]); tt.push_back(sg[12 * b + 7] * p.total_time[b]);
            shape.push_back({sg[12 * b + 8], sg[12 * b + 9], sg[12 * b + 10]}); margin.push_back(sg[12 * b + 11]);
        }
    const ALMTrajOpt::TrajFootprintCheck a = opt.footprintCheckSE2TrajBatch(traj, tf, tt, shape, margin);      // all layers, every 0.01 s, with the end point
    const ALMTrajOpt::TrajFootprintCheck c = opt.footprintCheckSE2TrajBatch(traj, tf, {}, shape, {}, UPH_FOOT_OCC_XY, 0.03, false);
    FILE* o = std::fopen(argv[2], "wb");
    double n = (double)traj.size();
    fwrite(&n, 8, 1, o);
    for (size_t k = 0; k < traj.size(); k++) { double q[3] = {(double)traj[k], tf[k], tt[k]}; fwrite(q, 8, 3, o); }
    put(o, a);
    put(o, c);
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_matches_ctypes_bit_for_bit(tmp_path, analytic_cells):
    """C8: ALMTrajOpt::footprintCheckSE2TrajBatch from a compiled C++ consumer (after planSE2TrajBatch) against plan_goals + footprint_check through ctypes, on the
    analytic terrain with discs tilted over it"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    rng = np.random.default_rng(31)
    cells = np.array(analytic_cells, dtype=np.float64).reshape(200, 200, -1, 4)
    xs = (np.arange(200) + 0.5) * 0.05 - 5.0
    near = np.zeros((200, 200), dtype=bool)
    for p in rng.uniform(-4.5, 4.5, (80, 2)):
        near |= np.hypot(xs[:, None] - p[0], xs[None, :] - p[1]) < 0.12
    cells[near, :, 2], cells[near, :, 3] = 0.8, 0.0
    cells = np.ascontiguousarray(cells.reshape(-1, 4))
    m = U.UnevenMap()
    m.set_cells(cells)
    ka = U.KinoAstar(m)
    S, G = scenes.random_queries(24, seed0=9900)
    B = S.shape[0]
    f0 = np.array([[0.0, 0.3, 0.5, -0.2, 0.95, 0.6][b % 6] for b in range(B)])
    f1 = np.array([[1.0, 0.6, 2.0, 0.4, 1.0, 0.5][b % 6] for b in range(B)])
    shape, margin = _random_shapes(rng, B) + [0.1, 0.0, 0.1], rng.uniform(0.0, 0.08, B)
    mk = dict(piece_len=0.3, mean_vel=0.5, init_time_times=1.2, yaw_piece_times=2.0, init_sig_vel=0.05, test_mode=0, test_max_vel=0.5)
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    plan = opt.plan_goals(ka, S, G, **mk)
    src_ = tmp_path / "fcheck.cpp"
    src_.write_text(CPP)
    exe = str(tmp_path / "fcheck")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src_), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2q", cells.shape[0], B))
        f.write(cells.tobytes())
        f.write(np.ascontiguousarray(np.concatenate([S, G, f0[:, None], f1[:, None], shape, margin[:, None]], axis=1), dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, dtype=np.float64)
    n = int(raw[0])
    live = [b for b in range(B) if plan[b]["status"] == 0 and plan[b]["ret"] != 4]
    want_tr = [plan[b]["traj_of"] for b in live]
    assert n == len(want_tr) >= 10 and raw.size == 1 + 3 * n + 2 * 12 * n
    q = raw[1:1 + 3 * n].reshape(n, 3)
    assert q[:, 0].astype(int).tolist() == want_tr
    res = raw[1 + 3 * n:].reshape(2, n, 12)
    wants = (opt.footprint_check(want_tr, shape[live], margin[live], q[:, 1], q[:, 2]),
             opt.footprint_check(want_tr, shape[live], 0.0, q[:, 1], None, dt=0.03, with_end=False, layers=FOOT_OCC_XY))
    for got, want in zip(res, wants):
        cpp = dict(first_t=got[:, 0], last_t=got[:, 1], first_mask=got[:, 2].astype(np.int32), first_cell=got[:, 3:5].astype(np.int32), counts=got[:, 5:10].astype(np.int32),
                   cells=got[:, 10:12].astype(np.int64))
        _eq(cpp, want, "adapter")
    print("C8: %d queries, %d with hits" % (n, int((res[0][:, 6] > 0).sum())))
    assert (res[0][:, 10] > res[0][:, 5]).any()
