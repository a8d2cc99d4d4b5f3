"""GPU tier of checking resident trajectories against the current map (uph_check_batch, uph_check_kernel).

Bar: every output of the device reduction EQUALS (np.array_equal, NaN = NaN) the numpy mirror check_rows applied to the rows the rollout writes for
the same trajectory -- its t and TERRAIN columns -- and to uph_frontend_query's occ at those rows' (x, y, yaw): full windows, windows cut at, between
and beyond rows, every lane / wave tail of the strided walk, local frames, fp32 cells, a map changed under the batch, NaN terrain.  A second,
independent kernel (the post-solve report) agrees on the maxima.  Source: 64 hill goals planned and solved by plan_goals."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_replan import _hill_map, _queries, _source
from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import CHECK_OCC_BIT, check_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST, TR = 1, 2
KEYS = ("first_t", "first_mask", "counts", "worst", "worst_t")
INF = float("inf")
NOLIM = np.full(7, INF)


def _valid(res):
    return [j for j, r in enumerate(res) if r["ret"] != 4 and np.isfinite(r["c_xy"]).all() and np.isfinite([r["T_xy"], r["T_yaw"]]).all()]


def _ref(opt, m, dt, with_end):
    """the rollout's rows of the resident batch and the map's occupancy at them: what the check is held against"""
    offs, rows = opt.rollout(dt, ST | TR, with_end=bool(with_end))
    occ = m.frontend_query(rows[:, 1:4])[1] if rows.shape[0] else np.zeros(0, dtype=np.int32)
    return offs, rows, occ


def _expect(ref, traj, lim, t_from=None, t_to=None):
    offs, rows, occ = ref
    n = len(traj)
    t_from = np.broadcast_to(0.0 if t_from is None else np.asarray(t_from, dtype=np.float64), (n,))
    t_to = np.broadcast_to(INF if t_to is None else np.asarray(t_to, dtype=np.float64), (n,))
    per = []
    for q, b in enumerate(traj):
        a, e = int(offs[b]), int(offs[b + 1])
        per.append(check_rows(rows[a:e, 0], rows[a:e, 9:16], occ[a:e], lim, t_from[q], t_to[q]))
    return {k: np.array([p[k] for p in per]) for k in KEYS}


def _same(got, want, tag=""):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (tag, k, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=True):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            assert False, (tag, k, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _median_limits(ref, traj):
    """per term the median over the trajectories of its maximum in the rows (|v| for the first four): about half of them violate it"""
    offs, rows, _ = ref
    mx = []
    for b in traj:
        T = rows[int(offs[b]):int(offs[b + 1]), 9:16]
        mx.append(np.concatenate([np.abs(T[:, :4]).max(axis=0), T[:, 4:].max(axis=0)]))
    return np.median(np.array(mx), axis=0)


@pytest.fixture(scope="module")
def hill():
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array(_valid(res), dtype=np.int32)
    assert len(ok) >= 40, len(ok)
    refs = {(dt, we): _ref(src, m, dt, we) for dt in (0.01, 0.03) for we in (0, 1)}
    lim = _median_limits(refs[(0.01, 0)], ok)
    return dict(m=m, ka=ka, S=S, G=G, src=src, res=res, ok=ok, refs=refs, lim=lim)


@pytest.mark.parametrize("with_end", [0, 1])
@pytest.mark.parametrize("dt", [0.01, 0.03])
def test_full_windows_equal_the_rollout_bit_for_bit(hill, dt, with_end):
    src, ok, ref = hill["src"], hill["ok"], hill["refs"][(dt, with_end)]
    lim = _median_limits(ref, ok)
    got = src.check(ok, dt=dt, with_end=with_end, limits=lim)
    _same(got, _expect(ref, ok, lim), "all terms")
    assert (got["counts"][:, 0] == np.diff(ref[0])[ok]).all() and (got["counts"][:, 0] > 50).all()
    for k in range(7):                  # one term at a time at its median: both branches occur, among the trajectories and inside each violator
        one = NOLIM.copy()
        one[k] = lim[k]
        g = src.check(ok, dt=dt, with_end=with_end, limits=one)
        _same(g, _expect(ref, ok, one), "term %d" % k)
        free = g["counts"][:, 2] == 0
        viol = g["first_mask"] != 0
        assert (viol & free).sum() >= 8 and (~viol).sum() >= 8, (k, viol.sum(), free.sum())
        assert (g["first_mask"][viol & free] == 1 << k).all() and np.isnan(g["first_t"][~viol]).all()
        assert ((g["worst"][:, k] > lim[k]) == (viol | ~free))[free].all()


def test_against_the_report(hill):
    """a second, independent kernel on the same samples: Solver::report's maxima (signed, from 0 / -1) follow from the check's worst values"""
    src, ok = hill["src"], hill["ok"]
    rep = src.getMaxVxAxAyCurAttSig()[ok]
    got = src.check(ok, dt=0.01, with_end=False, limits=NOLIM)
    for k in range(4):
        assert np.array_equal(got["worst"][:, k], np.abs(rep[:, k])), k
    assert np.array_equal(np.maximum(got["worst"][:, 4], -1.0), rep[:, 4])
    assert np.array_equal(np.maximum(got["worst"][:, 5], 0.0), rep[:, 5])
    assert (got["first_mask"] & 0x7f == 0).all()


@pytest.mark.parametrize("dt,with_end", [(0.01, 0), (0.03, 1)])
def test_windows(hill, dt, with_end):
    """t_from / t_to at 0, negative, exactly a row's t, between two rows, the total, beyond it, reversed, infinite: the literally selected rows"""
    src, ok, ref, lim = hill["src"], hill["ok"][:12], hill["refs"][(dt, with_end)], hill["lim"]
    offs, rows, _ = ref
    tr, tf, tt = [], [], []
    for b in ok:
        t = rows[int(offs[b]):int(offs[b + 1]), 0]
        total = hill["refs"][(dt, 1)][1][int(hill["refs"][(dt, 1)][0][b + 1]) - 1, 0]
        assert t.shape[0] > 40
        h = lambda i: 0.5 * (t[i] + t[i + 1])
        win = [(0.0, total), (0.0, 0.0), (-0.5, t[5]), (-2.0, -1.0), (t[3], t[10]), (t[7], t[7]), (np.nextafter(t[3], 9.0), np.nextafter(t[10], -9.0)),
               (h(3), h(10)), (h(6), h(6)), (t[-2], total), (total, total), (np.nextafter(total, 0.0), total), (h(20), total + 5.0),
               (total + 1.0, total + 2.0), (np.nextafter(total, 99.0), INF), (t[10], t[3]), (t[4], INF), (0.0, -INF), (-1e300, 1e300)]
        for a, e in win:
            tr.append(b), tf.append(a), tt.append(e)
    tr = np.array(tr, dtype=np.int32)
    got = src.check(tr, tf, tt, dt=dt, with_end=with_end, limits=lim)
    want = _expect(ref, tr, lim, tf, tt)
    _same(got, want, "windows")
    nw = len(tr) // len(ok)
    c = got["counts"][:nw, 0].tolist()
    assert c[1] == 1 and c[2] == 6 and c[3] == 0 and c[4] == 8 and c[5] == 1 and c[6] == 6 and c[7] == 7 and c[8] == 0 and c[10] == with_end
    assert c[13] == 0 and c[14] == 0 and c[15] == 0 and c[17] == 0 and c[0] == c[18] == int(offs[ok[0] + 1] - offs[ok[0]])
    empty = got["counts"][:, 0] == 0
    assert empty.sum() >= 5 * len(ok)
    assert np.isnan(got["first_t"][empty]).all() and (got["first_mask"][empty] == 0).all() and (got["worst"][empty] == -INF).all()
    assert np.isnan(got["worst_t"][empty]).all()
    # t_to = None is "to the end"
    _same(src.check(tr, tf, None, dt=dt, with_end=with_end, limits=lim), _expect(ref, tr, lim, tf, None), "t_to None")


def test_lane_and_wave_tails(hill):
    """windows of 1 .. 513 samples whose only violating sample sits first, last, at index 64 or at index 256 of the window: the strided walk of 256
    lanes and the wave / workgroup levels of the reduction.  The sample is a trajectory's strict maximum of one term, the limit the largest other
    value of the window"""
    src, ok, ref = hill["src"], hill["ok"], hill["refs"][(0.01, 0)]
    offs, rows, occ = ref
    peaks = []                          # (trajectory, term, row of its strict maximum, rows)
    for b in ok:
        a, e = int(offs[b]), int(offs[b + 1])
        if occ[a:e].any():
            continue
        T = rows[a:e, 9:16]
        M = np.concatenate([np.abs(T[:, :4]), T[:, 4:]], axis=1)
        for k in range(7):
            i = int(np.argmax(M[:, k]))
            if np.isfinite(M[:, k]).all() and (M[:, k] == M[i, k]).sum() == 1:
                peaks.append((int(b), k, i, e - a))
    done = 0
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 513):
        for p in sorted({0, n - 1, 64, 256}):
            if p >= n:
                continue
            fit = [(b, k, i, r) for b, k, i, r in peaks if i - p >= 0 and i - p + n <= r]
            assert fit, (n, p)
            b, k, i, _ = fit[(n + p) % len(fit)]
            a = int(offs[b])
            t = rows[a:int(offs[b + 1]), 0]
            col = rows[a + i - p:a + i - p + n, 9 + k]
            m = np.abs(col) if k < 4 else col
            lim = NOLIM.copy()
            lim[k] = np.delete(m, p).max() if n > 1 else np.nextafter(m[0], -INF)
            tf, tt = t[i - p], t[i - p + n - 1]
            got = src.check([b], tf, tt, dt=0.01, with_end=False, limits=lim)
            _same(got, _expect(ref, [b], lim, tf, tt), (n, p))
            assert got["counts"][0].tolist() == [n, 1, 0] and got["first_t"][0] == t[i] and got["first_mask"][0] == 1 << k, (n, p, got)
            assert got["worst"][0, k] == m[p] and got["worst_t"][0, k] == t[i]
            done += 1
    assert done == 22


def test_default_limits(hill):
    src, ok, ref = hill["src"], hill["ok"], hill["refs"][(0.01, 1)]
    lim = src.check_limits()
    assert lim.tolist() == [src.max_vel, src.max_acc_lon, src.max_acc_lat, src.max_kap, -src.min_cxi, src.max_sig, INF]
    a = src.check(ok)
    _same(a, src.check(ok, limits=lim), "defaults")
    _same(a, _expect(ref, ok, lim), "defaults vs rows")


def _tilt(m, p0, radius):
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    cells = np.array(m.map_buffer, dtype=np.float64).reshape(nx, ny, nyaw, 4)
    xs = (np.arange(nx) + 0.5) * m.xy_resolution + m.map_origin[0]
    ys = (np.arange(ny) + 0.5) * m.xy_resolution + m.map_origin[1]
    near = np.hypot(xs[:, None] - p0[0], ys[None, :] - p0[1]) < radius
    cells[near, :, 2], cells[near, :, 3] = 0.8, 0.0                          # normal tilted: c_normal 0.6 < min_cnormal 0.8
    m.set_cells(cells.reshape(-1, 4))


def test_map_changed_under_the_batch():
    """the cells within 0.4 m of one trajectory's mid pose are rebuilt tilted beyond min_cnormal: that trajectory reports its first violation among
    its rows in the patch, by attitude or occupancy; trajectories farther than 2.5 m answer as before, bit for bit; then the violators are refined
    from 0.5 s before first_t into a second context, whose check again equals its own rollout (no claim that the refined trajectory is feasible)"""
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array([j for j in _valid(res) if res[j]["ret"] == 0], dtype=np.int32)
    # the optimiser meets its limits to a tolerance: limits a little wider, so that the unchanged map violates nowhere along the victim
    lim = src.check_limits() * np.array([1.2, 1.2, 1.2, 1.2, 0.9, 1.5, 1.0])
    before = src.check(ok, limits=lim)
    ref0 = _ref(src, m, 0.01, 1)
    _same(before, _expect(ref0, ok, lim), "before")
    clean = np.nonzero(before["first_mask"] == 0)[0]
    assert clean.size >= 1
    v = int(clean[0])
    offs, rows, _ = ref0
    blk = lambda q: rows[int(offs[ok[q]]):int(offs[ok[q] + 1])]
    mine = blk(v)
    p0 = mine[mine.shape[0] // 2, 1:3].copy()
    far = [q for q in range(len(ok)) if q != v and np.hypot(*(blk(q)[:, 1:3] - p0).T).min() > 2.5]
    assert len(far) >= 8
    _tilt(m, p0, 0.4)
    after = src.check(ok, limits=lim)
    ref1 = _ref(src, m, 0.01, 1)
    _same(after, _expect(ref1, ok, lim), "after")
    # the patch and the cells interpolated with it: rows within 0.4 m + two cells
    inside = mine[np.hypot(*(mine[:, 1:3] - p0).T) < 0.4 + 2 * m.xy_resolution, 0]
    assert inside.min() <= after["first_t"][v] <= inside.max(), (after["first_t"][v], inside.min(), inside.max())
    assert after["first_mask"][v] & ((1 << 4) | (1 << CHECK_OCC_BIT)) and after["counts"][v, 2] > 0
    assert after["worst"][v, 4] > lim[4] and inside.min() <= after["worst_t"][v, 4] <= inside.max()
    for k in KEYS:
        assert np.array_equal(after[k][far], before[k][far], equal_nan=True), k
    # refine the violators from a little before their first violation, solve, check the new batch
    bad = np.nonzero(after["first_mask"] != 0)[0]
    assert v in bad
    dst = U.ALMTrajOpt(m)
    dst.set_rho(1.0)
    out = dst.refine(src, ok[bad], after["first_t"][bad] - 0.5)
    org = dst.origin()
    tr2 = np.array([r["traj_of"] for r in out if r["status"] == 0 and r["ret"] != 4], dtype=np.int32)
    assert tr2.size >= 1 and [int(org[j]) for j in tr2] == [q for q, r in enumerate(out) if r["status"] == 0 and r["ret"] != 4]
    again = dst.check(tr2, limits=lim)
    _same(again, _expect(_ref(dst, m, 0.01, 1), tr2, lim), "refined")
    assert (again["counts"][:, 0] > 0).all()


def test_nan_under_the_path():
    """one cell under a trajectory holds |zb| > 1 (sqrt of a negative number in the lookup): NaN terms violate at the first sample that reads the cell
    and read +inf; the other trajectories are unchanged"""
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array([j for j in _valid(res) if res[j]["ret"] == 0], dtype=np.int32)
    before = src.check(ok, limits=NOLIM)
    offs, rows, _ = _ref(src, m, 0.01, 1)
    blk = lambda q: rows[int(offs[ok[q]]):int(offs[ok[q] + 1])]
    mine = blk(0)
    p0 = mine[mine.shape[0] // 2, 1:3].copy()
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    cells = np.array(m.map_buffer, dtype=np.float64).reshape(nx, ny, nyaw, 4)
    ix, iy = (int(np.floor((p0[d] - m.map_origin[d]) / m.xy_resolution)) for d in range(2))
    cells[ix, iy, :, 2] = 8.0                                                    # its weight at p0 is at least 1/4: the interpolated |zb| exceeds 1 there
    m.set_cells(cells.reshape(-1, 4))
    after = src.check(ok, limits=NOLIM)
    ref1 = _ref(src, m, 0.01, 1)
    _same(after, _expect(ref1, ok, NOLIM), "nan")
    now = ref1[1][int(offs[ok[0]]):int(offs[ok[0] + 1])]
    nanrow = np.isnan(now[:, 9:16]).any(axis=1)
    assert nanrow.any() and np.hypot(*(now[nanrow, 1:3] - p0).T).max() < 3 * m.xy_resolution
    first = int(np.argmax(nanrow))
    assert after["first_t"][0] == now[first, 0] and after["first_mask"][0] & 0x7f
    hit = np.isnan(now[:, 9:16]).any(axis=0)
    assert (after["worst"][0, hit] == INF).all() and np.isfinite(after["worst"][0, ~hit]).all()
    for k in np.nonzero(hit)[0]:
        assert after["worst_t"][0, k] == now[int(np.argmax(np.isnan(now[:, 9 + k]))), 0]
    far = [q for q in range(1, len(ok)) if np.hypot(*(blk(q)[:, 1:3] - p0).T).min() > 1.0]
    assert len(far) >= 8
    for k in KEYS:
        assert np.array_equal(after[k][far], before[k][far], equal_nan=True), k


def test_local_frames_and_fp32_cells():
    """a grid beyond FRAME_EXTENT (every trajectory solved in its own local frame, the occupancy looked up in map coordinates) and an fp32-cell map"""
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
        for dt, we in ((0.01, 0), (0.03, 1)):
            ref = _ref(opt, m, dt, we)
            if tag == "frames":
                assert np.abs(ref[1][:, 1:3]).max() > 45.0
            lim = _median_limits(ref, tr)
            got = opt.check(tr, dt=dt, with_end=we, limits=lim)
            _same(got, _expect(ref, tr, lim), tag)
            assert (got["first_mask"] != 0).any() and (got["counts"][:, 0] > 30).all()
            t1 = ref[1][ref[0][1:] - 1, 0]
            _same(opt.check(tr, 0.3 * t1, 0.7 * t1, dt=dt, with_end=we, limits=lim), _expect(ref, tr, lim, 0.3 * t1, 0.7 * t1), tag + " windows")


def test_duplicates_and_query_order(hill):
    src, ok, ref, lim = hill["src"], hill["ok"], hill["refs"][(0.03, 1)], hill["lim"]
    rng = np.random.default_rng(3)
    tr = np.concatenate([ok, ok[:9], np.repeat(ok[4], 5)]).astype(np.int32)
    tf = rng.uniform(0.0, 2.0, tr.size)
    tf[-5:] = tf[4]
    tt = tf + rng.uniform(0.0, 6.0, tr.size)
    tt[-5:] = tt[4]
    got = src.check(tr, tf, tt, dt=0.03, limits=lim)
    _same(got, _expect(ref, tr, lim, tf, tt), "duplicates")
    for k in KEYS:
        assert np.array_equal(got[k][-5:], np.repeat(got[k][4:5], 5, axis=0), equal_nan=True)
    perm = rng.permutation(tr.size)
    sh = src.check(tr[perm], tf[perm], tt[perm], dt=0.03, limits=lim)
    for k in KEYS:
        assert np.array_equal(sh[k], got[k][perm], equal_nan=True), k


def _raw(c, tr, tf, tt=None, dt=0.01, with_end=1, n=None, null=()):
    tr = np.ascontiguousarray(tr, dtype=np.int32)
    tf = np.ascontiguousarray(tf, dtype=np.float64)
    tt = None if tt is None else np.ascontiguousarray(tt, dtype=np.float64)
    n = tr.size if n is None else n
    m = max(1, tr.size)
    o = dict(first_t=np.full(m, -9.0), first_mask=np.full(m, -9, dtype=np.int32), counts=np.full((m, 3), -9, dtype=np.int32),
             worst=np.full((m, 7), -9.0), worst_t=np.full((m, 7), -9.0))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(_lib.DP)
    rc = c.L.uph_check_batch(c.h if c is not None and "ctx" not in null else None, n, None if "traj" in null else ip(tr), None if "t_from" in null else dp(tf),
                             None if tt is None else dp(tt), dt, with_end, None, dp(o["first_t"]), ip(o["first_mask"]), ip(o["counts"]), dp(o["worst"]),
                             dp(o["worst_t"]))
    return rc, o


def test_refusals(hill):
    """each refusal of include/uneven_hip.h: UPH_ERR_INVALID (UPH_ERR_LIMIT for too many samples) with every output as it was pre-filled"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m, ka, src, ok = hill["m"], hill["ka"], hill["src"], hill["ok"]
    F = src.L.uph_batch_count(src.h)
    untouched = lambda o: all((o[k] == -9).all() for k in o)
    tr = ok[:4]

    def refused(rc, o, what, code=-1):
        assert rc == code and untouched(o), (what, rc)

    for null in (("ctx",), ("traj",), ("t_from",)):
        refused(*_raw(src, tr, np.zeros(4), null=null), null)
    refused(*_raw(src, tr, np.zeros(4), n=0), "n = 0")
    refused(*_raw(src, tr, np.zeros(4), n=-3), "n < 0")
    for dt in (0.0, -0.01, INF, float("nan")):
        refused(*_raw(src, tr, np.zeros(4), dt=dt), ("dt", dt))
    fresh = U.ALMTrajOpt(m)
    fresh.plan_goals_upload(ka, hill["S"][:8], hill["G"][:8])                 # uploaded, not solved: no resident trajectory
    rc, o = _raw(fresh, [0], [0.0])
    refused(rc, o, "not resident")
    assert b"resident" in src.L.uph_last_error()
    refused(*_raw(U.ALMTrajOpt(m), [0], [0.0]), "no batch")
    for bad in ([F], [-1], [int(ok[0]), F + 7]):
        refused(*_raw(src, bad, [0.5] * len(bad)), ("index", bad))
    for t in (float("nan"), INF, -INF):
        refused(*_raw(src, tr, [0.1, t, 0.2, 0.3]), ("t_from", t))
    refused(*_raw(src, tr, np.zeros(4), [1.0, 2.0, float("nan"), 3.0]), "NaN t_to")
    for t in (INF, -INF):                                                       # an infinite t_to is a window
        rc, o = _raw(src, tr, np.zeros(4), [1.0, t, 2.0, 3.0])
        assert rc == 0 and not untouched(o) and o["counts"][1, 0] == (0 if t < 0 else np.diff(hill["refs"][(0.01, 1)][0])[tr[1]])
    refused(*_raw(src, tr, np.zeros(4), dt=1e-6), "too many samples", code=_lib.UPH_ERR_LIMIT)
    # an UPH_RET_UNSUPPORTED slot: a problem beyond UPH_MAX_PIECE_XY next to ordinary ones
    probs = scenes.random_problems(3, seed0=2100)
    big = dict(probs[0])
    big["inner_xy"] = np.linspace([0.0, 0.0], [3.0, 0.5], 140).T.copy()
    big["inner_yaw"] = np.zeros(140)
    uns = U.ALMTrajOpt(m)
    uns.set_rho(1.0)
    assert uns.optimize_batch(probs + [big])[3]["ret"] == 4
    rc, o = _raw(uns, [0, 3], [0.0, 0.0])
    refused(rc, o, "unsupported slot")
    assert b"UNSUPPORTED" in src.L.uph_last_error()
    assert _raw(uns, [0, 1, 2], np.zeros(3))[0] == 0
    # an asynchronous solve pending
    src2, _ = _source(m, ka, hill["S"][:32], hill["G"][:32])
    src2.solve_async()
    rc, o = _raw(src2, [0], [0.0])
    src2.wait()
    refused(rc, o, "pending")
    assert b"in flight" in src.L.uph_last_error()
    # any output pointer may be NULL
    one = np.full(4, -9, dtype=np.int32)
    z = np.zeros(4)
    assert src.L.uph_check_batch(src.h, 4, tr.ctypes.data_as(C.POINTER(C.c_int32)), z.ctypes.data_as(_lib.DP), None, 0.01, 1, None, None,
                                 one.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None) == 0
    assert np.array_equal(one, src.check(tr)["first_mask"])


CPP = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
#include <cstdio>
using namespace uneven_hip;
static void put(FILE* o, const ALMTrajOpt::TrajCheck& r) {
    for (size_t q = 0; q < r.first_t.size(); q++) {
        double h[5] = {r.first_t[q], (double)r.first_mask[q], (double)r.counts[3 * q], (double)r.counts[3 * q + 1], (double)r.counts[3 * q + 2]};
        fwrite(h, 8, 5, o);
        fwrite(r.worst.data() + 7 * q, 8, 7, o);
        fwrite(r.worst_t.data() + 7 * q, 8, 7, o);
    }
}
int main(int argc, char** argv) {
    // in: {ncell, B}, cells, B x {start, goal, fractions of the planned duration the window starts and ends at}
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
    ALMTrajOpt opt;
    opt.setEnvironment(&map);
    std::vector<std::array<double, 3>> starts((size_t)hdr[1]), goals((size_t)hdr[1]);
    for (long long b = 0; b < hdr[1]; b++) for (int k = 0; k < 3; k++) { starts[b][k] = sg[8 * b + k]; goals[b][k] = sg[8 * b + 3 + k]; }
    uph_manager_params mgr{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5};
    ALMTrajOpt::GoalPlan p = opt.planSE2TrajBatch(kino, starts, goals, mgr);
    std::vector<int> traj;
    std::vector<double> tf, tt;
    for (long long b = 0; b < hdr[1]; b++)
        if (p.traj_of[b] >= 0 && p.ret[b] != UPH_RET_UNSUPPORTED) {
            traj.push_back(p.traj_of[b]); tf.push_back(sg[8 * b + 6] * p.total_time[b]); tt.push_back(sg[8 * b + 7] * p.total_time[b]);
        }
    const ALMTrajOpt::TrajCheck a = opt.checkSE2TrajBatch(traj, tf, tt);                 // the optimiser's limits, every 0.01 s, with the end point
    std::vector<double> lim = opt.checkLimits();
    for (int k = 0; k < 4; k++) lim[k] *= 0.5;
    const ALMTrajOpt::TrajCheck c = opt.checkSE2TrajBatch(traj, tf, {}, 0.03, false, lim.data());
    // out: n, per query traj, t_from, t_to; then the two results, per query first_t, first_mask, counts[3], worst[7], worst_t[7]
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
    """ALMTrajOpt::checkSE2TrajBatch from a compiled C++ consumer (after planSE2TrajBatch) against plan_goals + check through ctypes"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    ka = U.KinoAstar(m)
    S, G = scenes.random_queries(24, seed0=9900)
    f0 = np.array([[0.0, 0.3, 0.5, -0.2, 0.95, 0.6][b % 6] for b in range(S.shape[0])])
    f1 = np.array([[1.0, 0.6, 2.0, 0.4, 1.0, 0.5][b % 6] for b in range(S.shape[0])])
    mk = dict(piece_len=0.3, mean_vel=0.5, init_time_times=1.2, yaw_piece_times=2.0, init_sig_vel=0.05, test_mode=0, test_max_vel=0.5)
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    plan = opt.plan_goals(ka, S, G, **mk)
    src_ = tmp_path / "check.cpp"
    src_.write_text(CPP)
    exe = str(tmp_path / "check")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src_), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    cells = np.ascontiguousarray(analytic_cells, dtype=np.float64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2q", cells.shape[0], S.shape[0]))
        f.write(cells.tobytes())
        f.write(np.ascontiguousarray(np.concatenate([S, G, f0[:, None], f1[:, None]], axis=1), dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, dtype=np.float64)
    n = int(raw[0])
    want_tr = [plan[b]["traj_of"] for b in range(S.shape[0]) if plan[b]["status"] == 0 and plan[b]["ret"] != 4]
    assert n == len(want_tr) >= 10 and raw.size == 1 + 3 * n + 2 * 19 * n
    q = raw[1:1 + 3 * n].reshape(n, 3)
    assert q[:, 0].astype(int).tolist() == want_tr
    res = raw[1 + 3 * n:].reshape(2, n, 19)
    lim = opt.check_limits()
    lim[:4] *= 0.5
    for got, want in ((res[0], opt.check(want_tr, q[:, 1], q[:, 2])), (res[1], opt.check(want_tr, q[:, 1], None, dt=0.03, with_end=False, limits=lim))):
        cpp = dict(first_t=got[:, 0], first_mask=got[:, 1].astype(np.int32), counts=got[:, 2:5].astype(np.int32), worst=got[:, 5:12], worst_t=got[:, 12:19])
        _same(cpp, want, "adapter")
    assert (res[1][:, 1] != 0).any() and (res[0][:, 2] > 0).any() and (res[0][:, 2] == 0).any()
