"""GPU tier of the clearance layer (uph_clearance_*, csrc/clearance.hip) and of the query that reads it (uph_clearance_check_batch, csrc/traj_query.hip).

The layer is integer arithmetic on the body layer's bytes, the query a table look-up at cells formed by floor statements the mirror repeats: every comparison
is np.array_equal (NaN-aware) against the numpy mirrors of uneven_planner_amd/clearance.py, no tolerance anywhere.

C1: hand-set body bytes on the two small grids (sides no multiple of anything, 63 and 32 yaw bins), every rmax up to one wider than the grids, both polarities.
C2: the hill grid with the car's conservative layer.  C3: update(rect) against a fresh build, the chain after a real map update, and that nothing outside the
grown rect is written.  C4: freshness and lifetime.  C5: the query against the mirror.  C6: the tie to the footprint check.  C7: determinism, independent
layers, the C++ adapter.  tests/test_gpu_footprint_check.py has no way to MAKE a sample outside the grid; where a solved trajectory of C5's batch swings over
the border the outside branch runs here against the mirror (the count is printed, not required), and the mirror's own hand-made rows in
tests/test_clearance_cpu.py hold the branch in every case."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_replan import _hill_map, _queries, _source
from test_gpu_separation import _totals, _valid
from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import FOOT_OCC_XY, FOOT_OUTSIDE, check_window, footprint_cover, footprint_grid
from uneven_planner_amd.clearance import CLEAR_FAR, CLEAR_TO_FREE, CLEAR_TO_OCCUPIED, clearance_check_rows, clearance_rows, grow_rect

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAR = (0.45, 0.15, 0.3)
POINT = (0.0, 0.0, 0.0)
# (map_size_x, map_size_y, yaw_resolution) -> 40 x 30 x 63 and 37 x 53 x 32, as tests/test_gpu_body_layer.py makes them
GRIDS = {"40x30x63": (dict(map_size_x=1.99, map_size_y=1.49, yaw_resolution=0.101), (40, 30, 63)),
         "37x53x32": (dict(map_size_x=1.84, map_size_y=2.64, yaw_resolution=0.2), (37, 53, 32))}
KEYS = ("min_d2", "min_t", "min_cell", "first_t", "last_t", "counts")
INF = float("inf")


def _map(params=None):
    import uneven_planner_amd as U
    return U.UnevenMap(params=params)


def _flat(m):
    """flat free cells: a map whose occupancy is empty, for body layers whose bytes the test sets by hand"""
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    m.set_cells(np.zeros((nx * ny * nyaw, 4)))
    return m


def _tilt_discs(m, centres, radius):
    """the columns whose centre lies within radius of one of the centres tilted beyond min_cnormal (tests/test_gpu_body_layer.py's)"""
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


def _patterns(dims):
    nx, ny, nyaw = dims
    rng = np.random.default_rng(nx + ny)
    out = {"zeros": np.zeros(dims, dtype=np.int8), "ones": np.ones(dims, dtype=np.int8)}
    c = np.zeros(dims, dtype=np.int8)
    c[0, 0, 0] = c[0, ny - 1, 1] = c[nx - 1, 0, nyaw // 2] = c[nx - 1, ny - 1, nyaw - 1] = 1
    out["corners"] = c
    s = np.zeros(dims, dtype=np.int8)
    s[:, :, nyaw // 3] = 1
    out["one-slice"] = s
    for d in (0.002, 0.05, 0.5):
        out["random-%g" % d] = (rng.uniform(size=dims) < d).astype(np.int8)     # every slice drawn on its own
    return out


# ---- C1 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
def test_patterns_on_small_grids_against_the_mirror(grid):
    """C1"""
    import uneven_planner_amd as U
    params, dims = GRIDS[grid]
    m = _flat(_map(params))
    assert tuple(int(v) for v in m.voxel_num) == dims
    body = U.BodyLayer(m, POINT, 0.0, FOOT_OCC_XY)
    n_near = n_far = 0
    for name, b in _patterns(dims).items():
        body.set(b)
        for rmax in (1, 5, 13, 64, 254):
            for pol in (CLEAR_TO_OCCUPIED, CLEAR_TO_FREE):
                layer = U.ClearanceLayer(body, rmax, pol)
                info = layer.info()
                assert info["fresh"] and info["dims"] == list(dims) and info["rmax"] == rmax and info["polarity"] == pol
                got, want = layer.get(), clearance_rows(b, rmax, pol)
                assert got.dtype == np.uint16 and np.array_equal(got, want), (grid, name, rmax, pol, int((got != want).sum()))
                n_near += int(((got > 0) & (got != CLEAR_FAR)).sum())
                n_far += int((got == CLEAR_FAR).sum())
                layer.close()
    assert n_near > 0 and n_far > 0
    body.close()


# ---- C2 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_hill_grid_with_the_cars_layer_against_the_mirror():
    """C2: the hill as built with 60 discs tilted over it (tests/test_gpu_body_layer.py B2), the car's conservative layer"""
    import uneven_planner_amd as U
    m = _hill_map()
    rng = np.random.default_rng(12)
    _tilt_discs(m, rng.uniform(-4.8, 4.8, (60, 2)), 0.12)
    car = U.BodyLayer(m, CAR)
    b = car.get()
    assert 0 < b.sum() < b.size
    for rmax in (20, 64):
        layer = U.ClearanceLayer(car, rmax)
        got = layer.get()
        assert np.array_equal(got, clearance_rows(b, rmax)) and np.array_equal(got == 0, b == 1)
        assert layer.kernel_ms() > 0.0
        print("C2 rmax %d: %d cells far, max near %d, build %.3f ms" % (rmax, int((got == CLEAR_FAR).sum()), int(got[got != CLEAR_FAR].max()), layer.kernel_ms()))
        layer.close()
    depth = U.ClearanceLayer(car, 20, CLEAR_TO_FREE)
    assert np.array_equal(depth.get(), clearance_rows(b, 20, CLEAR_TO_FREE))
    depth.close()


# ---- C3 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", [(17, 18, 11, 12), (0, 6, 9, 21), (31, 40, 22, 30), (0, 40, 0, 30)], ids=["one-byte", "border", "corner", "whole"])
def test_update_equals_a_fresh_build(rect):
    """C3: body bytes changed inside a rect, update(rect) against a fresh build and the mirror, bit for bit, at a small rmax and one wider than the grid; a layer
    that does not hear of the change keeps its values"""
    import uneven_planner_amd as U
    params, dims = GRIDS["40x30x63"]
    nx, ny, nyaw = dims
    m = _flat(_map(params))
    body = U.BodyLayer(m, POINT, 0.0, FOOT_OCC_XY)
    rng = np.random.default_rng(sum(rect))
    b = (rng.uniform(size=dims) < 0.03).astype(np.int8)
    body.set(b)
    layers = [U.ClearanceLayer(body, 5), U.ClearanceLayer(body, 64), U.ClearanceLayer(body, 5, CLEAR_TO_FREE)]
    before = [l.get() for l in layers]
    x0, x1, y0, y1 = rect
    if (x1 - x0) * (y1 - y0) == 1:
        b[x0, y0, 7] ^= 1                   # one byte
    else:
        b[x0:x1, y0:y1] = rng.uniform(size=(x1 - x0, y1 - y0, nyaw)) < 0.2
    body.set(b)
    for l, old in zip(layers, before):
        assert l.info()["behind"] == 1 and np.array_equal(l.get(), old)
        l.update(rect)
        assert l.info()["fresh"]
        got = l.get()
        fresh = U.ClearanceLayer(body, l.rmax, l.polarity)
        assert not np.array_equal(got, old)
        assert np.array_equal(got, fresh.get()) and np.array_equal(got, clearance_rows(b, l.rmax, l.polarity)), (rect, l.rmax, l.polarity)
        fresh.close()
    # an empty rect is accepted, writes nothing and stamps
    body.set(b)
    keep = layers[0].get()
    layers[0].update((3, 3, 0, 5))
    assert np.array_equal(layers[0].get(), keep) and layers[0].info()["fresh"] and layers[0].kernel_ms() == 0.0
    for l in layers:
        l.close()


def test_nothing_outside_the_grown_rect_is_written():
    """C3, last case: two changes far apart and a rect that names one of them.  Inside the rect grown by rmax the field is the new build's; everywhere else --
    around the other change too -- it is still the old one"""
    import uneven_planner_amd as U
    params, dims = GRIDS["40x30x63"]
    m = _flat(_map(params))
    body = U.BodyLayer(m, POINT, 0.0, FOOT_OCC_XY)
    rng = np.random.default_rng(77)
    b = (rng.uniform(size=dims) < 0.01).astype(np.int8)
    body.set(b)
    rmax = 5
    layer = U.ClearanceLayer(body, rmax)
    old = layer.get()
    b[5, 5, :], b[33, 24, :] = 1 - b[5, 5, :], 1 - b[33, 24, :]
    body.set(b)
    named = (5, 6, 5, 6)
    layer.update(named)
    got, new = layer.get(), clearance_rows(b, rmax)
    g = grow_rect(dims[:2], named, rmax)
    assert g == (0, 11, 0, 11)
    inside = np.zeros(dims, dtype=bool)
    inside[g[0]:g[1], g[2]:g[3]] = True
    assert np.array_equal(got, np.where(inside, new, old))
    assert not np.array_equal(new[inside], old[inside]) and not np.array_equal(new[28:39, 19:30], old[28:39, 19:30])
    assert np.array_equal(got[28:39, 19:30], old[28:39, 19:30])
    layer.close()


def test_the_chain_after_a_real_map_update():
    """C3: uph_map_update on the hill cloud (tests/map_update_cases.py), then BodyLayer.update(changed), then ClearanceLayer.update of that rect grown by R"""
    import uneven_planner_amd as U
    import map_update_cases as MU
    m = _hill_map()
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    car = U.BodyLayer(m, CAR)
    layer = U.ClearanceLayer(car, 20)
    before = layer.get()
    info = m.update(MU.BOX, MU.scan(mound=0.6, sigma=0.07))
    assert info["n_changed"] > 0 and car.info()["behind"] == 1 and layer.info()["fresh"]
    w0 = car.writes()
    car.update(info["changed"])
    assert car.writes() == w0 + 1 and layer.info()["behind"] == 1
    rewritten = grow_rect((nx, ny), info["changed"], car.info()["R"])
    layer.update(rewritten)
    got = layer.get()
    fresh = U.ClearanceLayer(U.BodyLayer(m, CAR), 20)
    assert layer.info()["fresh"] and np.array_equal(got, fresh.get()) and np.array_equal(got, clearance_rows(car.get(), 20))
    assert not np.array_equal(got, before)
    print("C3 chain: changed %s, body rewrote %s, clearance rewrote %s, %d values differ, update %.3f ms" % (
        list(info["changed"]), rewritten, grow_rect((nx, ny), rewritten, 20), int((got != before).sum()), layer.kernel_ms()))


# ---- the solved batch of C4, C5 and C7 -----------------------------------------------------------------------------------------------------------------------
def _beside(st, side):
    """the point `side` metres to the left of the pose of a traj_states row"""
    return np.array([st[0] - side * np.sin(st[9]), st[1] + side * np.cos(st[9])])


@pytest.fixture(scope="module")
def hill():
    """16 hill goals solved on a map of their own, then discs of 0.1 m tilted 0.4 m beside the paths (the body layer's band does not reach them all: values
    above 0 along the paths, and 0 where a disc is close), the car's conservative layer and its clearance at rmax 20"""
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 16, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array(_valid(res), dtype=np.int32)
    assert len(ok) >= 8, len(ok)
    total = _totals(src)
    rng = np.random.default_rng(17)
    fr = rng.uniform(0.15, 0.85, (len(ok), 2))
    st = src.traj_states(np.repeat(ok, 2), (fr * total[ok][:, None]).ravel())
    side = np.where(np.arange(st.shape[0]) % 2 == 0, 0.4, -0.55)
    _tilt_discs(m, np.array([_beside(s, d) for s, d in zip(st, side)]), 0.1)
    car = U.BodyLayer(m, CAR)
    layer = U.ClearanceLayer(car, 20)
    return dict(m=m, ka=ka, src=src, ok=ok, total=total, car=car, layer=layer, D=layer.get(), times={})


def _times(hill, dt, with_end):
    """per resident trajectory the sample times of rollout(dt, with_end), computed once per (dt, with_end)"""
    key = (dt, bool(with_end))
    if key not in hill["times"]:
        offs, rows = hill["src"].rollout(dt, 1, with_end=bool(with_end))
        hill["times"][key] = [rows[int(offs[b]):int(offs[b + 1]), 0].copy() for b in range(len(offs) - 1)]
    return hill["times"][key]


def _expect(hill, opt, traj, src_traj, tf, tt, dt, with_end, below2, D=None):
    """the mirror's rows: per query the window's times (t_from <= t <= t_to in the rollout's table, checked against uph_check_window), the states there
    (traj_states of `opt`), their cells by footprint_cover's point statements, clearance_check_rows"""
    m = hill["m"]
    D = hill["D"] if D is None else D
    times = _times(hill, dt, with_end)
    n = len(traj)
    tt = np.full(n, INF) if tt is None else np.asarray(tt, dtype=np.float64)
    ts = []
    for q in range(n):
        t = times[int(src_traj[q])]
        sel = t[(t >= tf[q]) & (t <= tt[q])]
        lo, hi, end = check_window(dt, with_end, hill["total"][int(src_traj[q])], tf[q], tt[q])
        assert sel.shape[0] == hi - lo + end, (q, sel.shape[0], lo, hi, end)
        ts.append(sel)
    sizes = [t.shape[0] for t in ts]
    st = opt.traj_states(np.concatenate([np.full(k, b, dtype=np.int32) for k, b in zip(sizes, traj)]), np.concatenate(ts)) if sum(sizes) else np.zeros((0, 10))
    sts = np.split(st, np.cumsum(sizes)[:-1])
    rows = []
    for q in range(n):
        if sizes[q] == 0:
            rows.append(clearance_check_rows(ts[q], np.zeros((0, 3)), np.zeros(0, dtype=bool), D, D.shape, int(below2[q])))
            continue
        cv = footprint_cover(sts[q][:, [0, 1, 9]], sts[q][:, 6], POINT, 0.0, footprint_grid(m))
        rows.append(clearance_check_rows(ts[q], np.concatenate([cv["point"], cv["iw"][:, None]], axis=1), cv["ok"], D, D.shape, int(below2[q])))
    return {k: np.array([r[k] for r in rows]) for k in KEYS}, sizes


def _eq(got, want, tag=""):
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64), equal_nan=True), (tag, k, got[k], want[k])


def _c5_queries(hill, dt, with_end, seed):
    """per trajectory a full window, two partial ones, one of at most 41 samples (one wave) and an empty one (a gap between two samples), below2 cycling through
    1, 25, FAR; shuffled"""
    rng = np.random.default_rng(seed)
    times = _times(hill, dt, with_end)
    tr, tf, tt, b2 = [], [], [], []
    for k, b in enumerate(hill["ok"]):
        t = times[int(b)]
        i0, i1 = sorted(int(v) for v in rng.integers(0, t.shape[0] - 1, 2))
        j = int(rng.integers(0, t.shape[0] - 1))
        for a, e in ((0.0, INF), (t[i0], t[i1]), (t[i1], INF), (t[i0], t[min(i0 + 40, t.shape[0] - 1)]), (0.75 * t[j] + 0.25 * t[j + 1], 0.25 * t[j] + 0.75 * t[j + 1])):
            tr.append(int(b)); tf.append(a); tt.append(e); b2.append((1, 25, CLEAR_FAR)[len(tr) % 3])
    p = rng.permutation(len(tr))
    return np.array(tr, dtype=np.int32)[p], np.array(tf)[p], np.array(tt)[p], np.array(b2, dtype=np.int32)[p]


# ---- C5 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,with_end", [(0.01, True), (0.01, False), (0.05, True), (0.05, False)])
def test_the_query_against_the_mirror(hill, dt, with_end):
    """C5: full, partial and empty windows at both launch widths (256 lanes beyond 192 samples, one wave up to them), below2 1, 25 and FAR; a permutation of
    the queries and one query alone give the same rows"""
    src, layer = hill["src"], hill["layer"]
    tr, tf, tt, b2 = _c5_queries(hill, dt, with_end, 23)
    got = src.clearance(layer, tr, below2=b2, t_from=tf, t_to=tt, dt=dt, with_end=with_end)
    want, sizes = _expect(hill, src, tr, tr, tf, tt, dt, with_end, b2)
    _eq(got, want, (dt, with_end))
    assert np.array_equal(got["below2"], b2) and src.clearance_kernel_ms() > 0.0
    empty = np.array(sizes) == 0
    assert empty.sum() >= len(hill["ok"]) and (got["min_d2"][empty] == -1).all() and np.isnan(got["min_t"][empty]).all() and (got["min_cell"][empty] == -1).all()
    assert (got["counts"][:, 0] == sizes).all()
    outside = got["counts"][:, 2] > 0          # a solved trajectory may swing over the grid's border: value 0, counted, and no cell when it is the earliest 0
    assert (got["min_d2"][outside] == 0).all()
    print("C5 dt %g with_end %d: %d queries, %d samples, %d outside the grid in %d queries" % (dt, with_end, len(tr), sum(sizes), int(got["counts"][:, 2].sum()), int(outside.sum())))
    seen = got["min_d2"][~empty]
    assert (seen == 0).any() and ((seen > 0) & (seen < CLEAR_FAR)).any(), seen
    assert (dt != 0.01 or max(sizes) > 256) and 0 < min(s for s in sizes if s) <= 41         # both launch widths
    # min_d in metres
    res = hill["m"].xy_resolution
    d = got["min_d"]
    assert np.isnan(d[empty]).all() and np.array_equal(d[~empty], np.where(seen == CLEAR_FAR, INF, res * np.sqrt(seen.astype(np.float64))))
    # the same queries in another order, and one alone
    p = np.random.default_rng(5).permutation(len(tr))
    again = src.clearance(layer, tr[p], below2=b2[p], t_from=tf[p], t_to=tt[p], dt=dt, with_end=with_end)
    _eq(again, {k: got[k][p] for k in KEYS}, "permutation")
    q = int(np.nonzero(~empty)[0][0])
    alone = src.clearance(layer, tr[[q]], below2=b2[[q]], t_from=tf[[q]], t_to=tt[[q]], dt=dt, with_end=with_end)
    _eq(alone, {k: got[k][[q]] for k in KEYS}, "alone")


def test_below_in_metres_to_the_end_and_a_fleet(hill):
    """C5: `below` in metres is ceil((below / res)^2); t_to = None runs to the end; a TrajFleet the batch was adopted into answers with the same rows; the depth
    layer (CLEAR_TO_FREE) is read the same way"""
    import uneven_planner_amd as U
    src, m, ok, layer, car = hill["src"], hill["m"], hill["ok"], hill["layer"], hill["car"]
    n = len(ok)
    tf = np.zeros(n)
    got = src.clearance(layer, ok, below=0.2)
    assert (got["below2"] == 16).all()
    want, _ = _expect(hill, src, ok, ok, tf, None, 0.01, True, np.full(n, 16))
    _eq(got, want, "metres")
    _eq(src.clearance(layer, ok, below2=16), want, "below2")
    with pytest.raises(_lib.UnevenHipError, match="exactly one"):
        src.clearance(layer, ok)
    fleet = U.TrajFleet(m, n + 3)
    slots = np.random.default_rng(2).permutation(n + 3)[:n].astype(np.int32)
    fleet.adopt(src, ok, slots)
    rng = np.random.default_rng(9)
    a, e = rng.uniform(0.0, 0.4, n) * hill["total"][ok], rng.uniform(0.6, 1.1, n) * hill["total"][ok]
    b2 = np.array([(1, 25, CLEAR_FAR)[k % 3] for k in range(n)], dtype=np.int32)
    mine = src.clearance(layer, ok, below2=b2, t_from=a, t_to=e)
    _eq(fleet.clearance(layer, slots, below2=b2, t_from=a, t_to=e), mine, "fleet")
    _eq(mine, _expect(hill, src, ok, ok, a, e, 0.01, True, b2)[0], "windows")
    assert fleet.clearance_kernel_ms() > 0.0
    free = sorted(set(range(n + 3)) - set(slots.tolist()))
    with pytest.raises(_lib.UnevenHipError, match="empty slot"):
        fleet.clearance(layer, free[:1], below2=1)
    depth = U.ClearanceLayer(car, 20, CLEAR_TO_FREE)
    _eq(src.clearance(depth, ok, below2=b2, t_from=a, t_to=e), _expect(hill, src, ok, ok, a, e, 0.01, True, b2, D=depth.get())[0], "depth")
    depth.close()


# ---- C4 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_freshness_and_lifetime(hill):
    """C4: one write of the body layer behind -- the query is refused, update is accepted; two behind -- "rebuild"; the map written -- the query is refused
    until both layers follow; a body layer is not destroyed while a clearance layer names it; a context on another map is refused"""
    import uneven_planner_amd as U
    src, m, ok = hill["src"], hill["m"], hill["ok"]
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    car = U.BodyLayer(m, CAR)
    layer = U.ClearanceLayer(car, 20)
    want = src.clearance(layer, ok, below2=25)
    _eq(want, src.clearance(hill["layer"], ok, below2=25), "a second layer")
    b, keep = car.get(), layer.get()
    w0 = car.writes()
    car.set(b)
    assert car.writes() == w0 + 1 and layer.info()["behind"] == 1 and not layer.info()["fresh"]
    with pytest.raises(_lib.UnevenHipError, match="behind its body layer"):
        src.clearance(layer, ok, below2=25)
    layer.update((0, 0, 0, 0))                  # nothing changed: the empty rect
    assert layer.info()["fresh"]
    _eq(src.clearance(layer, ok, below2=25), want, "after the update")
    car.set(b)
    car.build()
    assert car.writes() == w0 + 3 and layer.info()["behind"] == 2
    with pytest.raises(_lib.UnevenHipError, match="rebuild"):
        layer.update((0, nx, 0, ny))
    assert layer.info()["behind"] == 2 and np.array_equal(layer.get(), keep)
    layer.build()
    assert layer.info()["fresh"] and np.array_equal(layer.get(), keep)
    # the map written (the same cells: the occupancy's write count moves, its bytes do not)
    m.set_cells(m.map_buffer)
    assert car.info()["behind"] == 1 and layer.info()["fresh"]
    with pytest.raises(_lib.UnevenHipError, match="behind the map"):
        src.clearance(layer, ok, below2=25)
    car.update((0, 0, 0, 0))
    with pytest.raises(_lib.UnevenHipError, match="behind its body layer"):
        src.clearance(layer, ok, below2=25)
    layer.update((0, 0, 0, 0))
    _eq(src.clearance(layer, ok, below2=25), want, "after the map write")
    # refusals of the query itself: nothing is written
    with pytest.raises(_lib.UnevenHipError, match="below2"):
        src.clearance(layer, ok[:2], below2=[3, -1])
    other = _map()
    foreign = U.ALMTrajOpt(other)
    with pytest.raises(_lib.UnevenHipError, match="another map"):
        foreign.clearance(layer, [0], below2=1)
    for bad_r, bad_p in ((0, 0), (255, 0), (20, 2), (20, -1)):
        with pytest.raises(_lib.UnevenHipError, match="rmax|polarity"):
            U.ClearanceLayer(car, bad_r, bad_p)
    for rect in ((5, 4, 0, 3), (0, 3, 7, 6), (-1, 3, 0, 3), (0, nx + 1, 0, 3), (0, 3, -2, 3), (0, 3, 0, ny + 1)):
        with pytest.raises(_lib.UnevenHipError, match="rect"):
            layer.update(rect)
    assert np.array_equal(layer.get(), keep)
    # lifetime
    second = U.ClearanceLayer(car, 5)
    with pytest.raises(_lib.UnevenHipError, match="clearance layer"):
        car.close()
    layer.close()
    with pytest.raises(_lib.UnevenHipError, match="clearance layer"):
        car.close()
    assert car.h and np.array_equal(car.get(), b)
    second.close()
    car.close()
    assert car.h is None
    # the module's layers follow the map write above
    hill["car"].update((0, 0, 0, 0))
    hill["layer"].update((0, 0, 0, 0))
    assert hill["layer"].info()["fresh"] and np.array_equal(hill["layer"].get(), hill["D"])


# ---- C6 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_tie_to_the_footprint_check():
    """C6: the scene of tests/test_gpu_footprint_check.py C3 -- 64 hill goals, a disc of 0.1 m tilted 0.2 m beside one trajectory's mid pose -- and the car's
    conservative layer.  A 0 of the body layer says that the rectangle at margin 0 covers no occupied column centre at any pose of the cell, so wherever the
    footprint check at margin 0 hits, D is 0: the samples below 1 start no later, end no earlier and are no fewer than the footprint check's hit samples"""
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array([j for j in _valid(res) if res[j]["ret"] == 0], dtype=np.int32)
    total = _totals(src)
    before = src.footprint_check(ok, CAR, 0.05)
    clean = np.nonzero((before["counts"][:, 1] == 0) & (src.check(ok, limits=np.full(7, INF))["counts"][:, 2] == 0))[0]
    v = int(clean[0])
    mid = src.traj_states([ok[v]], [0.5 * total[ok[v]]])[0]
    _tilt_discs(m, [_beside(mid, 0.2)], 0.1)
    car = U.BodyLayer(m, CAR)
    layer = U.ClearanceLayer(car, 20)
    fc = src.footprint_check(ok, CAR, 0.0, layers=FOOT_OCC_XY | FOOT_OUTSIDE)
    cl = src.clearance(layer, ok, below2=1)
    hit = fc["counts"][:, 1] > 0
    assert hit[v] and np.array_equal(cl["counts"][:, 0], fc["counts"][:, 0])
    assert (cl["counts"][:, 1] >= fc["counts"][:, 1]).all()
    assert (cl["first_t"][hit] <= fc["first_t"][hit]).all() and (cl["last_t"][hit] >= fc["last_t"][hit]).all()
    assert (cl["min_d2"][hit] == 0).all()
    print("C6: %d of %d trajectories hit at margin 0 (%d samples); %d samples with D = 0" % (int(hit.sum()), len(ok), int(fc["counts"][:, 1].sum()), int(cl["counts"][:, 1].sum())))


# ---- C7 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_determinism_and_independent_layers(hill):
    """C7: two builds give the same values, layers on one body layer do not see each other, the query gives the same rows twice"""
    import uneven_planner_amd as U
    src, ok, car = hill["src"], hill["ok"], hill["car"]
    a, b = U.ClearanceLayer(car, 20), U.ClearanceLayer(car, 7, CLEAR_TO_FREE)
    ga, gb = a.get(), b.get()
    assert np.array_equal(ga, hill["D"]) and not np.array_equal(ga, gb)
    for _ in range(2):
        a.build()
        b.build()
        assert np.array_equal(a.get(), ga) and np.array_equal(b.get(), gb)
    b.update((10, 60, 20, 90))
    assert np.array_equal(a.get(), ga) and np.array_equal(b.get(), gb)
    one = src.clearance(a, ok, below2=25)
    _eq(src.clearance(a, ok, below2=25), one, "twice")
    _eq(src.clearance(hill["layer"], ok, below2=25), one, "another layer of the same field")
    a.close()
    b.close()


CPP = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
#include <cstdio>
using namespace uneven_hip;
static void put(FILE* o, const ALMTrajOpt::TrajClearance& r) {
    for (size_t q = 0; q < r.min_d2.size(); q++) {
        double h[11] = {(double)r.min_d2[q], r.min_t[q], (double)r.min_cell[q][0], (double)r.min_cell[q][1], (double)r.min_cell[q][2], r.first_t[q], r.last_t[q],
                        (double)r.counts[4 * q], (double)r.counts[4 * q + 1], (double)r.counts[4 * q + 2], (double)r.counts[4 * q + 3]};
        fwrite(h, 8, 11, o);
    }
}
int main(int argc, char** argv) {
    // in: {ncell, B}, cells, the second state's cells, B x {start, goal, fractions of the planned duration the window starts and ends at}
    FILE* f = std::fopen(argv[1], "rb");
    long long hdr[2];
    if (!f || fread(hdr, 8, 2, f) != 2) return 2;
    std::vector<double> cells((size_t)hdr[0] * 4), cells2((size_t)hdr[0] * 4), sg((size_t)hdr[1] * 8);
    if (fread(cells.data(), 8, cells.size(), f) != cells.size() || fread(cells2.data(), 8, cells2.size(), f) != cells2.size() ||
        fread(sg.data(), 8, sg.size(), f) != sg.size()) return 2;
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
    std::vector<int32_t> b2;
    for (long long b = 0; b < hdr[1]; b++)
        if (p.traj_of[b] >= 0 && p.ret[b] != UPH_RET_UNSUPPORTED) {
            traj.push_back(p.traj_of[b]); tf.push_back(sg[8 * b + 6] * p.total_time[b]); tt.push_back(sg[8 * b + 7] * p.total_time[b]);
            b2.push_back(ClearanceLayer::below2(0.1 * (double)(b % 4), mp.xy_resolution));
        }
    const std::array<double, 3> car{0.45, 0.15, 0.3};
    FILE* o = std::fopen(argv[2], "wb");
    {
        BodyLayer body(map, car, BodyLayer::conservativeMargin(mp, car));
        ClearanceLayer layer(body, 20), depth(body, 9, UPH_CLEAR_TO_FREE);
        double n = (double)traj.size();
        fwrite(&n, 8, 1, o);
        for (size_t k = 0; k < traj.size(); k++) { double q[4] = {(double)traj[k], tf[k], tt[k], (double)b2[k]}; fwrite(q, 8, 4, o); }
        put(o, opt.clearanceSE2TrajBatch(layer, traj, tf, tt, b2));
        put(o, opt.clearanceSE2TrajBatch(depth, traj, tf, {}, b2, 0.03, false));
        std::vector<uint16_t> d = layer.get();
        fwrite(d.data(), 2, d.size(), o);
        // the map changes inside a rect: the chain of updates, and the refusal while the layers are behind
        map.setCells(cells2.data());
        bool refused = false;
        try { opt.clearanceSE2TrajBatch(layer, traj, tf, tt, b2); } catch (const std::runtime_error&) { refused = true; }
        const std::array<int32_t, 4> changed{60, 90, 60, 90};
        body.update(changed);
        const ClearanceLayer::Info behind = layer.info();
        layer.update(ClearanceLayer::growRect(behind.dims, changed, body.info().R));
        d = layer.get();
        fwrite(d.data(), 2, d.size(), o);
        put(o, opt.clearanceSE2TrajBatch(layer, traj, tf, tt, b2));
        double tail[4] = {refused ? 1.0 : 0.0, (double)behind.behind, layer.info().fresh() ? 1.0 : 0.0, (double)body.writes()};
        fwrite(tail, 8, 4, o);
    }
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_matches_ctypes_bit_for_bit(tmp_path, analytic_cells):
    """C7: uneven_hip::ClearanceLayer and ALMTrajOpt::clearanceSE2TrajBatch from a compiled C++ consumer (after planSE2TrajBatch) against the ctypes binding, on the
    analytic terrain with discs tilted over it, before and after a change of the map inside a rect"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    rng = np.random.default_rng(31)
    cells = np.array(analytic_cells, dtype=np.float64).reshape(200, 200, -1, 4)
    xs = (np.arange(200) + 0.5) * 0.05 - 5.0
    near = np.zeros((200, 200), dtype=bool)
    for p in rng.uniform(-4.5, 4.5, (40, 2)):
        near |= np.hypot(xs[:, None] - p[0], xs[None, :] - p[1]) < 0.12
    cells[near, :, 2], cells[near, :, 3] = 0.8, 0.0
    cells2 = cells.copy()
    cells2[70:80, 65:85, :, 2], cells2[70:80, 65:85, :, 3] = 0.8, 0.0          # a block inside the rect the consumer names
    cells, cells2 = np.ascontiguousarray(cells.reshape(-1, 4)), np.ascontiguousarray(cells2.reshape(-1, 4))
    m = U.UnevenMap()
    m.set_cells(cells)
    ka = U.KinoAstar(m)
    S, G = scenes.random_queries(8, seed0=9900)
    B = S.shape[0]
    f0 = np.array([[0.0, 0.3, 0.5, -0.2, 0.95, 0.6][b % 6] for b in range(B)])
    f1 = np.array([[1.0, 0.6, 2.0, 0.4, 1.0, 0.5][b % 6] for b in range(B)])
    mk = dict(piece_len=0.3, mean_vel=0.5, init_time_times=1.2, yaw_piece_times=2.0, init_sig_vel=0.05, test_mode=0, test_max_vel=0.5)
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    plan = opt.plan_goals(ka, S, G, **mk)
    src_ = tmp_path / "clear.cpp"
    src_.write_text(CPP)
    exe = str(tmp_path / "clear")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src_), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2q", cells.shape[0], B))
        f.write(cells.tobytes())
        f.write(cells2.tobytes())
        f.write(np.ascontiguousarray(np.concatenate([S, G, f0[:, None], f1[:, None]], axis=1), dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    n = int(np.frombuffer(raw[:8], dtype=np.float64)[0])
    live = [b for b in range(B) if plan[b]["status"] == 0 and plan[b]["ret"] != 4]
    want_tr = [plan[b]["traj_of"] for b in live]
    assert n == len(want_tr) >= 3
    at = 8
    q = np.frombuffer(raw[at:at + 32 * n], dtype=np.float64).reshape(n, 4)
    at += 32 * n
    assert q[:, 0].astype(int).tolist() == want_tr
    b2 = q[:, 3].astype(np.int32)
    cells_of = lambda below: (below / 0.05) * (below / 0.05)        # ceil((below / res)^2) in doubles: 0.1 * 3 is a little over 0.3, and 37 is its answer
    assert b2.tolist() == [int(np.ceil(cells_of(0.1 * float(b % 4)))) for b in live] and set(b2.tolist()) <= {0, 4, 16, 37}

    def rows():
        nonlocal at
        r = np.frombuffer(raw[at:at + 88 * n], dtype=np.float64).reshape(n, 11)
        at += 88 * n
        return dict(min_d2=r[:, 0], min_t=r[:, 1], min_cell=r[:, 2:5], first_t=r[:, 5], last_t=r[:, 6], counts=r[:, 7:11])

    def field():
        nonlocal at
        d = np.frombuffer(raw[at:at + 2 * m.ncell], dtype=np.uint16)
        at += 2 * m.ncell
        return d

    car = U.BodyLayer(m, CAR)
    layer, depth = U.ClearanceLayer(car, 20), U.ClearanceLayer(car, 9, CLEAR_TO_FREE)
    _eq(rows(), opt.clearance(layer, want_tr, below2=b2, t_from=q[:, 1], t_to=q[:, 2]), "adapter")
    _eq(rows(), opt.clearance(depth, want_tr, below2=b2, t_from=q[:, 1], t_to=None, dt=0.03, with_end=False), "adapter, depth")
    assert np.array_equal(field(), layer.get().ravel())
    m.set_cells(cells2)
    car.update((60, 90, 60, 90))
    layer.update(grow_rect((200, 200), (60, 90, 60, 90), car.info()["R"]))
    assert np.array_equal(field(), layer.get().ravel()) and np.array_equal(layer.get(), U.ClearanceLayer(U.BodyLayer(m, CAR), 20).get())
    _eq(rows(), opt.clearance(layer, want_tr, below2=b2, t_from=q[:, 1], t_to=q[:, 2]), "adapter, after the update")
    assert np.frombuffer(raw[at:at + 32], dtype=np.float64).tolist() == [1.0, 1.0, 1.0, float(car.writes())] and at + 32 == len(raw)
