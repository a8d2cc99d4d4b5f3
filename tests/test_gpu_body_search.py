"""GPU tier of the body-aware search (uph_kino_set_body_layer, the BODY instantiations of uph_kino_kernel): the front-end search reading a body layer where it
reads occ_r2 by default.

S1: the reads are the reference's -- with a layer that is occ_r2 in every slice (the all-zero shape), and with a layer set to a disc dilation D of occ_r2 against
    the oracle given D as its occ_r2, the search is the oracle's expansion for expansion, at both sine settings and in both layouts of an expansion.
S2: the layer's yaw matters -- a wall with a gap that admits the long thin car lengthwise only; and a layer set by hand that admits a band of headings in a slab.
S3: the chain the feature exists for -- a disc beside a solved path, the layer updated from the changed rect, the re-plan searched in body mode.
S4: set_body_layer(None) restores the default results; batch order and batch size do not show."""
import math

import numpy as np
import pytest

from test_gpu_replan import _hill_map, _queries, _source
from test_gpu_separation import _totals, _valid
from uneven_planner_amd.alm_traj_opt import footprint_cover, footprint_grid
from uneven_planner_amd.body_layer import FOOT_OCC_XY

pytestmark = pytest.mark.gpu
CAR = (0.45, 0.15, 0.3)
THIN = (0.45, 0.15, 0.1)
INF = float("inf")


def _same(dev, orc, tag=""):
    """tests/test_gpu_kino.py's bar: status, counters and the whole expansion sequence integer-exact, poses to 1e-9"""
    assert dev["status"] == orc["status"], (tag, dev["status"], orc["status"])
    assert dev["iter_num"] == orc["iter_num"] and dev["use_node_num"] == orc["use_node_num"], (tag, dev["iter_num"], orc["iter_num"], dev["use_node_num"], orc["use_node_num"])
    if "expanded" in dev:
        k = min(len(dev["expanded"]), len(orc["expanded"]))
        assert k == orc["n_expanded"] or k == len(dev["expanded"])
        neq = np.nonzero((dev["expanded"][:k] != orc["expanded"][:k]).any(axis=1))[0]
        assert neq.size == 0, "%s: expansion sequences part at step %d of %d" % (tag, neq[0], k)
    assert dev["n_path"] == orc["n_path"], (tag, dev["n_path"], orc["n_path"])
    if orc["n_path"]:
        assert np.abs(dev["path"] - orc["path"][:len(dev["path"])]).max() < 1e-9, tag


def _identical(a, b):
    return (a["status"] == b["status"] and a["iter_num"] == b["iter_num"] and a["use_node_num"] == b["use_node_num"] and a["n_path"] == b["n_path"]
            and np.array_equal(a["path"], b["path"]) and ("expanded" not in a or np.array_equal(a["expanded"], b["expanded"])))


def _dilate(occ2, r):
    """occ2 [nx][ny] dilated by the disc of r columns"""
    nx, ny = occ2.shape
    pad = np.zeros((nx + 2 * r, ny + 2 * r), dtype=bool)
    pad[r:r + nx, r:r + ny] = occ2 != 0
    out = np.zeros((nx, ny), dtype=bool)
    for a in range(-r, r + 1):
        for b in range(-r, r + 1):
            if a * a + b * b <= r * r:
                out |= pad[r + a:r + a + nx, r + b:r + b + ny]
    return out.astype(np.int8)


def _layer_read(m, layer_bytes, poses):
    """kOcc's own statements on a layer [nx][ny][nyaw]: -1 outside, else the byte"""
    nx, ny, nyaw = layer_bytes.shape
    p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    xy_inv, yaw_inv = 1.0 / m.xy_resolution, 1.0 / m.yaw_resolution
    ix = np.floor((p[:, 0] - m.map_origin[0]) * xy_inv).astype(np.int64)
    iy = np.floor((p[:, 1] - m.map_origin[1]) * xy_inv).astype(np.int64)
    iw = np.floor((p[:, 2] - m.map_origin[2]) * yaw_inv).astype(np.int64)
    out_ = (ix < 0) | (iy < 0) | (iw < 0) | (ix > nx - 1) | (iy > ny - 1) | (iw > nyaw - 1)
    got = layer_bytes[np.clip(ix, 0, nx - 1), np.clip(iy, 0, ny - 1), np.clip(iw, 0, nyaw - 1)].astype(np.int64)
    return np.where(out_, -1, got)


def _shot_start(path):
    """index of the first one-shot sample of a front_end_path: the shot's sample at l = 0 is the pose of the node it was shot from, the last pose of the node
    chain, so the path holds that pose twice in a row; nodes of a chain never repeat a pose (a repeated lattice key is a closed node)"""
    d = np.abs(path[1:] - path[:-1]).max(axis=1)
    rep = np.nonzero(d < 1e-12)[0]
    assert rep.size >= 1
    return int(rep[-1]) + 1


@pytest.fixture(scope="module")
def hill(oracle):
    """the hill map (free everywhere as built) with 40 discs of 0.12 m tilted over it"""
    from test_gpu_body_layer import _tilt_discs
    m = _hill_map()
    near = _tilt_discs(m, np.random.default_rng(21).uniform(-4.5, 4.5, (40, 2)), 0.12)
    assert near.sum() > 400 and np.array_equal(m.occ_r2_buffer.reshape(near.shape) != 0, near)
    g = oracle.OracleGrid()
    g.set_cells(m.map_buffer)
    g.set_occ(m.occ_buffer, m.occ_r2_buffer)
    return m, g


# ---- S1 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [None, dict(collision_interval=0.02)], ids=["spread", "walked"])
def test_the_reads_are_the_references(hill, oracle, params):
    import uneven_planner_amd as U
    m, g = hill
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    occ2 = m.occ_r2_buffer.reshape(nx, ny)
    S, G = _queries(m, 8, 4300)
    point = U.BodyLayer(m, (0.0, 0.0, 0.0), 0.0, FOOT_OCC_XY)
    assert np.array_equal(point.get(), np.repeat((occ2 != 0).astype(np.int8)[:, :, None], nyaw, axis=2))
    D = _dilate(occ2, 3)
    assert D.sum() > (occ2 != 0).sum() > 0
    dil = U.BodyLayer(m, (0.0, 0.0, 0.0), 0.0, FOOT_OCC_XY)
    dil.set(np.repeat(D[:, :, None], nyaw, axis=2))
    gd = oracle.OracleGrid()
    gd.set_cells(m.map_buffer)
    gd.set_occ(m.occ_buffer, D.ravel())
    want = {"point": [oracle.OracleKinoAstar(g, params).plan(s, gl) for s, gl in zip(S, G)],
            "dilated": [oracle.OracleKinoAstar(gd, params).plan(s, gl) for s, gl in zip(S, G)]}
    assert sum(w["status"] == 0 for w in want["point"]) >= 4
    assert any(not (a["status"] == b["status"] and a["iter_num"] == b["iter_num"]) for a, b in zip(want["point"], want["dilated"]))      # D changes the searches
    ka = U.KinoAstar(m, params=params)
    for wps in (2, 4, 6, 8):                       # every BODY = true instantiation of the kernel: four register budgets ...
        ka.set_wps(wps)
        for flags in (3, 1):                       # ... times sincosFast on, off (both with the dynamic hand-out)
            ka.set_flags(flags)
            for name, layer in (("point", point), ("dilated", dil)):
                ka.set_body_layer(layer)
                dev = ka.plan_batch(S, G, path_cap=1024, exp_cap=40000)
                for b in range(len(S)):
                    _same(dev[b], want[name][b], "%s wps %d flags %d query %d" % (name, wps, flags, b))
    ka.close()


# ---- S2 ---------------------------------------------------------------------------------------------------------------------------------------------------
WALL_X = (98, 102)               # columns of the wall: x in [-0.1, 0.1)
WALL_Y = (70, 130)               # it spans y in [-1.5, 1.5): it can be gone round


def _wall_map(analytic_cells, gap):
    """the analytic terrain with a wall four columns thick along y through the map's centre and a gap of `gap` columns centred at y = 0"""
    import uneven_planner_amd as U
    cells = np.array(analytic_cells, dtype=np.float64).reshape(200, 200, -1, 4)
    wall = np.zeros((200, 200), dtype=bool)
    wall[WALL_X[0]:WALL_X[1], WALL_Y[0]:WALL_Y[1]] = True
    wall[WALL_X[0]:WALL_X[1], 100 - gap // 2:100 + gap - gap // 2] = False
    cells[wall, :, 2], cells[wall, :, 3] = 0.8, 0.0
    m = U.UnevenMap()
    m.set_cells(cells.reshape(-1, 4))
    occ2 = m.occ_r2_buffer.reshape(200, 200) != 0
    assert np.array_equal(occ2[90:110, 60:140], wall[90:110, 60:140])
    return m


def _crossings(path):
    """y where the path's polyline crosses x = 0"""
    x, y = path[:, 0], path[:, 1]
    k = np.nonzero((x[:-1] < 0.0) != (x[1:] < 0.0))[0]
    t = x[k] / (x[k] - x[k + 1])
    return y[k] + t * (y[k + 1] - y[k])


S2_S = np.array([[-2.0, 0.0, 0.0], [-2.0, 0.4, 0.0], [-1.5, -0.5, 0.3], [-2.5, 0.1, -0.2]])
S2_G = np.array([[2.0, 0.0, 0.0], [2.0, -0.3, 0.0], [1.5, 0.4, 0.0], [2.5, 0.0, 0.2]])


def test_a_gap_the_body_fits_lengthwise_only(analytic_cells):
    """S2 (a) and (c): the gap (0.5 m) is wider than the inflated width and narrower than the inflated length"""
    import uneven_planner_amd as U
    m = _wall_map(analytic_cells, 10)
    layer = U.BodyLayer(m, THIN)
    hl, w = 0.3 + layer.margin, 0.1 + layer.margin
    assert 2.0 * w < 0.5 < 2.0 * hl
    bytes_ = layer.get()
    nyaw = bytes_.shape[2]
    psi = m.map_origin[2] + (np.arange(nyaw) + 0.5) * m.yaw_resolution
    off_axis = lambda w: np.minimum(np.abs(w), np.abs(np.pi - np.abs(w)))          # angle between a heading in [-pi, pi] and the gap's axis (the x axis)
    gap_cells = bytes_[WALL_X[0]:WALL_X[1], 95:105]
    assert (gap_cells[:, :, int(np.argmin(np.abs(psi)))] == 0).any() and gap_cells[:, :, int(np.argmin(np.abs(psi - np.pi / 2)))].all()      # lengthwise only
    ka = U.KinoAstar(m)
    ka.set_body_layer(layer)
    res = ka.plan_batch(S2_S, S2_G)
    n_end_in, bounds = 0, []
    for b, r in enumerate(res):
        assert r["status"] == 0, (b, r["status"])
        path = r["path"]
        k = _shot_start(path)
        assert (_layer_read(m, bytes_, path[k:]) == 0).all(), b
        yc = _crossings(path)
        assert yc.size == 1 and abs(yc[0]) < 0.25, (b, yc)                 # through the gap, once
        # a path pose is at most collision_interval / 2 = 0.03 m of arc past a pose the search sampled (the samples of a 0.15 m primitive lie at 0.06 and 0.12 m,
        # of a 0.075 m one at 0.06 m; a shot sample is sampled itself): that pose lies within one column of it in x and in y, read 0 there, and its yaw differs
        # by at most 0.03 tan(max_steer) / wheel_base = 0.063 rad.  So the pose's heading is within half a bin + 0.063 rad of a bin that is free in one of the
        # 3 x 3 columns around it.  Inside the wall's columns that admits headings along the gap only.
        inside = np.nonzero((path[:, 0] >= -0.1) & (path[:, 0] < 0.1))[0]
        assert inside.size >= 1
        for i in inside:
            ix, iy = int(np.floor((path[i, 0] + 5.0) / 0.05)), int(np.floor((path[i, 1] + 5.0) / 0.05))
            fb = ~bytes_[ix - 1:ix + 2, iy - 1:iy + 2].astype(bool).all(axis=(0, 1))
            assert fb.any(), (b, i)
            bound = off_axis(psi[fb]).max() + 0.5 * m.yaw_resolution + 0.03 * math.tan(0.5) / 0.26
            assert off_axis(path[i, 2]) <= bound, (b, i, path[i], bound)
            bounds.append(bound)
        n_end_in += int((_layer_read(m, bytes_, path[:k]) == 1).sum())
    print("S2a: %d node poses (end states, which the reference never samples) read 1 in the layer; %d poses inside the wall's columns, heading bounds %.3f .. %.3f rad"
          % (n_end_in, len(bounds), min(bounds), max(bounds)))
    # (c) the same bytes with the slices rolled by a quarter turn: the gap now admits the car sideways only, and the answers change
    layer.set(np.roll(bytes_, nyaw // 4, axis=2))
    rolled = ka.plan_batch(S2_S, S2_G)
    for b, (r, q) in enumerate(zip(res, rolled)):
        assert not _identical(r, q), b
    print("S2c: rolled layer statuses %s, crossings of x = 0 at y = %s" % ([q["status"] for q in rolled],
                                                                        [np.round(_crossings(q["path"]), 2).tolist() if q["status"] == 0 else None for q in rolled]))
    ka.close()


def test_a_gap_narrower_than_the_body(analytic_cells):
    """S2 (b): a 0.2 m gap.  The default search passes through it; the body-mode search goes round the wall's end or fails, and never crosses inside the gap"""
    import uneven_planner_amd as U
    m = _wall_map(analytic_cells, 4)
    layer = U.BodyLayer(m, THIN)
    assert 2.0 * (0.1 + layer.margin) > 0.2
    ka = U.KinoAstar(m)
    S, G = S2_S[:2], S2_G[:2]
    for r in ka.plan_batch(S, G):
        yc = _crossings(r["path"])
        assert r["status"] == 0 and yc.size == 1 and abs(yc[0]) < 0.1, (r["status"], yc)
    ka.set_body_layer(layer)
    body = ka.plan_batch(S, G)
    for r in body:
        assert r["status"] in (0, 3, 4), r["status"]
        if r["status"] == 0:
            yc = _crossings(r["path"])
            assert yc.size >= 1 and (np.abs(yc) > 1.5).all(), yc
            p = r["path"]
            assert not ((np.abs(p[:, 0]) < 0.1) & (np.abs(p[:, 1]) < 1.5)).any()
    print("S2b: body-mode statuses %s" % [r["status"] for r in body])
    ka.close()


def test_a_slab_that_admits_a_band_of_headings(analytic_cells):
    """S2 (d): the wall's own bound on the heading is loose (a four-column wall lets the thin car stand diagonally in the gap), so the yaw index of the read is
    held on a layer set by hand: in the slab |x| < 0.5 m every cell is 1 except in the yaw bins whose centre is within 0.3 rad of the x axis (either way round),
    everything else is free.  A sampled pose in the slab then has its yaw bin in that band, exactly; a node pose at least 0.05 m inside the slab lies at most 0.03 m
    of arc past a sampled pose (which is in the slab too), so within half a bin + 0.03 tan(max_steer) / wheel_base = 0.063 rad of the band.  A search that read
    a neighbouring slice, or the slices in another order, would let other headings in or find no way across."""
    import uneven_planner_amd as U
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    assert not m.occ_r2_buffer.reshape(200, 200)[80:120].any()
    layer = U.BodyLayer(m, (0.0, 0.0, 0.0), 0.0, FOOT_OCC_XY)
    nx, ny, nyaw = layer.dims
    psi = m.map_origin[2] + (np.arange(nyaw) + 0.5) * m.yaw_resolution
    off_axis = lambda w: np.minimum(np.abs(w), np.abs(np.pi - np.abs(w)))
    band = off_axis(psi) <= 0.3
    assert 8 <= band.sum() <= 14
    mine = np.zeros((nx, ny, nyaw), dtype=np.int8)
    mine[90:110, :, :] = (~band).astype(np.int8)[None, None, :]              # columns 90 .. 109: x in [-0.5, 0.5)
    layer.set(mine)
    ka = U.KinoAstar(m)
    S = np.array([[-2.0, 0.0, 0.0], [-2.0, 0.5, 0.0], [-2.2, -0.6, 0.4], [2.0, 0.3, 3.0]])
    G = np.array([[2.0, 0.0, 0.0], [2.0, -0.2, 0.0], [2.0, 0.2, 0.0], [-2.0, -0.2, 3.1]])
    free = ka.plan_batch(S, G)
    ka.set_body_layer(layer)
    slack = 0.5 * m.yaw_resolution + 0.03 * math.tan(0.5) / 0.26

    def hold(res, bins, tag):
        """every one-shot sample reads 0; every pose deep in the slab heads within `slack` of the centre of a bin that is free there"""
        centres = psi[bins]
        n_in, worst = 0, 0.0
        for b, r in enumerate(res):
            if r["status"] != 0:
                continue
            path = r["path"]
            assert (_layer_read(m, layer.get(), path[_shot_start(path):]) == 0).all(), (tag, b)
            deep = np.abs(path[:, 0]) <= 0.45
            assert deep.sum() >= 4, (tag, b)                                  # 0.9 m of path at 0.15 m or less between poses
            d = np.abs(path[deep, 2][:, None] - centres[None, :])
            d = np.minimum(d, 2.0 * np.pi - d).min(axis=1)
            assert (d <= slack).all(), (tag, b, path[deep, 2], d.max())
            n_in, worst = n_in + int(deep.sum()), max(worst, float(d.max()))
        return n_in, worst

    res = ka.plan_batch(S, G)
    assert [r["status"] for r in res] == [0] * 4 and [r["status"] for r in free] == [0] * 4
    assert all(_crossings(r["path"]).size == 1 for r in res)
    n_in, worst = hold(res, band, "band")
    assert n_in >= 16 and (off_axis(np.concatenate([r["path"][np.abs(r["path"][:, 0]) <= 0.45, 2] for r in res])) <= 0.3 + slack).all()
    # the same bytes a quarter turn round (16 bins): the slab now admits headings around +-pi / 2 only, and the answers change
    layer.set(np.roll(mine, nyaw // 4, axis=2))
    rolled = ka.plan_batch(S, G)
    assert all(not _identical(a, b) for a, b in zip(res, rolled))
    n_roll, worst_roll = hold(rolled, np.roll(band, nyaw // 4), "rolled")
    print("S2d: %d poses deep in the slab, at most %.3f rad from a free bin's centre (slack %.3f); rolled: statuses %s, %d poses, %.3f rad"
          % (n_in, worst, slack, [r["status"] for r in rolled], n_roll, worst_roll))
    ka.close()


# ---- S3 ---------------------------------------------------------------------------------------------------------------------------------------------------
S3_BACK = (0.5, 1.0, 1.5, 2.0, 3.0)          # seconds before footprint_check's first_t at which the victim is re-planned


def test_replan_after_a_footprint_hit_is_searched_where_the_body_fits():
    """tests/test_gpu_footprint_check.py's C3 scene: a disc of 0.1 m tilted 0.2 m beside a solved path, the car of half width 0.3.  The layer is updated from
    the changed rect and the victim re-planned from before footprint_check's first_t, with the default search and with the layer set.

    Asserted on the search's output, for every path either mode returns: a one-shot sample that reads 0 in the layer covers, by footprint_cover at margin 0, no
    surely-occupied column and none outside the grid (the margin theorem); every one-shot sample of a body-mode path reads 0.

    From 0.5 s before first_t the body-mode search has NO path (status 3, observed on 1x MI355X): the disc reaches 0.1 m into the car's swept width, 0.5 s are
    0.25 m, the search drives forward only and its tightest arc (wheel_base / tan(max_steer) = 0.476 m) moves the body 0.06 m sideways in that distance.  The
    default search does return a path from there -- one whose one-shot samples touch the disc (15 of 61 read 1 in the layer, 24 touch by footprint_cover).  So the
    same re-plan is made from 1, 1.5, 2 and 3 s before as well, where the car has the 0.4 m its tightest arc needs to move 0.16 m sideways: body mode must find
    a path from every one of the four, with no one-shot sample reading 1 or touching.
    footprint_check of the re-solved trajectories is printed, not asserted: the optimiser still moves the path with point terms."""
    import uneven_planner_amd as U
    from test_gpu_footprint_check import _beside, _tilt_discs
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    goal_of = np.nonzero(src.last_plan["traj_of"] >= 0)[0]
    ok = np.array([j for j in _valid(res) if res[j]["ret"] == 0], dtype=np.int32)
    total = _totals(src)
    before = src.footprint_check(ok, CAR, 0.05)
    clean = np.nonzero((before["counts"][:, 1] == 0) & (src.check(ok, limits=np.full(7, INF))["counts"][:, 2] == 0))[0]
    layer = U.BodyLayer(m, CAR)
    # the victim: the first clean trajectory whose own query has a body-mode path before the disc exists (its goal is not inside the band along the border)
    ka.set_body_layer(layer)
    pre = ka.plan_batch(S[goal_of[ok[clean]]], G[goal_of[ok[clean]]], path_cap=64, complete=False)
    ka.set_body_layer(None)
    fits = [q for q, r in zip(clean, pre) if r["status"] == 0]
    assert len(fits) >= 1
    v = int(fits[0])
    nx, ny, nyaw = (int(x) for x in m.voxel_num)
    occ_before = m.occ_r2_buffer.reshape(nx, ny).copy()
    mid = src.traj_states([ok[v]], [0.5 * total[ok[v]]])[0]
    _tilt_discs(m, [_beside(mid, 0.2)], 0.1)
    occ2 = m.occ_r2_buffer.reshape(nx, ny)
    ch = np.argwhere(occ2 != occ_before)
    assert len(ch) >= 8 and layer.info()["behind"] == 1
    rect = (int(ch[:, 0].min()), int(ch[:, 0].max()) + 1, int(ch[:, 1].min()), int(ch[:, 1].max()) + 1)
    layer.update(rect)
    bytes_ = layer.get()
    assert np.array_equal(bytes_, U.BodyLayer(m, CAR).get())
    after = src.footprint_check(ok[[v]], CAR, 0.05)
    assert after["counts"][0, 1] > 0
    t_sw = np.maximum(after["first_t"][0] - np.array(S3_BACK), 0.0)
    K = len(t_sw)
    goal = G[goal_of[ok[v]]]
    sw = src.traj_states(np.full(K, ok[v]), t_sw)
    starts = np.stack([sw[:, 0], sw[:, 1], sw[:, 6]], axis=1)
    grid = footprint_grid(m)
    status = {}
    for mode in ("default", "body"):
        ka.set_body_layer(layer if mode == "body" else None)
        found = ka.plan_batch(starts, np.repeat(goal[None, :], K, axis=0))
        status[mode] = [r["status"] for r in found]
        dst = U.ALMTrajOpt(m)
        dst.set_rho(1.0)
        out = dst.replan_goals(ka, src, np.full(K, ok[v]), t_sw)
        for k, r in enumerate(found):
            line = "search status %d" % r["status"]
            if r["status"] == 0:
                shot = r["path"][_shot_start(r["path"]):]
                reads = _layer_read(m, bytes_, shot)
                cv = footprint_cover(shot, shot[:, 2], CAR, 0.0, grid)
                sure = cv["g"] < -1e-9
                inside = (cv["ix"] >= 0) & (cv["ix"] < nx) & (cv["iy"] >= 0) & (cv["iy"] < ny)
                bad = sure & (~inside | (occ2[np.clip(cv["ix"], 0, nx - 1), np.clip(cv["iy"], 0, ny - 1)] != 0))
                own = np.floor((shot[:, :2] - m.map_origin[:2]) * (1.0 / m.xy_resolution)).astype(np.int64)      # the pose's own column, which the footprint rule covers too
                touching = bad.any(axis=1) | (occ2[np.clip(own[:, 0], 0, nx - 1), np.clip(own[:, 1], 0, ny - 1)] != 0)
                assert not (touching & (reads == 0)).any(), (mode, k)                 # the margin theorem
                if mode == "body":
                    assert (reads == 0).all() and not touching.any(), k
                line += ", %d poses, %d one-shot samples, %d read 1 in the layer, %d touch by footprint_cover" % (r["n_path"], len(shot), int((reads == 1).sum()),
                                                                                                               int(touching.sum()))
            if out[k]["status"] == 0 and out[k]["ret"] != 4:
                again = dst.footprint_check([out[k]["traj_of"]], CAR, 0.05)
                line += "; re-solved: ret %d, %d of %d samples hit, first at %s" % (out[k]["ret"], again["counts"][0, 1], again["counts"][0, 0], again["first_t"][0])
            print("S3 %s, %.1f s before first_t (t = %.2f s): %s" % (mode, S3_BACK[k], t_sw[k], line))
    assert status["default"][0] == 0                                  # the point search does not see the problem
    # from 1 s (0.5 m) and more before the first touch the forward-only car has room: 0.16 m sideways take 0.4 m on its tightest arc (0.476 (1 - cos(0.4 / 0.476)))
    assert status["body"][1:] == [0] * (len(S3_BACK) - 1), status["body"]
    print("S3: body-mode statuses by seconds before first_t %s: %s; default: %s" % (list(S3_BACK), status["body"], status["default"]))
    ka.close()


# ---- S4 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_none_restores_the_default_and_the_batch_does_not_show(hill):
    import uneven_planner_amd as U
    m, _ = hill
    S, G = _queries(m, 12, 4400)
    ka = U.KinoAstar(m)
    base = ka.plan_batch(S, G, exp_cap=40000)
    layer = U.BodyLayer(m, CAR)
    ka.set_body_layer(layer)
    body = ka.plan_batch(S, G, exp_cap=40000)
    assert any(not _identical(a, b) for a, b in zip(base, body))
    print("S4: default statuses %s, body statuses %s" % ([r["status"] for r in base], [r["status"] for r in body]))
    perm = np.random.default_rng(3).permutation(len(S))
    shuffled = ka.plan_batch(S[perm], G[perm], exp_cap=40000)
    for j, b in enumerate(perm):
        assert _identical(shuffled[j], body[b]), b
    for b in (0, 5, 11):
        assert _identical(ka.plan_batch(S[[b]], G[[b]], exp_cap=40000)[0], body[b]), b
    ka.set_body_layer(None)
    again = ka.plan_batch(S, G, exp_cap=40000)
    for a, b in zip(base, again):
        assert _identical(a, b)
    ka.close()
    layer.close()
