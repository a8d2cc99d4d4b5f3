"""Every grid-reading kernel on non-square grids and with yaw bin counts other than 64 (tests/grid_cases.py), against the oracle (run with
-m gpu on an MI355X; everything goes through the C-ABI).

The rest of the suite runs on square grids with 64 yaw bins, where a transposed nx / ny in an address and a yaw loop that assumes one trip of
a full wave are invisible.  Here: wide 120 x 70 x 64, tall 42 x 76 x 38 (sizes that are no multiple of the resolution, 26 idle lanes, 42 rows
over four slabs), fine 60 x 80 x 127 (a second trip of 63 lanes), one_over 70 x 40 x 65 (a second trip of one lane) and far 384 x 96 x 38
(local frames on a non-square grid).  tests/test_grids_cpu.py holds the code shared with the host to the oracle on the same grids, so a
failure here points at device-only code: the map build and update, the search, the C-ABI's grid set-up, the rollout and the check.

Every bar is the one the project already uses for the same quantity on the square grid (named at each assertion).  The worst error per
grid is kept in grid_cases.MEASURED; tools/grid_sweep_report.py runs this file and writes them to profiles/grid_sweep.txt.
"""
import math
import os
import re

import numpy as np
import pytest

import grid_cases as GC
import piece_sweep as PS
from conftest import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST, TR, PO = 1, 2, 4
AUTO, FORCED = (0, 0), (128, 2)
_vid = lambda v: "auto" if v == AUTO else "%dx%d" % v
_MAPS, _EVAL, _CLOUDS = {}, {}, {}


def _new_map(name, storage="f64", tile=None, **extra):
    import uneven_planner_amd as U
    m = U.UnevenMap(GC.map_params(name, **extra), storage=storage, tile=tile)
    GC.check_dims(name, m.voxel_num)
    return m


def _analytic(name, storage="f64"):
    """the device map holding the grid's analytic cells (once per module; read only) and the oracle's grid on the cells the map holds"""
    key = (name, storage)
    if key not in _MAPS:
        from oracle import oracle_py as O
        m = _new_map(name, storage).set_cells(GC.cells(name))
        og = GC.oracle_grid(O, name, m.map_buffer)
        GC.check_dims(name, og.dims)
        _MAPS[key] = (m, og)
    return _MAPS[key]


def _ctx(m, variant, params=None):
    import uneven_planner_amd as U
    opt = U.ALMTrajOpt(m, params=params)
    if variant != AUTO:
        opt.set_lanes(variant[0])
        opt.set_wps(variant[1])
    return opt


# ---- 1. lookups and front-end queries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.SMALL)
def test_lookups_match_the_oracle(oracle, name):
    """getAllWithGrad at test_terrain_lookup_matches_oracle's 1e-12 and getTerrainPosBatch at 1e-15 (the rollout sweep's bar for poses; heights below 2 m,
    unit vectors: a few last bits) on 5 000 poses up to 0.2 m outside every border plus the corners, the last row and column, the yaw seam and the overhanging strip.
    Coverage, from the positions alone: the corners read x index 0 and nx - 1, y index 0 and ny - 1, and every yaw bin a lookup can reach as
    its lower corner, every bin but the first as its upper one (one_over: bin 64 starts above pi, so it is only ever the upper corner)"""
    m, og = _analytic(name)
    nx, ny, nyaw = GC.DIMS[name]
    pos = GC.lookup_points(name)
    v0, g0 = og.all_with_grad(pos)
    v1, g1 = m.getAllWithGrad(pos)
    e = dict(values=np.abs(v0 - v1).max(), grads=np.abs(g0 - g1).max() / np.abs(g0).max())
    inmap = np.array([m.host.isInMap(p) for p in pos])
    vx, vy = GC.visited_xy(name, pos[inmap])
    _, _, w0, w1 = GC.lookup_corners(name, pos[inmap])
    lo, hi = GC.reachable_yaw_bins(name)
    assert {0, nx - 1} <= vx and {0, ny - 1} <= vy and 0.5 < inmap.mean() < 1.0
    assert lo == 0 and hi >= nyaw - 2 and set(w0.tolist()) == set(range(hi + 1)) and set(w1.tolist()) >= set(range(1, nyaw))
    assert (hi == nyaw - 1) == (name != "one_over") and ((0 in set(w1.tolist())) == (name != "one_over"))
    R, p = m.getTerrainPosBatch(pos)
    t = og.terrain(pos)
    zb = np.column_stack([t[:, 2], t[:, 3], np.sqrt(1.0 - t[:, 2] ** 2 - t[:, 3] ** 2)])
    xyaw = np.column_stack([np.cos(pos[:, 2]), np.sin(pos[:, 2]), np.zeros(len(pos))])
    yb = np.cross(zb, xyaw)
    yb /= np.linalg.norm(yb, axis=1)[:, None]
    xb = np.cross(yb, zb)
    e.update(pose_R=max(np.abs(R[:, :, 2] - zb).max(), np.abs(R[:, :, 1] - yb).max(), np.abs(R[:, :, 0] - xb).max()), pose_z=np.abs(p[:, 2] - t[:, 0]).max())
    print(name, GC.record("1_lookups", name, e))
    assert e["values"] < 1e-12 and e["grads"] < 1e-12 and e["pose_R"] < 1e-15 and e["pose_z"] < 1e-15, e
    assert np.array_equal(p[:, :2], pos[:, :2])


def _doctored(name):
    """the analytic cells with two occupied blocks: one occupied in every yaw bin (sigma above max_rho), one only in the last ceil(nyaw / 4) bins
    (|zb| large: c below min_cnormal there) -- on fine and one_over these include bins >= 64, the second trip of the commit kernels' yaw loop"""
    nx, ny, nyaw = GC.DIMS[name]
    c = np.array(GC.cells(name)).reshape(nx, ny, nyaw, 4)
    k = -(-nyaw // 4)
    a = (slice(nx // 6, nx // 6 + nx // 5), slice(ny // 2, ny // 2 + ny // 4))
    b = (slice(nx - nx // 4, nx - 1), slice(1, ny // 3))
    c[a[0], a[1], :, 1] = 0.2
    c[b[0], b[1], nyaw - k:, 2] = 0.7
    return c.reshape(-1, 4), a, b, k


@pytest.mark.parametrize("name", GC.SMALL)
def test_frontend_queries_and_occupancy_match_the_oracle(oracle, name):
    """uph_frontend_query and both occupancy layers as the device commits them against the oracle's compute_occ on the same cells
    (test_frontend_queries_match_the_oracle_and_the_host_mirror: occupancy equal, sigma at 1e-12), on a grid with a block occupied in every
    yaw bin and one occupied only in the last quarter of the bins"""
    nx, ny, nyaw = GC.DIMS[name]
    cells, a, b, k = _doctored(name)
    m = _new_map(name).set_cells(cells)
    og = GC.oracle_grid(oracle, name, m.map_buffer)
    og.compute_occ(min_cnormal=0.8, max_rho=0.05)
    occ_o, occ2_o = og.get_occ()
    assert np.array_equal(m.occ_buffer.astype(np.int8), occ_o) and np.array_equal(m.occ_r2_buffer.astype(np.int8), occ2_o)
    occ3 = occ_o.reshape(nx, ny, nyaw)
    assert occ3[a[0], a[1]].all() and occ3[b[0], b[1], nyaw - k:].all() and not occ3[b[0], b[1], :nyaw - k].any()
    assert occ2_o.reshape(nx, ny)[b[0], b[1]].all() and (name not in ("fine", "one_over") or nyaw - 1 >= 64)
    pos = GC.frontend_points(name)
    # inside the two blocks, the second one in its occupied and in its free bins
    ox, oy, ow = GC.origin(name)
    res, yres = GC.GRIDS[name]["xy_res"], GC.GRIDS[name]["yaw_res"]
    cen = lambda s, o: o + (0.5 * (s.start + s.stop)) * res
    pos[100:104] = [[cen(a[0], ox), cen(a[1], oy), 0.5], [cen(b[0], ox), cen(b[1], oy), ow + (nyaw - 0.5) * yres],
                    [cen(b[0], ox), cen(b[1], oy), ow + (nyaw - k + 0.5) * yres], [cen(b[0], ox), cen(b[1], oy), ow + (nyaw - k - 0.5) * yres]]
    sg, oc, oxy = m.frontend_query(pos)
    sg_o, oc_o, oxy_o = og.frontend_query(pos)
    assert np.array_equal(oc, oc_o) and np.array_equal(oxy, oxy_o)
    assert list(oc[100:104]) == [1, 1, 1, 0] and list(oxy[100:104]) == [1, 1, 1, 1]
    ix, iy, iw = GC.cell_index(name, pos[oc >= 0])
    assert {0, nx - 1} <= set(ix.tolist()) and {0, ny - 1} <= set(iy.tolist()) and set(iw.tolist()) == set(range(nyaw))
    e = dict(sigma=np.abs(sg - sg_o).max())
    print(name, GC.record("1_frontend", name, e))
    assert e["sigma"] < 1e-12
    assert (oc == 1).sum() > 50 and (oxy == 1).sum() > (oc == 1).sum() and (oc == -1).sum() > 0 and (oc == 0).sum() > 0
    for i in range(0, len(pos), 7):
        assert oc[i] == m.isOccupancy(pos[i]) and oxy[i] == m.isOccupancyXY(pos[i])


# ---- 2. fp32 storage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tall", "fine"])
def test_f32_storage_is_the_rounded_grid(oracle, name):
    """test_gpu_km2::test_f32_storage_is_the_rounded_f64_grid and ::test_f32_lookups_...: map_buffer of an fp32 map is the float-rounded grid,
    windows of it too, and the lookups equal the oracle's on the rounded cells (values 1e-12, gradients 1e-10)"""
    nx, ny, nyaw = GC.DIMS[name]
    m32, og = _analytic(name, "f32")
    rounded = np.asarray(GC.cells(name)).astype(np.float32).astype(np.float64)
    assert np.array_equal(m32.map_buffer, rounded) and m32.L.uph_map_storage_bytes(m32.h) == 4
    assert np.array_equal(m32.get_window(nx - 9, nx, 3, ny), rounded.reshape(nx, ny, nyaw, 4)[nx - 9:nx, 3:ny])
    pos = GC.lookup_points(name, n=4000, seed=12)
    v, g = m32.getAllWithGrad(pos)
    vo, go = og.all_with_grad(pos)
    e = dict(values=np.abs(v - vo).max(), grads=np.abs(g - go).max())
    print(name, GC.record("2_f32_lookups", name, e))
    assert e["values"] < 1e-12 and e["grads"] < 1e-10, e
    assert np.abs(rounded - GC.cells(name)).max() > 1e-9


# ---- 3. the plane-fit build ---------------------------------------------------------------------------------------------------------------------
def cliff_height(x, y):
    """the hill with a ramp of 0.6 m along the line y = 0.4 x + 0.1 (slope 1.5: c = 0.55 < min_cnormal, so the cells on it are occupied; the ramp
    is gentle enough for every ellipsoid on it to hold a full-rank set of points: the oracle's build has no degenerate cell there)"""
    from uneven_planner_amd import scenes
    return scenes.hill_height(x, y) + 0.3 * np.tanh((y - 0.4 * x - 0.1) / 0.2)


def _cloud(kind):
    """make_hill_cloud(n_side = 190, half = 3.6): the default cloud's point spacing (12 / 316 m), covering all four grids"""
    if kind not in _CLOUDS:
        from uneven_planner_amd import scenes
        hill = scenes.make_hill_cloud(n_side=190, half=3.6)
        _CLOUDS.update(hill=hill, cliff=scenes.make_hill_cloud(n_side=190, half=3.6, height=cliff_height), half=hill[hill[:, 0] < 0.0].copy())
    return _CLOUDS[kind]


def _slabs(name):
    """tall and one_over are built whole; wide and fine on the first two rows, four rows in the middle and the last two"""
    nx = GC.DIMS[name][0]
    return [(0, nx)] if name in ("tall", "one_over") else [(0, 2), (nx // 2 - 2, nx // 2 + 2), (nx - 2, nx)]


def _build_against_oracle(oracle, name, kind, degenerate_rule=False):
    nx, ny, nyaw = GC.DIMS[name]
    xyz = _cloud(kind)
    prm = GC.map_params(name)
    g = oracle.OracleGrid(**GC.GRIDS[name])
    GC.check_dims(name, g.dims)
    b = oracle.OracleMapBuilder(xyz=xyz)
    n = np.zeros(6)                                            # cells, off, compared (non-degenerate), off among them, occupancy differs among them, occupancy differs
    med, counts = [], dict(occupied_cells=0.0, empty_cells=0.0)
    for (x0, x1) in _slabs(name):
        m = _new_map(name)                                    # a fresh map per slab: everything outside the slab must stay untouched
        m.build(xyz, x0=x0, x1=x1)
        assert m.build_stats()["cell_iters"] == (x1 - x0) * ny * nyaw * int(m.params["iter_num"]) and m.params["iter_num"] == 2
        b.construct(g, map_params=prm, x0=x0, x1=x1)
        co, _ = g.get_cells()
        sl = slice(x0 * ny * nyaw, x1 * ny * nyaw)
        dev, orc = m.map_buffer[sl], co[sl]
        d = np.abs(dev - orc).max(axis=1)
        occ_o, _ = g.get_occ()
        keep = np.ones(len(d), dtype=bool)
        if degenerate_rule:
            # test_map_build_edge_and_empty_cells: at the cloud's border a fit sees one to three points, the covariance is rank deficient and its
            # "smallest" eigenvector arbitrary (in the reference as well); those cells are left out of the strict comparison
            keep = ~((np.abs(dev[:, 1]) < 1e-12) | (np.abs(orc[:, 1]) < 1e-12) | (dev[:, 1] == 1.0) | (orc[:, 1] == 1.0))
        dis = m.occ_buffer[sl] != occ_o[sl]
        n += [len(d), (d > 1e-9).sum(), keep.sum(), (d[keep] > 1e-9).sum(), dis[keep].sum(), dis.sum()]
        med.append(np.median(np.abs(dev[:, 0] - orc[:, 0])) if degenerate_rule else np.median(d))
        out = np.ones(nx * ny * nyaw, dtype=bool)
        out[sl] = False
        assert np.all(m.map_buffer[out] == 0.0) and np.all(m.c_buffer[out] == 1.0) and not m.occ_buffer[out].any(), (name, kind, x0, x1)
        counts["occupied_cells"] += float(occ_o[sl].sum())
        counts["empty_cells"] += float((orc[:, 1] == 0.0).sum())
    w = dict(counts, off_fraction=n[3] / n[2], occ_disagree=n[4] / n[2], median=max(med))
    if degenerate_rule:
        w.update(off_fraction_all_cells=n[1] / n[0], occ_disagree_all_cells=n[5] / n[0], degenerate_fraction=1.0 - n[2] / n[0])
    print(name, kind, GC.record("3_build_" + kind, name, w))
    return w


@pytest.mark.parametrize("name", GC.SMALL)
def test_build_matches_the_oracle(oracle, name):
    """uph_map_build against the oracle's constructMap at test_map_build_slab_matches_oracle's bar, unchanged: fewer than 1e-3 of the cells off by
    more than 1e-9, median below 1e-12, occupancy agreement above 0.999, cell_iters = rows ny nyaw iter_num, cells outside the slab untouched.
    tall and one_over whole; wide and fine on the first two rows, four rows in the middle and the last two"""
    w = _build_against_oracle(oracle, name, "hill")
    assert w["off_fraction"] < 1e-3 and w["median"] < 1e-12 and w["occ_disagree"] < 1e-3, w


@pytest.mark.parametrize("name", GC.SMALL)
def test_build_of_a_cloud_with_a_cliff(oracle, name):
    """the same bar on a cloud with a steep ramp across every slab: occupied cells exist (asserted of the oracle's layers)"""
    w = _build_against_oracle(oracle, name, "cliff")
    assert w["occupied_cells"] > 100
    assert w["off_fraction"] < 1e-3 and w["median"] < 1e-12 and w["occ_disagree"] < 1e-3, w


@pytest.mark.parametrize("name", GC.SMALL)
def test_build_of_a_cloud_that_covers_half_the_map(oracle, name):
    """a cloud on x < 0 only: the cells beyond it take the empty branch.  test_map_build_edge_and_empty_cells's bar: fewer than 1e-3 off among the
    cells that are degenerate on neither side (its exclusion), fewer than 1e-2 off among all compared cells, the median of |dz| below 1e-12 (z is
    well defined for a degenerate fit too); and the slab test's occupancy agreement among the non-degenerate cells.  The cloud's border, the line
    x = 0, runs through the middle slab of wide and fine and through the middle of tall and one_over: a third to a half of the compared cells are
    degenerate or empty"""
    w = _build_against_oracle(oracle, name, "half", degenerate_rule=True)
    assert w["empty_cells"] > 1000 and 0.05 < w["degenerate_fraction"] < 0.6
    assert w["off_fraction"] < 1e-3 and w["off_fraction_all_cells"] < 1e-2 and w["median"] < 1e-12 and w["occ_disagree"] < 1e-3, w


# ---- 4. slabs, tiles, the multi-slab build ------------------------------------------------------------------------------------------------------
ARRAYS = ("map_buffer", "c_buffer", "occ_buffer", "occ_r2_buffer")


def _grids(m):
    return {k: np.array(getattr(m, k)) for k in ARRAYS}


def _same_grids(got, want, tag):
    for k in ARRAYS:
        assert np.array_equal(got[k], want[k]), (tag, k, int((got[k] != want[k]).sum()))


def _whole(name, kind="hill"):
    if ("whole", name, kind) not in _MAPS:
        _MAPS[("whole", name, kind)] = _grids(_new_map(name).build(_cloud(kind)))
    return _MAPS[("whole", name, kind)]


def test_slab_pieces_equal_the_whole_build_on_tall():
    """build(x0, x1) over [0, 11), [11, 30), [30, 42) into one map = the whole build bit for bit, cells, c and both occupancy layers"""
    m = _new_map("tall")
    for (x0, x1) in ((0, 11), (30, 42), (11, 30)):
        m.build(_cloud("cliff"), x0=x0, x1=x1)
    _same_grids(_grids(m), _whole("tall", "cliff"), "pieces")


def test_fake_world_of_four_on_tall_is_bit_identical():
    """test_gpu_vocano's fake world of four and test_gpu_multi's single-process form on 42 rows: per = 11, a last slab of 9 rows, a staged gather"""
    import ctypes as C
    import torch
    import uneven_planner_amd as U
    from uneven_planner_amd.uneven_map import gather_slabs, slab_bounds
    nx, ny, nyaw = GC.DIMS["tall"]
    xyz, want = _cloud("cliff"), _whole("tall", "cliff")
    row, world = ny * nyaw * 4, 4
    slabs = []
    for rank in range(world):
        per, x0, x1 = slab_bounds(nx, rank, world)
        assert per == 11 and x1 - x0 == (11 if rank < 3 else 9)
        w = _new_map("tall").build(xyz, x0=x0, x1=x1, download=False)
        slab = torch.zeros(per * row, dtype=torch.float64, device="cuda:0")
        U._lib.check(w.L.uph_map_export_slab_dev(w.h, x0, x1, C.c_void_p(slab.data_ptr())), "export")
        slabs.append(slab)
    torch.cuda.synchronize()
    full = gather_slabs(slabs[0], nx, row, world, lambda f, s_: f.copy_(torch.cat(slabs))).contiguous()
    r = _new_map("tall")
    U._lib.check(r.L.uph_map_import_cells_dev(r.h, C.c_void_p(full.data_ptr())), "import")
    r.download()
    _same_grids(_grids(r), want, "fake world of four")
    G = U._lib.load().uph_device_count()
    maps = [_new_map("tall") if G < world else U.UnevenMap(GC.map_params("tall"), device=g) for g in range(world)]
    U.UnevenMap.build_multi(maps, xyz)
    for k, mm in enumerate(maps):
        _same_grids(_grids(mm), want, "build_multi map %d" % k)


def test_tile_and_window_on_tall():
    """a tile map holding rows [10, 30) of tall serves lookups bit-identical to the whole grid's; get_window on a window touching the last row and
    column equals the host buffer"""
    import uneven_planner_amd as U
    nx, ny, nyaw = GC.DIMS["tall"]
    m, _ = _analytic("tall")
    cells4 = np.asarray(GC.cells("tall")).reshape(nx, ny, nyaw, 4)
    t = _new_map("tall", tile=(10, 30))
    t.set_cells(cells4[10:30].reshape(-1, 4))
    assert np.array_equal(t.get_window(10, 30, 0, ny), cells4[10:30]) and np.array_equal(t.occ_r2_buffer, m.occ_r2_buffer.reshape(nx, ny)[10:30].ravel())
    ox, oy, _ = GC.origin("tall")
    res = GC.GRIDS["tall"]["xy_res"]
    rng = np.random.default_rng(4)
    pos = np.column_stack([rng.uniform(ox + 11.5 * res, ox + 28.5 * res, 2000), rng.uniform(oy - 0.1, -oy + 0.1, 2000), rng.uniform(-math.pi, math.pi, 2000)])
    vt, gt = t.getAllWithGrad(pos)
    vf, gf = m.getAllWithGrad(pos)
    assert np.array_equal(vt, vf) and np.array_equal(gt, gf) and np.abs(gf).max() > 0
    assert np.array_equal(m.get_window(nx - 5, nx, ny - 7, ny), cells4[nx - 5:, ny - 7:])
    assert np.array_equal(m.get_window(0, nx, ny - 1, ny), cells4[:, ny - 1:]) and np.array_equal(m.get_window(nx - 1, nx, 0, ny), cells4[nx - 1:])
    with pytest.raises(U._lib.UnevenHipError):
        m.get_window(0, ny, 0, 4)                             # ny rows: in range for y, beyond the last row


# ---- 5. the map update --------------------------------------------------------------------------------------------------------------------------
def _col_diff(a, b, nx, ny):
    d = (a["map_buffer"].reshape(nx, ny, -1) != b["map_buffer"].reshape(nx, ny, -1)).any(axis=2)
    d |= (a["c_buffer"].reshape(nx, ny, -1) != b["c_buffer"].reshape(nx, ny, -1)).any(axis=2)
    d |= (a["occ_buffer"].reshape(nx, ny, -1) != b["occ_buffer"].reshape(nx, ny, -1)).any(axis=2)
    d |= a["occ_r2_buffer"].reshape(nx, ny) != b["occ_r2_buffer"].reshape(nx, ny)
    return d


@pytest.mark.parametrize("name", ["tall", "one_over"])
def test_map_update_equals_a_rebuild(name):
    """uph_map_update with tests/map_update_cases.py's box (its size, placed off-centre on the rectangle) and a second box over the far corner
    (nx - 1, ny - 1): cells, c and both occupancy layers equal a fresh build_filtered of the edited cloud bit for bit, and the reported rect is
    the rect of the columns that differ (numpy)"""
    import uneven_planner_amd as U
    from map_update_cases import BOX, merged, rect_rule, scan
    nx, ny, nyaw = GC.DIMS[name]
    hx, hy = 0.5 * GC.GRIDS[name]["size_x"], 0.5 * GC.GRIDS[name]["size_y"]
    sx, sy = 0.25 * hx, -0.2 * hy
    box1 = (BOX[0] + sx, BOX[1] + sx, BOX[2] + sy, BOX[3] + sy)
    box2 = (hx - 0.55, hx + 0.2, hy - 0.45, hy + 0.2)
    xyz = _cloud("hill")
    m = _new_map(name).build(xyz)
    W = U.UnevenMap.filter_cloud(xyz)
    for tag, box, new in (("box", box1, scan(box1)), ("far corner", box2, scan(box2, seed=12, n_side=40, mound=0.2, sigma=0.12))):
        before = _grids(m)
        info = m.update(box, new)
        W = merged(W, box, new, U.UnevenMap.filter_cloud)
        dev = m.built_cloud()
        assert dev.shape == W.shape and np.array_equal(dev.view(np.uint32), W.view(np.uint32)), (name, tag)
        after = _grids(m)
        _same_grids(after, _grids(_new_map(name).build_filtered(W)), (name, tag))
        d = _col_diff(before, after, nx, ny)
        assert d.any() and info["n_changed"] == int(d.sum()), (name, tag, info["n_changed"], int(d.sum()))
        xs, ys = np.nonzero(d.any(axis=1))[0], np.nonzero(d.any(axis=0))[0]
        assert info["changed"] == (int(xs[0]), int(xs[-1]) + 1, int(ys[0]), int(ys[-1]) + 1), (name, tag, info["changed"])
        assert info["dirty"] == rect_rule(m.params, box) == m.update_rect(box) and info["full_refit"] == 0, (name, tag, info["dirty"])
        x0, x1, y0, y1 = info["dirty"]
        outside = np.ones((nx, ny), dtype=bool)
        outside[x0:x1, y0:y1] = False
        assert not d[outside].any() and info["n_refit"] == (x1 - x0) * (y1 - y0) + info["n_far"], (name, tag)
        if tag == "far corner":
            assert d[nx - 1, ny - 1] and info["dirty"][1] == nx and info["dirty"][3] == ny and info["changed"][1] == nx and info["changed"][3] == ny
        GC.record("5_map_update", name, {tag.replace(" ", "_") + "_changed_columns": float(d.sum())})


# ---- 6. the fbm fill ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["far", "tall", "fine", "one_over"])
def test_fbm_fill_matches_the_restated_fit(name):
    """uph_map_fill_fbm against test_gpu_km2.fit_cell (the surface and constructMap's fit restated in numpy) on 300 sampled cells that always include
    (nx - 1, ny - 1, nyaw - 1) and (0, ny - 1, 0), at that test's bars; the fp32 map is the rounded fp64 one.  far and tall (38 bins: idle lanes), and fine
    and one_over, where the fill's yaw loop takes a second trip"""
    from test_gpu_km2 import SMALL_FBM, fit_cell
    from uneven_planner_amd.uneven_map import fbm_table
    nx, ny, nyaw = GC.DIMS[name]
    m64 = _new_map(name).fill_fbm(SMALL_FBM)
    _MAPS[("fbm", name)] = m64
    tab = fbm_table(SMALL_FBM)
    cells = m64.map_buffer.reshape(nx, ny, nyaw, 4)
    rng = np.random.default_rng(5)
    pick = [(nx - 1, ny - 1, nyaw - 1), (0, ny - 1, 0), (nx - 1, 0, nyaw - 1), (0, 0, 0)]
    pick += [(int(rng.integers(nx)), int(rng.integers(ny)), int(rng.integers(nyaw))) for _ in range(296)]
    worst = np.zeros(4)
    for ix, iy, iw in pick:
        worst = np.maximum(worst, np.abs(cells[ix, iy, iw] - fit_cell(tab, m64, ix, iy, iw)))
    print(name, GC.record("6_fbm_fill", name, dict(z=worst[0], sigma=worst[1], zbx=worst[2], zby=worst[3])))
    assert worst[0] < 1e-10 and worst[1] < 1e-9 and worst[2] < 1e-8 and worst[3] < 1e-8, worst
    m32 = _new_map(name, storage="f32").fill_fbm(SMALL_FBM)
    assert np.array_equal(m32.map_buffer, m64.map_buffer.astype(np.float32).astype(np.float64)) and np.array_equal(m32.occ_r2_buffer, m64.occ_r2_buffer)


# ---- 7. the optimiser ---------------------------------------------------------------------------------------------------------------------------
def _states(probs, seed0):
    return [GC.state_for(p, seed0 + i) for i, p in enumerate(probs)]


def _problems(name):
    """the eight problems: 5 to 25 pieces, at least three with way-points beyond the short axis's half-length, one leaving over each border"""
    probs = GC.optimiser_problems(name)
    n = [p["inner_xy"].shape[1] + 1 for p in probs]
    assert len(probs) == 8 and min(n) >= 5 and max(n) <= 25, n
    assert sum(GC.beyond_short_half(name, p) for p in probs) >= 3
    ax = GC.halves(name)[0]
    out = [GC.leaves_map(name, p) for p in probs]
    assert sum(o[ax] for o in out) >= 1 and sum(o[1 - ax] for o in out) >= 1          # over the short border (end of the long axis) and over the long one
    return probs


def _evaluated(name, variant, storage="f64"):
    """upload + set_state + one evaluation at x0 of the eight problems (once per module): the context with the batch resident, and the downloads"""
    key = (name, variant, storage)
    if key not in _EVAL:
        m, og = _analytic(name, storage)
        probs = _problems(name)
        st = _states(probs, 500)
        opt = _ctx(m, variant)
        opt.upload(probs)
        opt.set_state(lam=[s["lam"] for s in st], mu=[s["mu"] for s in st], scale_cx=[s["scale_cx"] for s in st],
                      scale_fx=np.array([s["scale_fx"] for s in st]), rho=np.array([s["rho"] for s in st]))
        f, gs = opt.eval_batch(opt.x0_packed(probs))
        out = opt.download()
        _EVAL[key] = dict(opt=opt, probs=probs, st=st, out=[dict(o, f=f[i], g=gs[i]) for i, o in enumerate(out)], m=m, og=og)
    return _EVAL[key]


def _oracle_evals(oracle, og, probs, st, resident=None):
    """the oracle's evaluation at x0, and its calConstrainCostGrad alone on the trajectory the DEVICE holds (resident: the downloads with c_xy,
    c_yaw, T_xy, T_yaw) -- what uph_penalty_batch works on.  On the oracle's own trajectory the comparison would not be one of the same function:
    gdCyaw and gdTyaw are sums PER YAW PIECE, and with Nyaw = 2 Nxy the last sample of every position piece sits exactly on a yaw knot, where
    int(now_time / T_yaw) turns on the last bit of T.  The device forms T = expC2(tau) / N with contracted multiply-adds, now and then one double
    off the oracle's (inside the 1e-13 its T is held to); a sample on a knot then changes its piece on one side only -- the same objective (f and
    grad f agree at 1e-9), another split of it into pieces (seen on an MI355X: gdCyaw 8.1e-7 apart on one problem of wide, reproduced to all
    digits by the oracle alone with T_xy one double lower).  On equal durations every sample falls into the same piece on both sides, or the
    device's rule for it is wrong."""
    ref = []
    for k, (p, s) in enumerate(zip(probs, st)):
        a = oracle.OracleALM(og)
        x0 = a.setup(p)
        a.set_state(lam=s["lam"], mu=s["mu"], scale_cx=s["scale_cx"], scale_fx=s["scale_fx"])
        a.set_rho(s["rho"])
        f, g, _ = a.eval(x0)
        t = a.get_state()
        cxy, cyaw, txy, tyaw, _ = a.coeffs()
        r = dict(f=f, g=g, hx=t["hx"], gx=t["gx"], c_xy=cxy, c_yaw=cyaw, T_xy=txy, T_yaw=tyaw)
        if resident is not None:
            o = resident[k]
            a.set_coeffs(o["c_xy"], o["c_yaw"], o["T_xy"], o["T_yaw"])
            cost, gcx, gtx, gcy, gty = a.constrain_resident()
            t2 = a.get_state()
            r.update(pen_cost=cost, gdCxy=gcx, gdCyaw=gcy, gdTxy=gtx, gdTyaw=gty, pen_hx=t2["hx"], pen_gx=t2["gx"], T_differs=float((txy, tyaw) != (o["T_xy"], o["T_yaw"])))
        ref.append(r)
    return ref


def _worst(errs):
    out = {}
    for e in errs:
        for k, v in e.items():
            out[k] = max(out.get(k, 0.0), float(v))
    return out


CASES_7 = [(n, v, "f64") for n in GC.SMALL for v in (AUTO, FORCED)] + [("wide", AUTO, "f32")]
_id7 = lambda c: "%s-%s-%s" % (c[0], _vid(c[1]), c[2])


@pytest.mark.parametrize("case", CASES_7, ids=_id7)
def test_init_scaling_matches_the_oracle(oracle, case):
    """test_init_scaling_matches_oracle's bar: scale_fx and scale_cx at 1e-9"""
    name, variant, storage = case
    m, og = _analytic(name, storage)
    probs = _problems(name)
    opt = _ctx(m, variant)
    opt.upload(probs)
    opt.init_scaling_batch()
    out = opt.download()
    errs = []
    for p, o in zip(probs, out):
        a = oracle.OracleALM(og)
        a.init_scaling(a.setup(p))
        s = a.get_state()
        errs.append(dict(scale_fx=PS.rel1(s["scale_fx"], o["scale_fx"]), scale_cx=rel(s["scale_cx"], o["scale_cx"])))
    w = GC.record("7_init_scaling " + _vid(variant) + " " + storage, name, _worst(errs))
    print(_id7(case), w)
    assert all(v < 1e-9 for v in w.values()), (w, errs)


@pytest.mark.parametrize("case", CASES_7, ids=_id7)
def test_single_evaluation_penalty_and_report_match_the_oracle(oracle, case):
    """one evaluation (f, grad f, hx, gx, coefficients at 1e-9, T at 1e-13: test_single_evaluation_matches_oracle's bars), uph_penalty_batch alone at
    1e-9 (against the oracle's calConstrainCostGrad on the device's resident trajectory, see _oracle_evals) and the report at
    test_report_matches_oracle_on_same_trajectory's 1e-9, on the eight problems with random duals and scales"""
    name, variant, storage = case
    E = _evaluated(name, variant, storage)
    ref = _oracle_evals(oracle, E["og"], E["probs"], E["st"], resident=E["out"])
    errs = [PS.eval_errors(r, o) for r, o in zip(ref, E["out"])]
    w = GC.record("7_evaluation " + _vid(variant) + " " + storage, name, _worst(errs))
    print(_id7(case), w)
    assert all(v < (1e-13 if k == "T" else 1e-9) for k, v in w.items()), (w, errs)
    opt = E["opt"]
    rep = opt.getMaxVxAxAyCurAttSig()
    rerr = []
    for p, o, row in zip(E["probs"], E["out"], rep):
        a = oracle.OracleALM(E["og"])
        a.setup(p)
        a.set_coeffs(o["c_xy"], o["c_yaw"], o["T_xy"], o["T_yaw"])
        rerr.append(PS.report_errors(a.report(), row))
    w = GC.record("7_report " + _vid(variant) + " " + storage, name, _worst(rerr))
    assert all(v < 1e-9 for v in w.values()), (w, rerr)
    pen = opt.penalty_batch(repeat=1, store_residuals=True)
    out = opt.download()
    perr = [PS.penalty_errors(r, d, o["hx"], o["gx"]) for r, d, o in zip(ref, pen, out)]
    w = GC.record("7_penalty " + _vid(variant) + " " + storage, name, dict(_worst(perr), durations_one_double_apart=sum(r["T_differs"] for r in ref)))
    assert all(v < 1e-9 for k, v in w.items() if k != "durations_one_double_apart"), (w, perr)


@pytest.mark.parametrize("case", CASES_7, ids=_id7)
def test_capped_solves_match_the_oracle(oracle, case):
    """test_gpu_pieces::test_capped_solves on the eight problems: two ALM passes of at most 12 L-BFGS iterations, counters equal the oracle's, x and
    the cost at 1e-5, a second solve of the same batch bit-identical"""
    name, variant, storage = case
    m, og = _analytic(name, storage)
    probs = _problems(name)
    opt = _ctx(m, variant, params=PS.SOLVE_PARAMS)
    opt.set_rho(1.0)
    first = opt.optimize_batch(probs)
    opt.set_rho(1.0)
    second = opt.optimize_batch(probs)
    errs, bad = [], []
    for i, (p, o) in enumerate(zip(probs, first)):
        ro = oracle.OracleALM(og, PS.SOLVE_PARAMS).optimize(p)
        if (o["ret"], o["lbfgs_iters"], o["evals"]) != (ro["ret"], ro["lbfgs_iters"], ro["evals"]):
            bad.append((i, (o["ret"], o["lbfgs_iters"], o["evals"]), (ro["ret"], ro["lbfgs_iters"], ro["evals"])))
        errs.append(dict(x=PS.rel(ro["x"], o["x"]), cost=PS.rel1(ro["cost"], o["cost"])))
    w = GC.record("7_capped_solves " + _vid(variant) + " " + storage, name, _worst(errs))
    print(_id7(case), w)
    assert not bad, bad
    assert all(v < 1e-5 for v in w.values()), (w, errs)
    assert all(np.array_equal(a["x"], b["x"]) and a["evals"] == b["evals"] for a, b in zip(first, second))


# ---- 8. local frames ----------------------------------------------------------------------------------------------------------------------------
def test_local_frames_on_a_non_square_grid(oracle):
    """far reaches 48 m from the origin on x and 12 m on y: beyond FRAME_EXTENT on one axis only, so every trajectory is solved in its own local
    frame.  Problems within 10 m of the x = +48 border and within 4 m of either y border on the fbm cells, one evaluation against an oracle grid of
    the same geometry at test_far_from_origin_solves_meet_the_1e4_bar's per-evaluation bar (f 1e-12, grad f 1e-11); the way-points and the
    rollout come back in map coordinates.  The binding exposes no flag for "this context is framed": what is asserted is the library's documented
    condition for it, from the constant in csrc/uph_common.hpp"""
    from test_gpu_km2 import SMALL_FBM
    from uneven_planner_amd.resample import make_problem
    nx, ny, nyaw = GC.DIMS["far"]
    m = _MAPS.get(("fbm", "far")) or _new_map("far").fill_fbm(SMALL_FBM)
    src = open(os.path.join(ROOT, "uneven_planner_amd", "csrc", "uph_common.hpp")).read()
    extent = float(re.search(r"constexpr\s+double\s+FRAME_EXTENT\s*=\s*([0-9.]+)", src).group(1))
    assert abs(m.min_boundary[0]) > extent and abs(m.max_boundary[0]) > extent and abs(m.max_boundary[1]) < extent
    og = GC.oracle_grid(oracle, "far", m.map_buffer)
    GC.check_dims("far", og.dims)
    grid = (nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1])
    probs, seed = [], 7400
    while len(probs) < 8:
        rng = np.random.Generator(np.random.PCG64(seed))
        seed += 1
        side = 1.0 if len(probs) % 2 == 0 else -1.0
        s = (rng.uniform(38.5, 47.0), side * rng.uniform(8.5, 11.3), rng.uniform(-math.pi, math.pi))
        d, th = rng.uniform(3.0, 7.0), rng.uniform(-math.pi, math.pi)
        g = (s[0] + d * math.cos(th), s[1] + d * math.sin(th), rng.uniform(-math.pi, math.pi))
        if not (38.0 < g[0] < 47.5 and 8.0 < side * g[1] < 11.5):
            continue
        ix, iy, _ = GC.cell_index("far", [s, g])
        if m.occ_r2_buffer[ix * ny + iy].any():
            continue
        probs.append(make_problem(s, g))
    import uneven_planner_amd as U
    opt = U.ALMTrajOpt(m)
    opt.upload(probs)
    f, gs = opt.eval_batch(opt.x0_packed(probs))
    out = opt.download()
    errs = []
    for i, p in enumerate(probs):
        a = oracle.OracleALM(og)
        fo, go, _ = a.eval(a.setup(p))
        errs.append(dict(f=abs(f[i] - fo) / abs(fo), grad=rel(go, gs[i])))
        # results in map coordinates: the constant coefficients of the first piece are the start point, the rollout starts and ends on the problem's end points
        assert np.abs(out[i]["c_xy"][0] - p["init_xy"][:, 0]).max() < 1e-9, i
    offs, rows = opt.rollout(0.05, ST, with_end=True)
    for i, p in enumerate(probs):
        assert np.abs(rows[offs[i], 1:3] - p["init_xy"][:, 0]).max() < 1e-9 and np.abs(rows[offs[i + 1] - 1, 1:3] - p["end_xy"][:, 0]).max() < 1e-9, i
    assert rows[:, 1].min() > 36.0 and np.abs(rows[:, 2]).min() > 6.0
    w = GC.record("8_local_frames", "far", _worst(errs))
    print("far", w)
    assert w["f"] < 1e-12 and w["grad"] < 1e-11, (w, errs)


# ---- 9. the search ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.SMALL)
def test_search_expansion_sequences_are_the_oracles(oracle, name):
    """the batched device search against the oracle's KinoAstar::plan on the analytic cells with an occupied block in the middle, the oracle's grid
    carrying the device's occupancy layers, 16 queries across the long axis around the block: test_gpu_kino._same (status, counters and the whole
    expansion sequence integer-exact, poses at 1e-9).  At least 8 succeed and the mean iter_num exceeds 100 -- true of the oracle alone on the CPU
    (all 16 succeed; mean iter_num 816 / 223 / 179 / 159 on wide / tall / fine / one_over)"""
    import uneven_planner_amd as U
    from test_gpu_kino import _same
    nx, ny, nyaw = GC.DIMS[name]
    m = _new_map(name).set_cells(GC.search_cells(name))
    og = GC.oracle_grid(oracle, name, m.map_buffer)
    og.set_occ(m.occ_buffer, m.occ_r2_buffer)
    assert 50 < m.occ_r2_buffer.sum() < nx * ny // 4
    S, G = GC.search_queries(name)
    ka = U.KinoAstar(m)
    dev = ka.plan_batch(S, G, path_cap=1024, exp_cap=40000)
    ok = oracle.OracleKinoAstar(og)
    n_ok, iters = 0, []
    for b in range(len(S)):
        o = ok.plan(S[b], G[b])
        n_ok += o["status"] == 0
        iters.append(o["iter_num"])
        _same(dev[b], o, "%s query %d" % (name, b))
    assert n_ok >= 8 and np.mean(iters) > 100, (n_ok, np.mean(iters))
    GC.record("9_search", name, dict(successes=n_ok, mean_iter_num=np.mean(iters)))
    _MAPS[("search", name)] = (m, ka)


def test_plan_goals_upload_on_wide_equals_the_composed_chain():
    """one uph_plan_upload on wide against the composed host chain (search -> uph_resample_batch -> optimize_batch on a fresh context), bit for bit,
    as test_gpu_plan_chain::test_chain_equals_the_composed_chain"""
    import uneven_planner_amd as U
    from test_gpu_plan_chain import _check_chain, _composed, _same_probs, _same_results
    if ("search", "wide") in _MAPS:
        m, ka = _MAPS[("search", "wide")]
    else:
        m = _new_map("wide").set_cells(GC.search_cells("wide"))
        ka = U.KinoAstar(m)
    S, G = GC.search_queries("wide")
    comp = _composed(m, ka, S, G)
    assert len(comp["found"]) >= 8
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    out = opt.plan_goals(ka, S, G, full=True)
    _check_chain(opt, opt.last_plan, comp, "wide")
    _same_probs(opt.plan_staged(), comp["probs"], "wide")
    _same_results([out[b] for b in comp["found"]], comp["res"], "wide")


# ---- 10. reading trajectories back --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.SMALL)
def test_rollout_and_check_of_the_evaluated_batch(oracle, name):
    """rollout(0.01, STATE | TERRAIN | POSE) of the batch item 7 evaluated, at test_gpu_resident_sweep's bars: the time column is the running sum bit for
    bit, states against piece_sweep.ref_states and terms against ref_terms on this grid's oracle at 1e-12, poses against uph_terrain_pose_query at
    1e-15; uph_check_batch on full windows equals check_rows on those rows bit for bit.  The two trajectories that leave the map show it in the
    rollout (flat ground: sigma 0, att -1 beyond the border) and in the check (the occupied-or-outside bit and count)"""
    from test_gpu_check import _same
    from uneven_planner_amd.alm_traj_opt import CHECK_OCC_BIT, check_rows
    E = _evaluated(name, AUTO)
    opt, out, probs, m, og = E["opt"], E["out"], E["probs"], E["m"], E["og"]
    offs, rows = opt.rollout(0.01, ST | TR | PO, with_end=True)
    assert rows.shape == (offs[-1], 28) and np.isfinite(rows).all()
    terms = PS.ref_terms(og, rows[:, 1:9], m.params["gravity"])
    t_scale = np.maximum(1.0, np.abs(terms).max(axis=0))
    Rm, p = m.getTerrainPosBatch(rows[:, 1:4])
    poses = np.concatenate([Rm.transpose(0, 2, 1).reshape(-1, 9), p], axis=1)
    p_scale = np.maximum(1.0, np.abs(poses).max(axis=0))
    scaled = lambda a, b, s=None: float((np.abs(a - b) / (np.maximum(1.0, np.abs(b).max(axis=0)) if s is None else s)).max())
    occ = m.frontend_query(rows[:, 1:4])[1]
    errs, per = [], []
    for b, o in enumerate(out):
        a, e = int(offs[b]), int(offs[b + 1])
        nxy, nyw = o["c_xy"].shape[0] // 6, o["c_yaw"].shape[0] // 6
        total = PS.total_duration(o["T_xy"], o["T_yaw"], nxy, nyw)
        tab = PS.time_table(0.01, total)
        cnt = e - a - 1
        assert cnt == int(np.searchsorted(tab, total, "left")) and np.array_equal(rows[a:a + cnt, 0], tab[:cnt]) and rows[e - 1, 0] == total, (name, b)
        ref = PS.ref_states(o["c_xy"], o["c_yaw"], o["T_xy"], o["T_yaw"], nxy, nyw, rows[a:e, 0])[:, PS.ROW_OF_STATE]
        errs.append(dict(states=scaled(rows[a:e, 1:9], ref), terms=scaled(rows[a:e, 9:16], terms[a:e], t_scale), poses=scaled(rows[a:e, 16:28], poses[a:e], p_scale),
                         end_xy=float(np.abs(rows[e - 1, 1:3] - np.asarray(probs[b]["end_xy"])[:, 0]).max())))
        per.append(check_rows(rows[a:e, 0], rows[a:e, 9:16], occ[a:e], opt.check_limits()))
    w = GC.record("10_rollout", name, _worst(errs))
    print(name, w)
    assert w["states"] < 1e-12 and w["terms"] < 1e-12 and w["poses"] < 1e-15 and w["end_xy"] < 1e-9, (w, errs)
    got = opt.check(np.arange(len(out), dtype=np.int32), 0.0, None, dt=0.01, with_end=True)
    _same(got, {k: np.array([q[k] for q in per]) for k in per[0]}, name)
    assert np.array_equal(got["counts"][:, 0], np.diff(offs))
    # the trajectories that leave the map.  Two rules, as in the reference: a lookup is inside by POSITION (isInMap: within the boundary less 1e-4), a cell
    # query by INDEX (on tall the last cell overhangs the boundary by 0.04 m, so a pose there has no terrain and still a cell)
    hx, hy = 0.5 * GC.GRIDS[name]["size_x"], 0.5 * GC.GRIDS[name]["size_y"]
    nx, ny, nyaw = GC.DIMS[name]
    beyond = (np.abs(rows[:, 1]) > hx) | (np.abs(rows[:, 2]) > hy)
    ix, iy, iw = GC.cell_index(name, rows[:, 1:4])
    off_grid = (ix < 0) | (ix > nx - 1) | (iy < 0) | (iy > ny - 1) | (iw < 0) | (iw > nyaw - 1)
    assert np.all(rows[beyond, 14] == 0.0) and np.all(rows[beyond, 13] == -1.0) and np.array_equal(occ == -1, off_grid) and not (occ == 1).any()
    leaving = [b for b in range(len(out)) if off_grid[offs[b]:offs[b + 1]].any()]
    assert len(leaving) >= 2 and all(any(GC.leaves_map(name, probs[b])) for b in leaving) and all(beyond[offs[b]:offs[b + 1]].any() for b in leaving)
    assert np.array_equal(got["counts"][:, 2], [off_grid[offs[b]:offs[b + 1]].sum() for b in range(len(out))])
    # ... and with no limit on any term the first violation of a leaving trajectory is its first sample without a cell
    free = np.full(7, np.inf)
    got2 = opt.check(np.arange(len(out), dtype=np.int32), 0.0, None, dt=0.01, with_end=True, limits=free)
    per2 = [check_rows(rows[offs[b]:offs[b + 1], 0], rows[offs[b]:offs[b + 1], 9:16], occ[offs[b]:offs[b + 1]], free) for b in range(len(out))]
    _same(got2, {k: np.array([q[k] for q in per2]) for k in per2[0]}, name + ", no limits")
    for b in range(len(out)):
        if b in leaving:
            first = int(offs[b] + np.argmax(off_grid[offs[b]:offs[b + 1]]))
            assert got2["first_mask"][b] == 1 << CHECK_OCC_BIT and got2["first_t"][b] == rows[first, 0], (name, b)
        else:
            assert got2["first_mask"][b] == 0 and np.isnan(got2["first_t"][b]), (name, b)
