"""GPU tier of updating the map from a new scan in a box (uph_map_update, uph_map_build_filtered).

Bar: after every update the cells, c and both occupancy layers EQUAL (np.array_equal, whole grid) what uph_map_build_filtered gives on a fresh map
for the resident cloud W' = (W without the points in the box) ++ filter_cloud(new points in the box), and built_cloud() equals that W' bit for
bit.  The info fields are held to numpy counts over the grids before and after.  One case goes to the CPU oracle at test_gpu_map.py's own bar.
Default 200 x 200 x 64 grid, scenes.make_hill_cloud()."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from map_update_cases import BOX, in_box, merged, rect_rule, scan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX = NY = 200
NYAW = 64
ARRAYS = ("map_buffer", "c_buffer", "occ_buffer", "occ_r2_buffer")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _grids(m):
    return {k: np.array(getattr(m, k)) for k in ARRAYS}


def _same_grids(got, want, tag):
    for k in ARRAYS:
        assert np.array_equal(got[k], want[k]), (tag, k, int((got[k] != want[k]).sum()))


def _fresh(W):
    import uneven_planner_amd as U
    return _grids(U.UnevenMap().build_filtered(W))


def _col_diff(a, b):
    """(nx, ny) bool: columns where a cell, c or an occupancy byte differs"""
    d = (a["map_buffer"].reshape(NX, NY, -1) != b["map_buffer"].reshape(NX, NY, -1)).any(axis=2)
    d |= (a["c_buffer"].reshape(NX, NY, -1) != b["c_buffer"].reshape(NX, NY, -1)).any(axis=2)
    d |= (a["occ_buffer"].reshape(NX, NY, -1) != b["occ_buffer"].reshape(NX, NY, -1)).any(axis=2)
    d |= a["occ_r2_buffer"].reshape(NX, NY) != b["occ_r2_buffer"].reshape(NX, NY)
    return d


def _check_info(info, before, after, tag):
    d = _col_diff(before, after)
    assert info["n_changed"] == int(d.sum()), (tag, info["n_changed"], int(d.sum()))
    if d.any():
        xs, ys = np.nonzero(d.any(axis=1))[0], np.nonzero(d.any(axis=0))[0]
        assert info["changed"] == (int(xs[0]), int(xs[-1]) + 1, int(ys[0]), int(ys[-1]) + 1), (tag, info["changed"])
    else:
        assert info["changed"] == (0, 0, 0, 0), (tag, info["changed"])
    x0, x1, y0, y1 = info["dirty"]
    out = np.ones((NX, NY), dtype=bool)
    out[x0:x1, y0:y1] = False
    return d, out


@pytest.fixture(scope="module")
def base():
    """the hill cloud, its filtered form W, the grids of build(xyz), and the one-update case: scan, W', the fresh build of W'"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    xyz = scenes.make_hill_cloud()
    W = U.UnevenMap.filter_cloud(xyz)
    built = _grids(U.UnevenMap().build(xyz))
    new = scan()
    W1 = merged(W, BOX, new, U.UnevenMap.filter_cloud)
    return dict(xyz=xyz, W=W, built=built, new=new, W1=W1, fresh1=_fresh(W1))


def test_build_filtered_equals_build(base):
    import uneven_planner_amd as U
    m = U.UnevenMap().build_filtered(base["W"])
    _same_grids(_grids(m), base["built"], "build_filtered")
    assert np.array_equal(_bits(m.built_cloud()), _bits(base["W"]))
    # the crop box still applies, the order is kept
    odd = np.concatenate([base["W"][:500], np.array([[10.5, 0, 0], [np.nan, 0, 0.3], [0, 0, 5.5]], dtype=np.float32), base["W"][500:]])
    m2 = U.UnevenMap().build_filtered(odd)
    assert np.array_equal(_bits(m2.built_cloud()), _bits(base["W"]))
    _same_grids(_grids(m2), base["built"], "build_filtered + crop")


def test_one_update(base):
    import uneven_planner_amd as U
    m = U.UnevenMap().build(base["xyz"])
    before = _grids(m)
    _same_grids(before, base["built"], "build")
    new = base["new"]
    assert in_box(new, BOX).sum() < len(new) - 3 and np.isnan(new).any()          # points outside the box and a NaN point are in the scan
    info = m.update(BOX, new)
    after = _grids(m)
    W1 = base["W1"]
    dev = m.built_cloud()
    assert dev.shape == W1.shape and np.array_equal(_bits(dev), _bits(W1))
    n_in = int((in_box(new, BOX) & np.isfinite(new).all(axis=1)).sum())
    kept = int((~in_box(base["W"], BOX)).sum())
    assert info["n_cloud"] == len(W1) and info["n_removed"] == len(base["W"]) - kept and info["n_added"] == len(W1) - kept
    assert 0 < info["n_added"] < n_in                                               # the leaf of five points (at least) merged
    _same_grids(after, base["fresh1"], "update vs fresh build_filtered(W')")
    d, outside = _check_info(info, before, after, "one update")
    assert not d[outside].any()                                                     # cells outside dirty equal the pre-update cells
    assert info["dirty"] == rect_rule(m.params, BOX) == m.update_rect(BOX) and info["dirty"][2:] == (87, 117)
    area = (info["dirty"][1] - info["dirty"][0]) * (info["dirty"][3] - info["dirty"][2])
    assert info["n_refit"] == area + info["n_far"] and info["full_refit"] == 0
    assert info["n_changed"] > 400
    occ = after["occ_buffer"].reshape(NX, NY, NYAW)
    assert before["occ_buffer"].reshape(NX, NY, NYAW)[92:100].sum() == 0 and occ[92:100].sum() > 0      # occupied cells appear (the mound's flanks)
    st = info["stages_ms"]
    assert st["call"] > 0 and st["kernel"] > 0 and st["call"] >= st["kernel"]


def test_sequence_of_updates(base):
    """an update, an overlapping update, a remove-only update of a 1.2 m box (a hole: its inner columns take the global search and must be refitted by
    every later update, wherever its box lies), then an update far from the hole"""
    import uneven_planner_amd as U
    m = U.UnevenMap().build(base["xyz"])
    W = base["W"]
    box2 = (0.2, 1.1, 0.1, 1.0)
    hole = (-3.1, -1.9, 1.4, 2.6)
    box4 = (2.0, 2.6, -3.0, -2.5)
    steps = [("first", BOX, base["new"]), ("overlapping", box2, scan(box2, seed=12, n_side=40, mound=-0.15, sigma=0.2)),
             ("hole", hole, None), ("after the hole", box4, scan(box4, seed=13, n_side=30, mound=0.1, sigma=0.1, extras=False))]
    far_before = None
    for tag, box, new in steps:
        before = _grids(m)
        info = m.update(box, new)
        W = merged(W, box, new, U.UnevenMap.filter_cloud)
        assert np.array_equal(_bits(m.built_cloud()), _bits(W)), tag
        after = _grids(m)
        _same_grids(after, _fresh(W), tag)
        d, outside = _check_info(info, before, after, tag)
        assert info["full_refit"] == 0 and info["dirty"] == rect_rule(m.params, box), tag
        area = (info["dirty"][1] - info["dirty"][0]) * (info["dirty"][3] - info["dirty"][2])
        assert info["n_refit"] == area + info["n_far"], tag
        if tag == "hole":
            assert info["n_added"] == 0 and info["n_removed"] > 500
            far_before = info["n_far"]
        if tag == "after the hole":
            assert info["n_far"] > 0 and info["n_far"] > far_before       # the hole's inner columns: 1.2 m - 2 x 0.32 m across, about 11 x 11 of them
            assert not d[outside].any()                                  # ... and refitting them changed nothing


def test_origin_move_refits_everything(base):
    """a remove-only box over the cloud's minimum-x edge: the bucket origin moves, every held column is refitted"""
    import uneven_planner_amd as U
    m = U.UnevenMap().build(base["xyz"])
    before = _grids(m)
    W = base["W"]
    xmin = float(W[:, 0].min())
    box = (xmin - 0.1, xmin + 0.05, -7.0, 7.0)
    W2 = merged(W, box, None, None)
    assert 0 < len(W) - len(W2) and float(W2[:, 0].min()) != xmin
    info = m.update(box)
    assert info["full_refit"] == 1 and info["dirty"] == (0, NX, 0, NY) and info["n_refit"] == NX * NY and info["n_far"] == 0
    assert np.array_equal(_bits(m.built_cloud()), _bits(W2))
    after = _grids(m)
    _same_grids(after, _fresh(W2), "origin move")
    _check_info(info, before, after, "origin move")
    # the map keeps updating incrementally afterwards
    info2 = m.update(BOX, base["new"])
    assert info2["full_refit"] == 0
    _same_grids(_grids(m), _fresh(merged(W2, BOX, base["new"], U.UnevenMap.filter_cloud)), "after the origin move")


def test_update_against_the_oracle(base, oracle):
    """rows 92-99 after the one update against the oracle's constructMap on W' (no filters), at test_gpu_map.py's bar; no cell is excluded"""
    W1, got = base["W1"], base["fresh1"]
    import uneven_planner_amd as U
    m = U.UnevenMap().build(base["xyz"])
    m.update(BOX, base["new"])
    g = oracle.OracleGrid()
    oracle.OracleMapBuilder(xyz=W1, apply_filters=False).construct(g, x0=92, x1=100)
    co, _ = g.get_cells()
    sl = slice(92 * NY * NYAW, 100 * NY * NYAW)
    d = np.abs(m.map_buffer[sl] - co[sl]).max(axis=1)
    print("oracle: share off by more than 1e-9 %.3g, max %.3g, median %.3g" % ((d > 1e-9).mean(), d.max(), np.median(d)))
    assert (d > 1e-9).mean() < 1e-3, ((d > 1e-9).mean(), d.max())
    assert np.median(d) < 1e-12
    occ_o, _ = g.get_occ()
    occ_o = np.asarray(occ_o)[sl]
    assert int(occ_o.sum()) == 586                                                  # the oracle's count for this input (CPU, deterministic)
    agree = (m.occ_buffer[sl] == occ_o).mean()
    print("oracle: occupancy agreement %.6f, device count %d" % (agree, int(m.occ_buffer[sl].sum())))
    assert agree > 0.999
    assert np.array_equal(m.map_buffer[sl], got["map_buffer"][sl])


def test_the_loop_update_check(base):
    """plan and solve 64 hill goals, then a scan with a mound under one trajectory: check reports that trajectory inside the stretch whose rows lie in
    `changed`; trajectories whose rows all stay two cells outside `changed` answer bit for bit as before"""
    import uneven_planner_amd as U
    from test_gpu_check import KEYS, _ref, _valid
    from test_gpu_replan import _queries, _source
    from uneven_planner_amd.alm_traj_opt import CHECK_OCC_BIT
    m = U.UnevenMap().build(base["xyz"])
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array([j for j in _valid(res) if res[j]["ret"] == 0], dtype=np.int32)
    lim = src.check_limits() * np.array([1.2, 1.2, 1.2, 1.2, 0.9, 1.5, 1.0])
    before = src.check(ok, limits=lim)
    offs, rows, _ = _ref(src, m, 0.01, 1)
    blk = lambda q: rows[int(offs[ok[q]]):int(offs[ok[q] + 1])]
    clean = np.nonzero(before["first_mask"] == 0)[0]
    assert clean.size >= 1
    v = int(clean[0])
    mine = blk(v)
    p0 = mine[mine.shape[0] // 2, 1:3].copy()
    box = (p0[0] - 0.5, p0[0] + 0.5, p0[1] - 0.5, p0[1] + 0.5)
    info = m.update(box, scan(box, seed=14, n_side=50, mound=0.35, sigma=0.09, centre=(p0[0] + 0.07, p0[1] + 0.07), extras=False))
    assert info["full_refit"] == 0 and info["n_changed"] > 0
    cx0, cx1, cy0, cy1 = info["changed"]
    cell = lambda p: (np.floor((p[:, 0] - m.map_origin[0]) / m.xy_resolution).astype(int), np.floor((p[:, 1] - m.map_origin[1]) / m.xy_resolution).astype(int))

    def near_changed(p, pad):
        ix, iy = cell(p)
        return (ix >= cx0 - pad) & (ix < cx1 + pad) & (iy >= cy0 - pad) & (iy < cy1 + pad)
    after = src.check(ok, limits=lim)
    inside = mine[near_changed(mine[:, 1:3], 2), 0]                # rows in `changed` and the cells interpolated with it
    assert inside.size > 0
    assert after["first_mask"][v] & ((1 << 4) | (1 << 5) | (1 << CHECK_OCC_BIT)), after["first_mask"][v]      # attitude, sigma or occupancy
    assert inside.min() <= after["first_t"][v] <= inside.max(), (after["first_t"][v], inside.min(), inside.max())
    far = [q for q in range(len(ok)) if not near_changed(blk(q)[:, 1:3], 2).any()]
    assert len(far) >= 8 and v not in far
    for k in KEYS:
        assert np.array_equal(after[k][far], before[k][far], equal_nan=True), k


def _refused(m, box, xyz, n):
    fp = C.POINTER(C.c_float)
    b = np.asarray(box, dtype=np.float32)
    info = U_lib().MapUpdateInfo()
    return m.L.uph_map_update(m.h, b.ctypes.data_as(fp), None if xyz is None else xyz.ctypes.data_as(fp), n, C.byref(info))


def U_lib():
    import uneven_planner_amd as U
    return U._lib


def test_refusals_leave_everything_as_it_was(base):
    import uneven_planner_amd as U
    new = np.ascontiguousarray(base["new"])
    INVALID = U._lib.UPH_ERR_INVALID

    def state(m, cloud=True):
        m.download()
        return _grids(m), (m.built_cloud() if cloud else None)

    def unchanged(m, s0, tag, cloud=True):
        s1 = state(m, cloud)
        if m.map_buffer is not None:
            _same_grids(s1[0], s0[0], tag)
        else:
            assert np.array_equal(s1[0]["occ_r2_buffer"], s0[0]["occ_r2_buffer"]), tag
        if cloud:
            assert np.array_equal(_bits(s1[1]), _bits(s0[1])), tag
    # no build yet
    m = U.UnevenMap()
    s0 = state(m, cloud=False)
    assert _refused(m, BOX, new, len(new)) == INVALID
    unchanged(m, s0, "no build", cloud=False)
    with pytest.raises(U._lib.UnevenHipError):
        m.built_cloud()
    # a slab build leaves no resident cloud either
    m.build(base["xyz"], x0=90, x1=110)
    s0 = state(m)
    assert _refused(m, BOX, new, len(new)) == INVALID
    unchanged(m, s0, "slab build")
    # bad arguments on a map that could be updated
    m.build(base["xyz"])
    s0 = state(m)
    _same_grids(s0[0], base["built"], "build")
    nan = float("nan")
    for tag, box, xyz, n in [("nan box", (nan, 0.61, -0.27, 0.49), new, len(new)), ("nan box y", (-0.43, 0.61, -0.27, nan), new, len(new)),
                             ("reversed x", (0.61, -0.43, -0.27, 0.49), new, len(new)), ("reversed y", (-0.43, 0.61, 0.49, -0.27), new, len(new)),
                             ("n < 0", BOX, new, -1), ("null cloud", BOX, None, 5), ("empties the cloud", (-20.0, 20.0, -20.0, 20.0), None, 0)]:
        assert _refused(m, box, xyz, n) == INVALID, tag
        unchanged(m, s0, tag)
    assert m.L.uph_map_update(m.h, None, None, 0, None) == INVALID and m.L.uph_map_update(None, None, None, 0, None) == INVALID
    # ... which it still can: the refusals ended nothing
    m.update(BOX, new)
    _same_grids(_grids(m), base["fresh1"], "update after the refusals")
    # after set_cells the cells no longer derive from the cloud
    m.set_cells(base["built"]["map_buffer"])
    s0 = state(m)
    assert _refused(m, BOX, new, len(new)) == INVALID
    unchanged(m, s0, "after set_cells")
    m.build_filtered(base["W"])
    m.commit()                                                      # a commit says "the cells were written by someone else"
    assert _refused(m, BOX, new, len(new)) == INVALID
    # f32 and tile maps
    from uneven_planner_amd import scenes
    f = U.UnevenMap(storage="f32")
    f.set_cells(scenes.analytic_cells())
    s0 = state(f, cloud=False)
    assert _refused(f, BOX, new, len(new)) == INVALID
    unchanged(f, s0, "f32", cloud=False)
    fp = C.POINTER(C.c_float)
    assert f.L.uph_map_build_filtered(f.h, base["W"].ctypes.data_as(fp), len(base["W"]), 0, NX) == INVALID
    t = U.UnevenMap(tile=(80, 120))
    t.build(base["xyz"], x0=80, x1=120, download=False)
    s0 = state(t)
    assert _refused(t, BOX, new, len(new)) == INVALID
    unchanged(t, s0, "tile")


ADAPTER_MAIN = r"""
#include <cstdio>
#include <vector>
#include "uneven_hip_adapter.hpp"
using namespace uneven_hip;
static std::vector<float> readf(std::FILE* f) { long long n = 0; if (std::fread(&n, 8, 1, f) != 1) return {}; std::vector<float> v((size_t)n); if (n && std::fread(v.data(), 4, (size_t)n, f) != (size_t)n) v.clear(); return v; }
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    const std::vector<float> W = readf(f), box = readf(f), scan = readf(f);
    std::fclose(f);
    uph_map_params mp = {2, 10.0, 10.0, 0.2, 0.1, 0.1, 0.05, 0.1, 0.8, 0.05, 9.81};      // plan_manager/params/run_hill.yaml:2-14
    UnevenMapHandle map(mp);
    map.buildFilteredMap(W.data(), (long)(W.size() / 3));
    uph_map_update_info info;
    map.updateMap(box.data(), scan, info);
    int32_t d[3];
    uph_map_dims(map.get(), d);
    const size_t ncell = (size_t)d[0] * d[1] * d[2];
    std::vector<double> cells(ncell * 4), c(ncell);
    std::vector<char> occ(ncell), occ2((size_t)d[0] * d[1]);
    map.download(cells.data(), c.data(), occ.data(), occ2.data());
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 4;
    std::fwrite(&info, sizeof(info), 1, o);
    std::fwrite(cells.data(), 8, cells.size(), o); std::fwrite(c.data(), 8, c.size(), o);
    std::fwrite(occ.data(), 1, occ.size(), o); std::fwrite(occ2.data(), 1, occ2.size(), o);
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_update_matches_ctypes_bit_for_bit(tmp_path, base):
    import uneven_planner_amd as U
    src = tmp_path / "update_main.cpp"
    src.write_text(ADAPTER_MAIN)
    exe = str(tmp_path / "update_main")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for a in (base["W"], np.asarray(BOX, dtype=np.float32), base["new"]):
            a = np.ascontiguousarray(a, dtype=np.float32)
            f.write(struct.pack("<q", a.size))
            f.write(a.tobytes())
    subprocess.check_call([exe, fin, fout])
    m = U.UnevenMap().build_filtered(base["W"])
    info = m.update(BOX, base["new"])
    raw = open(fout, "rb").read()
    I = U._lib.MapUpdateInfo.from_buffer_copy(raw[:C.sizeof(U._lib.MapUpdateInfo)])
    assert tuple(I.dirty) == info["dirty"] and tuple(I.changed) == info["changed"]
    for k in ("n_refit", "n_far", "n_changed", "full_refit", "n_removed", "n_added", "n_cloud"):
        assert int(getattr(I, k)) == info[k], k
    o = C.sizeof(U._lib.MapUpdateInfo)
    ncell = NX * NY * NYAW
    cells = np.frombuffer(raw, dtype=np.float64, count=ncell * 4, offset=o).reshape(-1, 4)
    c = np.frombuffer(raw, dtype=np.float64, count=ncell, offset=o + ncell * 32)
    occ = np.frombuffer(raw, dtype=np.int8, count=ncell, offset=o + ncell * 40)
    occ2 = np.frombuffer(raw, dtype=np.int8, count=NX * NY, offset=o + ncell * 41)
    assert len(raw) == o + ncell * 41 + NX * NY
    _same_grids(dict(map_buffer=cells, c_buffer=c, occ_buffer=occ, occ_r2_buffer=occ2), _grids(m), "adapter")
    _same_grids(_grids(m), base["fresh1"], "ctypes")
