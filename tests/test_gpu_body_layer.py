"""GPU tier of the body layer (uph_body_layer_*, csrc/body_occ.hip): the map's occupancy dilated by the vehicle's rectangle per yaw bin.

Every layer comparison is np.array_equal against the numpy mirror body_layer_rows fed get_cells' occ_r2 and the exported stencil: the kernel is integer
arithmetic on those two inputs, so there is no tolerance.  Maps are made with set_cells, flat with tilted columns (a column tilted beyond min_cnormal is
occupied at every yaw, as tests/test_gpu_footprint_check.py's _tilt_discs makes them).

B1: grids whose sides are no multiple of the kernel's tile and whose yaw count is odd, occupancies from empty to full, shapes from a point to a stencil wider
    than the grid, every `layers`.  B2: the hill map.  B3: update(rect) against a fresh build.  B4: freshness.  B5: set / get, fp32 cells, a far map.
B6: determinism.  B7: refusals on live objects.  B8: the C++ adapter against ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from uneven_planner_amd import _lib, body_layer as BL
from uneven_planner_amd.body_layer import FOOT_OCC_XY, FOOT_OUTSIDE, body_layer_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAR = (0.45, 0.15, 0.3)
BOTH = FOOT_OCC_XY | FOOT_OUTSIDE
# (map_size_x, map_size_y, yaw_resolution) -> 40 x 30 x 63 and 37 x 53 x 32
GRIDS = {"40x30x63": (dict(map_size_x=1.99, map_size_y=1.49, yaw_resolution=0.101), (40, 30, 63)),
         "37x53x32": (dict(map_size_x=1.84, map_size_y=2.64, yaw_resolution=0.2), (37, 53, 32))}
# the point, the car at its conservative margin (None), a thin long body, a stencil wider than the grid (R = 38 > 37 > 30)
SHAPES = (((0.0, 0.0, 0.0), 0.0), (CAR, None), ((0.9, 0.1, 0.02), 0.01), ((1.8, 1.8, 0.5), 0.0))


def _map(params=None, storage="f64"):
    import uneven_planner_amd as U
    return U.UnevenMap(params=params, storage=storage)


def _set_occ(m, occ2):
    """flat cells, the columns of occ2 [nx][ny] tilted beyond min_cnormal: occupied at every yaw"""
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    cells = np.zeros((nx, ny, nyaw, 4))
    cells[np.asarray(occ2, dtype=bool), :, 2] = 0.8
    m.set_cells(cells.reshape(-1, 4))
    got = m.occ_r2_buffer.reshape(nx, ny)
    assert np.array_equal(got != 0, np.asarray(occ2, dtype=bool))
    return got


def _mirror(layer, occ2, cache=None):
    key = (tuple(layer.shape), layer.margin)
    st = cache.get(key) if cache is not None else None
    if st is None:
        st = layer.stencil()
        if cache is not None:
            cache[key] = st
    assert st["R"] == layer.info()["R"]
    return body_layer_rows(occ2, st["lo"], st["hi"], layer.layers)


def _tilt_discs(m, centres, radius):
    """the columns whose centre lies within radius of one of the centres tilted beyond min_cnormal (tests/test_gpu_footprint_check.py's, in one upload)"""
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


def _occupancies(nx, ny):
    rng = np.random.default_rng(nx * 100 + ny)
    out = {"empty": np.zeros((nx, ny), dtype=bool), "full": np.ones((nx, ny), dtype=bool), "random": rng.uniform(size=(nx, ny)) < 0.05}
    for name, (a, b) in (("c00", (0, 0)), ("c01", (0, ny - 1)), ("c10", (nx - 1, 0)), ("c11", (nx - 1, ny - 1)), ("centre", (nx // 2, ny // 2))):
        o = np.zeros((nx, ny), dtype=bool)
        o[a, b] = True
        out[name] = o
    return out


@pytest.mark.parametrize("grid", list(GRIDS))
def test_grids_occupancies_shapes_and_layers_against_the_mirror(grid):
    """B1"""
    import uneven_planner_amd as U
    params, dims = GRIDS[grid]
    m = _map(params)
    assert tuple(int(v) for v in m.voxel_num) == dims
    nx, ny, nyaw = dims
    cache, n_set, Rs = {}, 0, set()
    for name, occ in _occupancies(nx, ny).items():
        occ2 = _set_occ(m, occ)
        for shape, margin in SHAPES:
            for layers in (FOOT_OCC_XY, FOOT_OUTSIDE, BOTH):
                layer = U.BodyLayer(m, shape, margin, layers)
                info = layer.info()
                assert info["fresh"] and info["dims"] == [nx, ny, nyaw] and info["layers"] == layers and np.array_equal(info["shape"], shape)
                got = layer.get()
                want = _mirror(layer, occ2, cache)
                assert np.array_equal(got, want), (grid, name, shape, layers, int((got != want).sum()))
                if shape == (0.0, 0.0, 0.0) and layers == FOOT_OCC_XY:
                    assert np.array_equal(got, np.repeat((occ2 != 0).astype(np.int8)[:, :, None], nyaw, axis=2))
                n_set += int(got.sum())
                Rs.add(info["R"])
                layer.close()
    assert n_set > 0 and max(Rs) > max(nx, ny) - 16 and min(Rs) == 1
    print("B1 %s: stencil radii %s" % (grid, sorted(Rs)))


@pytest.fixture(scope="module")
def hill():
    from uneven_planner_amd import scenes
    m = _map()
    cloud = scenes.make_hill_cloud()
    m.build(cloud)
    return m, cloud


def test_hill_map_against_the_mirror(hill):
    """B2"""
    import uneven_planner_amd as U
    m, _ = hill
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    # the hill as built is free everywhere (the band along the border is all the car's layer holds); a copy with discs tilted over it is not
    m2 = _map()
    m2.set_cells(m.map_buffer)
    rng = np.random.default_rng(12)
    near = _tilt_discs(m2, rng.uniform(-4.8, 4.8, (60, 2)), 0.12)
    for mm in (m, m2):
        occ2 = mm.occ_r2_buffer.reshape(nx, ny)
        car = U.BodyLayer(mm, CAR)
        assert abs(car.margin - 0.0624) < 2e-4 and car.info()["R"] == 13 and car.layers == BOTH
        got = car.get()
        assert np.array_equal(got, _mirror(car, occ2))
        assert got.sum() > np.count_nonzero(occ2) * nyaw and not got.all()
        point = U.BodyLayer(mm, (0.0, 0.0, 0.0), 0.0, FOOT_OCC_XY)
        assert np.array_equal(point.get(), np.repeat((occ2 != 0).astype(np.int8)[:, :, None], nyaw, axis=2))
        assert car.kernel_ms() > 0.0
        print("B2: %d occupied columns, car layer %d of %d bytes set, build kernel %.3f ms" % (np.count_nonzero(occ2), int(got.sum()), got.size, car.kernel_ms()))
    assert np.array_equal(m2.occ_r2_buffer.reshape(nx, ny) != 0, near | (m.occ_r2_buffer.reshape(nx, ny) != 0)) and near.sum() > 500


@pytest.mark.parametrize("rect", [(17, 18, 11, 12), (0, 6, 9, 21), (31, 40, 22, 30), (0, 40, 0, 30)], ids=["one-column", "border", "corner", "whole"])
def test_update_equals_a_fresh_build(rect):
    """B3: occupancy changed inside a rect (columns set and columns cleared), update(rect) against build, bit for bit; a layer that does not hear of the
    change keeps its bytes"""
    import uneven_planner_amd as U
    params, (nx, ny, nyaw) = GRIDS["40x30x63"]
    m = _map(params)
    rng = np.random.default_rng(sum(rect))
    occ = rng.uniform(size=(nx, ny)) < 0.05
    _set_occ(m, occ)
    # (the car's own layer is nearly all ones on a grid this small: it is held to the rebuild, the two smaller bodies also to having changed)
    layers = [U.BodyLayer(m, CAR), U.BodyLayer(m, (0.9, 0.1, 0.02), 0.01, FOOT_OCC_XY), U.BodyLayer(m, (0.2, 0.1, 0.1), 0.02)]
    before = [l.get() for l in layers]
    x0, x1, y0, y1 = rect
    occ[x0:x1, y0:y1] = ~occ[x0:x1, y0:y1] if (x1 - x0) * (y1 - y0) == 1 else rng.uniform(size=(x1 - x0, y1 - y0)) < 0.3
    occ2 = _set_occ(m, occ)
    for l, b in zip(layers, before):
        assert l.info()["behind"] == 1 and np.array_equal(l.get(), b)
        l.update(rect)
        assert l.info()["fresh"]
        got = l.get()
        assert l is layers[0] or not np.array_equal(got, b)
        fresh = U.BodyLayer(m, l.shape, l.margin, l.layers).get()
        assert np.array_equal(got, fresh) and np.array_equal(got, _mirror(l, occ2))
    # an empty rect is accepted and writes nothing
    keep = layers[0].get()
    layers[0].update((3, 3, 0, 5))
    assert np.array_equal(layers[0].get(), keep)


def test_update_after_a_real_map_update(hill):
    """B3, last case: uph_map_update on the hill cloud (tests/map_update_cases.py), info.changed as the rect"""
    import uneven_planner_amd as U
    import map_update_cases as MU
    m, cloud = hill
    nx, ny, nyaw = (int(v) for v in m.voxel_num)
    layer = U.BodyLayer(m, CAR)
    before = layer.get()
    try:
        info = m.update(MU.BOX, MU.scan(mound=0.6, sigma=0.07))
        assert info["n_changed"] > 0 and layer.info()["behind"] == 1
        occ2 = m.occ_r2_buffer.reshape(nx, ny)
        layer.update(info["changed"])
        got = layer.get()
        assert np.array_equal(got, U.BodyLayer(m, CAR).get()) and np.array_equal(got, _mirror(layer, occ2))
        print("B3 map update: changed rect %s, %d layer bytes differ, update kernel %.3f ms" % (info["changed"], int((got != before).sum()), layer.kernel_ms()))
    finally:
        m.build(cloud)          # the module's hill map as the other tests expect it


def test_freshness():
    """B4"""
    import uneven_planner_amd as U
    params, (nx, ny, nyaw) = GRIDS["37x53x32"]
    m = _map(params)
    occ = np.zeros((nx, ny), dtype=bool)
    occ[20, 30] = True
    _set_occ(m, occ)
    layer = U.BodyLayer(m, CAR)
    ka = U.KinoAstar(m, slots=2)
    ka.set_body_layer(layer)
    S, G = np.array([[-0.5, -0.9, 0.0]]), np.array([[0.5, 0.9, 0.0]])
    first = ka.plan_batch(S, G)[0]
    assert first["status"] in (0, 2, 3, 4)
    occ[5, 5] = True
    _set_occ(m, occ)
    assert layer.info()["behind"] == 1 and not layer.info()["fresh"]
    with pytest.raises(_lib.UnevenHipError, match="stale"):
        ka.plan_batch(S, G)
    occ[6, 6] = True
    _set_occ(m, occ)
    assert layer.info()["behind"] == 2
    keep = layer.get()
    with pytest.raises(_lib.UnevenHipError, match="rebuild"):
        layer.update((0, nx, 0, ny))
    assert np.array_equal(layer.get(), keep) and layer.info()["behind"] == 2
    layer.build()
    assert layer.info()["fresh"] and np.array_equal(layer.get(), _mirror(layer, m.occ_r2_buffer.reshape(nx, ny)))
    assert ka.plan_batch(S, G)[0]["status"] in (0, 2, 3, 4)
    ka.set_body_layer(None)
    _set_occ(m, occ)
    assert ka.plan_batch(S, G)[0]["status"] in (0, 2, 3, 4)          # the default search does not ask the layer
    ka.close()
    layer.close()


def test_set_get_and_other_storage():
    """B5: set / get round-trip; a layer on fp32 cells and on a map far from the origin in cells (a 4 km map: trajectories there are solved in local frames;
    the layer is on the map's own grid) equals the mirror"""
    import uneven_planner_amd as U
    params, (nx, ny, nyaw) = GRIDS["40x30x63"]
    rng = np.random.default_rng(8)
    occ = rng.uniform(size=(nx, ny)) < 0.05
    m = _map(params)
    _set_occ(m, occ)
    layer = U.BodyLayer(m, CAR)
    want = layer.get()
    mine = (rng.uniform(size=(nx, ny, nyaw)) < 0.3).astype(np.int8)
    for bad in (7, -1, 2):                              # the search reads `== 1`: another value is refused, nothing written
        odd = mine.copy()
        odd[nx - 1, ny - 1, nyaw - 1] = bad
        with pytest.raises(_lib.UnevenHipError, match="0 .free. or 1"):
            layer.set(odd)
        assert np.array_equal(layer.get(), want) and layer.info()["fresh"]
    layer.set(mine)
    assert np.array_equal(layer.get(), mine) and layer.info()["fresh"]
    layer.build()
    assert np.array_equal(layer.get(), want)
    with pytest.raises(AssertionError):
        layer.set(mine[:-1])
    m32 = _map(params, storage="f32")
    _set_occ(m32, occ)
    assert np.array_equal(U.BodyLayer(m32, CAR).get(), want)
    # a long thin map: 4000 x 12 columns at 1 m, occupancy at both far ends
    far = dict(map_size_x=3999.5, map_size_y=11.5, xy_resolution=1.0, yaw_resolution=0.4)
    mf = _map(far)
    fx, fy, fw = (int(v) for v in mf.voxel_num)
    assert (fx, fy, fw) == (4000, 12, 16)
    occf = np.zeros((fx, fy), dtype=bool)
    occf[[0, 1, 3998, 3999, 2000], [0, 11, 5, 11, 6]] = True
    occ2 = _set_occ(mf, occf)
    lf = U.BodyLayer(mf, (2.5, 0.5, 1.0), 0.0)
    assert np.array_equal(lf.get(), _mirror(lf, occ2))


def test_determinism_and_independent_layers():
    """B6"""
    import uneven_planner_amd as U
    params, (nx, ny, nyaw) = GRIDS["37x53x32"]
    m = _map(params)
    rng = np.random.default_rng(9)
    occ2 = _set_occ(m, rng.uniform(size=(nx, ny)) < 0.05)
    a = U.BodyLayer(m, CAR)
    b = U.BodyLayer(m, (0.9, 0.1, 0.02), 0.01, FOOT_OCC_XY)
    ga, gb = a.get(), b.get()
    for _ in range(3):
        a.build()
        b.build()
        assert np.array_equal(a.get(), ga) and np.array_equal(b.get(), gb)
    b.set(np.zeros_like(gb))
    assert np.array_equal(a.get(), ga)
    b.build()
    assert np.array_equal(b.get(), gb) and np.array_equal(ga, _mirror(a, occ2)) and np.array_equal(gb, _mirror(b, occ2)) and not np.array_equal(ga, gb)


def test_refusals_on_live_objects():
    """B7: a tile map, a layer of another map, destroy while in use, the limits, bad layers, bad rects -- nothing written"""
    import uneven_planner_amd as U
    L = _lib.load()
    params, (nx, ny, nyaw) = GRIDS["40x30x63"]
    m, other = _map(params), _map(params)
    sh = np.array(CAR)
    dp = lambda a: a.ctypes.data_as(_lib.DP)
    h = C.c_void_p()
    tile = U.UnevenMap(params=params, tile=(0, 20))
    assert L.uph_body_layer_create(tile.h, dp(sh), 0.05, BOTH, C.byref(h)) == _lib.UPH_ERR_INVALID and not h.value and b"tile" in L.uph_last_error()
    for layers in (0, 2, 3, 6, 7, 8, -1):
        assert L.uph_body_layer_create(m.h, dp(sh), 0.05, layers, C.byref(h)) == _lib.UPH_ERR_INVALID and not h.value, layers
    big, one_sided = np.array([3.0, 3.0, 1.0]), np.array([6.0, 0.0, 0.0])
    assert L.uph_body_layer_create(m.h, dp(big), 0.0, BOTH, C.byref(h)) == _lib.UPH_ERR_LIMIT and not h.value and b"2^14" in L.uph_last_error()
    assert L.uph_body_layer_create(m.h, dp(one_sided), 0.0, BOTH, C.byref(h)) == _lib.UPH_ERR_LIMIT and not h.value and b"UPH_BODY_MAX_R" in L.uph_last_error()
    for bad in (np.array([-0.1, 0.1, 0.1]), np.array([0.1, np.nan, 0.1])):
        assert L.uph_body_layer_create(m.h, dp(bad), 0.0, BOTH, C.byref(h)) == _lib.UPH_ERR_INVALID and not h.value
    assert L.uph_body_layer_create(m.h, dp(sh), -0.01, BOTH, C.byref(h)) == _lib.UPH_ERR_INVALID and not h.value
    layer, foreign = U.BodyLayer(m, CAR), U.BodyLayer(other, CAR)
    keep = layer.get()
    for rect in ((5, 4, 0, 3), (0, 3, 7, 6), (-1, 3, 0, 3), (0, nx + 1, 0, 3), (0, 3, -2, 3), (0, 3, 0, ny + 1)):
        with pytest.raises(_lib.UnevenHipError, match="rect"):
            layer.update(rect)
    assert np.array_equal(layer.get(), keep)
    ka = U.KinoAstar(m, slots=2)
    with pytest.raises(_lib.UnevenHipError, match="another map"):
        ka.set_body_layer(foreign)
    ka.set_body_layer(layer)
    with pytest.raises(_lib.UnevenHipError, match="still names"):
        layer.close()
    assert layer.h and np.array_equal(layer.get(), keep)
    ka2 = U.KinoAstar(m, slots=2)
    ka2.set_body_layer(layer)
    ka.set_body_layer(None)
    with pytest.raises(_lib.UnevenHipError, match="still names"):
        layer.close()
    ka2.close()                      # destroying the context releases the layer as well
    layer.close()
    assert layer.h is None
    foreign.close()


CPP = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
#include <cstdio>
using namespace uneven_hip;
int main(int argc, char** argv) {
    // in: {ncell}, cells (analytic terrain with tilted discs), then the second state's cells; out: four layers and two paths
    FILE* f = std::fopen(argv[1], "rb");
    long long ncell;
    if (!f || fread(&ncell, 8, 1, f) != 1) return 2;
    std::vector<double> cells((size_t)ncell * 4), cells2((size_t)ncell * 4);
    if (fread(cells.data(), 8, cells.size(), f) != cells.size() || fread(cells2.data(), 8, cells2.size(), f) != cells2.size()) return 2;
    std::fclose(f);
    uph_map_params mp = {2, 10.0, 10.0, 0.2, 0.1, 0.1, 0.05, 0.1, 0.8, 0.05, 9.81};
    UnevenMapHandle map(mp, 0);
    map.setCells(cells.data());
    const std::array<double, 3> car{0.45, 0.15, 0.3};
    const double mg = BodyLayer::conservativeMargin(mp, car);
    FILE* o = std::fopen(argv[2], "wb");
    {
        BodyLayer layer(map, car, mg);
        BodyLayer xy(map, car, 0.02, UPH_FOOT_OCC_XY);
        std::vector<char> a = layer.get(), b = xy.get();
        fwrite(a.data(), 1, a.size(), o);
        fwrite(b.data(), 1, b.size(), o);
        KinoAstar kino;
        kino.setEnvironment(&map);
        kino.setBodyLayer(&layer);
        std::array<double, 3> s{4.3, -4.3, 1.57}, g{1.0, -1.5, 2.36};
        std::vector<VecN<3>> p = kino.plan(s, g);
        double n = (double)p.size();
        fwrite(&n, 8, 1, o);
        for (const VecN<3>& q : p) { double r[3] = {q[0], q[1], q[2]}; fwrite(r, 8, 3, o); }
        map.setCells(cells2.data());
        const BodyLayer::Info i = layer.info();
        double st[3] = {(double)i.behind, (double)i.R, i.margin};
        fwrite(st, 8, 3, o);
        bool refused = false;
        try { kino.plan(s, g); } catch (const std::runtime_error&) { refused = true; }
        layer.update({60, 90, 60, 90});
        a = layer.get();
        fwrite(a.data(), 1, a.size(), o);
        xy.build();
        b = xy.get();
        fwrite(b.data(), 1, b.size(), o);
        double tail[2] = {refused ? 1.0 : 0.0, layer.info().fresh() ? 1.0 : 0.0};
        fwrite(tail, 8, 2, o);
        kino.setBodyLayer(nullptr);
    }
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_matches_ctypes_bit_for_bit(tmp_path, analytic_cells):
    """B8: uneven_hip::BodyLayer and KinoAstar::setBodyLayer from a compiled C++ consumer against the ctypes binding"""
    import struct
    import uneven_planner_amd as U
    rng = np.random.default_rng(31)
    cells = np.array(analytic_cells, dtype=np.float64).reshape(200, 200, -1, 4)
    xs = (np.arange(200) + 0.5) * 0.05 - 5.0
    near = np.zeros((200, 200), dtype=bool)
    for p in rng.uniform(-4.5, 4.5, (40, 2)):
        near |= np.hypot(xs[:, None] - p[0], xs[None, :] - p[1]) < 0.12
    near[170:200, 0:30] = near[105:135, 55:85] = False          # around the start (186, 14) and the goal (120, 70) of the adapter's query
    cells[near, :, 2], cells[near, :, 3] = 0.8, 0.0
    cells2 = cells.copy()
    cells2[70:80, 65:85, :, 2], cells2[70:80, 65:85, :, 3] = 0.8, 0.0          # a block inside the rect the consumer names
    cells, cells2 = np.ascontiguousarray(cells.reshape(-1, 4)), np.ascontiguousarray(cells2.reshape(-1, 4))
    src_ = tmp_path / "blayer.cpp"
    src_.write_text(CPP)
    exe = str(tmp_path / "blayer")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src_), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<q", cells.shape[0]))
        f.write(cells.tobytes())
        f.write(cells2.tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    m = U.UnevenMap()
    m.set_cells(cells)
    n = m.ncell
    layer, xy = U.BodyLayer(m, CAR), U.BodyLayer(m, CAR, 0.02, FOOT_OCC_XY)
    at = 0
    take = lambda k: np.frombuffer(raw[at:at + k], dtype=np.int8)
    assert np.array_equal(take(n), layer.get().ravel())
    at += n
    assert np.array_equal(take(n), xy.get().ravel()) and take(n).any()
    at += n
    ka = U.KinoAstar(m)
    ka.set_body_layer(layer)
    want = ka.plan([4.3, -4.3, 1.57], [1.0, -1.5, 2.36])
    npath = int(np.frombuffer(raw[at:at + 8], dtype=np.float64)[0])
    at += 8
    got = np.frombuffer(raw[at:at + 24 * npath], dtype=np.float64).reshape(npath, 3)
    at += 24 * npath
    assert npath == len(want) and np.array_equal(got, want)
    print("B8: the adapter's body-mode path has %d poses" % npath)
    st = np.frombuffer(raw[at:at + 24], dtype=np.float64)
    at += 24
    m.set_cells(cells2)
    info = layer.info()
    assert st.tolist() == [1.0, float(info["R"]), info["margin"]] and info["behind"] == 1
    layer.update((60, 90, 60, 90))
    xy.build()
    assert np.array_equal(take(n), layer.get().ravel()) and np.array_equal(layer.get(), U.BodyLayer(m, CAR).get())
    at += n
    assert np.array_equal(take(n), xy.get().ravel())
    at += n
    assert np.frombuffer(raw[at:at + 16], dtype=np.float64).tolist() == [1.0, 1.0] and at + 16 == len(raw)
