"""CPU tier of the non-square grids (tests/grid_cases.py): the code the host and the device share -- HostGridView, terrain_dev.hpp and
solver_program.hpp through the emulator, the C-ABI's `.map` reader / writer, the slab plan of the multi-GPU build -- against the oracle on
grids with nx != ny and 38 / 64 / 65 / 127 yaw bins.  Green here means that a failure of tests/test_gpu_grids.py points at device-only code."""
import ctypes as C

import numpy as np
import pytest

import emu_bridge as E
import grid_cases as GC
from conftest import rel


def _emu(oracle, name):
    return E.Emu(GC.cells(name), oracle.map_params_vec(GC.map_params(name)), oracle.params_vec())


@pytest.mark.parametrize("name", GC.SMALL)
def test_lookups_of_the_emulator_and_the_host_view_match_the_oracle(oracle, name):
    """terrain_dev.hpp compiled for the host and HostGridView against the oracle's lookups at 1e-12 (the bar of test_emu_terrain_eval_scaling and
    test_host_grid_view_matches_oracle), on random points up to 0.2 m outside the border, the corners, the last row and column, the yaw seam and
    the overhanging strip; the points reach the first and the last x / y index and every yaw bin a lookup can reach"""
    from uneven_planner_amd.host_map import HostGridView
    nx, ny, nyaw = GC.check_dims(name)
    og = GC.oracle_grid(oracle, name)
    hv = HostGridView(GC.cells(name), **GC.map_params(name))
    GC.check_dims(name, og.dims, hv.voxel_num)
    pos = GC.lookup_points(name, n=1500, seed=5)
    v0, g0 = og.all_with_grad(pos)
    v1, g1 = _emu(oracle, name).terrain(pos)
    e = dict(emu_values=np.abs(v0 - v1).max(), emu_grads=np.abs(g0 - g1).max() / np.abs(g0).max())
    assert e["emu_values"] < 1e-12 and e["emu_grads"] < 1e-12, e
    inmap = np.array([hv.isInMap(p) for p in pos])
    assert 0.5 < inmap.mean() < 1.0 and np.all(g0[~inmap] == 0.0) and np.all(v0[~inmap] == v0[~inmap][0])      # outside the map: flat ground, no gradient
    ix, iy, w0, w1 = GC.lookup_corners(name, pos[inmap])
    lo, hi = GC.reachable_yaw_bins(name)
    vx, vy = GC.visited_xy(name, pos[inmap])
    assert {0, nx - 1} <= vx and {0, ny - 1} <= vy and ix.min() < 0 and iy.min() < 0           # (a lower corner below the grid: clamped)
    assert set(w0.tolist()) == set(range(lo, hi + 1)) and lo == 0 and hi >= nyaw - 2
    assert set(w1.tolist()) >= set(range(1, nyaw))
    sub = pos[:400]
    want = og.terrain(sub)
    got = np.array([hv.getTerrain(p) for p in sub])
    e["host_terrain"] = np.abs(want - got).max()
    ins = inmap[:400]
    e["host_variables"] = np.abs(og.terrain_variables(sub[ins]) - np.array([hv.getTerrainVariables(p) for p in sub[ins]])).max()
    assert e["host_terrain"] < 1e-12 and e["host_variables"] < 1e-12, e


@pytest.mark.parametrize("lanes", [64, 256])
@pytest.mark.parametrize("name", GC.SMALL)
def test_emulator_evaluation_and_scaling_match_the_oracle(oracle, name, lanes):
    """one evaluation with random duals and scales, and initScaling, of the workgroup program at test_emu_terrain_eval_scaling's bars: the three
    problems along the long axis (way-points beyond the short axis's half-length, asserted) and two random ones of the rectangle"""
    E.lib().emu_set_lanes(lanes)
    og = GC.oracle_grid(oracle, name)
    emu = _emu(oracle, name)
    probs = GC.optimiser_problems(name)[:5]
    assert sum(GC.beyond_short_half(name, p) for p in probs) >= 2 and len(probs) >= 4
    try:
        for i, prob in enumerate(probs):
            st = GC.state_for(prob, 300 + i)
            a = oracle.OracleALM(og)
            x0 = a.setup(prob)
            a.set_state(lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], scale_fx=st["scale_fx"])
            a.set_rho(st["rho"])
            f, g, _ = a.eval(x0)
            s = a.get_state()
            r = emu.run(0, prob, x0, lam=st["lam"], mu=st["mu"], scale_cx=st["scale_cx"], rho=st["rho"], scale_fx=st["scale_fx"])
            assert abs(f - r["f"]) / abs(f) < 1e-11, (name, i)
            assert rel(g, r["g"]) < 1e-10 and rel(s["hx"], r["hx"]) < 1e-10 and rel(s["gx"], r["gx"]) < 1e-10, (name, i)
            assert rel(a.coeffs()[0], r["c_xy"]) < 1e-11 and rel(a.coeffs()[1], r["c_yaw"]) < 1e-10, (name, i)
            a2 = oracle.OracleALM(og)
            x0 = a2.setup(prob)
            a2.init_scaling(x0)
            s2 = a2.get_state()
            r2 = emu.run(1, prob, x0)
            assert abs(s2["scale_fx"] - r2["scale_fx"]) / s2["scale_fx"] < 1e-10 and rel(s2["scale_cx"], r2["scale_cx"]) < 1e-10, (name, i)
    finally:
        E.lib().emu_set_lanes(256)                  # (the default of the scaffolding)


@pytest.mark.parametrize("name", ["tall", "one_over"])
def test_map_cache_of_the_c_abi_on_a_non_square_grid(tmp_path, oracle, name):
    """uph_map_save_csv / uph_map_load_csv / the side-car against the oracle's writer and reader (as
    test_map_cache_in_the_c_abi_against_the_oracle_and_the_mirror: same bytes, same doubles) where nx != ny != nyaw: lines in the last row, column
    and bin are kept, lines with ix = nx, iy = ny, iw = nyaw dropped -- and on `tall` lines with ix = ny - 1 (in range for y, out of range for x)
    and ix = ny"""
    import uneven_planner_amd as U
    L, OL = U._lib.load(), oracle.lib()
    nx, ny, nyaw = GC.check_dims(name)
    rng = np.random.default_rng(9)
    g = oracle.OracleGrid(**GC.GRIDS[name])
    GC.check_dims(name, g.dims)
    dims = (C.c_int32 * 3)(nx, ny, nyaw)
    cells = np.column_stack([rng.normal(size=g.ncell) * 10.0 ** rng.integers(-7, 3, g.ncell), rng.uniform(0, 0.2, g.ncell), rng.uniform(-0.3, 0.3, g.ncell),
                             rng.uniform(-0.3, 0.3, g.ncell)])
    g.set_cells(cells)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    p_or, p_c = str(tmp_path / "oracle.map"), str(tmp_path / "cabi.map")
    assert OL.orc_map_write_csv(g.h, p_or.encode()) == 0
    assert L.uph_map_save_csv(p_c.encode(), dp(np.ascontiguousarray(cells)), dims) == 0
    assert open(p_c, "rb").read() == open(p_or, "rb").read()
    got, cbuf, nl = np.full((g.ncell, 4), 7.0), np.zeros(g.ncell), C.c_int64(0)
    assert L.uph_map_load_csv(p_or.encode(), dims, dp(got), dp(cbuf), C.byref(nl)) == 0 and nl.value == g.ncell
    g2 = oracle.OracleGrid(**GC.GRIDS[name])
    assert OL.orc_map_read_csv(g2.h, p_c.encode()) == 0
    assert np.array_equal(got, g2.get_cells()[0]) and np.array_equal(cbuf, g2.get_cells()[1])
    # a partial, shuffled file plus hand-written lines at and beyond every index limit
    lines = open(p_c).read().splitlines()
    keep = [lines[i] for i in rng.permutation(len(lines))[: len(lines) // 5]]
    tail = ",1.5,0.25,0.125,-0.5"
    inside = [(nx - 1, ny - 1, nyaw - 1), (nx - 1, 0, 0), (0, ny - 1, 0), (0, 0, nyaw - 1)]
    outside = [(nx, 0, 0), (0, ny, 0), (0, 0, nyaw), (-1, 0, 0), (0, -1, 0)]
    if ny > nx:
        outside += [(ny - 1, 3, 1), (ny, 3, 1)]   # an x index that y could hold (and the first one y cannot): out of range for x
        inside.append((3, ny - 1, 1))
    else:
        outside.append((3, nx - 1, 1))            # in range for x, out of range for y
        inside.append((nx - 1, 3, 1))
    keep += ["%d,%d,%d" % t + tail for t in inside + outside] + ["3,4", ""]
    p_part = str(tmp_path / "partial.map")
    open(p_part, "w").write("\n".join(keep) + "\n")
    got2, c2 = np.full((g.ncell, 4), 7.0), np.zeros(g.ncell)
    assert L.uph_map_load_csv(p_part.encode(), dims, dp(got2), dp(c2), C.byref(nl)) == 0
    g3 = oracle.OracleGrid(**GC.GRIDS[name])
    assert OL.orc_map_read_csv(g3.h, p_part.encode()) == 0
    assert np.array_equal(got2, g3.get_cells()[0]) and np.array_equal(c2, g3.get_cells()[1])
    assert nl.value == len(lines) // 5 + len(inside)
    for (x, y, w) in inside:
        assert list(got2[(x * ny + y) * nyaw + w]) == [1.5, 0.25, 0.125, -0.5], (x, y, w)
    # side-car: bit exact; the transposed grid is another grid
    p_b = str(tmp_path / "cabi.map.bin")
    assert L.uph_map_save_bin(p_b.encode(), dp(np.ascontiguousarray(cells)), dims) == 0
    back = np.zeros((g.ncell, 4))
    assert L.uph_map_load_bin(p_b.encode(), dims, dp(back)) == 0 and np.array_equal(back, cells)
    assert L.uph_map_load_bin(p_b.encode(), (C.c_int32 * 3)(ny, nx, nyaw), dp(back)) == -4       # UPH_ERR_LIMIT


def test_slab_plan_of_42_rows():
    """`tall` has 42 rows: over four devices 11 + 11 + 11 + 9 (staged: 4 does not divide 42), over five 9 + 9 + 9 + 9 + 6"""
    import uneven_planner_amd as U
    from uneven_planner_amd.uneven_map import slab_bounds
    L = U._lib.load()
    for n, want, per_want in ((4, [(0, 11), (11, 22), (22, 33), (33, 42)], 11), (5, [(0, 9), (9, 18), (18, 27), (27, 36), (36, 42)], 9)):
        x0, x1, per, inpl = (C.c_int32 * n)(), (C.c_int32 * n)(), C.c_int32(0), C.c_int32(0)
        assert L.uph_multi_slab_plan(GC.DIMS["tall"][0], n, x0, x1, C.byref(per), C.byref(inpl)) == 0
        assert [(int(a), int(b)) for a, b in zip(x0, x1)] == want and per.value == per_want and inpl.value == 0
        assert want == [slab_bounds(42, r, n)[1:] for r in range(n)]
