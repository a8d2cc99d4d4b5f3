"""Non-square grids and yaw bin counts other than 64 (TEST INFRASTRUCTURE), shared by tests/test_grids_cpu.py and tests/test_gpu_grids.py.

Every other test of the suite runs on a square grid with 64 yaw bins, where a transposed nx / ny and a yaw loop that assumes one trip of a
full wave are invisible.  The grids here have nx != ny, sizes that are no multiple of the resolution, and 38 / 65 / 127 yaw bins: a wave with
idle lanes, a second trip of one lane, a second trip of 63 lanes.

    name       size x * y [m]   xy_res   yaw_res   nx * ny * nyaw
    wide       6.0 * 3.5        0.05     0.1       120 * 70 * 64     nx > ny, the shipped yaw count
    tall       2.9 * 5.3        0.07     0.17      42 * 76 * 38      ny > nx, the last cell overhangs the boundary, 26 idle lanes, 42 rows over 4 slabs
    fine       3.0 * 4.0        0.05     0.05      60 * 80 * 127     two trips of the yaw loop, the second with 63 lanes
    one_over   3.5 * 2.0        0.05     0.0989    70 * 40 * 65      a second trip of one lane
    far        96 * 24          0.25     0.17      384 * 96 * 38     beyond FRAME_EXTENT on x only: local frames on a non-square grid

DIMS is what the tests expect; they assert it against scenes.grid_dims, the oracle's dims and the map's voxel_num and trust none of them.
This module holds no fixtures: the callers hand in the `oracle` module.  Generators draw from the RECTANGLE (scenes.random_problems draws
from a square); their streams are their own."""
import math

import numpy as np

GRIDS = {
    "wide": dict(size_x=6.0, size_y=3.5, xy_res=0.05, yaw_res=0.1),
    "tall": dict(size_x=2.9, size_y=5.3, xy_res=0.07, yaw_res=0.17),
    "fine": dict(size_x=3.0, size_y=4.0, xy_res=0.05, yaw_res=0.05),
    "one_over": dict(size_x=3.5, size_y=2.0, xy_res=0.05, yaw_res=0.0989),
    "far": dict(size_x=96.0, size_y=24.0, xy_res=0.25, yaw_res=0.17),
}
DIMS = {"wide": (120, 70, 64), "tall": (42, 76, 38), "fine": (60, 80, 127), "one_over": (70, 40, 65), "far": (384, 96, 38)}
SMALL = ("wide", "tall", "fine", "one_over")
YAW_SPAN = 2.0 * math.pi + 5e-2                  # uneven_map.cpp:96

_CACHE = {}
MEASURED = {}                                    # (test, grid) -> {quantity: worst error}: filled by record(), written by write_report()


def map_params(name, **extra):
    """the map parameter block of a grid (the keys of HILL_MAP_PARAMS that differ from run_hill.yaml)"""
    g = GRIDS[name]
    return dict(map_size_x=g["size_x"], map_size_y=g["size_y"], xy_resolution=g["xy_res"], yaw_resolution=g["yaw_res"], **extra)


def origin(name):
    g = GRIDS[name]
    return -g["size_x"] / 2.0, -g["size_y"] / 2.0, -YAW_SPAN / 2.0


def cells(name):
    """scenes.analytic_cells on this grid's geometry (once per process; read only)"""
    if ("cells", name) not in _CACHE:
        from uneven_planner_amd import scenes
        c = scenes.analytic_cells(**GRIDS[name])
        c.setflags(write=False)
        _CACHE[("cells", name)] = c
    return _CACHE[("cells", name)]


def oracle_grid(O, name, grid_cells=None):
    """the oracle's grid of this geometry holding `grid_cells` (default: the analytic cells); a new object per call"""
    og = O.OracleGrid(**GRIDS[name])
    og.set_cells(cells(name) if grid_cells is None else grid_cells)
    return og


def check_dims(name, *others):
    """DIMS[name] against scenes.grid_dims and every (nx, ny, nyaw) triple handed in"""
    from uneven_planner_amd import scenes
    want = DIMS[name]
    assert scenes.grid_dims(**GRIDS[name]) == want, (name, scenes.grid_dims(**GRIDS[name]))
    for d in others:
        assert tuple(int(v) for v in d) == want, (name, tuple(d), want)
    return want


def halves(name):
    """(long axis 0 / 1, half-length of the long axis, half-length of the short axis)"""
    g = GRIDS[name]
    ax = 0 if g["size_x"] > g["size_y"] else 1
    return ax, 0.5 * max(g["size_x"], g["size_y"]), 0.5 * min(g["size_x"], g["size_y"])


# ---- indices written literally (coverage conditions: never taken from the library) ---------------------------------------------------------
def lookup_corners(name, pos):
    """(ix, iy, w0, w1) of the interpolation corners of uneven_map.h:268-284 for positions inside the map with yaw in [-pi, pi]: the lower
    corner's unclamped x / y index and the two yaw bins"""
    g = GRIDS[name]
    ox, oy, ow = origin(name)
    nyaw = DIMS[name][2]
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    wm = pos[:, 2] - 0.5 * g["yaw_res"]
    wm = np.where(wm < -math.pi, wm + 2.0 * math.pi, wm)
    ix = np.floor((pos[:, 0] - 0.5 * g["xy_res"] - ox) / g["xy_res"]).astype(np.int64)
    iy = np.floor((pos[:, 1] - 0.5 * g["xy_res"] - oy) / g["xy_res"]).astype(np.int64)
    iw = np.floor((wm - ow) / g["yaw_res"]).astype(np.int64)
    return ix, iy, iw % nyaw, (iw + 1) % nyaw


def visited_xy(name, pos):
    """the sets of x and of y indices the eight corners of the lookups at `pos` read (boundIndex clamps both corners, uneven_map.h:398-409).  On
    `tall` the centre of the last cell lies beyond the boundary, so nx - 1 and ny - 1 are only ever the UPPER corner."""
    nx, ny, _ = DIMS[name]
    ix, iy, _, _ = lookup_corners(name, pos)
    vx = set(np.clip(ix, 0, nx - 1).tolist()) | set(np.clip(ix + 1, 0, nx - 1).tolist())
    vy = set(np.clip(iy, 0, ny - 1).tolist()) | set(np.clip(iy + 1, 0, ny - 1).tolist())
    return vx, vy


def reachable_yaw_bins(name):
    """the yaw bins a lookup can have as its LOWER corner: wm = normSO2(yaw - res / 2) lies in [-pi, pi], so bins whose lower edge lies above
    pi are never w0 (one_over: bin 64 starts at 3.163) -- and then bin 0 is never w1"""
    g = GRIDS[name]
    ow = origin(name)[2]
    lo = int(math.floor((-math.pi - ow) / g["yaw_res"]))
    hi = int(math.floor((math.pi - ow) / g["yaw_res"]))
    return lo, min(hi, DIMS[name][2] - 1)


def cell_index(name, pos):
    """posToIndex (uneven_map.h:411-418), unclamped"""
    g = GRIDS[name]
    ox, oy, ow = origin(name)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    return (np.floor((pos[:, 0] - ox) / g["xy_res"]).astype(np.int64), np.floor((pos[:, 1] - oy) / g["xy_res"]).astype(np.int64),
            np.floor((pos[:, 2] - ow) / g["yaw_res"]).astype(np.int64))


# ---- query points --------------------------------------------------------------------------------------------------------------------------
def lookup_points(name, n=5000, seed=11, beyond=0.2, yaw_lim=math.pi):
    """n random poses up to `beyond` metres outside the border on every side, then the hand-placed ones: the four corners at +-(size / 2 - 5e-5),
    the last row and the last column, the yaw seam, and (where size / res is no integer) the strip the last cell overhangs"""
    g = GRIDS[name]
    hx, hy = 0.5 * g["size_x"], 0.5 * g["size_y"]
    nx, ny, nyaw = DIMS[name]
    ox, oy, _ = origin(name)
    res = g["xy_res"]
    rng = np.random.default_rng(seed)
    pos = np.column_stack([rng.uniform(-hx - beyond, hx + beyond, n), rng.uniform(-hy - beyond, hy + beyond, n), rng.uniform(-yaw_lim, yaw_lim, n)])
    e = 5e-5
    hand = [[sx * (hx - e), sy * (hy - e), w] for sx in (-1, 1) for sy in (-1, 1) for w in (0.3, -2.9)]
    # inside the last row / column (cell centres of index n - 1 lie at most half a cell below the border) and inside the first
    for t in np.linspace(-0.9, 0.9, 7):
        hand += [[min(ox + (nx - 0.75) * res, hx - 2e-4), t * hy, 1.1 * t], [t * hx, min(oy + (ny - 0.75) * res, hy - 2e-4), -2.0 * t],
                 [ox + 0.3 * res, t * hy, 0.7], [t * hx, oy + 0.3 * res, -0.7]]
    # the yaw seam: wm = yaw - res / 2 wraps below -pi; the last reachable bin as w0, the first as w0
    hr = 0.5 * g["yaw_res"]
    for w in (-3.095, 3.095, -3.14159, 3.14159, -math.pi + hr - 0.003, -math.pi + hr + 0.003, math.pi - 1e-9, -math.pi + 1e-9):
        hand += [[0.1, -0.2, w], [-0.37 * hx, 0.41 * hy, w]]
    # the overhanging strip: between the boundary and the far edge of the last cell there is no map; just inside the boundary the lower corner
    # is the last cell or the one before it
    for t in (-0.8, 0.0, 0.8):
        hand += [[hx - 1.5e-4, t * hy, 0.2], [t * hx, hy - 1.5e-4, 0.2], [hx - 0.4 * res, t * hy, -1.0], [t * hx, hy - 0.4 * res, 2.0]]
    hand = np.array(hand)
    hand[:, 2] = np.clip(hand[:, 2], -yaw_lim, yaw_lim)
    pos[:len(hand)] = hand
    return pos


def frontend_points(name, n=5000, seed=23):
    """lookup_points with yaws up to 3.4 (isOccupancy indexes the raw yaw: bins up to nyaw - 1 and beyond) plus the seam values +-3.17"""
    pos = lookup_points(name, n, seed, yaw_lim=3.4)
    k = n - 8
    pos[k:k + 4, :2] = [[0.1, -0.2], [0.1, -0.2], [-0.3, 0.25], [-0.3, 0.25]]
    pos[k:k + 4, 2] = [3.17, -3.17, 3.17, -3.17]
    return pos


# ---- problems and search queries over the rectangle ----------------------------------------------------------------------------------------
def rect_problems(name, n, seed0=7000, margin=0.3, pieces=(5, 25), **mk):
    """one PCG64 stream per problem (seed0 + i): start, goal ~ U(rectangle shrunk by `margin`), yaws ~ U(-pi, pi); accepted when the resampled path
    has pieces[0] .. pieces[1] position pieces"""
    from uneven_planner_amd.resample import make_problem
    g = GRIDS[name]
    hx, hy = 0.5 * g["size_x"] - margin, 0.5 * g["size_y"] - margin
    out = []
    for i in range(n):
        rng = np.random.Generator(np.random.PCG64(seed0 + i))
        while True:
            s = (rng.uniform(-hx, hx), rng.uniform(-hy, hy), rng.uniform(-math.pi, math.pi))
            e = (rng.uniform(-hx, hx), rng.uniform(-hy, hy), rng.uniform(-math.pi, math.pi))
            p = make_problem(s, e, **mk)
            if pieces[0] <= p["inner_xy"].shape[1] + 1 <= pieces[1]:
                out.append(p)
                break
    return out


def long_axis_problems(name, margin=0.3):
    """three problems that run along the LONG axis from end to end (both diagonals and the middle line), so that their way-points lie beyond the
    half-length of the short axis: an index computed with the wrong dimension leaves the grid there"""
    from uneven_planner_amd.resample import make_problem
    ax, hl, hs = halves(name)
    a, b = hl - margin, hs - margin
    ends = [((-a, -b), (a, b)), ((a, -0.5 * b), (-a, 0.6 * b)), ((-a, 0.2 * b), (a, -0.1 * b))]
    out = []
    for (l0, s0), (l1, s1) in ends:
        p0, p1 = ((l0, s0), (l1, s1)) if ax == 0 else ((s0, l0), (s1, l1))
        th = math.atan2(p1[1] - p0[1], p1[0] - p0[0])
        out.append(make_problem((p0[0], p0[1], th + 0.3), (p1[0], p1[1], th - 0.4)))
    return out


def leaving_problems(name):
    """two problems that leave the map: one over the border at the end of the long axis (the SHORT border), one over the long border"""
    from uneven_planner_amd.resample import make_problem
    ax, hl, hs = halves(name)
    over_short = ((hl - 0.9, 0.3 * hs), (hl + 0.5, 0.5 * hs))          # (along, across)
    over_long = ((0.2 * hl, hs - 0.8), (0.5 * hl, hs + 0.45))
    out = []
    for (l0, s0), (l1, s1) in (over_short, over_long):
        p0, p1 = ((l0, s0), (l1, s1)) if ax == 0 else ((s0, l0), (s1, l1))
        th = math.atan2(p1[1] - p0[1], p1[0] - p0[0])
        out.append(make_problem((p0[0], p0[1], th + 0.1), (p1[0], p1[1], th + 0.2)))
    return out


def way_points(prob):
    """(2, Nxy + 1): start, inner way-points, end"""
    return np.concatenate([np.asarray(prob["init_xy"])[:, :1], np.asarray(prob["inner_xy"]).reshape(2, -1), np.asarray(prob["end_xy"])[:, :1]], axis=1)


def beyond_short_half(name, prob):
    """does a way-point lie further along the long axis than the short axis's half-length?"""
    ax, _, hs = halves(name)
    return bool(np.abs(way_points(prob)[ax]).max() > hs)


def leaves_map(name, prob):
    g = GRIDS[name]
    w = way_points(prob)
    return bool(np.abs(w[0]).max() > 0.5 * g["size_x"]), bool(np.abs(w[1]).max() > 0.5 * g["size_y"])


def optimiser_problems(name):
    """the eight problems of the optimiser tests: three along the long axis, three random ones, one leaving over each border"""
    if ("opt", name) not in _CACHE:
        _CACHE[("opt", name)] = long_axis_problems(name) + rect_problems(name, 3, seed0=7100 + 10 * SMALL.index(name)) + leaving_problems(name)
    return _CACHE[("opt", name)]


def state_for(prob, seed, int_K=16):
    """deterministic duals and scales (piece_sweep.sweep_state's rule): lambda ~ 0.1 N(0, 1), mu >= 0 with about 30 % zeros, scales in [0.2, 1]"""
    rng = np.random.default_rng(int(seed))
    S = (prob["inner_xy"].shape[1] + 1) * (int_K + 1)
    return dict(lam=rng.normal(size=S) * 0.1, mu=np.abs(rng.normal(size=6 * S)) * 0.1 * (rng.uniform(size=6 * S) < 0.7),
                scale_cx=rng.uniform(0.2, 1.0, size=7 * S), scale_fx=0.37, rho=3.0)


BLOCK_HALF = (0.35, 0.3)                          # half-extent (along, across) of the occupied block of the search scene


def search_cells(name):
    """the analytic cells with a block in the middle whose sigma lies above max_rho: occupied in every yaw bin"""
    if ("search", name) not in _CACHE:
        nx, ny, nyaw = DIMS[name]
        g = GRIDS[name]
        ax = halves(name)[0]
        c = np.array(cells(name)).reshape(nx, ny, nyaw, 4)
        hx, hy = (BLOCK_HALF if ax == 0 else BLOCK_HALF[::-1])
        i0, i1 = int((0.5 * g["size_x"] - hx) / g["xy_res"]), int(math.ceil((0.5 * g["size_x"] + hx) / g["xy_res"]))
        j0, j1 = int((0.5 * g["size_y"] - hy) / g["xy_res"]), int(math.ceil((0.5 * g["size_y"] + hy) / g["xy_res"]))
        c[i0:i1, j0:j1, :, 1] = 0.2
        c = c.reshape(-1, 4)
        c.setflags(write=False)
        _CACHE[("search", name)] = c
    return _CACHE[("search", name)]


def search_queries(name, n=16, margin=0.3):
    """n start / goal pairs ACROSS the long axis around the block: starts on one side of it, goals on the other, alternating sides, spread over the
    short axis; headings roughly towards the goal"""
    ax, hl, hs = halves(name)
    rng = np.random.default_rng(900 + SMALL.index(name))
    S, G = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        sgn = 1.0 if i % 2 == 0 else -1.0
        l0, l1 = -sgn * rng.uniform(0.55 * hl, hl - margin), sgn * rng.uniform(0.55 * hl, hl - margin)
        s0, s1 = rng.uniform(-(hs - margin), hs - margin), rng.uniform(-(hs - margin), hs - margin)
        p0, p1 = ((l0, s0), (l1, s1)) if ax == 0 else ((s0, l0), (s1, l1))
        th = math.atan2(p1[1] - p0[1], p1[0] - p0[0])
        S[i] = [p0[0], p0[1], th + rng.uniform(-0.6, 0.6)]
        G[i] = [p1[0], p1[1], th + rng.uniform(-0.6, 0.6)]
    S[:, 2] = np.arctan2(np.sin(S[:, 2]), np.cos(S[:, 2]))
    G[:, 2] = np.arctan2(np.sin(G[:, 2]), np.cos(G[:, 2]))
    return S, G


# ---- the records -----------------------------------------------------------------------------------------------------------------------------
def record(test, grid, errs):
    """keep the worst value per quantity of a (test, grid); errs: {quantity: value}.  Returns errs."""
    slot = MEASURED.setdefault((str(test), str(grid)), {})
    for q, e in errs.items():
        slot[q] = max(float(e), slot.get(q, -math.inf))
    return errs


def write_report(path, header=""):
    """the worst error of every (test, grid) recorded in this process"""
    with open(path, "w") as fh:
        if header:
            fh.write(header.rstrip("\n") + "\n")
        fh.write("%-30s %-9s %s\n" % ("test", "grid", "worst value of every quantity"))
        for (test, grid), per_q in sorted(MEASURED.items()):
            fh.write("%-30s %-9s %s\n" % (test, grid, "  ".join("%s %.3g" % (k, v) for k, v in sorted(per_q.items()))))
