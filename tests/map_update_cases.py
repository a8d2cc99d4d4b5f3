"""Inputs and numpy mirrors shared by the map-update tests (tests/test_map_update_cpu.py, tests/test_gpu_map_update.py) and tools/map_update_*.py:
the box and scan of the one-update case, the resident cloud W' as the issue of uph_map_update defines it, and the refit rect written literally."""
import math

import numpy as np

BOX = (-0.43, 0.61, -0.27, 0.49)


def in_box(xyz, box):
    """closed box {x_min, x_max, y_min, y_max}, compared in float32 as the device compares"""
    b = np.asarray(box, dtype=np.float32)
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (p[:, 0] >= b[0]) & (p[:, 0] <= b[1]) & (p[:, 1] >= b[2]) & (p[:, 1] <= b[3])


def scan(box=BOX, seed=11, n_side=52, mound=0.25, sigma=0.09, centre=None, extras=True):
    """a scan of the box: n_side x n_side jittered lattice over it on hill_height plus a Gaussian mound (height `mound`, width `sigma`) at `centre`
    (default: the box centre); with extras five points inside one 1 cm leaf, points outside the box and one NaN point"""
    from uneven_planner_amd import scenes
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = (float(v) for v in box)
    cx, cy = (0.5 * (x0 + x1), 0.5 * (y0 + y1)) if centre is None else centre
    ii, jj = np.meshgrid(np.arange(n_side), np.arange(n_side), indexing="ij")
    x = x0 + (ii + rng.random(ii.shape)) * (x1 - x0) / n_side
    y = y0 + (jj + rng.random(jj.shape)) * (y1 - y0) / n_side
    h = lambda x, y: scenes.hill_height(x, y) + mound * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma ** 2))
    pts = np.stack([x.ravel(), y.ravel(), h(x, y).ravel()], axis=1)
    if extras:
        lx, ly = cx + 0.2034, cy - 0.1512                     # five points of one leaf: x, y and z each stay inside one centimetre
        lz = math.floor(h(lx, ly) * 100.0) / 100.0 + 0.002
        leaf = np.array([[lx + 0.001 * k, ly + 0.0005 * k, lz + 0.001 * k] for k in range(5)])
        out = np.array([[x1 + 0.3, cy, 0.5], [x0 - 0.02, y0 - 0.02, 0.4], [cx, y1 + 1.0, 0.6], [7.0, 7.0, 0.4]])
        out[:, 2] = h(out[:, 0], out[:, 1])
        nan = np.array([[cx, np.nan, 0.5]])
        pts = np.concatenate([pts[:1000], leaf, out[:2], nan, pts[1000:], out[2:]])
    return pts.astype(np.float32)


def merged(W, box, new, filter_cloud):
    """W' = (W without the points whose (x, y) lie in the box, order kept) ++ filter_cloud(points of new that are finite and lie in the box)"""
    W = np.asarray(W, dtype=np.float32).reshape(-1, 3)
    kept = W[~in_box(W, box)]
    if new is None or len(new) == 0:
        return kept
    new = np.asarray(new, dtype=np.float32).reshape(-1, 3)
    sel = new[in_box(new, box) & np.isfinite(new).all(axis=1)]
    if len(sel) == 0:
        return kept
    return np.concatenate([kept, filter_cloud(sel)])


def rect_rule(params, box):
    """uph_map_update_rect written literally: column x belongs when box[0] - Rm <= (x + 0.5) res + origin_x <= box[1] + Rm in double, Rm = (double)Rst + res,
    Rst = (float)(0.12 + max ellipsoid) + 1e-3f; (x0, x1, y0, y1) half-open, zeros when empty"""
    res = float(params["xy_resolution"])
    rst = np.float32(0.12 + max(params["ellipsoid_x"], params["ellipsoid_y"], params["ellipsoid_z"])) + np.float32(1.0e-3)
    assert rst.dtype == np.float32
    rm = float(rst) + res
    b = [float(v) for v in np.asarray(box, dtype=np.float32)]
    out = []
    for lo, hi, size in ((b[0], b[1], params["map_size_x"]), (b[2], b[3], params["map_size_y"])):
        n = int(math.ceil(size / res))
        c = (np.arange(n) + 0.5) * res + (-size / 2.0)
        idx = np.nonzero((lo - rm <= c) & (c <= hi + rm))[0]
        out.append((int(idx[0]), int(idx[-1]) + 1) if idx.size else None)
    if out[0] is None or out[1] is None:
        return (0, 0, 0, 0)
    return out[0] + out[1]
