"""Cost of the clearance layer: python tools/clearance_probe.py [Q = 4096] [out.json = profiles/clearance_probe.json] [repeats = 15]
The hill map with 60 discs of 0.12 m tilted over it; the car (0.45 + 0.15 m x 2 * 0.3 m) at its conservative margin as the body layer; 64 hill goals planned and
solved on the map before the discs.  `repeats` rounds after a warm-up round, the calls alternated inside a round:
  build    ClearanceLayer.build() at rmax 20 and 64      -- both passes over the whole grid: HIP events around the two launches, and the wall clock of the call
  update   ClearanceLayer.update(a 20 x 20 rect)         -- pass 1 over the rect's rows, pass 2 over the rect grown by rmax
  query    ALMTrajOpt.clearance over Q windows           -- uph_clearance_check_kernel, kernel milliseconds and the wall clock of the blocking call
  context  ALMTrajOpt.footprint_check over the same windows at margin 0.05, all layers: what one margin of the question costs without the field
Median (min - max) of every series goes to the JSON.  Nothing is asserted."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402
from uneven_planner_amd.clearance import CLEAR_FAR, clearance_rows      # noqa: E402

args = sys.argv[1:]
Q = int(args[0]) if len(args) > 0 else 4096
OUT = args[1] if len(args) > 1 else os.path.join("profiles", "clearance_probe.json")
REP = max(3, int(args[2])) if len(args) > 2 else 15
CAR, RECT, RMAX = np.array([0.45, 0.15, 0.3]), (90, 110, 90, 110), (20, 64)
m = U.UnevenMap()
m.build(scenes.make_hill_cloud())
nx, ny, nyaw = (int(v) for v in m.voxel_num)
ka = U.KinoAstar(m)
S, G = scenes.random_queries(64, seed0=14000, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]))
opt = U.ALMTrajOpt(m)
opt.set_rho(1.0)
plan = opt.plan_goals(ka, S, G)
live = np.array([p["traj_of"] for p in plan if p["status"] == 0 and p["ret"] != 4], dtype=np.int32)
offs, rows = opt.rollout(1.0, 1, with_end=True)
total = rows[offs[1:] - 1, 0]
# the discs: tilted columns, set after the solve (the trajectories stay resident; the queries read the map as it is now)
rng = np.random.default_rng(12)
cells = np.array(m.map_buffer, dtype=np.float64).reshape(nx, ny, nyaw, 4)
xs = (np.arange(nx) + 0.5) * m.xy_resolution + m.map_origin[0]
ys = (np.arange(ny) + 0.5) * m.xy_resolution + m.map_origin[1]
near = np.zeros((nx, ny), dtype=bool)
for p in rng.uniform(-4.8, 4.8, (60, 2)):
    near |= np.hypot(xs[:, None] - p[0], ys[None, :] - p[1]) < 0.12
cells[near, :, 2], cells[near, :, 3] = 0.8, 0.0
m.set_cells(cells.reshape(-1, 4))
car = U.BodyLayer(m, CAR)
layers = {r: U.ClearanceLayer(car, r) for r in RMAX}
tr = live[np.arange(Q) % len(live)]
tf = rng.uniform(0.0, 0.5, Q) * total[tr]
tt = tf + rng.uniform(0.1, 0.5, Q) * total[tr]
rec = {"build": U._lib.build_id(), "grid": [nx, ny, nyaw], "shape": CAR.tolist(), "margin": car.margin, "R": car.info()["R"], "values": nx * ny * nyaw,
       "update_rect": list(RECT), "repeats": REP, "queries": Q, "trajectories": int(len(live))}
body = car.get()
for r, l in layers.items():
    got = l.get()
    rec["rmax_%d_equals_mirror" % r] = bool(np.array_equal(got, clearance_rows(body, r)))
    rec["rmax_%d_far_values" % r] = int((got == CLEAR_FAR).sum())


def series(runs):
    a = np.array(runs, dtype=np.float64)
    return {"runs": [round(float(v), 4) for v in a], "median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


t = {}
for rnd in range(REP + 1):
    row = {}
    for r, l in layers.items():
        row["build_rmax%d_call_ms" % r] = timed(l.build)
        row["build_rmax%d_kernel_ms" % r] = l.kernel_ms()
        row["update_rmax%d_call_ms" % r] = timed(lambda: l.update(RECT))
        row["update_rmax%d_kernel_ms" % r] = l.kernel_ms()
    out = {}
    row["query_call_ms"] = timed(lambda: out.update(opt.clearance(layers[20], tr, below2=16, t_from=tf, t_to=tt)))
    row["query_kernel_ms"] = opt.clearance_kernel_ms()
    fc = {}
    row["footprint_check_call_ms"] = timed(lambda: fc.update(opt.footprint_check(tr, CAR, 0.05, tf, tt)))
    row["footprint_check_kernel_ms"] = opt.footprint_check_kernel_ms()
    if rnd > 0:
        for k, v in row.items():
            t.setdefault(k, []).append(v)
for k, v in t.items():
    rec[k] = series(v)
rec["query_samples"] = int(out["counts"][:, 0].sum())
rec["query_below_0.2m"] = int(out["counts"][:, 1].sum())
rec["footprint_check_hit_samples"] = int(fc["counts"][:, 1].sum())
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print("clearance probe, build %s: grid %s, body R %d, %d queries over %d trajectories, %d samples; equals mirror: %s" % (
    rec["build"], rec["grid"], rec["R"], Q, len(live), rec["query_samples"], [rec["rmax_%d_equals_mirror" % r] for r in RMAX]))
for k in t:
    print("  %-28s %.3f (%.3f - %.3f) ms" % (k, rec[k]["median"], rec[k]["min"], rec[k]["max"]))
