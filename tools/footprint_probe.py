"""Cost of the oriented-rectangle footprints against the discs: python tools/footprint_probe.py [B = 4096] [out.json] [repeats = 15]
Source: B hill goals planned and solved by ALMTrajOpt.plan_goals, as tools/delay_probe.py; the valid resident trajectories are the fleet.  Vehicle i starts at
t0[i], uniform in [0, 60] s of the common clock.  `repeats` rounds after a warm-up round, the calls alternated inside a round:
  pair     one query per vehicle, vehicle i against vehicle i + 1 over [30, 35] s at dt = 0.05 (101 samples: one <64> launch):
             separation            ALMTrajOpt.separation, R = 0.2 m            -- uph_separation_kernel
             footprint_separation  the same queries, cars of 0.6 m x 0.3 m     -- uph_footprint_kernel
           HIP events around the launches (separation_kernel_ms / footprint_kernel_ms) and the wall clock of the whole blocking call
  fleet    the first 64 vehicles over [20, 40] s at dt = 0.05 (401 samples: <256> launches), t0 drawn again in [15, 25] s so that they move in the window:
             conflicts             discs of the circumscribed radius + margin  -- extents, the host broad phase, uph_separation_kernel
             footprint_conflicts   the cars, the same margin                   -- extents, the host broad phase, uph_footprint_kernel
           the same two numbers, and what each reports
Median (min - max) of every series goes to the JSON, with the ratios of the medians."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402
from uneven_planner_amd.alm_traj_opt import separation_times     # noqa: E402

args = sys.argv[1:]
B = int(args[0]) if len(args) > 0 else 4096
OUT = args[1] if len(args) > 1 else None
REP = max(3, int(args[2])) if len(args) > 2 else 15
DT, T_FROM, T_TO, RADIUS = 0.05, 30.0, 35.0, 0.1
CAR, MARGIN = np.array([0.45, 0.15, 0.15]), 0.05
FLEET, F_FROM, F_TO = 64, 20.0, 40.0
m = U.UnevenMap()
m.build(scenes.make_hill_cloud())
nx, ny = int(m.voxel_num[0]), int(m.voxel_num[1])
S, G = scenes.random_queries(B, seed0=1000, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]))
ka = U.KinoAstar(m, slots=min(B, 4096))
src = U.ALMTrajOpt(m)
src.set_rho(1.0)
src.plan_goals(ka, S, G)
offs = src.rollout_plan(DT, True)
valid = np.nonzero(np.diff(offs) > 0)[0].astype(np.int32)
n = int(valid.size)
rng = np.random.default_rng(91)
t0 = rng.uniform(0.0, 60.0, n)
other, t0_other = np.roll(valid, -1), np.roll(t0, -1)
fleet = valid[:FLEET]
t0_fleet = rng.uniform(15.0, 25.0, fleet.size)
rho = float(np.hypot(max(CAR[0], CAR[1]), CAR[2]))
rec = {"build": U._lib.build_id(), "goals": B, "resident": int(src.L.uph_batch_count(src.h)), "vehicles": n, "dt": DT, "window": [T_FROM, T_TO],
       "samples_per_query": int(separation_times(T_FROM, T_TO, DT).shape[0]), "radius": RADIUS, "shape": CAR.tolist(), "margin": MARGIN, "fleet": int(fleet.size),
       "fleet_window": [F_FROM, F_TO], "fleet_samples": int(separation_times(F_FROM, F_TO, DT).shape[0]), "repeats": REP}


def stat(v):
    return dict(runs=[round(float(x), 4) for x in v], median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def timed(call, kernel_ms):
    a = time.perf_counter()
    r = call()
    return r, 1e3 * (time.perf_counter() - a), kernel_ms()


series = ("separation", "footprint_separation", "conflicts", "footprint_conflicts")
runs = {"%s_%s_ms" % (s, w): [] for s in series for w in ("kernel", "call")}
for k in range(REP + 1):                    # the first round allocates device buffers and loads the code objects: not recorded
    out = {}
    out["separation"] = timed(lambda: src.separation(valid, other, T_FROM, T_TO, 2.0 * RADIUS, t0_a=t0, t0_b=t0_other, dt=DT), src.separation_kernel_ms)
    out["footprint_separation"] = timed(lambda: src.footprint_separation(valid, other, T_FROM, T_TO, CAR, CAR, 2.0 * MARGIN, t0_a=t0, t0_b=t0_other, dt=DT),
                                        src.footprint_kernel_ms)
    out["conflicts"] = timed(lambda: src.conflicts(fleet, rho + MARGIN, F_FROM, F_TO, t0=t0_fleet, dt=DT), src.separation_kernel_ms)
    out["footprint_conflicts"] = timed(lambda: src.footprint_conflicts(fleet, CAR, MARGIN, F_FROM, F_TO, t0=t0_fleet, dt=DT), src.footprint_kernel_ms)
    if k:
        for s in series:
            runs[s + "_call_ms"].append(out[s][1])
            runs[s + "_kernel_ms"].append(out[s][2])
    print("round %d: %s" % (k, ", ".join("%s %.4f / %.3f" % (s, out[s][2], out[s][1]) for s in series)), flush=True)
sep, foot, con, fcon = (out[s][0] for s in series)
rec.update({key: stat(v) for key, v in runs.items()})
med = lambda key: rec[key]["median"]
rec.update(pair_kernel_ratio=med("footprint_separation_kernel_ms") / med("separation_kernel_ms"), pair_call_ratio=med("footprint_separation_call_ms") / med("separation_call_ms"),
           fleet_kernel_ratio=med("footprint_conflicts_kernel_ms") / med("conflicts_kernel_ms"), fleet_call_ratio=med("footprint_conflicts_call_ms") / med("conflicts_call_ms"),
           pair_queries_below_discs=int((sep["counts"][:, 1] > 0).sum()), pair_queries_below_footprints=int((foot["counts"][:, 1] > 0).sum()),
           pair_queries_overlapping=int((foot["counts"][:, 2] > 0).sum()), fleet_conflicts_discs=con["n_conflicts"], fleet_conflicts_footprints=fcon["n_conflicts"],
           fleet_candidates_discs=con["n_candidates"], fleet_candidates_footprints=fcon["n_candidates"])
line = json.dumps(rec, indent=1)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
assert set(map(tuple, fcon["pairs"].tolist())) <= set(map(tuple, con["pairs"].tolist())), "a footprint conflict the circumscribed discs do not report"
