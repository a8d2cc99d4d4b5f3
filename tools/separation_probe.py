"""Cost of finding conflicts between resident trajectories on a common clock: python tools/separation_probe.py [B = 4096] [out.json] [repeats = 7]
Source: B hill goals planned and solved by ALMTrajOpt.plan_goals; the valid resident trajectories are the fleet.  Vehicle i starts at t0[i], uniform in
[0, 60] s of the common clock, and is a disc of 0.1 m; the window is [30, 35] s at dt = 0.05 (101 samples), so some vehicles wait at their starts, some
drive and some have arrived.  `repeats` rounds after a warm-up round, the calls alternated inside a round:
  conflicts   ALMTrajOpt.conflicts over the fleet -- uph_extent_kernel, the host broad phase, uph_separation_kernel on its candidates: HIP events around the
              launches (separation_kernel_ms) and the wall clock of the whole blocking call
  separation  ALMTrajOpt.separation of one query per vehicle (vehicle i against vehicle i + 1, R = 0.2 m) -- the same two numbers
  extent      ALMTrajOpt.extent of the fleet -- the same two numbers
  recipe      what separation replaces: the STATE rollout of the batch at dt 0.05 to the host and, per query, numpy on the rows of both trajectories -- each
              shifted to the common clock by its t0 and held at its first / last row outside its own time -- through separation_rows (wall clock, the
              rollout with its download and the numpy part also apart).  The recipe samples each trajectory on its own additive time table, not on the
              common clock, so it agrees with the device to the distance a vehicle moves in dt, not bit for bit; the probe checks that much.
Median (min - max) of every series goes to the JSON."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402
from uneven_planner_amd.alm_traj_opt import separation_rows, separation_times     # noqa: E402

args = sys.argv[1:]
B = int(args[0]) if len(args) > 0 else 4096
OUT = args[1] if len(args) > 1 else None
REP = max(3, int(args[2])) if len(args) > 2 else 7
DT, T_FROM, T_TO, RADIUS = 0.05, 30.0, 35.0, 0.1
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
tau = separation_times(T_FROM, T_TO, DT)
rec = {"build": U._lib.build_id(), "goals": B, "resident": int(src.L.uph_batch_count(src.h)), "vehicles": n, "dt": DT, "window": [T_FROM, T_TO],
       "samples_per_query": int(tau.shape[0]), "radius": RADIUS, "repeats": REP, "pairs": n * (n - 1) // 2, "state_rollout_rows": int(offs[-1]),
       "state_rollout_bytes": int(offs[-1]) * 9 * 8}


def stat(v):
    return dict(runs=[round(float(x), 4) for x in v], median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def on_clock(blk, start):
    """the rows of one trajectory's rollout at the common clock's samples: the row whose t is nearest below tau - start, the first / last outside"""
    k = np.clip(np.searchsorted(blk[:, 0], tau - start, side="right") - 1, 0, blk.shape[0] - 1)
    return blk[k, 1:3]


def recipe():
    a = time.perf_counter()
    o, rows = src.rollout(DT, channels=1, with_end=True)
    b = time.perf_counter()
    least = np.zeros(n)
    below = np.zeros(n, dtype=np.int64)
    for q in range(n):
        i, j = valid[q], other[q]
        r = separation_rows(tau, on_clock(rows[o[i]:o[i + 1]], t0[q]), on_clock(rows[o[j]:o[j + 1]], t0_other[q]), 2.0 * RADIUS)
        least[q], below[q] = r["min_d2"], r["counts"][1]
    c = time.perf_counter()
    return least, below, 1e3 * (b - a), 1e3 * (c - b)


runs = {k: [] for k in ("conflicts_kernel_ms", "conflicts_call_ms", "separation_kernel_ms", "separation_call_ms", "extent_kernel_ms", "extent_call_ms",
                        "recipe_rollout_ms", "recipe_numpy_ms", "recipe_total_ms")}
for k in range(REP + 1):                    # the first round allocates device buffers and loads the code objects: not recorded
    ms = {}
    a = time.perf_counter()
    con = src.conflicts(valid, RADIUS, T_FROM, T_TO, t0=t0, dt=DT, cap=1 << 20)
    ms["conflicts_call_ms"], ms["conflicts_kernel_ms"] = 1e3 * (time.perf_counter() - a), src.separation_kernel_ms()
    a = time.perf_counter()
    sep = src.separation(valid, other, T_FROM, T_TO, 2.0 * RADIUS, t0_a=t0, t0_b=t0_other, dt=DT)
    ms["separation_call_ms"], ms["separation_kernel_ms"] = 1e3 * (time.perf_counter() - a), src.separation_kernel_ms()
    a = time.perf_counter()
    ext = src.extent(valid, T_FROM, T_TO, t0=t0, dt=DT)
    ms["extent_call_ms"], ms["extent_kernel_ms"] = 1e3 * (time.perf_counter() - a), src.separation_kernel_ms()
    least, below, ms["recipe_rollout_ms"], ms["recipe_numpy_ms"] = recipe()
    ms["recipe_total_ms"] = ms["recipe_rollout_ms"] + ms["recipe_numpy_ms"]
    if k:
        for key, v in ms.items():
            runs[key].append(v)
    print("round %d: %s" % (k, ", ".join("%s %.3f" % (key[:-3], v) for key, v in ms.items())), flush=True)
# the recipe's rows lag the common clock by less than dt: at most 0.5 m/s x 0.05 s per vehicle and a little more for the limits the solver leaves violated
slack = 2.0 * 1.0 * DT
diff = float(np.abs(np.sqrt(least) - np.sqrt(sep["min_d2"])).max())
pairs = {tuple(p) for p in con["pairs"].tolist()}
found = [(min(q, (q + 1) % n), max(q, (q + 1) % n)) for q in np.nonzero(sep["counts"][:, 1] > 0)[0]]
missed = 0 if con["n_conflicts"] > len(pairs) else sum(1 for p in found if p not in pairs)      # every single query that found a conflict is in the fleet's list
rec.update(recipe_distance_diff_max=diff, recipe_distance_slack=slack, single_conflicts_missing_from_the_fleet=missed)
rec.update({key: stat(v) for key, v in runs.items()})
rec.update(n_candidates=con["n_candidates"], n_conflicts=con["n_conflicts"], candidate_fraction=con["n_candidates"] / max(1, rec["pairs"]),
           single_queries_below=int((sep["counts"][:, 1] > 0).sum()), recipe_queries_below=int((below > 0).sum()),
           moving_in_window=int(((ext["box"][:, 1] > ext["box"][:, 0]) | (ext["box"][:, 3] > ext["box"][:, 2])).sum()))
line = json.dumps(rec, indent=1)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
assert diff <= slack, "the recipe and the device disagree"
assert missed == 0, "conflicts() misses a pair separation() finds"
