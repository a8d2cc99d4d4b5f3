"""Cost of clearing conflicts between resident trajectories by delaying starts: python tools/delay_probe.py [B = 4096] [out.json] [repeats = 7]
Source: B hill goals planned and solved by ALMTrajOpt.plan_goals; the valid resident trajectories are the fleet, in priority order.  Vehicle i starts at
t0[i], uniform in [0, 60] s of the common clock, and is a disc of 0.1 m; the window is [30, 35] s at dt = 0.05 (101 samples); the delays are D = 32 steps
of 0.5 s from 0.  `repeats` rounds after a warm-up round, the calls alternated inside a round:
  delays   ALMTrajOpt.delays over the fleet -- uph_delay_extent_kernel, the host broad phase and its levels, uph_delay_sweep_kernel per level: HIP events
           around the launches (delay_kernel_ms) and the wall clock of the whole blocking call
  sweep    ALMTrajOpt.delay_sweep of one query per vehicle (vehicle i against vehicle i + 1, R = 0.2 m, vehicle i + 1 delayed) -- the same two numbers
  extent   ALMTrajOpt.delay_extent of the fleet -- the same two numbers
  recipe   what the sweep replaces: one ALMTrajOpt.separation call per delay over the same queries, vehicle i + 1 started at t0 + delta_j -- the sum of
           separation_kernel_ms and the wall clock of the D blocking calls.  It returns the same numbers bit for bit; the probe checks that.
Median (min - max) of every series goes to the JSON."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402
from uneven_planner_amd.alm_traj_opt import delay_times, separation_times     # noqa: E402

args = sys.argv[1:]
B = int(args[0]) if len(args) > 0 else 4096
OUT = args[1] if len(args) > 1 else None
REP = max(3, int(args[2])) if len(args) > 2 else 7
DT, T_FROM, T_TO, RADIUS = 0.05, 30.0, 35.0, 0.1
D, STEP = 32, 0.5
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
delta = delay_times(0.0, STEP, D)
rec = {"build": U._lib.build_id(), "goals": B, "resident": int(src.L.uph_batch_count(src.h)), "vehicles": n, "dt": DT, "window": [T_FROM, T_TO],
       "samples_per_query": int(separation_times(T_FROM, T_TO, DT).shape[0]), "radius": RADIUS, "delays": D, "delay_step": STEP, "repeats": REP}


def stat(v):
    return dict(runs=[round(float(x), 4) for x in v], median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def recipe():
    least, when, below = np.zeros((n, D)), np.zeros((n, D)), np.zeros((n, D), dtype=np.int32)
    kernel = 0.0
    a = time.perf_counter()
    for j in range(D):
        r = src.separation(valid, other, T_FROM, T_TO, 2.0 * RADIUS, t0_a=t0, t0_b=t0_other + delta[j], dt=DT)
        kernel += src.separation_kernel_ms()
        least[:, j], when[:, j], below[:, j] = r["min_d2"], r["min_t"], r["counts"][:, 1]
    return least, when, below, kernel, 1e3 * (time.perf_counter() - a)


runs = {k: [] for k in ("delays_kernel_ms", "delays_call_ms", "sweep_kernel_ms", "sweep_call_ms", "extent_kernel_ms", "extent_call_ms", "recipe_kernel_ms",
                        "recipe_call_ms")}
for k in range(REP + 1):                    # the first round allocates device buffers and loads the code objects: not recorded
    ms = {}
    a = time.perf_counter()
    sched = src.delays(valid, RADIUS, T_FROM, T_TO, 0.0, STEP, D, t0=t0, dt=DT)
    ms["delays_call_ms"], ms["delays_kernel_ms"] = 1e3 * (time.perf_counter() - a), src.delay_kernel_ms()
    a = time.perf_counter()
    sweep = src.delay_sweep(valid, other, T_FROM, T_TO, 2.0 * RADIUS, 0.0, STEP, D, t0_a=t0, t0_b=t0_other, dt=DT)
    ms["sweep_call_ms"], ms["sweep_kernel_ms"] = 1e3 * (time.perf_counter() - a), src.delay_kernel_ms()
    a = time.perf_counter()
    ext = src.delay_extent(valid, T_FROM, T_TO, 0.0, STEP, D, t0=t0, dt=DT)
    ms["extent_call_ms"], ms["extent_kernel_ms"] = 1e3 * (time.perf_counter() - a), src.delay_kernel_ms()
    least, when, below, ms["recipe_kernel_ms"], ms["recipe_call_ms"] = recipe()
    if k:
        for key, v in ms.items():
            runs[key].append(v)
    print("round %d: %s" % (k, ", ".join("%s %.3f" % (key[:-3], v) for key, v in ms.items())), flush=True)
same = bool(np.array_equal(sweep["min_d2"], least) and np.array_equal(sweep["min_t"], when, equal_nan=True) and np.array_equal(sweep["below"], below))
before = src.conflicts(valid, RADIUS, T_FROM, T_TO, t0=t0, dt=DT, cap=0)
after = src.conflicts(valid, RADIUS, T_FROM, T_TO, t0=sched["start"], dt=DT, cap=1 << 20)
left_placed = int((sched["choice"][after["pairs"][:, 1]] >= 0).sum())
rec.update(sweep_equals_recipe=same, left_placed=left_placed)
rec.update({key: stat(v) for key, v in runs.items()})
rec.update(n_candidates=sched["n_candidates"], n_rounds=sched["n_rounds"], n_unresolved=sched["n_unresolved"], delayed=int((sched["choice"] > 0).sum()),
           conflicts_before=before["n_conflicts"], conflicts_after=after["n_conflicts"], queries_below_at_delay_0=int((sweep["below"][:, 0] > 0).sum()),
           queries_never_clear=int((sweep["first_clear"] < 0).sum()), moving_in_window=int(((ext["box"][:, 1] > ext["box"][:, 0]) | (ext["box"][:, 3] > ext["box"][:, 2])).sum()))
line = json.dumps(rec, indent=1)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
assert same, "the sweep and the separation call per delay disagree"
assert left_placed == 0, "a vehicle that was given a delay is still in a conflict"
