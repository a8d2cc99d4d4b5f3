"""Cost of clearing footprint conflicts between resident trajectories by delaying starts: python tools/footprint_delay_probe.py [B = 4096] [out.json] [repeats = 7]
Source, fleet, window and delays are tools/delay_probe.py's: B hill goals planned and solved by ALMTrajOpt.plan_goals, the valid resident trajectories in priority
order, vehicle i started at t0[i], uniform in [0, 60] s of the common clock; the window is [30, 35] s at dt = 0.05 (101 samples); D = 32 delays of 0.5 s from 0.
The vehicle is DESIGN.md 7p's car: front 0.45 m, rear 0.15 m, half width 0.15 m, a margin of 0.05 m each (M = 0.1 m for a pair).  `repeats` rounds after a
warm-up round, the calls alternated inside a round:
  sweep    ALMTrajOpt.footprint_delay_sweep of one query per vehicle (vehicle i against vehicle i + 1, vehicle i + 1 delayed) -- uph_footprint_sweep_kernel: HIP
           events around the launches (delay_kernel_ms) and the wall clock of the whole blocking call
  recipe   what the sweep replaces: one ALMTrajOpt.footprint_separation call per delay over the same queries, vehicle i + 1 started at t0 + delta_j -- the sum
           of footprint_kernel_ms and the wall clock of the D blocking calls.  It returns the same numbers bit for bit; the probe asserts that.
  disc     ALMTrajOpt.delay_sweep over the same queries on the circumscribed discs (R = rho_i + m_i + rho_j + m_j) -- uph_delay_sweep_kernel, the same two numbers
  delays   ALMTrajOpt.footprint_delays over the fleet against ALMTrajOpt.delays on the radii rho_i + m_i: kernel and call time of each, and how many vehicles
           each postpones
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
DT, T_FROM, T_TO = 0.05, 30.0, 35.0
D, STEP = 32, 0.5
CAR, M_EACH = (0.45, 0.15, 0.15), 0.05
RHO = float(np.hypot(max(CAR[0], CAR[1]), CAR[2]))
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
       "samples_per_query": int(separation_times(T_FROM, T_TO, DT).shape[0]), "shape": list(CAR), "margin_each": M_EACH, "disc_radius_each": RHO + M_EACH, "delays": D,
       "delay_step": STEP, "repeats": REP}


def stat(v):
    return dict(runs=[round(float(x), 4) for x in v], median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def recipe():
    least, when = np.zeros((n, D)), np.zeros((n, D))
    below, over = np.zeros((n, D), dtype=np.int32), np.zeros((n, D), dtype=np.int32)
    kernel = 0.0
    a = time.perf_counter()
    for j in range(D):
        r = src.footprint_separation(valid, other, T_FROM, T_TO, CAR, CAR, 2.0 * M_EACH, t0_a=t0, t0_b=t0_other + delta[j], dt=DT)
        kernel += src.footprint_kernel_ms()
        least[:, j], when[:, j], below[:, j], over[:, j] = r["min_c2"], r["min_t"], r["counts"][:, 1], r["counts"][:, 2]
    return least, when, below, over, kernel, 1e3 * (time.perf_counter() - a)


KEYS = ("sweep", "recipe", "disc", "delays", "disc_delays")
runs = {"%s_%s_ms" % (k, w): [] for k in KEYS for w in ("kernel", "call")}
for k in range(REP + 1):                    # the first round allocates device buffers and loads the code objects: not recorded
    ms = {}
    a = time.perf_counter()
    sweep = src.footprint_delay_sweep(valid, other, T_FROM, T_TO, CAR, CAR, 2.0 * M_EACH, 0.0, STEP, D, t0_a=t0, t0_b=t0_other, dt=DT)
    ms["sweep_call_ms"], ms["sweep_kernel_ms"] = 1e3 * (time.perf_counter() - a), src.delay_kernel_ms()
    least, when, below, over, ms["recipe_kernel_ms"], ms["recipe_call_ms"] = recipe()
    a = time.perf_counter()
    disc = src.delay_sweep(valid, other, T_FROM, T_TO, 2.0 * (RHO + M_EACH), 0.0, STEP, D, t0_a=t0, t0_b=t0_other, dt=DT)
    ms["disc_call_ms"], ms["disc_kernel_ms"] = 1e3 * (time.perf_counter() - a), src.delay_kernel_ms()
    a = time.perf_counter()
    sched = src.footprint_delays(valid, CAR, M_EACH, T_FROM, T_TO, 0.0, STEP, D, t0=t0, dt=DT)
    ms["delays_call_ms"], ms["delays_kernel_ms"] = 1e3 * (time.perf_counter() - a), src.delay_kernel_ms()
    a = time.perf_counter()
    dsched = src.delays(valid, RHO + M_EACH, T_FROM, T_TO, 0.0, STEP, D, t0=t0, dt=DT)
    ms["disc_delays_call_ms"], ms["disc_delays_kernel_ms"] = 1e3 * (time.perf_counter() - a), src.delay_kernel_ms()
    if k:
        for key, v in ms.items():
            runs[key].append(v)
    print("round %d: %s" % (k, ", ".join("%s %.3f" % (key[:-3], v) for key, v in ms.items())), flush=True)
same = bool(np.array_equal(sweep["min_c2"], least) and np.array_equal(sweep["min_t"], when, equal_nan=True) and np.array_equal(sweep["below"], below) and
            np.array_equal(sweep["overlapping"], over))
before = src.footprint_conflicts(valid, CAR, M_EACH, T_FROM, T_TO, t0=t0, dt=DT, cap=0)
after = src.footprint_conflicts(valid, CAR, M_EACH, T_FROM, T_TO, t0=sched["start"], dt=DT, cap=1 << 20)
left_placed = int((sched["choice"][after["pairs"][:, 1]] >= 0).sum())
disc_before = src.conflicts(valid, RHO + M_EACH, T_FROM, T_TO, t0=t0, dt=DT, cap=0)
rec.update(sweep_equals_recipe=same, left_placed=left_placed)
rec.update({key: stat(v) for key, v in runs.items()})
rec.update(n_candidates=sched["n_candidates"], n_rounds=sched["n_rounds"], n_unresolved=sched["n_unresolved"], delayed=int((sched["choice"] > 0).sum()),
           disc_n_candidates=dsched["n_candidates"], disc_n_rounds=dsched["n_rounds"], disc_n_unresolved=dsched["n_unresolved"], disc_delayed=int((dsched["choice"] > 0).sum()),
           conflicts_before=before["n_conflicts"], conflicts_after=after["n_conflicts"], disc_conflicts_before=disc_before["n_conflicts"],
           queries_below_at_delay_0=int((sweep["below"][:, 0] > 0).sum()), queries_overlapping_at_delay_0=int((sweep["overlapping"][:, 0] > 0).sum()),
           disc_queries_below_at_delay_0=int((disc["below"][:, 0] > 0).sum()), queries_never_clear=int((sweep["first_clear"] < 0).sum()))
line = json.dumps(rec, indent=1)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
assert same, "the footprint sweep and the footprint_separation call per delay disagree"
assert left_placed == 0, "a vehicle that was given a delay is still in a footprint conflict"
