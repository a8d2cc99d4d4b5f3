"""Cost of locating poses on a solved hill batch and of finding rect crossings: python tools/locate_probe.py [B = 16384] [out.json] [repeats = 7]
Source: B hill goals planned and solved by ALMTrajOpt.plan_goals.  One query per valid resident trajectory: a time t_c uniform in [0.2, 0.8] of its
duration, the pose 0.05 m to the left of the trajectory there, a 2 m x 2 m rect centred on that pose.  Two workloads, dt 0.01 with the end point:
  tracking  the window t_c +- 0.5 s (101 samples)
  lost      the full window
For each, `repeats` rounds after a warm-up round, the calls alternated inside a round:
  locate    ALMTrajOpt.locate -- uph_locate_kernel: HIP events around the launch(es) (locate_kernel_ms), and the wall clock of the whole blocking call
  within    ALMTrajOpt.within -- uph_within_kernel: the same two numbers
  check     ALMTrajOpt.check on the same (trajectory, window) pairs -- uph_check_kernel: HIP events (check_kernel_ms): the bar
  host      what locate replaces: the STATE rollout of the batch to the host, then numpy argmin of the squared distance over each window (wall clock,
            the two parts also apart)
  recipe    what within replaces: the STATE rollout at dt 0.05 to the host and the rect test of every row per trajectory (wall
            clock; once per round, it has no window)
Median (min - max) of every series goes to the JSON."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402

args = sys.argv[1:]
B = int(args[0]) if len(args) > 0 else 16384
OUT = args[1] if len(args) > 1 else None
REP = max(3, int(args[2])) if len(args) > 2 else 7
m = U.UnevenMap()
m.build(scenes.make_hill_cloud())
nx, ny = int(m.voxel_num[0]), int(m.voxel_num[1])
S, G = scenes.random_queries(B, seed0=1000, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]))
ka = U.KinoAstar(m, slots=min(B, 4096))
src = U.ALMTrajOpt(m)
src.set_rho(1.0)
src.plan_goals(ka, S, G)
offs = src.rollout_plan(0.01, True)
valid = np.nonzero(np.diff(offs) > 0)[0].astype(np.int32)
o1, r1 = src.rollout(1.0, channels=1, with_end=True)
total = r1[o1[1:] - 1, 0][valid]
rng = np.random.default_rng(77)
tc = rng.uniform(0.2, 0.8, valid.size) * total
st = src.traj_states(valid, tc)
sp = np.maximum(np.hypot(st[:, 2], st[:, 3]), 1e-12)
poses = np.stack([st[:, 0] - 0.05 * st[:, 3] / sp, st[:, 1] + 0.05 * st[:, 2] / sp, st[:, 9]], axis=1)
rects = np.stack([poses[:, 0] - 1.0, poses[:, 0] + 1.0, poses[:, 1] - 1.0, poses[:, 1] + 1.0], axis=1)
rec = {"build": U._lib.build_id(), "goals": B, "resident": int(src.L.uph_batch_count(src.h)), "trajectories": int(valid.size), "dt": 0.01, "with_end": True,
       "repeats": REP, "rows": int(offs[-1]), "state_rollout_bytes": int(offs[-1]) * 9 * 8, "locate_output_bytes": int(valid.size) * 144,
       "within_output_bytes": int(valid.size) * 24, "query_bytes": int(valid.size) * 80}


def stat(v):
    return dict(runs=[round(float(x), 4) for x in v], median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def host_locate(tf, tt):
    """the STATE rollout to the host + numpy argmin over each window"""
    t0 = time.perf_counter()
    o, rows = src.rollout(0.01, channels=1, with_end=True)
    t1 = time.perf_counter()
    near = np.full(valid.size, np.nan)
    for q, b in enumerate(valid):
        blk = rows[o[b]:o[b + 1]]
        sel = (tf[q] <= blk[:, 0]) & (blk[:, 0] <= tt[q])
        if sel.any():
            w = blk[sel]
            ex, ey = w[:, 1] - poses[q, 0], w[:, 2] - poses[q, 1]
            near[q] = w[np.argmin(ex * ex + ey * ey), 0]
    t2 = time.perf_counter()
    return near, 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def recipe(rect):
    """rollout(0.05, channels=1) and the rect test of every row"""
    t0 = time.perf_counter()
    o, rows = src.rollout(0.05, channels=1)
    lo, hi = np.array([rect[0], rect[2]]), np.array([rect[1], rect[3]])
    hit = [b for b in range(len(o) - 1) if ((rows[o[b]:o[b + 1], 1:3] >= lo) & (rows[o[b]:o[b + 1], 1:3] <= hi)).all(axis=1).any()]
    return hit, 1e3 * (time.perf_counter() - t0)


one_rect = np.array([-2.0, 2.0, -2.0, 2.0])                 # a changed region in the middle of the map, for the recipe and its replacement
for name, tf, tt in (("tracking", tc - 0.5, tc + 0.5), ("lost", np.zeros(valid.size), np.full(valid.size, np.inf))):
    runs = {k: [] for k in ("locate_kernel_ms", "locate_call_ms", "within_kernel_ms", "within_call_ms", "check_kernel_ms", "check_call_ms",
                            "host_rollout_ms", "host_argmin_ms", "host_total_ms", "recipe_ms", "within_one_rect_call_ms", "within_one_rect_kernel_ms")}
    for k in range(REP + 1):                # the first round allocates device buffers and loads the code objects: not recorded
        ms = {}
        t0 = time.perf_counter()
        loc = src.locate(valid, poses, tf, tt)
        ms["locate_call_ms"], ms["locate_kernel_ms"] = 1e3 * (time.perf_counter() - t0), src.locate_kernel_ms()
        t0 = time.perf_counter()
        chk = src.check(valid, tf, tt)
        ms["check_call_ms"], ms["check_kernel_ms"] = 1e3 * (time.perf_counter() - t0), src.check_kernel_ms()
        t0 = time.perf_counter()
        wit = src.within(valid, rects, tf, tt)
        ms["within_call_ms"], ms["within_kernel_ms"] = 1e3 * (time.perf_counter() - t0), src.locate_kernel_ms()
        near, ms["host_rollout_ms"], ms["host_argmin_ms"] = host_locate(tf, tt)
        ms["host_total_ms"] = ms["host_rollout_ms"] + ms["host_argmin_ms"]
        hit, ms["recipe_ms"] = recipe(one_rect)
        t0 = time.perf_counter()
        w1 = src.within(valid, one_rect, dt=0.05, with_end=False)
        ms["within_one_rect_call_ms"], ms["within_one_rect_kernel_ms"] = 1e3 * (time.perf_counter() - t0), src.locate_kernel_ms()
        if k:
            for key, v in ms.items():
                runs[key].append(v)
    assert np.array_equal(near, loc["near_t"], equal_nan=True), "the host argmin and the device disagree"
    assert valid[w1["counts"][:, 1] > 0].tolist() == hit, "the recipe and within() disagree"
    assert np.array_equal(chk["counts"][:, 0], loc["count"]) and np.array_equal(wit["counts"][:, 0], loc["count"])
    rec[name] = {key: stat(v) for key, v in runs.items()}
    rec[name].update(samples=int(loc["count"].sum()), samples_per_query_median=float(np.median(loc["count"])), refined=int(loc["refined"].sum()),
                     inside_trajectories=int((wit["counts"][:, 1] > 0).sum()), recipe_hits=len(hit),
                     long_queries=int((loc["count"] > 192).sum()), t_error_max=float(np.nanmax(np.abs(loc["t"] - tc))))
line = json.dumps(rec, indent=1)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
