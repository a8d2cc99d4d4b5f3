"""Cost of the footprint check: python tools/footprint_check_probe.py [B = 4096] [out.json = profiles/footprint_check_probe.json] [repeats = 15]
Source: B hill goals planned and solved by ALMTrajOpt.plan_goals, as tools/footprint_probe.py; every valid resident trajectory is one query over its full window at
dt = 0.01 with the end row.  The car is the footprint probe's (0.45 + 0.15 m x 2 * 0.3 m) with a margin of 0.05 m: about 200 columns of the 0.05 m grid per sample.
`repeats` rounds after a warm-up round, the calls alternated inside a round:
  footprint_check   ALMTrajOpt.footprint_check, all layers   -- uph_footprint_check_kernel: HIP events around the launches and the wall clock of the blocking call
  check             ALMTrajOpt.check of the same windows     -- uph_check_kernel, as context only: it evaluates the terrain terms and reads ONE column per sample
and, once, on the first 64 trajectories, the recipe the query replaces: the STATE rows from the device (traj_states), get_cells' occupancy already on the host, and
footprint_check_rows in numpy -- stated as what it is, 64 trajectories, and scaled to the batch in `recipe_scaled_ms`.
Median (min - max) of every series goes to the JSON."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402
from uneven_planner_amd.alm_traj_opt import footprint_check_columns, footprint_check_rows, footprint_grid     # noqa: E402

args = sys.argv[1:]
B = int(args[0]) if len(args) > 0 else 4096
OUT = args[1] if len(args) > 1 else os.path.join("profiles", "footprint_check_probe.json")
REP = max(3, int(args[2])) if len(args) > 2 else 15
DT, CAR, MARGIN, RECIPE = 0.01, np.array([0.45, 0.15, 0.3]), 0.05, 64
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
samples = int(np.diff(offs)[valid].sum())
rec = {"build": U._lib.build_id(), "goals": B, "resident": int(src.L.uph_batch_count(src.h)), "queries": int(valid.size), "dt": DT, "with_end": True, "samples": samples,
       "shape": CAR.tolist(), "margin": MARGIN, "box_columns_bound": footprint_check_columns(CAR, MARGIN, m.xy_resolution), "repeats": REP}


def stat(v):
    return dict(runs=[round(float(x), 4) for x in v], median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def timed(call, kernel_ms):
    a = time.perf_counter()
    r = call()
    return r, 1e3 * (time.perf_counter() - a), kernel_ms()


series = ("footprint_check", "check")
runs = {"%s_%s_ms" % (s, w): [] for s in series for w in ("kernel", "call")}
for k in range(REP + 1):                    # the first round allocates device buffers and loads the code objects: not recorded
    out = {}
    out["footprint_check"] = timed(lambda: src.footprint_check(valid, CAR, MARGIN, dt=DT), src.footprint_check_kernel_ms)
    out["check"] = timed(lambda: src.check(valid, dt=DT), src.check_kernel_ms)
    if k:
        for s in series:
            runs[s + "_call_ms"].append(out[s][1])
            runs[s + "_kernel_ms"].append(out[s][2])
    print("round %d: %s" % (k, ", ".join("%s %.4f / %.3f" % (s, out[s][2], out[s][1]) for s in series)), flush=True)
got = out["footprint_check"][0]
rec.update({key: stat(v) for key, v in runs.items()})
rec.update(covered_columns=int(got["cells"][:, 0].sum()), hit_columns=int(got["cells"][:, 1].sum()), hit_samples=int(got["counts"][:, 1].sum()),
           queries_with_hits=int((got["counts"][:, 1] > 0).sum()), columns_per_sample=float(got["cells"][:, 0].sum()) / max(samples, 1),
           kernel_ns_per_sample=1e6 * rec["footprint_check_kernel_ms"]["median"] / max(samples, 1),
           kernel_ns_per_column=1e6 * rec["footprint_check_kernel_ms"]["median"] / max(int(got["cells"][:, 0].sum()), 1))

# the recipe being replaced, on the first RECIPE trajectories: states to the host, then the numpy mirror per trajectory
few = valid[:RECIPE]
grid = footprint_grid(m)
a = time.perf_counter()
roffs, rows = src.rollout(DT, 1, with_end=True, b0=0, b1=int(few[-1]) + 1)
ts = [rows[int(roffs[b]):int(roffs[b + 1]), 0] for b in few]
st = src.traj_states(np.concatenate([np.full(t.shape[0], b, dtype=np.int32) for t, b in zip(ts, few)]), np.concatenate(ts))
b_ = time.perf_counter()
at, hits = 0, 0
for t in ts:
    s = st[at:at + t.shape[0]]
    at += t.shape[0]
    hits += int(footprint_check_rows(t, s[:, [0, 1, 9]], s[:, 6], CAR, MARGIN, grid, m.occ_buffer, m.occ_r2_buffer)["sure"]["counts"][1])
c_ = time.perf_counter()
few_samples = int(sum(t.shape[0] for t in ts))
rec.update(recipe_trajectories=int(few.size), recipe_samples=few_samples, recipe_download_ms=1e3 * (b_ - a), recipe_numpy_ms=1e3 * (c_ - b_),
           recipe_scaled_ms=1e3 * (c_ - a) * samples / max(few_samples, 1), recipe_hit_samples=hits, device_hit_samples_same=int(got["counts"][:RECIPE, 1].sum()))
line = json.dumps(rec, indent=1)
print(line)
with open(OUT, "w") as f:
    f.write(line + "\n")
