"""Refining against re-planning on a solved hill batch: python tools/refine_probe.py [B = 16384] [out.json]
Source: B hill goals planned and solved by ALMTrajOpt.plan_goals.  Query q takes valid trajectory q % F at half its duration, on the unchanged map:
  refine: ALMTrajOpt.refine_upload -- uph_refine_upload (the rest of each trajectory as the initial guess, no search)
  replan: ALMTrajOpt.replan_goals_upload(goals=None) -- uph_replan_upload (a new search from the switch state to the source's end pose)
Wall clock of each upload, the two methods alternated and each run twice on contexts of their own (the first run allocates device buffers); then
two solves of each batch, alternated: solve-kernel ms (HIP events), mean and median L-BFGS iterations, ALM passes and the converged fraction.
Kernel times of the whole call come from a run of this script under `rocprofv3 --kernel-trace --stats`."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
OUT = sys.argv[2] if len(sys.argv) > 2 else None
m = U.UnevenMap()
m.build(scenes.make_hill_cloud())
nx, ny = int(m.voxel_num[0]), int(m.voxel_num[1])
S, G = scenes.random_queries(B, seed0=1000, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]))
ka = U.KinoAstar(m, slots=min(B, 4096))
src = U.ALMTrajOpt(m)
src.set_rho(1.0)
t0 = time.perf_counter()
src.plan_goals(ka, S, G)
rec = {"goals": B, "source_plan_goals_s": time.perf_counter() - t0, "source_resident": int(src.L.uph_batch_count(src.h))}
# half of each trajectory's duration (the end row of a dt = 1 s rollout holds it); unsupported slots have no rows, non-finite ones are skipped
offs, rows = src.rollout(1.0, channels=1, with_end=True)
valid = np.array([j for j in np.nonzero(np.diff(offs) > 0)[0] if np.isfinite(rows[offs[j]:offs[j + 1]]).all()])
tr = valid[np.arange(B) % len(valid)].astype(np.int32)
ts = 0.5 * rows[offs[tr + 1] - 1, 0]
rec["switch_trajectories"] = int(len(valid))
dsts = {}
for k in range(2):
    for way in ("refine", "replan"):
        dst = U.ALMTrajOpt(m)
        dst.set_rho(1.0)
        t0 = time.perf_counter()
        plan = dst.refine_upload(src, tr, ts) if way == "refine" else dst.replan_goals_upload(ka, src, tr, ts, goals=None)
        rec["%s_upload_s_run%d" % (way, k)] = time.perf_counter() - t0
        rec["%s_uploaded" % way] = int((plan["traj_of"] >= 0).sum())
        dsts[way] = (dst, plan)
for k in range(2):
    for way in ("refine", "replan"):
        dst, plan = dsts[way]
        dst.solve()
        s = dst.stats()
        found = np.nonzero(plan["traj_of"] >= 0)[0]
        res = dst._download_block(plan["n_inner_xy"][found], plan["n_inner_yaw"][found], False)
        it = np.array([r["lbfgs_iters"] for r in res])
        alm = np.array([r["alm_iters"] for r in res])
        ret = np.array([r["ret"] for r in res])
        rec["%s_solve_run%d" % (way, k)] = dict(kernel_ms=s["kernel_ms"], problems=int(len(res)), lbfgs_iters_mean=float(it.mean()),
                                                 lbfgs_iters_median=float(np.median(it)), alm_passes_mean=float(alm.mean()),
                                                 converged_frac=float((ret == 0).mean()), ret_counts={int(v): int((ret == v).sum()) for v in np.unique(ret)})
line = json.dumps(rec, indent=1)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
