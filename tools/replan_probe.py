"""Re-planning from states on resident trajectories at scale: python tools/replan_probe.py [B = 16384] [out.json]
Source: B hill goals planned and solved by ALMTrajOpt.plan_goals.  Query q switches trajectory q % F at half its duration to a new hill goal.
  replan:   ALMTrajOpt.replan_goals_upload -- uph_replan_upload (switch-state kernel, search from the states, resampling + x0 scatter on the device)
  plan:     ALMTrajOpt.plan_goals_upload from the same starts (the switch states' x, y, yaw) to the same goals -- uph_plan_upload
  composed: the host chain of tests/test_gpu_replan.py -- KinoAstar.plan_batch (paths downloaded, clipped ones searched again) -> resample_batch
            (uph_resample_batch, host C++) -> the start boundaries patched -> ctypes packing + uph_batch_upload
Wall clock (perf_counter) of each upload, each way run twice on its own contexts (the first run allocates device buffers); the solve is not part of
any of them.  The kernel time of uph_switch_state_kernel comes from a run of this script under `rocprofv3 --kernel-trace --stats`."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import resample as R  # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
OUT = sys.argv[2] if len(sys.argv) > 2 else None
m = U.UnevenMap()
m.build(scenes.make_hill_cloud())
nx, ny = int(m.voxel_num[0]), int(m.voxel_num[1])
grid = (nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1])
S, G = scenes.random_queries(B, seed0=1000, occ_r2=m.occ_r2_buffer, grid=grid)
_, G2 = scenes.random_queries(B, seed0=500000, occ_r2=m.occ_r2_buffer, grid=grid)
ka = U.KinoAstar(m, slots=min(B, 4096))
src = U.ALMTrajOpt(m)
src.set_rho(1.0)
t0 = time.perf_counter()
src.plan_goals(ka, S, G)
rec = {"goals": B, "source_plan_goals_s": time.perf_counter() - t0, "source_resident": int(src.L.uph_batch_count(src.h))}
# half of each trajectory's duration (the end row of a dt = 1 s rollout holds it); unsupported slots have no rows and are not switched from
offs, rows = src.rollout(1.0, channels=1, with_end=True)
valid = np.nonzero(np.diff(offs) > 0)[0]
tr = valid[np.arange(B) % len(valid)].astype(np.int32)
ts = 0.5 * rows[offs[tr + 1] - 1, 0]
sw = None
for k in range(2):
    dst = U.ALMTrajOpt(m)
    dst.set_rho(1.0)
    t0 = time.perf_counter()
    plan = dst.replan_goals_upload(ka, src, tr, ts, goals=G2)
    t1 = time.perf_counter()
    sw = plan["switch_states"]
    rec["replan_upload_s_run%d" % k] = t1 - t0
    rec["replan_found"] = int((plan["traj_of"] >= 0).sum())
    rec["replan_search_kernel_s_run%d" % k] = ka.stats()["kernel_ms"] * 1e-3
starts = np.ascontiguousarray(sw[:, [0, 1, 6]])
for k in range(2):
    dst = U.ALMTrajOpt(m)
    dst.set_rho(1.0)
    t0 = time.perf_counter()
    plan = dst.plan_goals_upload(ka, starts, G2)
    rec["plan_upload_s_run%d" % k] = time.perf_counter() - t0
    rec["plan_found"] = int((plan["traj_of"] >= 0).sum())
for k in range(2):
    t0 = time.perf_counter()
    sr = ka.plan_batch(starts, G2, path_cap=768, complete=True)
    t1 = time.perf_counter()
    found = [b for b, r in enumerate(sr) if r["status"] == 0]
    probs = R.resample_batch([sr[b]["path"] for b in found])
    t2 = time.perf_counter()
    for b, p in zip(found, probs):
        p["init_xy"] = np.array(p["init_xy"], dtype=np.float64)
        p["init_xy"][:, 1], p["init_xy"][:, 2] = sw[b, 2:4], sw[b, 4:6]
        p["init_yaw"] = np.array(p["init_yaw"], dtype=np.float64)
        p["init_yaw"][1], p["init_yaw"][2] = sw[b, 7], sw[b, 8]
    t3 = time.perf_counter()
    dst = U.ALMTrajOpt(m)
    dst.set_rho(1.0)
    t4 = time.perf_counter()
    dst.upload(probs)
    t5 = time.perf_counter()
    rec["composed_run%d" % k] = {"search_s": t1 - t0, "resample_s": t2 - t1, "patch_s": t3 - t2, "upload_s": t5 - t4, "sum_s": (t1 - t0) + (t2 - t1) + (t3 - t2) + (t5 - t4),
                                 "found": len(found)}
line = json.dumps(rec, indent=1)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
