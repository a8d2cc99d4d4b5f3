"""Outputs of the existing calls that share code with uph_replan_upload, for bit-identity checks across library builds:
python tools/replan_bitid.py OUT.npz [B = 1024] -- on B hill goals: uph_plan_upload's staged problems (uph_plan_staged) and the solved
coefficients, the report (uph_report_batch) and the rollout (uph_rollout_batch, every channel, dt 0.05 with the end point).  Run it once per
library (UNEVENHIP_LIB selects another build) and compare the files with np.array_equal."""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402

out = sys.argv[1]
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
m = U.UnevenMap()
m.build(scenes.make_hill_cloud())
nx, ny = int(m.voxel_num[0]), int(m.voxel_num[1])
S, G = scenes.random_queries(B, seed0=1000, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]))
ka = U.KinoAstar(m)
opt = U.ALMTrajOpt(m)
opt.set_rho(1.0)
res = [r for r in opt.plan_goals(ka, S, G) if "c_xy" in r]
st = opt.plan_staged()
arrs = {}
for k in ("init_xy", "end_xy", "init_yaw", "end_yaw", "inner_xy", "inner_yaw"):
    arrs["staged_" + k] = np.concatenate([np.asarray(p[k], dtype=np.float64).ravel() for p in st])
arrs["staged_total_time"] = np.array([p["total_time"] for p in st])
arrs["status"] = opt.last_plan["status"]
arrs["c_xy"] = np.concatenate([r["c_xy"].ravel() for r in res])
arrs["c_yaw"] = np.concatenate([r["c_yaw"].ravel() for r in res])
arrs["report"] = opt.getMaxVxAxAyCurAttSig()
arrs["rollout_offsets"], arrs["rollout"] = opt.rollout(0.05, channels=7, with_end=True)
np.savez(out, build=np.array(U._lib.build_id() or ""), **arrs)
print("%s: build %s  goals %d  resident %d  rollout rows %d" % (out, U._lib.build_id(), B, len(st), arrs["rollout"].shape[0]))
