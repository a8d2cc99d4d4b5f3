"""Outputs of the existing calls that share code with uph_refine_upload, for bit-identity checks across library builds:
python tools/refine_bitid.py OUT.npz [B = 1024] -- on B hill goals: uph_plan_upload's staged problems and solved coefficients, the report and the
rollout (every channel, dt 0.05 with the end point), then uph_replan_upload from half of each duration (new goals, and goals == NULL): its switch
states, staged problems and solved coefficients.  Run it once per library (UNEVENHIP_LIB selects another build) and compare the files with
np.array_equal (NaN equal to NaN)."""
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
grid = (nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1])
S, G = scenes.random_queries(B, seed0=1000, occ_r2=m.occ_r2_buffer, grid=grid)
_, G2 = scenes.random_queries(B, seed0=500000, occ_r2=m.occ_r2_buffer, grid=grid)
ka = U.KinoAstar(m)
opt = U.ALMTrajOpt(m)
opt.set_rho(1.0)
arrs = {}


def record(tag, o, res):
    st = o.plan_staged()
    for k in ("init_xy", "end_xy", "init_yaw", "end_yaw", "inner_xy", "inner_yaw"):
        arrs[tag + "staged_" + k] = np.concatenate([np.asarray(p[k], dtype=np.float64).ravel() for p in st])
    arrs[tag + "staged_total_time"] = np.array([p["total_time"] for p in st])
    arrs[tag + "status"] = o.last_plan["status"]
    arrs[tag + "c_xy"] = np.concatenate([r["c_xy"].ravel() for r in res])
    arrs[tag + "c_yaw"] = np.concatenate([r["c_yaw"].ravel() for r in res])


res = [r for r in opt.plan_goals(ka, S, G) if "c_xy" in r]
record("plan_", opt, res)
arrs["plan_report"] = opt.getMaxVxAxAyCurAttSig()
arrs["plan_rollout_offsets"], arrs["plan_rollout"] = opt.rollout(0.05, channels=7, with_end=True)
offs, rows = opt.rollout(1.0, channels=1, with_end=True)
valid = np.nonzero(np.diff(offs) > 0)[0]
tr = valid[np.arange(B) % len(valid)].astype(np.int32)
ts = 0.5 * rows[offs[tr + 1] - 1, 0]
for tag, goals in (("replan_new_", G2), ("replan_same_", None)):
    dst = U.ALMTrajOpt(m)
    dst.set_rho(1.0)
    r2 = [r for r in dst.replan_goals(ka, opt, tr, ts, goals=goals) if "c_xy" in r]
    record(tag, dst, r2)
    arrs[tag + "switch_states"] = dst.last_plan["switch_states"]
np.savez(out, build=np.array(U._lib.build_id() or ""), **arrs)
print("%s: build %s  goals %d  resident %d  rollout rows %d" % (out, U._lib.build_id(), B, len(res), arrs["plan_rollout"].shape[0]))
