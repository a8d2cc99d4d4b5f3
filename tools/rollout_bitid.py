"""Outputs that share device code with the trajectory rollout, for bit-identity checks across library builds:
python tools/rollout_bitid.py OUT.npz [B = 1024] -- the report (uph_report_batch) of a solved hill batch and uph_terrain_pose_query on the
20 000-point set of tests/test_gpu_parity.py.  Run it once per library (UNEVENHIP_LIB selects another build) and compare the files with
np.array_equal."""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402

out = sys.argv[1]
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
m = U.UnevenMap()
m.set_cells(scenes.analytic_cells())
opt = U.ALMTrajOpt(m)
opt.upload(scenes.random_problems(B, seed0=1000))
opt.solve()
res = opt.download(full=False)
report = opt.getMaxVxAxAyCurAttSig()
rng = np.random.default_rng(11)
n = 20000
pos = np.column_stack([rng.uniform(-5.2, 5.2, n), rng.uniform(-5.2, 5.2, n), rng.uniform(-np.pi, np.pi, n)])
pos[:8] = [[0, 0, -3.095], [0, 0, 3.14159], [0, 0, -3.14159], [4.99995, 0, 0], [-4.9998, -4.9998, 1.0], [5.5, 0, 0], [0.0123, 4.97, -3.12], [1, 1, 3.1]]
R, p = m.getTerrainPosBatch(pos)
cxy = np.concatenate([r["c_xy"].ravel() for r in res])
np.savez(out, report=report, pose_R=R, pose_p=p, c_xy=cxy, build=np.array(U._lib.build_id() or ""))
print("%s: build %s  B %d  report rows %d  poses %d" % (out, U._lib.build_id(), B, report.shape[0], n))
