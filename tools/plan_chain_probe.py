"""Goals -> solved trajectories on the hill scene, two ways: python tools/plan_chain_probe.py [B = 16384] [out.json]
  composed: KinoAstar.plan_batch (paths downloaded, path_cap 768, clipped ones searched again) -> resample_batch (uph_resample_batch, host C++)
            -> ctypes packing -> one uph_optimize_batch call (upload, initScaling, solve, download of x and the coefficients)
  chain:    ALMTrajOpt.plan_goals -- uph_plan_upload (search into HBM, resampling + x0 scatter on the device) + uph_batch_solve + download
Wall clock of every stage (perf_counter), each way run twice on its own contexts (the first run allocates device buffers and builds the
MINCO operators); `native_sum` is the composed chain's native part as bench.py's pipeline record counts it: search kernel + host resample +
one warm uph_optimize_batch call.  The kernel times of uph_plan_resample_kernel / uph_plan_scatter_kernel come from a run of this script under
`rocprofv3 --kernel-trace --stats`."""
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
S, G = scenes.random_queries(B, seed0=1000, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]))
ka = U.KinoAstar(m, slots=min(B, 4096))
ka.plan_batch(S[:64], G[:64], path_cap=1)
rec = {"goals": B}


def composed(tag):
    t0 = time.perf_counter()
    sr = ka.plan_batch(S, G, path_cap=768, complete=True)
    t1 = time.perf_counter()
    search_kernel_s = ka.stats()["kernel_ms"] * 1e-3
    paths = [q["path"] for q in sr if q["status"] == 0]
    t2 = time.perf_counter()
    probs = R.resample_batch(paths)
    t3 = time.perf_counter()
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    prep = opt.prepare_boundary(probs)
    t4 = time.perf_counter()
    out = opt.optimize_boundary(probs, prepared=prep)
    t5 = time.perf_counter()
    opt.set_rho(1.0)
    opt.optimize_boundary(probs, prepared=prep)        # the same call on a warm context
    rec[tag] = {"search_wall_s": t1 - t0, "search_kernel_s": search_kernel_s, "resample_s": t3 - t2, "packing_s": t4 - t3, "optimise_first_call_s": t5 - t4,
                "optimise_call_s": opt.last_boundary_s, "wall_s": t5 - t0, "paths_found": len(paths),
                "native_sum_s": search_kernel_s + (t3 - t2) + opt.last_boundary_s}
    return out


def chain(tag, opt):
    t0 = time.perf_counter()
    plan = opt.plan_goals_upload(ka, S, G)
    t1 = time.perf_counter()
    opt.solve()
    t2 = time.perf_counter()
    found = np.nonzero(plan["traj_of"] >= 0)[0]
    res = opt._download_block(plan["n_inner_xy"][found], plan["n_inner_yaw"][found], False)      # (what plan_goals downloads)
    t3 = time.perf_counter()
    out = [dict(status=int(s)) for s in plan["status"]]
    for j, b in enumerate(found):
        out[b] = dict(res[j], status=int(plan["status"][b]))
    t4 = time.perf_counter()
    rec[tag] = {"upload_s": t1 - t0, "search_kernel_s": ka.stats()["kernel_ms"] * 1e-3, "solve_s": t2 - t1, "solve_kernel_s": opt.stats()["kernel_ms"] * 1e-3,
                "download_s": t3 - t2, "per_goal_dicts_s": t4 - t3, "wall_s": t4 - t0, "paths_found": int(found.size)}
    return out


c_out = composed("composed_1")
composed("composed_2")
o1 = U.ALMTrajOpt(m)
o1.set_rho(1.0)
chain("plan_goals_stages_1", o1)
o1.set_rho(1.0)
chain("plan_goals_stages_2", o1)                  # the same context again: warm
for rep in (1, 2):                                # the public call as a whole (the same context, warm)
    o1.set_rho(1.0)
    t0 = time.perf_counter()
    p_out = o1.plan_goals(ka, S, G)
    rec["plan_goals_%d" % rep] = {"wall_s": time.perf_counter() - t0}
found = [b for b, q in enumerate(p_out) if "ret" in q]
rec["same_as_composed"] = bool(len(found) == len(c_out) and all(
    p_out[b]["ret"] == c["ret"] and p_out[b]["cost"] == c["cost"] and np.array_equal(p_out[b]["x"], c["x"]) for b, c in zip(found, c_out)))
rec["plan_goals_wall_vs_composed_native_sum"] = rec["plan_goals_2"]["wall_s"] / rec["composed_2"]["native_sum_s"]
rec["plan_goals_wall_vs_composed_wall"] = rec["plan_goals_2"]["wall_s"] / rec["composed_2"]["wall_s"]
print(json.dumps(rec, indent=1))
if OUT:
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
