"""Cost of checking a solved hill batch against the map: python tools/check_probe.py [B = 16384] [out.json] [repeats = 7]
Source: B hill goals planned and solved by ALMTrajOpt.plan_goals.  Every valid resident trajectory, full windows, dt 0.01 with the end point.  Three
things on the same samples, `repeats` times each, alternated:
  check   ALMTrajOpt.check -- uph_check_kernel: HIP events around the launch (check_kernel_ms), and the wall clock of the whole blocking call
  report  getMaxVxAxAyCurAttSig -- the solver kernel's MODE 3 launch: HIP events (uph_batch_stats)
  rollout uph_rollout_batch_dev, TERRAIN channel only, into a device tensor: the wall clock of the blocking call (launch records up, kernel, stream
          synchronised); the library keeps no event pair around this launch
`rollout-only` as the first argument measures the rollout alone: python tools/check_probe.py rollout-only [B] [out.json] [repeats], for a run on
another build of the library (UNEVENHIP_LIB: the parent commit's, which has no check).  The kernel-only durations of all three come from a run of
this script under `rocprofv3 --kernel-trace --stats`."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402

args = sys.argv[1:]
only_rollout = bool(args) and args[0] == "rollout-only"
if only_rollout:
    args = args[1:]
B = int(args[0]) if len(args) > 0 else 16384
OUT = args[1] if len(args) > 1 else None
REP = max(5, int(args[2])) if len(args) > 2 else 7
m = U.UnevenMap()
m.build(scenes.make_hill_cloud())
nx, ny = int(m.voxel_num[0]), int(m.voxel_num[1])
S, G = scenes.random_queries(B, seed0=1000, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]))
ka = U.KinoAstar(m, slots=min(B, 4096))
src = U.ALMTrajOpt(m)
src.set_rho(1.0)
src.plan_goals(ka, S, G)
offs = src.rollout_plan(0.01, True)
rec = {"build": U._lib.build_id(), "goals": B, "resident": int(src.L.uph_batch_count(src.h)), "dt": 0.01, "with_end": True, "repeats": REP,
       "rows": int(offs[-1]), "terrain_rollout_bytes": int(offs[-1]) * 7 * 8}
valid = np.nonzero(np.diff(offs) > 0)[0].astype(np.int32)
rec["trajectories"] = int(valid.size)
runs = {"rollout_terrain_call_ms": []}
if not only_rollout:
    runs.update(check_kernel_ms=[], check_call_ms=[], report_kernel_ms=[])
for k in range(REP + 1):                    # the first round allocates device buffers: not recorded
    t0 = time.perf_counter()
    _, rows = src.rollout(0.01, channels=2, with_end=True, device=True)
    ms = [("rollout_terrain_call_ms", 1e3 * (time.perf_counter() - t0))]
    del rows
    if not only_rollout:
        t0 = time.perf_counter()
        c = src.check(valid, dt=0.01, with_end=True)
        ms += [("check_call_ms", 1e3 * (time.perf_counter() - t0)), ("check_kernel_ms", src.check_kernel_ms())]
        src.getMaxVxAxAyCurAttSig()
        ms.append(("report_kernel_ms", src.stats()["kernel_ms"]))
    if k:
        for name, v in ms:
            runs[name].append(v)
if not only_rollout:
    rec["samples_checked"] = int(c["counts"][:, 0].sum())
    rec["violating_trajectories"] = int((c["first_mask"] != 0).sum())
    rec["occupied_trajectories"] = int((c["counts"][:, 2] > 0).sum())
    rec["check_output_bytes"] = int(valid.size) * 136
for name, v in runs.items():
    rec[name] = dict(runs=[round(x, 4) for x in v], median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
line = json.dumps(rec, indent=1)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
