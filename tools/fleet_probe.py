"""python tools/fleet_probe.py [OUT.json]: adopting 4096 hill trajectories (capped solves) into a TrajFleet in one call -- uph_fleet_kernel_ms and the wall time of the
call, nine repetitions -- beside uph_batch_download with c_xy / c_yaw for the same 4096, the only route without a fleet; checks that the fleet holds the download's doubles"""
import ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import uneven_planner_amd as U
from uneven_planner_amd import scenes, _lib
B = 4096
m = U.UnevenMap()
m.build(scenes.make_hill_cloud())
nx, ny = int(m.voxel_num[0]), int(m.voxel_num[1])
probs = scenes.random_problems(B, seed0=1000, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]))
opt = U.ALMTrajOpt(m, params=dict(inner_max_iter=12.0, max_iter=1.0))
opt.set_rho(1.0)
opt.upload(probs)
opt.solve()
sizes = opt._sizes
res = (_lib.Result * B)()
cx = [np.zeros(12 * s["Nxy"]) for s in sizes]
cy = [np.zeros(6 * s["Nyaw"]) for s in sizes]
for i in range(B):
    res[i].c_xy = cx[i].ctypes.data_as(_lib.DP); res[i].c_yaw = cy[i].ctypes.data_as(_lib.DP)
dl = []
for _ in range(9):
    t = time.perf_counter(); rc = opt.L.uph_batch_download(opt.h, res); dl.append((time.perf_counter() - t) * 1e3); assert rc == 0
fleet = U.TrajFleet(m, B)
tr = np.arange(B, dtype=np.int32)
sl = np.random.default_rng(1).permutation(B).astype(np.int32)
km, wall = [], []
for _ in range(9):
    t = time.perf_counter(); fleet.adopt(opt, tr, sl); wall.append((time.perf_counter() - t) * 1e3); km.append(fleet.adopt_kernel_ms())
g = fleet.get(sl)
ok = all(np.array_equal(g["c_xy"][q, :cx[q].size], cx[q]) and np.array_equal(g["c_yaw"][q, :cy[q].size], cy[q]) for q in range(B))
doubles = int(sum(c.size for c in cx) + sum(c.size for c in cy))
out = dict(B=B, coefficient_doubles=doubles, coefficient_MB=doubles * 8 / 1e6, mean_Nxy=float(np.mean([s["Nxy"] for s in sizes])), adopt_kernel_ms=sorted(km), adopt_kernel_ms_median=float(np.median(km)),
           adopt_call_wall_ms_median=float(np.median(wall)), download_wall_ms=sorted(dl), download_wall_ms_median=float(np.median(dl)), equal=bool(ok))
print(json.dumps(out))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"))
