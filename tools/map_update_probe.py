"""Cost of updating the hill map from a scan of a box against rebuilding it: python tools/map_update_probe.py [out.json] [repeats = 7]
Per box side 0.5, 1, 2 and 4 m (centred at (0.09, 0.11)): one warm-up, then `repeats` rounds of
  update  uph_map_update of the box with a fresh scan of it (a jittered lattice at the cloud's density, a mound that moves from round to round): its stages
          (uph_map_update_stages; the fit kernel by HIP events) and the refit column count
  build   uph_map_build, on a second map, of the same merged RAW cloud (the hill cloud without the box's points ++ the scan): its stages
          (uph_map_build_stages) -- the yardstick
alternated in the same run, no host download in either.  spread = max - min over the rounds."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402
from map_update_cases import in_box, scan   # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
REP = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
xyz = scenes.make_hill_cloud()
density = 316 / 12.0                        # lattice points per metre of make_hill_cloud
rec = {"build": U._lib.build_id(), "cloud_points": int(len(xyz)), "repeats": REP, "boxes": []}
summ = lambda v: dict(runs=[round(float(x), 4) for x in v], median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), spread=float(np.max(v) - np.min(v)))
for side in (0.5, 1.0, 2.0, 4.0):
    box = (0.09 - side / 2, 0.09 + side / 2, 0.11 - side / 2, 0.11 + side / 2)
    mu, mb = U.UnevenMap(), U.UnevenMap()
    mu.build(xyz, download=False)
    keep = xyz[~in_box(xyz, box)]
    ust, bst, nref, nchg, full = [], [], [], [], 0
    for k in range(REP + 1):                # the first round allocates device buffers: not recorded
        new = scan(box, seed=100 + k, n_side=max(4, int(round(side * density))), mound=0.2, sigma=0.09, centre=(0.09 + 0.02 * k, 0.11 - 0.015 * k), extras=False)
        info = mu.update(box, new, download=False)
        mb.build(np.concatenate([keep, new]), download=False)
        if k:
            ust.append(info["stages_ms"]), bst.append(mb.build_stats()["stages_ms"]), nref.append(info["n_refit"]), nchg.append(info["n_changed"])
            full += info["full_refit"]
    b = {"side_m": side, "box": [round(v, 4) for v in box], "scan_points": int(len(new)), "cloud_after": info["n_cloud"], "n_refit": nref, "n_changed": nchg,
         "full_refits": full, "update_ms": {s: summ([u[s] for u in ust]) for s in ust[0]}, "build_ms": {s: summ([u[s] for u in bst]) for s in bst[0]}}
    for s, t in (("call", "call"), ("kernel", "kernel")):
        u, f = b["update_ms"][s], b["build_ms"][t]
        b["%s_saving_ms" % s] = f["median"] - u["median"]
        b["%s_saving_beyond_spread" % s] = bool(f["min"] - u["max"] > 0.0 and f["median"] - u["median"] > max(f["spread"], u["spread"]))
    rec["boxes"].append(b)
    # the updated map still equals a rebuild of its resident cloud
    mu.download()
    chk = U.UnevenMap().build_filtered(mu.built_cloud())
    b["equals_rebuild"] = bool(np.array_equal(mu.map_buffer, chk.map_buffer) and np.array_equal(mu.occ_buffer, chk.occ_buffer))
    del mu, mb, chk
line = json.dumps(rec, indent=1)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
