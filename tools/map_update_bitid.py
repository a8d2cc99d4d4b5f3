"""uph_map_build's results on the hill, desert and volcano clouds, for bit-identity checks across library builds (the fit kernel and the commit kernel share
their bodies with uph_map_update's column-list forms since that call exists):
python tools/map_update_bitid.py OUT.npz -- cells, c and both occupancy layers of a whole-grid build per cloud.  Run it once per library (UNEVENHIP_LIB
selects another build), then python tools/map_update_bitid.py compare A.npz B.npz [report.txt] (np.array_equal per array)."""
import os
import sys

import numpy as np

if sys.argv[1] == "compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    lines = ["builds: %s  %s" % (a["build"], b["build"])]
    same = sorted(a.files) == sorted(b.files)
    for k in a.files:
        if k == "build" or k not in b.files:
            continue
        eq = a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
        same = same and eq
        lines.append("%-24s shape %-16s bit-identical: %s" % (k, a[k].shape, eq))
    lines.append("ALL IDENTICAL" if same else "DIFFERENT")
    print("\n".join(lines))
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if same else 1)

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402

out = sys.argv[1]
golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
clouds = [("hill", scenes.make_hill_cloud())] + [(nm, np.load(os.path.join(golden, "%s_xyz.npz" % nm))["xyz"]) for nm in ("desert", "vocano")]
arrs = {}
for nm, xyz in clouds:
    m = U.UnevenMap()
    m.build(xyz)
    arrs[nm + "_cells"], arrs[nm + "_c"], arrs[nm + "_occ"], arrs[nm + "_occ_r2"] = m.map_buffer, m.c_buffer, m.occ_buffer, m.occ_r2_buffer
    arrs[nm + "_cloud"] = m.built_cloud().view(np.uint32)
    print("%s: %d points, %d filtered, %d occupied cells" % (nm, len(xyz), len(arrs[nm + "_cloud"]), int(m.occ_buffer.sum())))
    del m
np.savez(out, build=np.array(U._lib.build_id() or ""), **arrs)
print("%s: build %s" % (out, U._lib.build_id()))
