"""Cost of the body layer: python tools/body_layer_probe.py [B = 4096] [out.json = profiles/body_layer_probe.json] [repeats = 15]
The hill map; the car (0.45 + 0.15 m x 2 * 0.3 m) at its conservative margin (uph_body_layer_margin: 0.062 m, stencil radius 13 columns), layers XY | OUTSIDE.
`repeats` rounds after a warm-up round, the calls alternated inside a round:
  build    BodyLayer.build()                   -- uph_body_layer_kernel over the whole grid: HIP events around the launch, and the wall clock of the blocking call
  update   BodyLayer.update(a 20 x 20 rect)    -- the same kernel over the rect grown by the stencil radius
  recipe   what a caller had to do without the layer, stated as such and timed on the host: get_cells' occ_r2 through body_layer_rows in numpy (the upload
           that recipe would also need has no entry point to time)
  search   B hill queries through KinoAstar.plan_batch (paths clipped at 64 poses, as tools/kino_probe.py), default and with the layer set: searches per second of the
           blocking call and the kernel's milliseconds.  The layer read is 3-D where occ_r2 is 2-D, and some goals are blocked for the body: the status histograms of
           both modes go to the JSON.
  large    BodyLayer.build() of a 6 m x 1 m body (3.0, 3.0, 0.5) at margin 0, stencil radius 61 of the 64 the kernel admits: each 8 x 8 tile stages 130 x 130
           columns for its 64, and 130 of its 256 threads scan -- the kernel's worst shape on this grid
Median (min - max) of every series goes to the JSON.  Nothing is asserted."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402
from uneven_planner_amd.body_layer import body_layer_rows       # noqa: E402

args = sys.argv[1:]
B = int(args[0]) if len(args) > 0 else 4096
OUT = args[1] if len(args) > 1 else os.path.join("profiles", "body_layer_probe.json")
REP = max(3, int(args[2])) if len(args) > 2 else 15
CAR, RECT = np.array([0.45, 0.15, 0.3]), (90, 110, 90, 110)
m = U.UnevenMap()
m.build(scenes.make_hill_cloud())
nx, ny, nyaw = (int(v) for v in m.voxel_num)
layer = U.BodyLayer(m, CAR)
info = layer.info()
st = layer.stencil()
cols = (st["hi"] - st["lo"] + 1).clip(min=0).sum(axis=1)
rec = {"build": U._lib.build_id(), "grid": [nx, ny, nyaw], "shape": CAR.tolist(), "margin": info["margin"], "layers": info["layers"], "R": info["R"],
       "stencil_columns_per_bin": [int(cols.min()), int(cols.max())], "layer_bytes": nx * ny * nyaw, "update_rect": list(RECT), "repeats": REP}


def series(runs):
    a = np.array(runs, dtype=np.float64)
    return {"runs": [round(float(v), 4) for v in a], "median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


occ2 = m.occ_r2_buffer.reshape(nx, ny)
got = layer.get()
rec["layer_bytes_set"] = int(got.sum())
rec["equals_mirror"] = bool(np.array_equal(got, body_layer_rows(occ2, st["lo"], st["hi"], info["layers"])))
S, G = scenes.random_queries(B, seed0=1000, occ_r2=m.occ_r2_buffer, grid=(nx, ny, m.xy_resolution, m.map_origin[0], m.map_origin[1]))
ka = U.KinoAstar(m, slots=min(B, 4096))
big = U.BodyLayer(m, (3.0, 3.0, 0.5), 0.0)
rec["large_R"] = big.info()["R"]
t = {k: [] for k in ("large_build_kernel_ms", "large_build_call_ms", "build_kernel_ms", "build_call_ms", "update_kernel_ms", "update_call_ms", "recipe_numpy_ms", "search_default_call_ms", "search_default_kernel_ms",
                     "search_body_call_ms", "search_body_kernel_ms")}
hist = {}
for rnd in range(REP + 1):
    row = {}
    row["build_call_ms"] = timed(layer.build)
    row["build_kernel_ms"] = layer.kernel_ms()
    row["large_build_call_ms"] = timed(big.build)
    row["large_build_kernel_ms"] = big.kernel_ms()
    row["update_call_ms"] = timed(lambda: layer.update(RECT))
    row["update_kernel_ms"] = layer.kernel_ms()

    def recipe():
        b = np.zeros(nx * ny, dtype=np.int8)
        U._lib.check(m.L.uph_map_get_cells(m.h, None, None, None, b.ctypes.data_as(C.c_char_p)), "uph_map_get_cells")
        body_layer_rows(b.reshape(nx, ny), st["lo"], st["hi"], info["layers"])
    row["recipe_numpy_ms"] = timed(recipe)
    for mode, lay in (("default", None), ("body", layer)):
        ka.set_body_layer(lay)
        out = []
        row["search_%s_call_ms" % mode] = timed(lambda: out.extend(ka.plan_batch(S, G, path_cap=64, complete=False)))
        row["search_%s_kernel_ms" % mode] = ka.stats()["kernel_ms"]
        h = np.bincount([r["status"] for r in out], minlength=7).tolist()
        assert hist.setdefault(mode, h) == h        # the search is deterministic
    if rnd > 0:
        for k, v in row.items():
            t[k].append(v)
for k, v in t.items():
    rec[k] = series(v)
rec["searches"] = B
rec["status_histogram"] = {k: dict(zip(("ok", "start", "goal", "no_path", "pool", "cap", "internal"), v)) for k, v in hist.items()}
for mode in ("default", "body"):
    rec["search_%s_per_s" % mode] = B / (rec["search_%s_call_ms" % mode]["median"] * 1e-3)
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
fmt = lambda k: "%.3f (%.3f - %.3f)" % (rec[k]["median"], rec[k]["min"], rec[k]["max"])
print("body layer probe, build %s: grid %s, R %d, %d-%d columns per bin, equals mirror: %s" % (rec["build"], rec["grid"], rec["R"], cols.min(), cols.max(), rec["equals_mirror"]))
for k in t:
    print("  %-26s %s ms" % (k, fmt(k)))
print("  searches/s default %.0f, body %.0f; statuses %s" % (rec["search_default_per_s"], rec["search_body_per_s"], rec["status_histogram"]))
