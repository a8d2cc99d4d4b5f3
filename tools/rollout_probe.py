"""Cost of the trajectory rollout (uph_rollout_*) on a solved hill batch: python tools/rollout_probe.py [B = 16384].
Prints the solve launch, then the median wall milliseconds (plan + launch + synchronise; the host variant also its PCIe copy) of
  POSE only at 0.03 s with the end point (visSE3Traj's path), all channels at 0.01 s (the report's grid), device variant against host variant.
The kernel's own time comes from a run under `rocprofv3 --kernel-trace --stats -- python tools/rollout_probe.py` (uph_rollout_kernel)."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import torch                                # noqa: E402
import uneven_planner_amd as U              # noqa: E402
from uneven_planner_amd import scenes       # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
REPS = 5
m = U.UnevenMap()
m.set_cells(scenes.analytic_cells())
opt = U.ALMTrajOpt(m)
probs = scenes.random_problems(B, seed0=1000)
opt.upload(probs)
opt.solve()
st = opt.stats()
print("B = %d  solve launch %.1f ms" % (B, st["kernel_ms"]))
L = opt.L


def timed(fn):
    fn()                                    # warm-up (buffers grow once)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


for name, dt, ch, we in (("pose 0.03 s + end", 0.03, 4, 1), ("all channels 0.01 s", 0.01, 7, 0)):
    offs = opt.rollout_plan(dt, we)
    ncol = len(U.alm_traj_opt.rollout_columns(ch))
    rows = int(offs[-1])
    dev = torch.empty((rows, ncol), dtype=torch.float64, device="cuda:0")
    host = np.empty((rows, ncol))
    t_plan = timed(lambda: opt.rollout_plan(dt, we))
    t_dev = timed(lambda: U._lib.check(L.uph_rollout_batch_dev(opt.h, dt, we, ch, 0, B, C.c_void_p(dev.data_ptr())), "dev"))
    t_host = timed(lambda: U._lib.check(L.uph_rollout_batch(opt.h, dt, we, ch, 0, B, host.ctypes.data_as(U._lib.DP)), "host"))
    same = np.array_equal(dev.cpu().numpy(), host)
    print("%-22s rows %10d  %6.2f GB  plan %6.2f ms  device variant %8.2f ms  host variant %8.2f ms  (device == host: %s)"
          % (name, rows, rows * ncol * 8 / 1e9, t_plan, t_dev, t_host, same))
    del dev, host
    torch.cuda.empty_cache()
