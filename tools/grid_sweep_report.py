"""Runs tests/test_gpu_grids.py on the GPU and writes what it measured: the worst error of every test on every grid of tests/grid_cases.py
(non-square grids, 38 / 64 / 65 / 127 yaw bins), and for the plane-fit build the fraction of cells off by more than 1e-9.

    python tools/grid_sweep_report.py profiles/grid_sweep.txt [extra pytest arguments]

The exit status is pytest's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import pytest
    out = sys.argv[1]
    rc = pytest.main([os.path.join(ROOT, "tests", "test_gpu_grids.py"), "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider", "--durations=15"] + sys.argv[2:])
    import grid_cases as GC
    import uneven_planner_amd as U
    head = ("grid sweep, tests/test_gpu_grids.py (pytest exit status %d), library build %s\n"
            "grids (nx x ny x nyaw): %s\n"
            "1_lookups, 1_frontend, 2_f32_lookups: absolute (grads: relative to the largest), bars 1e-12 (pose_R, pose_z 1e-15; fp32 grads 1e-10)\n"
            "3_build_*: off_fraction = compared cells off by more than 1e-9 (bar 1e-3; half cloud: among the cells degenerate on neither side, and\n"
            "  off_fraction_all_cells with bar 1e-2), median (bar 1e-12; half cloud: of |dz|), occ_disagree (bar 1e-3; half cloud: non-degenerate cells);\n"
            "  occupied_cells / empty_cells are counts over the compared slabs of the oracle's grid\n"
            "6_fbm_fill: absolute against the numpy restatement, bars z 1e-10, sigma 1e-9, zb 1e-8\n"
            "7_*: relative errors against the oracle (T: absolute, bar 1e-13), bars 1e-9, capped solves 1e-5; variants auto and 128x2, storage f64 / f32\n"
            "7_penalty: against the oracle's calConstrainCostGrad on the device's resident trajectory; durations_one_double_apart = problems whose\n"
            "  device durations differ from the oracle's in the last bit\n"
            "8_local_frames: bars f 1e-12, grad 1e-11\n"
            "10_rollout: |d| / max(1, |ref|), bars 1e-12 (poses 1e-15, end_xy 1e-9 absolute)\n"
            "the occupancy layers, slabs / tiles / multi-slab builds, the map update, the search, the plan chain and the check are compared exactly\n"
            % (int(rc), U._lib.build_id(), "  ".join("%s %dx%dx%d" % ((k,) + v) for k, v in GC.DIMS.items())))
    GC.write_report(out, head)
    print(open(out).read())
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
