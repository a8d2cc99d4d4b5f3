"""Runs tests/test_gpu_query_sweep.py on the GPU and writes what it measured: for the queries that read resident trajectories back on a window or a common clock
(locate / within, extent, separation, footprints, the delay sweeps, the fleet calls) over every piece count 1..128 x four yaw ratios, the worst error of each
recorded test (the names starting with q_), per quantity and where it occurred.

    python tools/query_sweep_report.py profiles/query_sweep.txt [extra pytest arguments]

The exit status is pytest's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import pytest
    out = sys.argv[1]
    rc = pytest.main([os.path.join(ROOT, "tests", "test_gpu_query_sweep.py"), "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider"] + sys.argv[2:])
    import piece_sweep as PS
    import uneven_planner_amd as U
    head = ("query sweep, tests/test_gpu_query_sweep.py (pytest exit status %d), library build %s\n"
            "q_clock_states: uph_traj_states at the clock kernels' sample times u = tau - t0 (W1: full windows at 0.05 s, W2: 192 samples at 0.01 s around an arrival,\n"
            "  W3: W2's windows at 0.05 s; side a / b of the pair) against query_sweep.ref_clock_states, |d| / max(1, |ref|) per column block, bar 1e-12\n"
            "q_separation: |sqrt(min_d2) - sqrt(ref)| in metres against ref_clock_states alone; recorded, no bar (the outputs are held bit for bit to the mirrors on\n"
            "  the device's states)\n"
            "q_locate: the largest |g| / G of the refined time (P3 of tests/test_gpu_locate.py, G = 1e-9 max(1, |v|^2 + |e| |a|)) on x0, which is no solved trajectory;\n"
            "  recorded, no bar\n"
            "separation, extent, the delay sweeps, locate's coarse stage, within and the fleet calls are compared bit for bit and record nothing\n"
            % (int(rc), U._lib.build_id()))
    PS.write_report(out, None, head, only=lambda test: test.startswith("q_"))
    print(open(out).read())
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
