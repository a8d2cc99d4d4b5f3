"""Runs tests/test_gpu_pieces.py on the GPU and writes what it measured: the worst error of every (test, variant) of the piece-count sweep and where
it occurred, next to the oracle's own floor on the same problems (the oracle against its rebuild with FMA contraction).

    python tools/piece_sweep_report.py profiles/r07_piece_sweep.txt [extra pytest arguments]

The exit status is pytest's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import pytest
    out = sys.argv[1]
    rc = pytest.main([os.path.join(ROOT, "tests", "test_gpu_pieces.py"), "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider"] + sys.argv[2:])
    import piece_sweep as PS
    import uneven_planner_amd as U
    from oracle import oracle_py as O
    from uneven_planner_amd import scenes
    cells = scenes.analytic_cells()
    og = O.OracleGrid()
    og.set_cells(cells)
    floor = PS.fma_floor(O, og, cells)
    head = ("piece-count sweep, tests/test_gpu_pieces.py (pytest exit status %d), library build %s\n"
            "relative errors against the oracle (T: absolute); bars: 1e-9 (grad f from 64 pieces on: 1e-8; capped solves: 1e-5; fp32 cells: f 1e-11, grad f 1e-10)\n"
            % (int(rc), U._lib.build_id()))
    PS.write_report(out, floor, head)
    print(open(out).read())
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
