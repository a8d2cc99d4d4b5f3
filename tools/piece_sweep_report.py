"""Runs tests/test_gpu_pieces.py and tests/test_gpu_resident_sweep.py on the GPU and writes what they measured: the worst error of every (test, variant)
of the piece-count sweeps and where it occurred, next to the oracle's own floor on the same problems (the oracle against its rebuild with FMA
contraction).  The solve / scaling / penalty kernels go to the first file; the kernels that read a resident trajectory back (report, rollout,
traj_states, check, refine staging: the tests recorded as r_*) with the forced variants' report-equals-rollout flags go to the second.

    python tools/piece_sweep_report.py profiles/r07_piece_sweep.txt profiles/r08_resident_sweep.txt [extra pytest arguments]

The exit status is pytest's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import pytest
    out, out_res = sys.argv[1], sys.argv[2]
    rc = pytest.main([os.path.join(ROOT, "tests", "test_gpu_pieces.py"), os.path.join(ROOT, "tests", "test_gpu_resident_sweep.py"), "-m", "gpu", "-q", "-s",
                      "-p", "no:cacheprovider"] + sys.argv[3:])
    import piece_sweep as PS
    import uneven_planner_amd as U
    from oracle import oracle_py as O
    from uneven_planner_amd import scenes
    cells = scenes.analytic_cells()
    og = O.OracleGrid()
    og.set_cells(cells)
    resident = lambda test: test.startswith("r_")
    head = ("piece-count sweep, tests/test_gpu_pieces.py (pytest exit status %d for both sweep files), library build %s\n"
            "relative errors against the oracle (T: absolute); bars: 1e-9 (grad f from 64 pieces on: 1e-8; capped solves: 1e-5; fp32 cells: f 1e-11, grad f 1e-10)\n"
            % (int(rc), U._lib.build_id()))
    PS.write_report(out, PS.fma_floor(O, og, cells), head, only=lambda test: not resident(test))
    head = ("resident-trajectory sweep, tests/test_gpu_resident_sweep.py (pytest exit status %d for both sweep files), library build %s\n"
            "r_report: against the oracle's report on the downloaded coefficients, maxima = |d| / (|ref| + 1e-3) over columns 0-5 and nonhol = |d| / max(1, ref), bar 1e-9;\n"
            "  rollout_sum = column 6 against the sum of the context's own rollout (bar 1e-12, automatic variant only)\n"
            "r_report_vs_rollout_bits: report_ne_rollout = 1 when the first six columns are not bit-equal to report_from_terms of the context's own rollout\n"
            "  (asserted 0 for the automatic variant, recorded for the forced ones)\n"
            "r_rollout_*, r_traj_states, r_refine_staging_*: |d| / max(1, |ref|) against ref_states / ref_terms / the pose query, bars 1e-12 (poses 1e-15, end_xy 1e-9 absolute)\n"
            "the check (test_check_every_piece_count) is compared bit for bit and records nothing\n"
            % (int(rc), U._lib.build_id()))
    PS.write_report(out_res, PS.report_floor(O, og, cells), head, only=resident)
    print(open(out).read())
    print(open(out_res).read())
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
