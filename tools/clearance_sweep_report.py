"""Runs tests/test_gpu_clearance_sweep.py on the GPU and tests/test_clearance_sweep_cpu.py (the emulator), and writes what they measured: the worst
error of every (test, variant) of the clearance term's sweep against the oracle with the term and where it occurred, and the disagreement of the oracle's two
builds (default and -DORACLE_EIGEN_REDUX=1) on every solve case, with and without the term.

    python tools/clearance_sweep_report.py profiles/clearance_sweep.txt [extra pytest arguments]

The exit status is pytest's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import pytest
    out = sys.argv[1]
    rc = pytest.main([os.path.join(ROOT, "tests", "test_gpu_clearance_sweep.py"), os.path.join(ROOT, "tests", "test_clearance_sweep_cpu.py"), "-q", "-s", "-p", "no:cacheprovider"]
                     + sys.argv[2:])
    import piece_sweep as PS
    import uneven_planner_amd as U
    from oracle import oracle_py as O
    from uneven_planner_amd import scenes
    cells = scenes.analytic_cells()
    og = O.OracleGrid()
    og.set_cells(cells)
    term = (PS.CLR_RMAX, PS.CLR_D_SAFE, PS.CLR_SOLVE_WEIGHT)
    fit = PS.solve_fitness(O, og, cells, PS.clearance_layer(), term)
    head = ("clearance-term sweep, tests/test_gpu_clearance_sweep.py (s*) and tests/test_clearance_sweep_cpu.py (cpu_*: the emulator) (pytest exit status %d), library build %s\n"
            "layer: lattice %s on %s, rmax %d; d_safe %.3g m; weight %.3g (evaluations and penalty), %.3g (solves)\n"
            "relative errors against the oracle with the term (T: absolute); bars: s1 / s5 / s6 1e-9 (grad f from 64 pieces on: 1e-8, T 1e-13), s2 / s4 / pen_* 1e-9,\n"
            "s3 1e-5; s3's cost allows for the oracle's own jump (piece_sweep.cost_jumps, cost_error): *_cost_raw holds the plain relative difference of the cost\n"
            "next to the largest jump, per variant; the table below has the jump of every case\n"
            % (int(rc), U._lib.build_id(), PS.CLR_LATTICE, PS.CLR_DIMS, PS.CLR_RMAX, PS.CLR_D_SAFE, PS.CLR_WEIGHT, PS.CLR_SOLVE_WEIGHT))
    PS.write_report(out, None, head)
    with open(out, "a") as fh:
        fh.write("\nthe oracle against the oracle rebuilt with -DORACLE_EIGEN_REDUX=1 on the solve cases (ratio 2, SOLVE_PARAMS, rho 1): counters equal, x and cost apart (relative)\n")
        fh.write("%-5s %-22s %-11s %-11s %-11s %-11s %-11s %-10s %s\n" % ("Nxy", "counters on / off", "x on", "x off", "cost on", "cost off", "term moves x", "cost jump", "fit"))
        for n, r in fit.items():
            fh.write("%-5d %-22s %-11.3e %-11.3e %-11.3e %-11.3e %-11.3e %-10.3e %s\n" % (n, "%s / %s" % (r["counters_on"], r["counters_off"]), r["dx_on"], r["dx_off"], r["dcost_on"],
                                                                                  r["dcost_off"], r["moved"], r["cost_jump"], r["fit"]))
        fh.write("\nthe returned cost of every solve case whose oracle cost lies on a jump: relative difference to the oracle's as measured (on the oracle's side of the jump: about 0;\n"
                 "on the other side: the jump), per variant; bar: within 1e-5 (device) / 1e-7 (emulator) of one of the two\n")
        for (test, variant), raw in sorted(PS.COST_RAW.items()):
            for where, r in sorted(raw.items()):
                if r["oracle_jump"] > 0.0:
                    fh.write("%-24s %-8s %-12s cost_raw %-11.3e oracle_jump %-11.3e -> %.3e\n" % (test, variant, where, r["cost_raw"], r["oracle_jump"],
                                                                                                min(r["cost_raw"], abs(r["cost_raw"] - r["oracle_jump"]))))
        fh.write("left out of the solve tests: %s\n" % (list(PS.CLR_SOLVE_LEFT_OUT) or "none"))
    print(open(out).read())
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
