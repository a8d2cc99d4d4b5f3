"""CPU tier of the common-clock query sweep: the conditions tests/query_sweep.py's generator promises, proven from the reference alone (PS.ref_states and the
footprint mirror) on the oracle's coefficients at x0 -- the evaluations test_pieces_cpu.py already caches.  tests/test_gpu_query_sweep.py relies on them: which
launch width a set runs at, that both ends of the clamp fall inside the windows, that the radii, shapes and margins split the samples.  The figures in the
comments were measured with this file; the device's coefficients differ from the oracle's at 1e-9, so the asserted ones keep slack."""
import numpy as np
import pytest

import piece_sweep as PS
import query_sweep as QS

_Q = {}


@pytest.fixture(scope="module")
def sweep(oracle, oracle_grid):
    if "Q" not in _Q:
        cases = PS.all_cases()
        ev = PS.oracle_evals(oracle, oracle_grid, cases)
        _Q["coeffs"] = [ev[c] for c in cases]
        _Q["Q"] = QS.build(_Q["coeffs"])
    return _Q["Q"], _Q["coeffs"]


def test_the_sets_run_at_the_widths_they_are_meant_for(sweep):
    """469 trajectories of 0.36 s to 91.7 s; W1: 645 to 1920 samples (the 256-lane kernels), 548 481 in all; W2: 192 each (the one-wave kernels at their
    longest window), t_to exactly on the last sample; W3: 39 each"""
    Q, coeffs = sweep
    B = len(coeffs)
    total = Q["total"]
    assert B == 469 and 0.3 < total.min() < 0.4 and 91.0 < total.max() < 92.5, (B, total.min(), total.max())
    k1, k2, k3 = Q["W1"]["K"], Q["W2"]["K"], Q["W3"]["K"]
    print("W1: K %d .. %d, %d samples; W2: %d samples; W3: K %d .. %d" % (k1.min(), k1.max(), k1.sum(), k2.sum(), k3.min(), k3.max()))
    assert k1.min() > 600 and k1.max() < 2000 and 520000 < k1.sum() < 580000
    assert (k2 == QS.K_ARRIVAL).all() and k2.sum() == 90048 and (k3 == 39).all()
    assert all(t[-1] == e for t, e in zip(Q["W2"]["taus"], Q["W2"]["tt"]))
    # few pieces meet many, neighbours meet neighbours, nobody meets itself
    w1, w2 = Q["W1"], Q["W2"]
    nxy = np.array([QS.pieces_of(o)[0] for o in coeffs])
    assert (w1["ta"] != w1["tb"]).all() and (w2["ta"] != w2["tb"]).all() and np.array_equal(w2["tb"], (w2["ta"] + 1) % B)
    # (the sweep is ratio-major with 128, 128, 128 and 85 cases: B - 1 - a pairs 1 position piece with 85 and 128 with 86, and 1 yaw piece with 254)
    met = set(zip(nxy[w1["ta"]].tolist(), nxy[w1["tb"]].tolist()))
    nyaw = np.array([QS.pieces_of(o)[1] for o in coeffs])
    assert {(1, 85), (85, 1), (128, 86), (86, 128)} <= met and (1, 254) in set(zip(nyaw[w1["ta"]].tolist(), nyaw[w1["tb"]].tolist()))


def test_both_ends_of_the_clamp_fall_inside_the_windows(sweep):
    """W1: the first sample finds both vehicles before their starts and the last finds both after their arrivals; W2: side a arrives inside the window"""
    Q, _ = sweep
    total = Q["total"]
    w = Q["W1"]
    for q, tau in enumerate(w["taus"]):
        for tr, t0 in ((w["ta"][q], w["t0a"][q]), (w["tb"][q], w["t0b"][q])):
            assert tau[0] - t0 < 0.0 and tau[-1] - t0 > total[tr], q
            assert ((tau - t0 > 0.0) & (tau - t0 < total[tr])).sum() >= 6, q             # ... and moves in between (the shortest lasts 0.36 s)
    w = Q["W2"]
    cross = [tau[0] - w["t0a"][q] < total[w["ta"][q]] < tau[-1] - w["t0a"][q] for q, tau in enumerate(w["taus"])]
    assert all(cross)
    w = Q["W3"]
    assert all(tau[0] - w["t0a"][q] < total[w["ta"][q]] < tau[-1] - w["t0a"][q] for q, tau in enumerate(w["taus"]))


def test_the_radii_split_the_samples(sweep):
    """the median radius leaves samples below and not below in all 469 queries of W1 and in 468 of W2 (the rest: the distance is the median at more than
    half of the samples); radius 0 has nothing below, 100 m everything"""
    Q, _ = sweep
    for name, least in (("W1", 469), ("W2", 455)):
        w = Q[name]
        d2 = [((a[:, :2] - b[:, :2]) ** 2).sum(axis=1) for a, b in zip(w["ref_a"], w["ref_b"])]
        below = np.array([(d < r * r).sum() for d, r in zip(d2, w["median"])])
        mixed = int(((below > 0) & (below < w["K"])).sum())
        print("%s: %d of %d median-radius queries have samples below and not below" % (name, mixed, w["K"].size))
        assert mixed >= least, (name, mixed)
        zero, huge = w["radius"] == 0.0, w["radius"] == 100.0
        assert zero.sum() >= 60 and huge.sum() >= 40 and not (zero & huge).any()
        assert all((d < 100.0 ** 2).all() for d, h in zip(d2, huge) if h)
        assert (w["radius"][~zero & ~huge] == w["median"][~zero & ~huge]).all()


def test_the_footprints_split_the_samples(sweep):
    """with the generator's shapes and margins, by the footprint mirror on the reference poses -- W1: 465 of 469 queries hold overlapping and non-overlapping
    samples, 342 hold more samples below than overlapping, 2 of 548 481 samples are undecided at TOL = 1e-9 m^2; W2: 83 queries mix, 2 of 90 048 samples are
    undecided.  The cap of 0.1 % undecided samples is the one test_gpu_footprint.py works under."""
    Q, _ = sweep
    for name, mix_least, wider_least in (("W1", 400, 250), ("W2", 30, 0)):
        w = Q[name]
        assert (w["sa"] > 0.0).all() and (w["sb"] > 0.0).all() and (w["m"] >= 0.0).all() and (w["m"][::4] == 0.0).all() and (w["m"] > 0.0).sum() > 300
        mix = wider = undecided = 0
        for q in range(w["K"].size):
            pa, pb = w["ref_a"][q][:, [0, 1, 9]], w["ref_b"][q][:, [0, 1, 9]]
            below, clear, over, und = QS.footprint_classes(pa, pb, w["sa"][q], w["sb"][q], w["m"][q])
            mix += bool(over.any() and not over.all())
            wider += bool(below.sum() > over.sum())
            undecided += int(und.sum())
        print("%s: overlap mixes in %d queries, more below than overlapping in %d, %d of %d samples undecided" % (name, mix, wider, undecided, w["K"].sum()))
        assert mix >= mix_least and wider >= wider_least, (name, mix, wider)
        assert undecided <= 1e-3 * w["K"].sum(), (name, undecided)


def test_ref_clock_states_is_ref_states_at_the_clamped_time(sweep):
    Q, coeffs = sweep
    o, total = coeffs[200], Q["total"][200]
    tau = np.array([990.0, 1000.0, 1000.0 + 0.5 * total, 1000.0 + total + 1e-3, 1000.0 + total + 7.0])
    got = QS.ref_clock_states(o, total, tau, 1000.0)
    nx, ny = QS.pieces_of(o)
    want = PS.ref_states(o["c_xy"], o["c_yaw"], o["T_xy"], o["T_yaw"], nx, ny, [0.0, 0.0, (1000.0 + 0.5 * total) - 1000.0, total, total])
    assert np.array_equal(got, want) and not np.array_equal(got[1], got[2]) and not np.array_equal(got[2], got[3])
