"""Common-clock queries over the piece sweep (TEST INFRASTRUCTURE): deterministic windows, starts, radii and footprints for every trajectory of
piece_sweep.all_cases(), and the plain reference of a vehicle's state on the clock.

The kernels that read resident trajectories on a common clock (uph_extent_kernel, uph_separation_kernel / uph_footprint_kernel, uph_delay_sweep_kernel,
uph_delay_extent_kernel) inline the trajectory evaluation once per vehicle, with that vehicle's piece counts, durations and coefficient offsets, and clamp the
vehicle's own time with the smaller of two running sums.  This module pairs the sweep's trajectories so that those differ as much as they can inside one
query, and places the windows so that both ends of the clamp fall inside them:

  W1 "full"     trajectory a against b = B - 1 - a (1 piece meets 85 with 254 yaw pieces, 128 meet 86; a + 1 where that is a itself), starts anywhere in 5 s
                around 1000 s, a window from before both starts to after both arrivals at dt = 0.05: 645 to 1920 samples, the 256-lane kernels.
  W2 "arrival"  a against its neighbour in the coefficient arrays b = (a + 1) mod B, starts 0.4 s apart at most, 192 samples at dt = 0.01 -- the longest
                window of the one-wave kernels -- around a's arrival, t_to exactly on the last sample.
  W3            W2's windows at W1's dt (39 samples).  A call takes ONE dt, so W1 and W2 cannot share a launch; W1 + W3 is the launch that mixes both widths.

No fixtures here and nothing of the product but the numpy mirrors of its documented rules: tests/test_query_sweep_cpu.py proves the generator's conditions on
the oracle's coefficients, tests/test_gpu_query_sweep.py runs it on the device's.  (The device's coefficients differ from the oracle's at 1e-9, so the two
tiers see the same windows -- the draws do not depend on the coefficients -- with totals and radii that differ in the last digits.)
"""
import numpy as np

import piece_sweep as PS
from uneven_planner_amd.alm_traj_opt import footprint_clearance2, separation_times

SEED = 4690
DT_FULL, DT_ARRIVAL, K_ARRIVAL = 0.05, 0.01, 192
TOL = 1e-9                                      # test_gpu_footprint.py's TOL, m^2
SETS = ("W1", "W2", "W3")


def pieces_of(o):
    return o["c_xy"].shape[0] // 6, o["c_yaw"].shape[0] // 6


def total_of(o):
    return PS.total_duration(o["T_xy"], o["T_yaw"], *pieces_of(o))


def ref_clock_states(out_b, total_b, tau, t0):
    """the state of the vehicle (trajectory out_b = dict(c_xy, c_yaw, T_xy, T_yaw), started at t0) at the clock's times tau: PS.ref_states at u = tau - t0
    clamped to [0, total_b] -- at its start before it leaves, at its goal after it arrives"""
    u = np.asarray(tau, dtype=np.float64) - float(t0)
    u = np.where(u <= 0.0, 0.0, np.where(u >= total_b, total_b, u))
    nx, ny = pieces_of(out_b)
    return PS.ref_states(out_b["c_xy"], out_b["c_yaw"], out_b["T_xy"], out_b["T_yaw"], nx, ny, u)


def _shapes(rng, n):
    """front, rear, half width of a small car.  No zero component: all sweep trajectories start in one pose, two parked vehicles with a zero extent would
    sit at g = 0 exactly"""
    return np.stack([rng.uniform(0.1, 0.5, n), rng.uniform(0.0, 0.3, n), rng.uniform(0.05, 0.25, n)], axis=1)


def windows(total):
    """the queries of W1, W2 and W3 from the trajectories' durations total (B,): per set a dict of ta, tb (int32), t0a, t0b, tf, tt, sa, sb (n, 3), m and
    the scalar dt.  Every draw has a fixed place in one stream, whatever the durations are."""
    total = np.asarray(total, dtype=np.float64)
    B = total.shape[0]
    rng = np.random.default_rng(SEED)
    a = np.arange(B, dtype=np.int32)
    U = lambda lo, hi: rng.uniform(lo, hi, B)
    # W1
    b = (B - 1 - a).astype(np.int32)
    b[b == a] += 1
    t0a, t0b = 1000.0 + U(0.0, 5.0), 1000.0 + U(0.0, 5.0)
    tf = np.minimum(t0a, t0b) - U(0.2, 1.0)
    tt = np.maximum(t0a + total[a], t0b + total[b]) + U(0.2, 1.0)
    w1 = dict(ta=a, tb=b, t0a=t0a, t0b=t0b, tf=tf, tt=tt, dt=DT_FULL)
    # W2: a crosses its arrival clamp about the middle of the window
    b = ((a + 1) % B).astype(np.int32)
    t0a = 1000.0 + U(0.0, 2.0)
    t0b = t0a + U(-0.4, 0.4)
    tf = t0a + total[a] - 0.96 + U(-0.2, 0.2)
    tt = tf + (K_ARRIVAL - 1) * DT_ARRIVAL                          # tau_191 as separation_times forms it: exactly on the last sample
    w2 = dict(ta=a, tb=b, t0a=t0a, t0b=t0b, tf=tf, tt=tt, dt=DT_ARRIVAL)
    w3 = dict(w2, dt=DT_FULL)
    out = dict(W1=w1, W2=w2, W3=w3)
    for name in ("W1", "W2"):
        out[name].update(sa=_shapes(rng, B), sb=_shapes(rng, B), m=U(0.0, 0.3) * (np.arange(B) % 4 != 0))
    out["W3"].update({k: out["W2"][k] for k in ("sa", "sb", "m")})
    return out


def median_radii(pa, pb):
    """per query the median distance of its samples: first_t / last_t fall anywhere in the window"""
    return np.array([np.sqrt(np.median(((x[:, :2] - y[:, :2]) ** 2).sum(axis=1))) for x, y in zip(pa, pb)])


def build(coeffs):
    """everything of the sweep's queries that follows from the trajectories coeffs[b] = dict(c_xy, c_yaw, T_xy, T_yaw) alone: per set of SETS the windows()
    entries, taus (per query the sample times), ref_a / ref_b (per query the (K, 10) reference states of the two vehicles), K, median (the median
    radii) and radius (the median, every 7th query 0 -- nothing is below --, every 11th 100 m -- everything is)."""
    total = np.array([total_of(o) for o in coeffs])
    Q = windows(total)
    Q["total"] = total
    for name in SETS:
        w = Q[name]
        n = w["ta"].shape[0]
        w["taus"] = [separation_times(w["tf"][q], w["tt"][q], w["dt"]) for q in range(n)]
        w["K"] = np.array([t.shape[0] for t in w["taus"]])
        w["ref_a"] = [ref_clock_states(coeffs[w["ta"][q]], total[w["ta"][q]], w["taus"][q], w["t0a"][q]) for q in range(n)]
        w["ref_b"] = [ref_clock_states(coeffs[w["tb"][q]], total[w["tb"][q]], w["taus"][q], w["t0b"][q]) for q in range(n)]
        w["median"] = median_radii(w["ref_a"], w["ref_b"])
        w["radius"] = w["median"].copy()
        w["radius"][3::7] = 0.0
        w["radius"][5::11] = 100.0
    return Q


def footprint_classes(pa, pb, sa, sb, margin):
    """test_gpu_footprint.py's classes of the samples of one query on the poses pa, pb (K, 3: x, y, raw yaw): (surely below, surely clear, overlapping by the
    mirror, undecided)"""
    c2, over, g = footprint_clearance2(pa[:, :2], pa[:, 2], sa, pb[:, :2], pb[:, 2], sb, gap=True)
    M2 = margin * margin
    sure_below = (g < -TOL) | (c2 < M2 - TOL)
    sure_clear = (g > TOL) & (c2 > M2 + TOL)
    return sure_below, sure_clear, over, ~sure_below & ~sure_clear


def concat(Q, names, keys):
    """the named sets' per-query arrays one after the other"""
    return {k: np.concatenate([Q[n][k] for n in names]) for k in keys}
