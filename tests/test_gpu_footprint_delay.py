"""GPU tier of the start delays with oriented rectangles (uph_footprint_delay_sweep_batch, uph_footprint_delays_batch; uph_footprint_sweep_kernel).  The
yardstick is the existing device path: every number must be the one footprint_separation() returns for the shifted start, bit for bit.

S1 (exact): every array of footprint_delay_sweep() EQUALS (np.array_equal, NaN = NaN) footprint_separation() called once per delay j with t0_b + delta_j.
S2: known answers -- a trajectory against itself at delta = 0, a delay longer than the window, K = 0 rows, all-zero shapes against delay_sweep().
S3: two contexts -- refined trajectories (a second object, also in local frames and on fp32 cells) swept against their sources, from either side.
S4: no pair the broad phase drops (delay_extent's boxes, footprint_radii's radii) is below under any of 16 x 16 combinations of delays.
S5: footprint_delays() EQUALS delay_schedule, the sequential greedy, driven by footprint_separation() over the same candidates; with the starts it returns
    applied, footprint_conflicts() finds no pair whose later vehicle was placed.
S6: refusals on live contexts, launches split at 2^20 rows, a permutation / one width / a repeated call, the C++ adapter against ctypes.
S7: S1 on the resident trajectories of every piece count (tests/query_sweep.py's windows).
Source: the 64 solved hill goals of test_gpu_delay.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import query_sweep as QS
from test_gpu_delay import _first_clear, _fleet, _tails, hill      # noqa: F401  (hill: the module-scoped fixture)
from test_gpu_pieces import dev                                    # noqa: F401  (dev: the module-scoped map fixture)
from test_gpu_replan import _source
from test_gpu_resident_sweep import _auto
from test_gpu_separation import _bc, _same, _totals
from uneven_planner_amd import _lib
from uneven_planner_amd.alm_traj_opt import conflict_candidates, delay_levels, delay_schedule, delay_times, footprint_radii, separation_times

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
WKEYS = ("min_c2", "min_t", "below", "overlapping", "first_clear", "counts")
TILE = _lib.DELAY_TILE
CAR = (0.45, 0.15, 0.15)                        # DESIGN.md 7p's car: 0.45 + 0.15 m x 0.3 m
SHAPES = np.array([CAR, (0.4, 0.0, 0.2), (0.3, 0.2, 0.0), (0.0, 0.0, 0.0), (0.2, 0.5, 0.1), (0.0, 0.35, 0.25)])    # rear = 0, half_width = 0, all zero among them


def _looped(A, ta, tb, tf, tt, sa, sb, margin, delay0, step, D, t0_a=0.0, t0_b=0.0, other=None, dt=0.01):
    """the recipe the sweep replaces and the yardstick of S1: a footprint_separation() call per delay, b started at t0_b + delta_j"""
    n = len(ta)
    delta = delay_times(delay0, step, D)
    t0_b = _bc(t0_b, n)
    out = dict(min_c2=np.zeros((n, D)), min_t=np.zeros((n, D)), below=np.zeros((n, D), dtype=np.int32), overlapping=np.zeros((n, D), dtype=np.int32))
    for j in range(D):
        r = A.footprint_separation(ta, tb, tf, tt, sa, sb, margin, t0_a=t0_a, t0_b=t0_b + delta[j], other=other, dt=dt)
        out["min_c2"][:, j], out["min_t"][:, j], out["below"][:, j], out["overlapping"][:, j] = r["min_c2"], r["min_t"], r["counts"][:, 1], r["counts"][:, 2]
        out["counts"] = r["counts"][:, 0].copy()
    out["first_clear"] = _first_clear(out["below"])
    return out


def _held(A, ta, tb, tf, tt, sa, sb, margin, delay0, step, D, tag="", **kw):
    """footprint_delay_sweep() held to S1"""
    got = A.footprint_delay_sweep(ta, tb, tf, tt, sa, sb, margin, delay0, step, D, **kw)
    want = _looped(A, ta, tb, tf, tt, sa, sb, margin, delay0, step, D, **kw)
    _same(got, want, WKEYS, tag)
    assert np.array_equal(got["first_clear"], _first_clear(got["below"])), tag
    assert (got["overlapping"] <= got["below"]).all() and (got["below"] <= got["counts"][:, None]).all(), tag
    return got


def _edge_queries(hill, Ks, seed):
    """test_gpu_delay._tails' queries -- exactly K samples each, a clock around 1000 s -- with every fifth a trajectory against itself from the same start (two
    different rectangles that both hold the trajectory's point), shapes cycling through SHAPES on both sides of the others, and the margin the query's own
    smallest clearance at delay 0 times 0.7, 1.25 or 2.5"""
    src = hill["src"]
    ta, tb, tf, tt, t0a, t0b, _, dt = _tails(hill, Ks, seed)
    own = np.arange(len(Ks)) % 5 == 2
    tb, t0b = np.where(own, ta, tb).astype(np.int32), np.where(own, t0a, t0b)
    sa, sb = SHAPES[np.arange(len(Ks)) % len(SHAPES)], SHAPES[(np.arange(len(Ks)) // 2 + 1) % len(SHAPES)]
    sa[own], sb[own] = SHAPES[0], SHAPES[4]     # (against itself: two rectangles with the trajectory's point inside, so that "overlapping" is no knife's edge)
    least = np.sqrt(src.footprint_separation(ta, tb, tf, tt, sa, sb, 0.0, t0_a=t0a, t0_b=t0b, dt=dt)["min_c2"])
    margin = np.where(np.isfinite(least) & (least > 0.0), least * np.array([0.7, 1.25, 2.5])[np.arange(len(Ks)) % 3], 1.0)
    return ta, tb, tf, tt, t0a, t0b, sa, sb, margin, own, dt


S1_KS = (0, 1, 63, 64, 65, 127, 128, 129, 192, 193, 257)


@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 130, 257])
def test_sweep_equals_footprint_separation_per_delay_at_every_edge(hill, D):
    """S1: K on both sides of a wave, of a tile and of the lengths at which the launch width changes (K * D around 192), D on both sides of one wave and of 256
    lanes (lanes that share a delay, a lane per delay, several passes), in one launch that mixes both kernels, holds duplicates and comes shuffled; a negative
    delay0 and a table that contains delta = 0 (D = 1 cannot have both: it runs once with each)"""
    assert TILE == 128
    src = hill["src"]
    Ks = np.array(S1_KS * 3)
    ta, tb, tf, tt, t0a, t0b, sa, sb, margin, own, dt = _edge_queries(hill, Ks, 153 + D)
    rng = np.random.default_rng(D)
    dup = np.array([5, 5, 9, 20, 9, 0, 1], dtype=np.int64)
    idx = np.concatenate([np.arange(Ks.size), dup])
    idx = idx[rng.permutation(idx.size)]
    step = max(0.013, 3.0 / D)
    zero_at = min(2, D - 1)
    delay0 = -zero_at * step
    kw = dict(t0_a=t0a[idx], t0_b=t0b[idx], dt=dt)
    if D == 1:
        _held(src, ta[idx], tb[idx], tf[idx], tt[idx], sa[idx], sb[idx], margin[idx], -0.7, step, D, tag="edges D=1, negative delay0", **kw)
    else:
        assert delay0 < 0.0
    assert delay_times(delay0, step, D)[zero_at] == 0.0
    got = _held(src, ta[idx], tb[idx], tf[idx], tt[idx], sa[idx], sb[idx], margin[idx], delay0, step, D, tag="edges D=%d" % D, **kw)
    assert np.array_equal(got["counts"], Ks[idx]) and got["below"].shape == (idx.size, D)
    work = Ks[idx] * D
    assert (work > 192).any() and (work <= 192).any()              # both launch widths
    empty = Ks[idx] == 0
    assert (got["min_c2"][empty] == INF).all() and np.isnan(got["min_t"][empty]).all() and (got["below"][empty] == 0).all() and (got["overlapping"][empty] == 0).all()
    assert (got["first_clear"][empty] == 0).all()
    # the equality is not vacuous: rows that overlap, rows that are below without overlapping, rows that are clear -- among the queries with samples
    some = Ks[idx] > 0
    over, below = got["overlapping"][some], got["below"][some]
    print("D = %d: rows overlapping %d, below without overlap %d, clear %d of %d" % (D, (over > 0).sum(), ((below > 0) & (over == 0)).sum(), (below == 0).sum(), below.size))
    assert (over > 0).any() and ((below > 0) & (over == 0)).any() and (below == 0).any()
    # a trajectory against itself at delta = 0 overlaps at every sample
    mine = own[idx] & some
    assert mine.any() and (got["overlapping"][mine, zero_at] == Ks[idx][mine]).all() and (got["min_c2"][mine, zero_at] == 0.0).all()
    # the same query answers the same wherever it stands in the launch, and alone
    for q in np.unique(dup):
        rows = np.nonzero(idx == q)[0]
        assert rows.size >= 2
        for k in WKEYS:
            for r in rows[1:]:
                assert np.array_equal(got[k][r], got[k][rows[0]], equal_nan=True), (q, k)
    for r in (int(np.argmax(Ks[idx])), int(np.nonzero(Ks[idx] == TILE)[0][0]), int(np.nonzero(Ks[idx] == 1)[0][0])):
        q = idx[r]
        one = src.footprint_delay_sweep([ta[q]], [tb[q]], tf[q], tt[q], sa[q], sb[q], margin[q], delay0, step, D, t0_a=t0a[q], t0_b=t0b[q], dt=dt)
        for k in WKEYS:
            assert np.array_equal(one[k][0], got[k][r], equal_nan=True), (q, k)
    assert src.delay_kernel_ms() > 0.0


def test_sweep_over_whole_trajectories(hill):
    """S1: windows from before both starts to after both ends on a clock around 1000 s (many tiles), starts that differ, D = 16 at 0.5 s from -1 s; a margin no
    delay clears and a margin 0"""
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    rng = np.random.default_rng(161)
    D, delay0, step, dt = 16, -1.0, 0.5, 0.05
    ta, tb = ok, np.roll(ok, 7)
    t0_a, t0_b = 1000.0 + rng.uniform(0.0, 5.0, ok.size), 1000.0 + rng.uniform(0.0, 5.0, ok.size)
    tf = np.minimum(t0_a, t0_b) - rng.uniform(0.2, 1.5, ok.size)
    tt = np.maximum(t0_a + total[ta], t0_b + total[tb] + delay0 + step * D) + rng.uniform(0.2, 1.0, ok.size)
    margin = rng.uniform(0.0, 3.0, ok.size)
    margin[:3], margin[3:6] = 1e3, 0.0
    sa, sb = SHAPES[np.arange(ok.size) % len(SHAPES)], np.tile(CAR, (ok.size, 1))
    got = _held(src, ta, tb, tf, tt, sa, sb, margin, delay0, step, D, tag="full", t0_a=t0_a, t0_b=t0_b, dt=dt)
    K = np.array([separation_times(tf[q], tt[q], dt).shape[0] for q in range(ok.size)])
    assert np.array_equal(got["counts"], K) and (K > 3 * TILE * (0.01 / dt)).all()
    assert (got["first_clear"][:3] == -1).all() and np.isfinite(got["min_c2"]).all()
    assert (got["below"][3:6] == got["overlapping"][3:6]).all()                             # M = 0: below means overlapping
    assert (got["min_t"] >= tf[:, None]).all() and (got["min_t"] <= tt[:, None]).all()
    assert (got["below"].max(axis=1) > got["below"].min(axis=1)).sum() >= ok.size // 4      # the delay matters


def test_known_answers(hill):
    """S2"""
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    n, D = ok.size, 5
    # a trajectory against itself with the same start: at delta = 0 the two rectangles coincide at every sample
    tf, tt = 999.5, 1000.0 + total[ok] + 0.5
    for shape, margin in ((CAR, 0.25), (CAR, 0.0), ((0.0, 0.0, 0.0), 0.0)):
        r = src.footprint_delay_sweep(ok, ok, tf, tt, shape, shape, margin, 0.0, 0.75, D, t0_a=1000.0, t0_b=1000.0, dt=0.05)
        assert (r["counts"] > 60).all() and (r["overlapping"][:, 0] == r["counts"]).all() and (r["below"][:, 0] == r["counts"]).all()
        assert (r["min_c2"][:, 0] == 0.0).all() and (r["min_t"][:, 0] == tf).all()
        assert (r["min_c2"] == 0.0).all() and (r["min_t"] == tf).all() and (r["overlapping"] >= 1).all()         # both stand at the start at the first sample
        assert (r["first_clear"] == -1).all()
    # a delay longer than the window: b stays parked at its start, every row of a query is the same and is footprint_separation's against the parked b
    tb = np.roll(ok, 5)
    t0_a, t0_b = 50.0 + 0.1 * np.arange(n), 52.0 - 0.05 * np.arange(n)
    f, t = 49.0, 50.0 + float(total.max()) + 6.0
    r = _held(src, ok, tb, f, t, CAR, SHAPES[1], 0.3, t - 40.0, 3.0, D, tag="parked", t0_a=t0_a, t0_b=t0_b, dt=0.05)
    assert (t0_b + (t - 40.0) > t).all()
    far = src.footprint_separation(ok, tb, f, t, CAR, SHAPES[1], 0.3, t0_a=t0_a, t0_b=1e6, dt=0.05)
    for j in range(D):
        assert np.array_equal(r["min_c2"][:, j], far["min_c2"]) and np.array_equal(r["min_t"][:, j], far["min_t"]) and np.array_equal(r["below"][:, j], far["counts"][:, 1])
        assert np.array_equal(r["overlapping"][:, j], far["counts"][:, 2])
    # K = 0: +inf, NaN, 0, 0 and a first_clear of 0
    r = src.footprint_delay_sweep(ok, tb, 60.0, 59.0, CAR, CAR, 2.0, 0.0, 0.5, D, t0_a=t0_a, t0_b=t0_b)
    assert (r["min_c2"] == INF).all() and np.isnan(r["min_t"]).all() and (r["below"] == 0).all() and (r["overlapping"] == 0).all()
    assert (r["first_clear"] == 0).all() and (r["counts"] == 0).all()
    # all-zero shapes are points: min_c2 is delay_sweep()'s min_d2 with radius = margin, to the rounding of the rule's rotations (1e-12 relative)
    t0_a, t0_b = 1000.0 + 0.3 * np.arange(n), 1001.0 + 0.2 * np.arange(n)
    tt = float((t0_a + total[ok]).max()) + 3.0
    z = (0.0, 0.0, 0.0)
    pts = src.footprint_delay_sweep(ok, tb, 999.0, tt, z, z, 0.5, -1.0, 0.5, 8, t0_a=t0_a, t0_b=t0_b, dt=0.05)
    disc = src.delay_sweep(ok, tb, 999.0, tt, 0.5, -1.0, 0.5, 8, t0_a=t0_a, t0_b=t0_b, dt=0.05)
    assert (disc["min_d2"] > 0.0).all() and np.array_equal(pts["counts"], disc["counts"])
    rel = np.abs(pts["min_c2"] - disc["min_d2"]) / disc["min_d2"]
    print("points against discs: largest relative difference of the minimum %.3g" % rel.max())
    assert (rel <= 1e-12).all() and (pts["overlapping"] == 0).all()


def _refined_swept(src, m, tr, total, tag, t0_b):
    """S3's setup, as test_gpu_delay._refined_swept: trajectories tr of src refined from 0.3 of their duration into a second object; each refined trajectory
    swept against its source, and the source against it"""
    import uneven_planner_amd as U
    tr = np.asarray(tr, dtype=np.int32)
    t_sw = 0.3 * total[tr]
    dst = U.ALMTrajOpt(m)
    dst.set_rho(1.0)
    out = dst.refine(src, tr, t_sw)
    use = [q for q, r in enumerate(out) if r["status"] == 0 and r.get("ret", 4) != 4 and np.isfinite(r["c_xy"]).all()]
    assert len(use) >= max(3, len(tr) // 2), (tag, len(use))
    ta = np.array([out[q]["traj_of"] for q in use], dtype=np.int32)
    tb, t_sw = tr[use], t_sw[use]
    t0_b = _bc(t0_b, len(tr))[use]
    t0_a = t0_b + t_sw
    tt = np.maximum(t0_a + _totals(dst)[ta], t0_b + total[tb]) + 2.5
    D, delay0, step = 7, -0.6, 0.3
    sa, sb = SHAPES[np.arange(ta.size) % len(SHAPES)], np.tile(CAR, (ta.size, 1))
    for dt in (0.01, 0.05):
        got = _held(dst, ta, tb, t0_b - 0.5, tt, sa, sb, 0.05, delay0, step, D, tag=tag, t0_a=t0_a, t0_b=t0_b, other=src, dt=dt)
        assert (got["counts"] > 3.0 / dt).all()
    # delta_2 = 0: the refined trajectory starts where its source is, in its pose: the cars overlap there
    assert delay_times(delay0, step, D)[2] == 0.0
    at = dst.footprint_delay_sweep(ta, tb, t0_a, t0_a, CAR, CAR, 0.0, delay0, step, D, t0_a=t0_a, t0_b=t0_b, other=src)
    assert (at["counts"] == 1).all() and (at["overlapping"][:, 2] == 1).all() and (at["min_c2"][:, 2] == 0.0).all()
    # the order of the contexts: the source swept against the refined trajectories
    _held(src, tb, ta, t0_b - 0.5, tt, sb, sa, 0.05, delay0, step, D, tag=tag + " back", t0_a=t0_b, t0_b=t0_a, other=dst, dt=0.05)
    return dst


def test_two_contexts_refined_against_their_sources(hill):
    """S3"""
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    _refined_swept(src, hill["m"], ok[:16], total, "hill", 1000.0 + 0.25 * np.arange(16))


def test_two_contexts_in_local_frames_and_on_fp32_cells():
    """S3: a grid beyond FRAME_EXTENT (every trajectory in its own local frame, each side with its own context's shift) and an fp32-cell map, built as
    test_gpu_delay.test_two_contexts_in_local_frames_and_on_fp32_cells builds them"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    big = U.UnevenMap(dict(map_size_x=160.0, map_size_y=160.0, xy_resolution=0.25)).fill_fbm()
    nx, ny = int(big.voxel_num[0]), int(big.voxel_num[1])
    far, seed = [], 7300
    while len(far) < 6:
        p = scenes.local_problems(1, seed0=seed, half=75.0, dmin=4.0, dmax=9.0, occ_r2=big.occ_r2_buffer, grid=(nx, ny, big.xy_resolution, big.map_origin[0], big.map_origin[1]))[0]
        seed += 1
        if max(abs(p["init_xy"][0, 0]), abs(p["init_xy"][1, 0])) > 45.0:
            far.append(p)
    m32 = U.UnevenMap(dict(map_size_x=32.0, map_size_y=32.0, xy_resolution=0.25), storage="f32").fill_fbm(dict(patch_lambda=5.0, rough_threshold=0.5))
    nx, ny = int(m32.voxel_num[0]), int(m32.voxel_num[1])
    p32 = scenes.local_problems(6, seed0=5000, half=14.0, dmin=4.0, dmax=12.0, occ_r2=m32.occ_r2_buffer,
                                grid=(nx, ny, m32.xy_resolution, m32.map_origin[0], m32.map_origin[1]))
    for tag, m, probs in (("frames", big, far), ("f32", m32, p32)):
        opt = U.ALMTrajOpt(m)
        opt.set_rho(1.0)
        opt.optimize_batch(probs)
        tr = np.arange(len(probs), dtype=np.int32)
        total = _totals(opt)
        if tag == "frames":
            assert np.abs(opt.traj_states(tr, np.zeros(tr.size))[:, :2]).max() > 45.0
        _refined_swept(opt, m, tr, total, tag, 12.5)
        _held(opt, tr, np.roll(tr, 1), 0.0, total.max() + 4.0, CAR, SHAPES[4], 3.0, 0.0, 0.4, 9, tag=tag + " own", t0_a=0.5 * np.arange(tr.size), t0_b=1.0, dt=0.05)


def _least_clearance(src, tr, t0, tf, tt, shape, dt):
    n = tr.size
    iu, ju = np.triu_indices(n, 1)
    return iu, ju, np.sqrt(src.footprint_separation(tr[iu], tr[ju], tf, tt, shape[iu], shape[ju], 0.0, t0_a=t0[iu], t0_b=t0[ju], dt=dt)["min_c2"])


def test_the_swept_broad_phase_loses_nothing(hill):
    """S4: the fleet of test_gpu_delay (24 vehicles 0.4 s apart), 16 delays of 0.5 s.  A pair that uph_conflict_candidates drops on delay_extent's boxes with
    footprint_radii's radii is below at no sample, whichever of the 16 x 16 combinations of delays the two take (footprint_separation on every combination).
    The margin is the first of a fixed list at which the broad phase both drops and keeps pairs"""
    src, tr, t0, tf, tt = _fleet(hill)
    n, D, step, dt = tr.size, 16, 0.5, 0.05
    delta = delay_times(0.0, step, D)
    shape = np.tile(CAR, (n, 1))
    shape[1::3] = SHAPES[4]
    swept = src.delay_extent(tr, tf, tt, 0.0, step, D, t0=t0, dt=dt)
    iu, ju = np.triu_indices(n, 1)
    for m_each in (0.05, 0.5, 0.0, 1.5, 3.0):
        margin = np.full(n, m_each)
        radius = footprint_radii(shape, margin)
        kept = set(map(tuple, conflict_candidates(swept["box"], radius).tolist()))
        if 1 <= len(kept) < iu.size:
            break
    dropped = np.array([(i, j) for i, j in zip(iu, ju) if (i, j) not in kept])
    print("fleet: margin %.2f, %d of %d pairs dropped on swept boxes" % (m_each, len(dropped), iu.size))
    assert 1 <= len(dropped) < iu.size and len(kept) >= 1
    di, dj = dropped[:, 0], dropped[:, 1]
    P = di.size
    for ja in range(D):                                             # one call per delay of a: the dropped pairs under every delay of b
        qi, qj = np.repeat(di, D), np.repeat(dj, D)
        r = src.footprint_separation(tr[qi], tr[qj], tf, tt, shape[qi], shape[qj], margin[qi] + margin[qj], t0_a=t0[qi] + delta[ja], t0_b=t0[qj] + np.tile(delta, P), dt=dt)
        assert (r["counts"][:, 1] == 0).all() and (r["counts"][:, 0] > 0).all(), ja
        # the sweep says the same
        full = src.footprint_delay_sweep(tr[di], tr[dj], tf, tt, shape[di], shape[dj], margin[di] + margin[dj], 0.0, step, D, t0_a=t0[di] + delta[ja], t0_b=t0[dj], dt=dt)
        assert (full["below"] == 0).all() and np.array_equal(full["min_c2"].reshape(-1), r["min_c2"]), ja
    # ... and the rule is not vacuous: kept pairs are below under some delays (the margin as wide as the radii allow)
    ki, kj = np.array(sorted(kept)).T
    wide = src.footprint_delay_sweep(tr[ki], tr[kj], tf, tt, shape[ki], shape[kj], radius[ki] + radius[kj], 0.0, step, D, t0_a=t0[ki], t0_b=t0[kj], dt=dt)
    assert (wide["below"] > 0).any()


def _greedy(src, tr, t0, shape, margin, tf, tt, delay0, step, D, dt, n_delays=None):
    """delay_schedule driven by footprint_separation() over the candidates of the swept boxes with footprint_radii's radii"""
    delta = delay_times(delay0, step, D)
    box = src.delay_extent(tr, tf, tt, delay0, step, D, t0=t0, dt=dt)["box"]
    pairs = conflict_candidates(box, footprint_radii(shape, margin))

    def sweep(h, at, i):
        return src.footprint_separation(np.full(D, tr[h]), np.full(D, tr[i]), tf, tt, shape[h], shape[i], margin[h] + margin[i], t0_a=t0[h] + delta[at], t0_b=t0[i] + delta,
                                        dt=dt)["counts"][:, 1]

    want = delay_schedule(sweep, pairs, tr.size, n_delays=n_delays)
    want["start"] = t0 + delta[np.maximum(want["choice"], 0)]
    want["n_candidates"], want["n_unresolved"] = pairs.shape[0], int((want["choice"] < 0).sum())
    want["n_rounds"] = int(delay_levels(pairs, tr.size).max())
    return want


def _schedule_held(src, got, tr, t0, shape, margin, tf, tt, delay0, step, D, dt, n_delays=None, tag="footprint delays"):
    want = _greedy(src, tr, t0, shape, margin, tf, tt, delay0, step, D, dt, n_delays=n_delays)
    _same(got, want, ("choice", "start", "blocker"), tag)
    assert (got["n_candidates"], got["n_rounds"], got["n_unresolved"]) == (want["n_candidates"], want["n_rounds"], want["n_unresolved"]), tag
    return want


def test_the_schedule_is_the_sequential_greedy(hill):
    """S5: 24 cars that start `stagger` apart, D = 16 delays of 0.5 s, DESIGN.md 7p's car with M = 0.1 per pair.  The stagger is the first of a fixed list at
    which a vehicle waits and the candidates have more than one level; the assertions on these are made on that run and are not relaxed"""
    src, ok, total = hill["src"], hill["ok"], hill["total"]
    n, D, step, dt = 24, 16, 0.5, 0.05
    tr = ok[:n]
    shape, margin = np.tile(CAR, (n, 1)), np.full(n, 0.05)
    for stagger in (0.4, 0.2, 0.1, 0.8, 0.0, 1.6):
        t0 = 1000.0 + stagger * np.arange(n)
        tf, tt = 999.0, float((t0 + total[tr]).max()) + 1.0
        got = src.footprint_delays(tr, shape, margin, tf, tt, 0.0, step, D, t0=t0, dt=dt)
        print("stagger %.1f: choice %s rounds %d candidates %d unresolved %d" % (stagger, got["choice"].tolist(), got["n_rounds"], got["n_candidates"], got["n_unresolved"]))
        if (got["choice"] > 0).any() and got["n_rounds"] >= 2:
            break
    assert (got["choice"] > 0).any() and got["n_rounds"] >= 2
    assert src.delay_kernel_ms() > 0.0
    _schedule_held(src, got, tr, t0, shape, margin, tf, tt, 0.0, step, D, dt)
    assert got["choice"][0] == 0 and ((got["blocker"] >= 0) == (got["choice"] < 0)).all()
    # with the effective starts applied no conflict is left whose later vehicle was placed
    left = src.footprint_conflicts(tr, shape, margin, tf, tt, t0=got["start"], dt=dt)
    before = src.footprint_conflicts(tr, shape, margin, tf, tt, t0=t0, dt=dt)
    print("footprint conflicts: %d before, %d after (unresolved %s)" % (before["n_conflicts"], left["n_conflicts"], np.nonzero(got["choice"] < 0)[0].tolist()))
    assert before["n_conflicts"] >= 1 and (got["choice"][left["pairs"][:, 1]] < 0).all()
    # recorded, not asserted: what the remedy on the circumscribed discs would have postponed
    disc = src.delays(tr, np.hypot(max(CAR[0], CAR[1]), CAR[2]) + margin, tf, tt, 0.0, step, D, t0=t0, dt=dt)
    print("postponed or unresolved: discs rho + m %d of %d vehicles (%d unresolved), rectangles %d (%d unresolved)" % (
        (disc["choice"] != 0).sum(), n, disc["n_unresolved"], (got["choice"] != 0).sum(), got["n_unresolved"]))
    # one delay for all: stay or fail
    one = src.footprint_delays(tr, shape, margin, tf, tt, 0.0, step, D, t0=t0, n_delays=1, dt=dt)
    _schedule_held(src, one, tr, t0, shape, margin, tf, tt, 0.0, step, D, dt, n_delays=np.ones(n, dtype=np.int32), tag="footprint delays, one each")
    assert set(one["choice"].tolist()) <= {0, -1} and np.array_equal(one["start"], t0)
    # per-vehicle limits, shapes and margins, a table that does not start at 0
    nd = 1 + (np.arange(n) * 5) % D
    shape2 = SHAPES[np.arange(n) % len(SHAPES)]
    margin2 = 0.02 + 0.1 * (np.arange(n) % 3)
    got2 = src.footprint_delays(tr, shape2, margin2, tf, tt, 0.25, 0.3, D, t0=t0, n_delays=nd, dt=dt)
    _schedule_held(src, got2, tr, t0, shape2, margin2, tf, tt, 0.25, 0.3, D, dt, n_delays=nd, tag="footprint delays, limits")
    assert (got2["choice"] < nd).all() and got2["start"][0] == t0[0] + 0.25


def _raw(src, call, null=(), n=None, **kw):
    """one of the two device calls through ctypes on pre-filled outputs: (rc, outputs)"""
    a = dict(tr=[0, 1, 2, 3], tb=[1, 2, 3, 0], t0=np.zeros(4), t0b=np.zeros(4), tf=np.zeros(4), tt=np.full(4, 5.0), sa=np.tile(CAR, (4, 1)), sb=np.tile(CAR, (4, 1)),
             mg=np.full(4, 0.1), dt=None, delay0=0.0, step=0.5, D=4, other=None, nd=None, f=0.0, t=5.0)
    a.update(kw)
    if a["dt"] is None:
        a["dt"] = 0.05 if call == "delays" else 0.01
    tr, tb = np.ascontiguousarray(a["tr"], dtype=np.int32), np.ascontiguousarray(a["tb"], dtype=np.int32)
    t0, t0b, tf, tt, sa, sb, mg = (np.ascontiguousarray(a[k], dtype=np.float64) for k in ("t0", "t0b", "tf", "tt", "sa", "sb", "mg"))
    nd = None if a["nd"] is None else np.ascontiguousarray(a["nd"], dtype=np.int32)
    n = tr.size if n is None else n
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda v: v.ctypes.data_as(_lib.DP)
    arg = lambda name, v: None if name in null else v
    rows = 4 * max(1, min(a["D"], 4096))
    if call == "sweep":
        o = dict(min_c2=np.full(rows, -9.0), min_t=np.full(rows, -9.0), below=np.full(rows, -9, dtype=np.int32), over=np.full(rows, -9, dtype=np.int32),
                 first=np.full(4, -9, dtype=np.int32), K=np.full(4, -9, dtype=np.int32))
        rc = src.L.uph_footprint_delay_sweep_batch(arg("ctx", src.h), None if a["other"] is None else a["other"].h, n, arg("traj_a", ip(tr)), arg("traj_b", ip(tb)),
                                                   arg("t0_a", dp(t0)), arg("t0_b", dp(t0b)), arg("t_from", dp(tf)), arg("t_to", dp(tt)), a["dt"], arg("shape_a", dp(sa)),
                                                   arg("shape_b", dp(sb)), arg("margin", dp(mg)), a["delay0"], a["step"], a["D"], dp(o["min_c2"]), dp(o["min_t"]),
                                                   ip(o["below"]), ip(o["over"]), ip(o["first"]), ip(o["K"]))
    else:
        o = dict(choice=np.full(4, -9, dtype=np.int32), start=np.full(4, -9.0), blocker=np.full(4, -9, dtype=np.int32), nk=np.full(1, -9, dtype=np.int64),
                 nr=np.full(1, -9, dtype=np.int32), nu=np.full(1, -9, dtype=np.int32))
        rc = src.L.uph_footprint_delays_batch(arg("ctx", src.h), n, arg("traj", ip(tr)), arg("t0", dp(t0)), arg("shape", dp(sa)), arg("margin", dp(mg)),
                                              None if nd is None else ip(nd), a["f"], a["t"], a["dt"], a["delay0"], a["step"], a["D"], ip(o["choice"]), dp(o["start"]),
                                              ip(o["blocker"]), o["nk"].ctypes.data_as(C.POINTER(C.c_int64)), ip(o["nr"]), ip(o["nu"]))
    return rc, o


def test_refusals(hill):
    """S6: each refusal of include/uneven_hip.h on live contexts -- those of the footprint calls and those of the delay calls --: UPH_ERR_INVALID (UPH_ERR_LIMIT
    where it says so) with every output as it was pre-filled"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m, ka, src, ok = hill["m"], hill["ka"], hill["src"], hill["ok"]
    F = src.L.uph_batch_count(src.h)
    tr = ok[:4]
    fresh = U.ALMTrajOpt(m)
    fresh.plan_goals_upload(ka, hill["S"][:8], hill["G"][:8])                 # uploaded, not solved: no resident trajectory
    probs = scenes.random_problems(3, seed0=2100)                              # an UPH_RET_UNSUPPORTED slot next to ordinary ones
    big = dict(probs[0])
    big["inner_xy"] = np.linspace([0.0, 0.0], [3.0, 0.5], 140).T.copy()
    big["inner_yaw"] = np.zeros(140)
    uns = U.ALMTrajOpt(m)
    uns.set_rho(1.0)
    assert uns.optimize_batch(probs + [big])[3]["ret"] == 4
    src2, _ = _source(m, ka, hill["S"][:32], hill["G"][:32])

    def refused(res, what, code=-1, word=None):
        rc, o = res
        assert rc == code and all((o[k] == -9).all() for k in o), (what, rc, src.L.uph_last_error())
        assert word is None or word in src.L.uph_last_error(), (what, src.L.uph_last_error())

    names = {"sweep": b"uph_footprint_delay_sweep_batch", "delays": b"uph_footprint_delays_batch"}
    run = lambda call, a=src, **kw: _raw(a, call, **dict(dict(tr=tr, tb=tr), **kw))
    for call, nulls in (("sweep", ("ctx", "traj_a", "traj_b", "t0_a", "t0_b", "t_from", "t_to", "shape_a", "shape_b", "margin")),
                        ("delays", ("ctx", "traj", "t0", "shape", "margin"))):
        for null in nulls:
            refused(run(call, null=(null,)), (call, null), word=names[call])
    car4 = np.tile(CAR, (4, 1))
    for call in ("sweep", "delays"):
        # what the footprint calls refuse: shapes and margins, ahead of everything else
        for v in (NAN, INF, -INF, -1e-9):
            for col in range(3):
                s = car4.copy()
                s[2, col] = v
                refused(run(call, sa=s), (call, "shape", v, col), word=b"shape")
                refused(run(call, sa=s, tr=[-1, 0, 0, 0], D=0), (call, "shape first", v, col), word=b"shape")
                if call == "sweep":
                    refused(run(call, sb=s), (call, "shape_b", v, col), word=b"shape_b")
            refused(run(call, mg=np.array([0.1, v, 0.1, 0.1])), (call, "margin", v), word=b"margin")
        # what uph_separation_batch / uph_conflicts_batch refuse
        for n in (0, -3):
            refused(run(call, n=n), (call, "n", n))
        for dt in (0.0, -0.01, INF, NAN):
            refused(run(call, dt=dt), (call, "dt", dt))
        refused(run(call, dt=1e-7), (call, "too many samples"), code=_lib.UPH_ERR_LIMIT)
        refused(run(call, fresh, tr=[0, 1, 2, 3], tb=[0, 1, 2, 3]), (call, "not resident"), word=b"resident")
        refused(run(call, U.ALMTrajOpt(m)), (call, "no batch"))
        refused(run(call, uns, tr=[0, 3, 1, 2], tb=[0, 1, 2, 0]), (call, "unsupported slot"), word=b"UNSUPPORTED")
        for bad in ([int(ok[0]), F, int(ok[1]), int(ok[2])], [-1, 0, 0, 0]):
            refused(run(call, tr=bad), (call, "index", bad))
        src2.solve_async()                                                      # an asynchronous solve pending
        res = run(call, src2, tr=[0, 1, 2, 3], tb=[0, 1, 2, 3])
        src2.wait()
        refused(res, (call, "pending"), word=b"in flight")
        for v in (NAN, INF, -INF):
            bad = np.array([0.0, v, 0.0, 0.0])
            refused(run(call, t0=bad), (call, "t0", v))
            if call == "delays":
                refused(run(call, f=v), (call, "t_from", v)), refused(run(call, t=v), (call, "t_to", v))
            else:
                refused(run(call, tf=bad), (call, "t_from", v)), refused(run(call, tt=bad + 5.0), (call, "t_to", v))
            # the delays
            refused(run(call, delay0=v), (call, "delay0", v)), refused(run(call, step=v), (call, "step", v))
        for step in (0.0, -0.5):
            refused(run(call, step=step), (call, "step", step))
        for D in (0, -2):
            refused(run(call, D=D), (call, "D", D))
        refused(run(call, D=4097), (call, "D"), code=_lib.UPH_ERR_LIMIT, word=b"4096")
        # K * D > 2^26: 20001 samples at 4096 delays
        refused(run(call, D=4096, tt=np.full(4, 200.0), t=200.0, dt=0.01), (call, "K * D"), code=_lib.UPH_ERR_LIMIT, word=b"2^26")
        # a delayed start that is not finite (t0 is finite, the table is a table)
        key = "t0b" if call == "sweep" else "t0"
        refused(run(call, **{key: np.array([0.0, 0.0, 1.7e308, 0.0]), "delay0": 1.7e308}), (call, "start"))
        refused(run(call, step=1e308, D=4), (call, "start, by the last delay"), word=b"not finite")
    for nd in ([1, 2, 0, 4], [1, 2, 5, 4], [-1, 1, 1, 1]):
        refused(run("delays", nd=nd), ("n_delays", nd), word=b"n_delays")
    refused(run("delays", sa=[[1e308, 0.0, 1e308]] * 4, mg=np.full(4, 1e308)), "radius overflow", word=b"radius")
    # side b is checked against ITS context
    refused(run("sweep", other=uns, tb=[0, 3, 1, 2]), "unsupported slot of b")
    refused(run("sweep", other=fresh), "b not resident")
    src2.solve_async()
    res = run("sweep", other=src2, tb=[0, 1, 2, 3])
    src2.wait()
    refused(res, "b pending")
    assert run("sweep", uns, tr=[0, 1, 2, 0], other=src)[0] == 0
    # what is allowed: any output NULL, a reversed window, margin 0, zero shapes, n_delays at both ends of its range
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda v: v.ctypes.data_as(_lib.DP)
    z4, w4, z43 = np.zeros(4), np.full(4, 5.0), np.zeros((4, 3))
    cnt = np.full(4, -9, dtype=np.int32)
    assert src.L.uph_footprint_delay_sweep_batch(src.h, None, 4, ip(tr), ip(tr), dp(z4), dp(z4), dp(z4), dp(w4), 0.01, dp(z43), dp(z43), dp(z4), 0.0, 0.5, 4, None, None, None,
                                                 None, None, ip(cnt)) == 0
    assert cnt.tolist() == [separation_times(0.0, 5.0, 0.01).shape[0]] * 4
    assert src.L.uph_footprint_delay_sweep_batch(src.h, None, 4, ip(tr), ip(tr), dp(z4), dp(z4), dp(w4), dp(z4), 0.01, dp(car4), dp(car4), dp(z4), 0.0, 0.5, 4, None, None,
                                                 None, None, None, None) == 0
    assert src.L.uph_footprint_delays_batch(src.h, 4, ip(tr), dp(z4), dp(car4), dp(z4), None, 0.0, 5.0, 0.05, 0.0, 0.5, 4, None, None, None, None, None, None) == 0
    rc, o = run("delays", nd=[1, 4, 4, 1], mg=np.full(4, 50.0))               # everybody in everybody's way, whatever the delay
    assert rc == 0 and o["choice"].tolist() == [0, -1, -1, -1] and o["blocker"].tolist() == [-1, 0, 0, 0] and (o["nk"][0], o["nr"][0], o["nu"][0]) == (6, 3, 3)
    assert o["start"].tolist() == [0.0] * 4


def test_launches_are_split_at_2_20_rows(hill):
    """S6: 300 queries at D = 4096 are 1.2 M rows, more than the device holds at a time: the same rows as the queries sent one by one"""
    src, ok = hill["src"], hill["ok"]
    n, D = 300, 4096
    assert n * D > _lib.DELAY_ROWS
    rng = np.random.default_rng(183)
    ta, tb = ok[np.arange(n) % ok.size], ok[(np.arange(n) * 7 + 3) % ok.size]
    t0a, t0b = 1000.0 + rng.uniform(0.0, 3.0, n), 1000.0 + rng.uniform(0.0, 3.0, n)
    tf = 1003.0 + rng.uniform(0.0, 4.0, n)
    tt = tf + 0.05 * rng.integers(0, 3, n)                          # K = 1, 2 or 3
    margin = rng.uniform(0.2, 5.0, n)
    sa, sb = SHAPES[np.arange(n) % len(SHAPES)], SHAPES[(np.arange(n) // 3) % len(SHAPES)]
    got = src.footprint_delay_sweep(ta, tb, tf, tt, sa, sb, margin, -2.0, 0.002, D, t0_a=t0a, t0_b=t0b, dt=0.05)
    assert got["below"].shape == (n, D) and set(got["counts"].tolist()) == {1, 2, 3}
    for q in range(n):
        one = src.footprint_delay_sweep(ta[q:q + 1], tb[q:q + 1], tf[q], tt[q], sa[q], sb[q], margin[q], -2.0, 0.002, D, t0_a=t0a[q], t0_b=t0b[q], dt=0.05)
        for k in WKEYS:
            assert np.array_equal(one[k][0], got[k][q], equal_nan=True), (q, k)
    # ... and a few of them against the yardstick itself
    few = np.array([0, 255, 256, 299])
    _held(src, ta[few], tb[few], tf[few], tt[few], sa[few], sb[few], margin[few], -2.0, 0.002 * 64, D // 64, tag="chunks", t0_a=t0a[few], t0_b=t0b[few], dt=0.05)
    assert (got["below"] > 0).any() and (got["below"] == 0).any()


def test_the_answer_does_not_depend_on_the_launch(hill):
    """S6: a permutation of the queries, a launch of one width only and a repeated call give the same rows, bit for bit"""
    src = hill["src"]
    Ks = np.array(S1_KS * 2)
    ta, tb, tf, tt, t0a, t0b, sa, sb, margin, _, dt = _edge_queries(hill, Ks, 191)
    D, delay0, step = 12, -0.5, 0.25
    call = lambda idx: src.footprint_delay_sweep(ta[idx], tb[idx], tf[idx], tt[idx], sa[idx], sb[idx], margin[idx], delay0, step, D, t0_a=t0a[idx], t0_b=t0b[idx], dt=dt)
    every = np.arange(Ks.size)
    base = call(every)
    again = call(every)
    perm = np.random.default_rng(7).permutation(Ks.size)
    mixed = call(perm)
    for k in WKEYS:
        assert np.array_equal(base[k], again[k], equal_nan=True), k
        assert np.array_equal(base[k][perm], mixed[k], equal_nan=True), k
    for idx in (np.nonzero(Ks * D > 192)[0], np.nonzero(Ks * D <= 192)[0]):     # 256 lanes alone, one wave alone
        assert idx.size >= 2
        part = call(idx)
        for k in WKEYS:
            assert np.array_equal(base[k][idx], part[k], equal_nan=True), k


CPP = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
#include <cstdio>
using namespace uneven_hip;
int main(int argc, char** argv) {
    // in: {ncell, B}, cells, B x {start, goal, start time on the common clock, margin}
    FILE* f = std::fopen(argv[1], "rb");
    long long hdr[2];
    if (argc < 3 || !f || fread(hdr, 8, 2, f) != 2) return 2;
    std::vector<double> cells((size_t)hdr[0] * 4), sg((size_t)hdr[1] * 8);
    if (fread(cells.data(), 8, cells.size(), f) != cells.size() || fread(sg.data(), 8, sg.size(), f) != sg.size()) return 2;
    std::fclose(f);
    uph_map_params mp = {2, 10.0, 10.0, 0.2, 0.1, 0.1, 0.05, 0.1, 0.8, 0.05, 9.81};
    UnevenMapHandle map(mp, 0);
    map.setCells(cells.data());
    KinoAstar kino;
    kino.setEnvironment(&map);
    ALMTrajOpt opt, second;
    opt.setEnvironment(&map);
    second.setEnvironment(&map);
    std::vector<std::array<double, 3>> starts((size_t)hdr[1]), goals((size_t)hdr[1]);
    for (long long b = 0; b < hdr[1]; b++) for (int k = 0; k < 3; k++) { starts[b][k] = sg[8 * b + k]; goals[b][k] = sg[8 * b + 3 + k]; }
    uph_manager_params mgr{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5};
    ALMTrajOpt::GoalPlan p = opt.planSE2TrajBatch(kino, starts, goals, mgr);
    second.planSE2TrajBatch(kino, starts, goals, mgr);
    std::vector<int> traj, other, nd;
    std::vector<double> t0, mg, tf, tt, t0b;
    std::vector<std::array<double, 3>> sa, sb;
    for (long long b = 0; b < hdr[1]; b++)
        if (p.traj_of[b] >= 0 && p.ret[b] != UPH_RET_UNSUPPORTED) {
            traj.push_back(p.traj_of[b]); t0.push_back(sg[8 * b + 6]); mg.push_back(sg[8 * b + 7]);
            tf.push_back(sg[8 * b + 6] - 0.5); tt.push_back(sg[8 * b + 6] + 12.0);
            sa.push_back({0.45, 0.15, 0.15}); sb.push_back({0.2 + 0.05 * (double)(b % 4), 0.1 * (double)(b % 3), 0.1});
        }
    const size_t n = traj.size();
    for (size_t k = 0; k < n; k++) { other.push_back(traj[(k + 1) % n]); t0b.push_back(t0[(k + 1) % n]); nd.push_back(1 + (int)(k % 12)); }
    const int D = 12;
    const ALMTrajOpt::TrajFootprintDelaySweep s = opt.footprintDelaySweepSE2TrajBatch(traj, other, t0, t0b, tf, tt, sa, sb, mg, -1.0, 0.5, D);
    const ALMTrajOpt::TrajFootprintDelaySweep x = opt.footprintDelaySweepSE2TrajBatch(traj, other, t0, t0b, tf, tt, sa, sb, mg, -1.0, 0.5, D, 0.05, &second);
    const ALMTrajOpt::TrajDelays d = opt.footprintDelaysSE2TrajBatch(traj, t0, sb, mg, 99.0, 130.0, 0.0, 0.5, D);
    const ALMTrajOpt::TrajDelays l = opt.footprintDelaysSE2TrajBatch(traj, t0, sb, mg, 99.0, 130.0, 0.0, 0.5, D, nd, 0.1);
    // out: n, per query traj; the two sweeps (4 D + 2 per query), the two schedules (3 counts, then 3 per vehicle)
    FILE* o = std::fopen(argv[2], "wb");
    double nn = (double)n;
    fwrite(&nn, 8, 1, o);
    for (size_t k = 0; k < n; k++) { double q = (double)traj[k]; fwrite(&q, 8, 1, o); }
    for (const ALMTrajOpt::TrajFootprintDelaySweep* r : {&s, &x})
        for (size_t q = 0; q < n; q++) {
            for (int j = 0; j < D; j++) {
                double h[4] = {r->min_c2[q * D + j], r->min_t[q * D + j], (double)r->below[q * D + j], (double)r->overlapping[q * D + j]};
                fwrite(h, 8, 4, o);
            }
            double h[2] = {(double)r->first_clear[q], (double)r->counts[q]};
            fwrite(h, 8, 2, o);
        }
    for (const ALMTrajOpt::TrajDelays* r : {&d, &l}) {
        double h[3] = {(double)r->n_candidates, (double)r->n_rounds, (double)r->n_unresolved};
        fwrite(h, 8, 3, o);
        for (size_t k = 0; k < n; k++) { double w[3] = {(double)r->choice[k], r->start[k], (double)r->blocker[k]}; fwrite(w, 8, 3, o); }
    }
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_matches_ctypes_bit_for_bit(tmp_path, analytic_cells):
    """S6: ALMTrajOpt::footprintDelaySweepSE2TrajBatch (one object and two) / footprintDelaysSE2TrajBatch from a compiled C++ consumer (after planSE2TrajBatch)
    against plan_goals + footprint_delay_sweep / footprint_delays through ctypes"""
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    ka = U.KinoAstar(m)
    S, G = scenes.random_queries(24, seed0=9900)
    t0 = 100.0 + 0.5 * np.arange(S.shape[0])
    mg = 0.02 + 0.05 * (np.arange(S.shape[0]) % 5)
    mk = dict(piece_len=0.3, mean_vel=0.5, init_time_times=1.2, yaw_piece_times=2.0, init_sig_vel=0.05, test_mode=0, test_max_vel=0.5)
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    plan = opt.plan_goals(ka, S, G, **mk)
    second = U.ALMTrajOpt(m)
    second.set_rho(1.0)
    second.plan_goals(ka, S, G, **mk)
    src_ = tmp_path / "fdelay.cpp"
    src_.write_text(CPP)
    exe = str(tmp_path / "fdelay")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src_), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    cells = np.ascontiguousarray(analytic_cells, dtype=np.float64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2q", cells.shape[0], S.shape[0]))
        f.write(cells.tobytes())
        f.write(np.ascontiguousarray(np.concatenate([S, G, t0[:, None], mg[:, None]], axis=1), dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, dtype=np.float64)
    n, D = int(raw[0]), 12
    live = [b for b in range(S.shape[0]) if plan[b]["status"] == 0 and plan[b]["ret"] != 4]
    tr = np.array([plan[b]["traj_of"] for b in live], dtype=np.int32)
    assert n == len(tr) >= 10 and raw[1:1 + n].astype(int).tolist() == tr.tolist()
    t0, mg = t0[live], mg[live]
    sa = np.tile(CAR, (n, 1))
    sb = np.array([[0.2 + 0.05 * (b % 4), 0.1 * (b % 3), 0.1] for b in live])
    tf, tt = t0 - 0.5, t0 + 12.0
    tb, t0b = np.roll(tr, -1), np.roll(t0, -1)
    at = 1 + n
    per = 4 * D + 2
    for want in (opt.footprint_delay_sweep(tr, tb, tf, tt, sa, sb, mg, -1.0, 0.5, D, t0_a=t0, t0_b=t0b),
                 opt.footprint_delay_sweep(tr, tb, tf, tt, sa, sb, mg, -1.0, 0.5, D, t0_a=t0, t0_b=t0b, other=second, dt=0.05)):
        blk = raw[at:at + per * n].reshape(n, per)
        rows = blk[:, :4 * D].reshape(n, D, 4)
        _same(dict(min_c2=rows[:, :, 0], min_t=rows[:, :, 1], below=rows[:, :, 2].astype(np.int32), overlapping=rows[:, :, 3].astype(np.int32),
                   first_clear=blk[:, -2].astype(np.int32), counts=blk[:, -1].astype(np.int32)), want, WKEYS, "adapter footprint sweep")
        assert (blk[:, -1] > 100).all() and np.isfinite(rows[:, :, 0]).all()
        at += per * n
    nd = 1 + np.arange(n) % 12
    for want in (opt.footprint_delays(tr, sb, mg, 99.0, 130.0, 0.0, 0.5, D, t0=t0), opt.footprint_delays(tr, sb, mg, 99.0, 130.0, 0.0, 0.5, D, t0=t0, n_delays=nd, dt=0.1)):
        assert tuple(int(v) for v in raw[at:at + 3]) == (want["n_candidates"], want["n_rounds"], want["n_unresolved"])
        rows = raw[at + 3:at + 3 + 3 * n].reshape(n, 3)
        at += 3 + 3 * n
        _same(dict(choice=rows[:, 0].astype(np.int32), start=rows[:, 1], blocker=rows[:, 2].astype(np.int32)), want, ("choice", "start", "blocker"), "adapter footprint delays")
    assert at == raw.size


# ---- S7: every piece count.  The resident batch is test_gpu_resident_sweep._auto's (no solve; shared with test_gpu_query_sweep.py), the windows, starts, shapes and
# margins tests/query_sweep.py's.
def test_sweep_equals_footprint_separation_at_every_piece_count(dev):
    """S7: S1 on the 469 trajectories of the piece sweep -- 1 to 128 position pieces, every yaw ratio -- over W2 (192 samples around an arrival, one wave with
    D = 1 and 256 lanes beyond), W3 (39 samples) and W1 (whole trajectories, many tiles) with delays on both sides of 0"""
    R = _auto(dev)
    opt = R["opt"]
    total = np.array([QS.total_of(o) for o in R["out"]])
    Q = QS.windows(total)
    for name, D, delay0, step in (("W2", 1, 0.0, 0.5), ("W2", 5, -0.4, 0.2), ("W3", 70, -1.0, 0.03), ("W1", 3, -0.5, 0.5)):
        w = Q[name]
        got = _held(opt, w["ta"], w["tb"], w["tf"], w["tt"], w["sa"], w["sb"], w["m"], delay0, step, D, tag="pieces %s D=%d" % (name, D), t0_a=w["t0a"], t0_b=w["t0b"],
                    dt=w["dt"])
        # (every sweep trajectory starts in one pose: W1's windows open on two vehicles parked on each other, so none of its rows is clear)
        assert (got["counts"] > 0).all() and (got["below"] > 0).any() and (got["below"] < got["counts"][:, None]).any() and (got["overlapping"] < got["below"]).any()
