"""GPU tier of the fleet of resident trajectories (uph_fleet_create / _adopt / _release / _info / _get, uph_fleet_adopt_kernel; TrajFleet).  Adoption is a copy:
every comparison here is np.array_equal (NaN = NaN) against the SAME call on the object a trajectory was solved in.

F1 every piece count: the whole piece sweep (1 .. 128 position pieces, four yaw ratios) adopted in reversed slot order in one call, caps 128 / 256.
F2 tight caps, neighbours of a replaced slot, one slot, more adoptions than a workgroup has lanes, one source into two slots.
F3 a fleet from two objects: plan, adopt, refine from the FLEET, adopt back; every pair and the fleet-wide calls against the cross-context calls on the two sources.
F4 the fleet as src of refine / replan.    F5 local frames and fp32 cells.    F6 release and empty slots.    F7 refusals.    F8 the C++ adapter."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import piece_sweep as PS
from test_gpu_pieces import dev      # noqa: F401  (the module-scoped map fixture of the sweep)
from test_gpu_replan import _hill_map, _queries, _source
from test_gpu_resident_sweep import _auto, _knot_times, _rollout, _total
from test_gpu_separation import _totals, _valid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, LIMIT = -1, -4
MK = dict(piece_len=0.3, mean_vel=0.5, init_time_times=1.2, yaw_piece_times=2.0, init_sig_vel=0.05, test_mode=0, test_max_vel=0.5)


def _eq(got, want, tag=""):
    """two dicts of arrays (or two arrays) equal bit for bit, NaN = NaN"""
    if not isinstance(got, dict):
        got, want = dict(v=got), dict(v=want)
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for k in got:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (tag, k, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            assert False, (tag, k, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _pieces(r):
    return r["c_xy"].shape[0] // 6, r["c_yaw"].shape[0] // 6


def _holds(fleet, slots, results, tag=""):
    """uph_fleet_get of `slots` equals the sources' downloads `results`: counts, T, ret_code, every coefficient double"""
    g = fleet.get(slots)
    for q, r in enumerate(results):
        nx, ny = _pieces(r)
        assert (g["n_xy"][q], g["n_yaw"][q], g["ret"][q]) == (nx, ny, r["ret"]), (tag, q)
        assert g["T_xy"][q] == r["T_xy"] and g["T_yaw"][q] == r["T_yaw"], (tag, q)
        assert np.array_equal(g["c_xy"][q, :12 * nx], np.asarray(r["c_xy"]).ravel()) and np.array_equal(g["c_yaw"][q, :6 * ny], np.asarray(r["c_yaw"]).ravel()), (tag, q)
    return g


def _segments(offs, rows, order):
    return np.concatenate([rows[int(offs[b]):int(offs[b + 1])] for b in order]) if len(order) else rows[:0]


# ---- F1 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_piece_count_adopted_in_one_call(dev):      # noqa: F811
    import uneven_planner_amd as U
    R = _auto(dev)
    opt, out, cases = R["opt"], R["out"], R["cases"]
    B = len(cases)
    nxs = sorted({_pieces(o)[0] for o in out})
    ny_max = max(_pieces(o)[1] for o in out)
    assert nxs == list(range(1, 129)) and 250 <= ny_max <= 256 and any(_pieces(o) == (1, 1) for o in out)
    fleet = U.TrajFleet(dev, B, 128, 256)
    assert fleet.L.uph_batch_count(fleet.h) == B and not fleet.occupied.any()
    src_traj, slot = np.arange(B, dtype=np.int32), np.arange(B, dtype=np.int32)[::-1].copy()
    fleet.adopt(opt, src_traj, slot)
    assert fleet.occupied.all() and (fleet.t0 == 0.0).all() and fleet.adopt_kernel_ms() > 0.0
    g = _holds(fleet, slot, out, "sweep")
    # beyond a trajectory's coefficients its slot is as created: zeros (nothing was written past the counts)
    for q, o in enumerate(out):
        nx, ny = _pieces(o)
        assert not g["c_xy"][q, 12 * nx:].any() and not g["c_yaw"][q, 6 * ny:].any(), q
    # caps that are exactly the sweep's largest counts: the longest trajectories fill their slots to the last double, no slack before the next slot
    exact = U.TrajFleet(dev, B, 128, ny_max)
    exact.adopt(opt, src_traj, slot)
    _holds(exact, slot, out, "sweep, exact caps")
    assert any(_pieces(o)[0] == 128 for o in out) and sum(_pieces(o)[1] == ny_max for o in out) >= 1
    del exact
    # the source is unchanged
    again = opt.download()
    for o, a in zip(out, again):
        assert np.array_equal(o["c_xy"], a["c_xy"]) and np.array_equal(o["c_yaw"], a["c_yaw"]) and o["T_xy"] == a["T_xy"]
    # traj_states at the sweep's knot times
    tr, ts = [], []
    for b, o in enumerate(out):
        nx, ny = _pieces(o)
        total = _total(o)
        t = [0.0, -0.25, total, np.nextafter(total, 0.0), total + 3.0] + _knot_times(o["T_xy"], nx) + _knot_times(o["T_yaw"], ny)
        tr.append(np.full(len(t), b, dtype=np.int32)), ts.append(np.array(t))
    tr, ts = np.concatenate(tr), np.concatenate(ts)
    _eq(fleet.traj_states(slot[tr], ts), opt.traj_states(tr, ts), "traj_states")
    # the rollout, all channels, with the end row: slot order is the reversed batch order
    offs, rows = _rollout(R, 0.05, 7, 0, B)
    foffs, frows = fleet.rollout(0.05, 7, with_end=True)
    assert np.array_equal(np.diff(foffs), np.diff(offs)[::-1])
    _eq(frows, _segments(offs, rows, range(B - 1, -1, -1)), "rollout")
    # check, locate, within, extent: the same call on the slot and on the source trajectory
    total = np.array([_total(o) for o in out])
    q2 = np.concatenate([src_traj, src_traj])
    tf, tt = np.concatenate([np.zeros(B), 0.3 * total]), np.concatenate([np.full(B, np.inf), 0.6 * total])
    _eq(fleet.check(slot[q2], tf, tt), opt.check(q2, tf, tt), "check")
    assert np.array_equal(fleet.check_limits(), opt.check_limits())
    at = opt.traj_states(src_traj, 0.37 * total)
    poses = at[:, [0, 1, 9]] + np.array([0.05, -0.03, 0.1])
    _eq(fleet.locate(slot, poses), opt.locate(src_traj, poses), "locate")
    rects = np.stack([at[:, 0] - 0.5, at[:, 0] + 0.5, at[:, 1] - 0.5, at[:, 1] + 0.5], axis=1)
    _eq(fleet.within(slot, rects), opt.within(src_traj, rects), "within")
    t0 = 100.0 + 0.1 * np.arange(B)
    _eq(fleet.extent(slot, 99.0, t0 + total + 1.0, t0=t0), opt.extent(src_traj, 99.0, t0 + total + 1.0, t0=t0), "extent")
    # getTraj is the source's
    for b in (0, B // 2, B - 1):
        a, f = opt.getTraj(b), fleet.getTraj(int(slot[b]))
        assert np.array_equal(a.pos_coeffs, f.pos_coeffs) and np.array_equal(a.yaw_coeffs, f.yaw_coeffs) and a.getTotalDuration() == f.getTotalDuration()


# ---- the hill source: 64 goals planned once per module -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hill():
    import uneven_planner_amd as U
    m = _hill_map()
    ka = U.KinoAstar(m)
    S, G = _queries(m, 64, 14000)
    src, res = _source(m, ka, S, G)
    ok = np.array(_valid(res), dtype=np.int32)
    assert len(ok) >= 40, len(ok)
    total = _totals(src)
    _, G2 = _queries(m, 64, 15000)
    return dict(m=m, ka=ka, src=src, res=res, ok=ok, total=total, G2=G2)


# ---- F2 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_tight_caps_and_neighbours(hill):
    import uneven_planner_amd as U
    m, src, res, ok = hill["m"], hill["src"], hill["res"], hill["ok"]
    E = U._lib.UnevenHipError
    by_nx = sorted(ok.tolist(), key=lambda b: _pieces(res[b]))
    short, mid, long_ = by_nx[0], by_nx[len(by_nx) // 2], by_nx[-1]
    assert _pieces(res[short])[0] < _pieces(res[mid])[0] < _pieces(res[long_])[0]
    # caps that equal one trajectory's counts; one piece more is UPH_ERR_LIMIT and takes the admissible query ahead of it down with it
    nx, ny = _pieces(res[mid])
    tight = U.TrajFleet(m, 3, nx, ny)
    tight.adopt(src, [mid], [0])
    _holds(tight, [0], [res[mid]], "tight")
    before = tight.get([0, 1, 2])
    with pytest.raises(E, match=r"uph_fleet_adopt failed \(-4\).*query 1 "):
        tight.adopt(src, [mid, long_], [1, 2])
    assert tight.occupied.tolist() == [True, False, False]
    _eq(tight.get([0, 1, 2]), before, "tight after the refusal")
    _eq(tight.traj_states([0], [1.0]), src.traj_states([mid], [1.0]))
    # replace an occupied slot by a shorter and then a longer trajectory: the slots on either side do not change in a single double, over the whole cap
    fl = U.TrajFleet(m, 3)
    fl.adopt(src, [long_, mid, short], [0, 1, 2], t0=[1.0, 2.0, 3.0])
    sides = fl.get([0, 2])
    for new, start in ((short, 4.0), (long_, 5.0)):
        fl.adopt(src, [new], [1], t0=start)
        _eq(fl.get([0, 2]), sides, "neighbours")
        _holds(fl, [1], [res[new]], "replaced")
        assert fl.t0.tolist() == [1.0, start, 3.0]
        _eq(fl.traj_states([0, 1, 2], [0.7, 0.7, 0.7]), src.traj_states([long_, new, short], [0.7, 0.7, 0.7]))
    # one slot, one adoption
    one = U.TrajFleet(m, 1)
    one.adopt(src, [short], [0])
    _holds(one, [0], [res[short]], "one slot")
    # more adoptions in one call than a workgroup has lanes, every source several times
    n = 300
    many = U.TrajFleet(m, n, 128, 256)
    st = ok[np.arange(n) % ok.size]
    sl = np.random.default_rng(3).permutation(n).astype(np.int32)
    many.adopt(src, st, sl)
    _holds(many, sl, [res[b] for b in st], "many")
    assert many.occupied.all()
    # a fleet adopted from a fleet
    copy = U.TrajFleet(m, 4, 128, 256)
    copy.adopt(many, sl[:4], [3, 2, 1, 0], t0=7.5)
    _holds(copy, [3, 2, 1, 0], [res[b] for b in st[:4]], "fleet to fleet")


# ---- F3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _grouped(owners, iu, ju, call):
    """the existing cross-context calls over pairs (iu[k], ju[k]) of vehicles owned by `owners[i] = (object, trajectory)`: one call per pair of objects, the rows put
    back in pair order.  call(A, ta, tb, other, idx) -> dict of arrays over the pairs idx."""
    out = {}
    objs = []
    for o, _ in owners:
        if not any(o is p for p in objs):
            objs.append(o)
    for A in objs:
        for B in objs:
            idx = np.array([k for k in range(len(iu)) if owners[iu[k]][0] is A and owners[ju[k]][0] is B], dtype=np.int64)
            if idx.size == 0:
                continue
            ta = np.array([owners[i][1] for i in iu[idx]], dtype=np.int32)
            tb = np.array([owners[j][1] for j in ju[idx]], dtype=np.int32)
            r = call(A, ta, tb, None if B is A else B, idx)
            for k, v in r.items():
                if k not in out:
                    out[k] = np.zeros((len(iu),) + v.shape[1:], dtype=v.dtype)
                out[k][idx] = v
    return out


def _listed(rows, iu, ju, first):
    """what a fleet-wide conflicts call must list, from the pair rows: the pairs with a sample below, in (i, j) order"""
    hit = np.nonzero(rows["counts"][:, 1] > 0)[0]
    return dict(pairs=np.stack([iu[hit], ju[hit]], axis=1).astype(np.int32), rows=np.stack([rows[k][hit] for k in (first, "min_t", "first_t", "last_t")], axis=1),
                below=rows["counts"][hit, 1])


@pytest.fixture(scope="module")
def two(hill):
    """the fleet after one cycle: every valid trajectory of src adopted, some refined FROM THE FLEET into fresh and adopted back into their slots"""
    import uneven_planner_amd as U
    m, src, ok, total = hill["m"], hill["src"], hill["ok"], hill["total"]
    n = ok.size
    t0 = 1000.0 + 0.4 * np.arange(n)
    fleet = U.TrajFleet(m, n)
    fleet.adopt(src, ok, np.arange(n), t0=t0)
    bad = np.arange(1, n, 4, dtype=np.int32)
    t_sw = 0.3 * total[ok[bad]]
    fresh = U.ALMTrajOpt(m)
    fresh.set_rho(1.0)
    out = fresh.refine(fleet, bad, t_sw)
    use = np.array([q for q, r in enumerate(out) if r["status"] == 0 and r.get("ret", 4) != 4 and np.isfinite(r["c_xy"]).all()], dtype=np.int64)
    assert use.size >= max(3, bad.size // 2), use.size
    new = np.array([out[q]["traj_of"] for q in use], dtype=np.int32)
    t0 = t0.copy()
    t0[bad[use]] = t0[bad[use]] + t_sw[use]
    fleet.adopt(fresh, new, bad[use], t0=t0[bad[use]])
    owners = [(src, int(b)) for b in ok]
    for q, s in zip(new, bad[use]):
        owners[int(s)] = (fresh, int(q))
    assert np.array_equal(fleet.t0, t0) and fleet.occupied.all()
    _holds(fleet, bad[use], [out[q] for q in use], "refined and adopted back")
    end = max(float(_totals(o)[b]) + t0[i] for i, (o, b) in enumerate(owners))
    return dict(fleet=fleet, fresh=fresh, owners=owners, t0=t0, n=n, tf=999.0, tt=end + 1.0, refined=bad[use])


def test_a_fleet_from_two_objects(hill, two):
    from uneven_planner_amd.alm_traj_opt import conflict_candidates, delay_levels, delay_schedule, delay_times, footprint_radii
    fleet, owners, t0, n, tf, tt = (two[k] for k in ("fleet", "owners", "t0", "n", "tf", "tt"))
    dt = 0.05
    iu, ju = np.triu_indices(n, 1)
    assert sum(o is two["fresh"] for o, _ in owners) >= 3
    # every pair: the fleet's rows are the cross-context rows of the two source objects
    least = _grouped(owners, iu, ju, lambda A, ta, tb, other, idx: A.separation(ta, tb, tf, tt, 0.0, t0_a=t0[iu[idx]], t0_b=t0[ju[idx]], other=other, dt=dt))
    radius = np.full(n, 0.5 * np.median(np.sqrt(least["min_d2"])))
    R = radius[iu] + radius[ju]
    sep = _grouped(owners, iu, ju, lambda A, ta, tb, other, idx: A.separation(ta, tb, tf, tt, R[idx], t0_a=t0[iu[idx]], t0_b=t0[ju[idx]], other=other, dt=dt))
    _eq(fleet.separation(iu, ju, tf, tt, R, t0_a=t0[iu], t0_b=t0[ju], dt=dt), sep, "separation")
    rng = np.random.default_rng(53)
    shape = np.stack([rng.uniform(0.4, 0.5, n), rng.uniform(0.1, 0.2, n), rng.uniform(0.12, 0.18, n)], axis=1)
    margin = rng.uniform(0.0, 0.1, n) * (np.arange(n) % 3 != 0)
    M = margin[iu] + margin[ju]
    foot = _grouped(owners, iu, ju, lambda A, ta, tb, other, idx: A.footprint_separation(ta, tb, tf, tt, shape[iu[idx]], shape[ju[idx]], M[idx], t0_a=t0[iu[idx]],
                                                                                        t0_b=t0[ju[idx]], other=other, dt=dt))
    _eq(fleet.footprint_separation(iu, ju, tf, tt, shape[iu], shape[ju], M, t0_a=t0[iu], t0_b=t0[ju], dt=dt), foot, "footprint_separation")
    # the fleet-wide lists (t0 = None: the stored starts) are the brute force over those rows
    sl = np.arange(n, dtype=np.int32)
    want = _listed(sep, iu, ju, "min_d2")
    got = fleet.conflicts(sl, radius, tf, tt, dt=dt)
    assert 0 < want["pairs"].shape[0] < iu.size and got["n_conflicts"] == want["pairs"].shape[0] and got["n_candidates"] < iu.size
    _eq({k: got[k] for k in ("pairs", "rows", "below")}, want, "conflicts")
    wantf = _listed(foot, iu, ju, "min_c2")
    gotf = fleet.footprint_conflicts(sl, shape, margin, tf, tt, dt=dt)
    assert 0 < wantf["pairs"].shape[0] < iu.size and gotf["n_conflicts"] == wantf["pairs"].shape[0]
    _eq({k: gotf[k] for k in ("pairs", "rows", "below")}, wantf, "footprint_conflicts")
    # the schedules: the sequential greedy (delay_schedule) driven by the cross-context pair calls over the swept-box candidates
    D, step = 8, 0.5
    delta = delay_times(0.0, step, D)
    v = np.concatenate([two["refined"][:4], np.setdiff1d(np.arange(n), two["refined"])[:12]]).astype(np.int32)      # 16 vehicles of both objects, in this priority order
    own = [owners[i] for i in v]
    box = np.zeros((v.size, 4))
    for o in (hill["src"], two["fresh"]):
        k = np.array([q for q in range(v.size) if own[q][0] is o], dtype=np.int64)
        box[k] = o.delay_extent([own[q][1] for q in k], tf, tt, 0.0, step, D, t0=t0[v[k]], dt=dt)["box"]
    _eq(fleet.delay_extent(v, tf, tt, 0.0, step, D, dt=dt)["box"], box, "delay_extent")

    def pair_call(h, i, fn):
        (A, a), (B, b) = own[h], own[i]
        return fn(A, np.full(D, a, dtype=np.int32), np.full(D, b, dtype=np.int32), None if B is A else B)

    for tag, rad_or_margin, cand_r, call, sweep_of in (
            ("delays", radius[v], radius[v], lambda: fleet.delays(v, radius[v], tf, tt, 0.0, step, D, dt=dt),
             lambda h, at, i: pair_call(h, i, lambda A, ta, tb, other: A.separation(ta, tb, tf, tt, radius[v[h]] + radius[v[i]], t0_a=t0[v[h]] + delta[at], t0_b=t0[v[i]] + delta,
                                                                                    other=other, dt=dt))["counts"][:, 1]),
            ("footprint_delays", margin[v], footprint_radii(shape[v], margin[v]), lambda: fleet.footprint_delays(v, shape[v], margin[v], tf, tt, 0.0, step, D, dt=dt),
             lambda h, at, i: pair_call(h, i, lambda A, ta, tb, other: A.footprint_separation(ta, tb, tf, tt, shape[v[h]], shape[v[i]], margin[v[h]] + margin[v[i]],
                                                                                              t0_a=t0[v[h]] + delta[at], t0_b=t0[v[i]] + delta, other=other, dt=dt))["counts"][:, 1])):
        pairs = conflict_candidates(box, cand_r)
        want = delay_schedule(sweep_of, pairs, v.size)
        got = call()
        assert np.array_equal(got["choice"], want["choice"]) and np.array_equal(got["blocker"], want["blocker"]), (tag, got["choice"], want["choice"])
        assert np.array_equal(got["start"], t0[v] + delta[np.maximum(want["choice"], 0)]), tag
        assert (got["n_candidates"], got["n_rounds"], got["n_unresolved"]) == (pairs.shape[0], int(delay_levels(pairs, v.size).max()), int((want["choice"] < 0).sum())), tag
    # the fleet as `other` of a source object, either side
    k = np.arange(min(12, iu.size))
    a_obj = hill["src"]
    mine = np.array([i for i in range(n) if owners[i][0] is a_obj][:k.size], dtype=np.int64)
    ta = np.array([owners[i][1] for i in mine], dtype=np.int32)
    peer = np.roll(np.arange(n), 5)[mine].astype(np.int32)
    x = a_obj.separation(ta, peer, tf, tt, 0.5, t0_a=t0[mine], t0_b=t0[peer], other=fleet, dt=dt)
    y = fleet.separation(mine, peer, tf, tt, 0.5, t0_a=t0[mine], t0_b=t0[peer], dt=dt)
    z = fleet.separation(mine, ta, tf, tt, 0.5, t0_a=t0[mine], t0_b=t0[mine], other=a_obj, dt=dt)
    _eq(x, y, "fleet as side b")
    assert (z["min_d2"] == 0.0).all() and (z["counts"][:, 1] == z["counts"][:, 0]).all()


# ---- F4 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _same_plans(a, b, tag):
    pa, pb = a.last_plan, b.last_plan
    _eq({k: pa[k] for k in ("status", "traj_of", "n_inner_xy", "n_inner_yaw", "switch_states")}, {k: pb[k] for k in ("status", "traj_of", "n_inner_xy", "n_inner_yaw", "switch_states")}, tag)
    sa, sb = a.plan_staged(), b.plan_staged()
    assert len(sa) == len(sb) >= 1, tag
    for x, y in zip(sa, sb):
        _eq({k: np.asarray(x[k]) for k in x}, {k: np.asarray(y[k]) for k in y}, tag + " staged")


def _same_solves(ra, rb, tag):
    assert len(ra) == len(rb)
    for x, y in zip(ra, rb):
        assert set(x) == set(y), tag
        _eq({k: np.asarray(x[k]) for k in x}, {k: np.asarray(y[k]) for k in y}, tag + " solved")


def test_the_fleet_as_src_of_refine_and_replan(hill):
    import uneven_planner_amd as U
    m, ka, src, ok, total, G2 = (hill[k] for k in ("m", "ka", "src", "ok", "total", "G2"))
    n = 12
    slots = np.random.default_rng(9).permutation(n).astype(np.int32)
    fleet = U.TrajFleet(m, n)
    fleet.adopt(src, ok[:n], slots, t0=50.0)
    t_sw = np.concatenate([0.35 * total[ok[:n - 2]], [-1.0, 0.0]])
    a, b = U.ALMTrajOpt(m), U.ALMTrajOpt(m)
    for o in (a, b):
        o.set_rho(1.0)
    ra, rb = a.refine(src, ok[:n], t_sw), b.refine(fleet, slots, t_sw)
    _same_plans(a, b, "refine")
    _same_solves(ra, rb, "refine")
    for goals, tag in ((G2[:n], "replan, new goals"), (None, "replan, the same goals")):
        ra, rb = a.replan_goals(ka, src, ok[:n], t_sw, goals=goals, **MK), b.replan_goals(ka, fleet, slots, t_sw, goals=goals, **MK)
        _same_plans(a, b, tag)
        _same_solves(ra, rb, tag)
        assert sum(r["status"] == 0 for r in ra) >= n // 2, tag
    # the fleet is as it was
    _holds(fleet, slots, [hill["res"][int(j)] for j in ok[:n]], "after serving as src")


# ---- F5 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_local_frames_and_fp32_cells():
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
    p32 = scenes.local_problems(6, seed0=5000, half=14.0, dmin=4.0, dmax=12.0, occ_r2=m32.occ_r2_buffer, grid=(nx, ny, m32.xy_resolution, m32.map_origin[0], m32.map_origin[1]))
    for tag, m, probs in (("frames", big, far), ("f32", m32, p32)):
        opt = U.ALMTrajOpt(m)
        opt.set_rho(1.0)
        res = opt.optimize_batch(probs)
        assert all(r["ret"] != 4 for r in res), tag
        tr = np.arange(len(probs), dtype=np.int32)
        slot = np.array([5, 2, 7, 0, 3, 6], dtype=np.int32)
        fleet = U.TrajFleet(m, 8)
        fleet.adopt(opt, tr, slot, t0=0.5 * tr)
        g = _holds(fleet, slot, res, tag)                  # map coordinates, as the download's
        if tag == "frames":
            assert np.abs(g["c_xy"][:, :2]).max() > 45.0
        _eq(fleet.check(slot, 0.0, None), opt.check(tr, 0.0, None), tag + " check")
        offs, rows = opt.rollout(0.05, 7, with_end=True)
        foffs, frows = fleet.rollout(0.05, 7, with_end=True)
        order = [int(np.nonzero(slot == s)[0][0]) for s in range(8) if s in slot]
        _eq(frows, _segments(offs, rows, order), tag + " rollout")
        assert foffs[2] == foffs[1] and foffs[5] == foffs[4]          # slots 1 and 4 are empty: no rows
        # a second round of adoptions moves trajectories to other slots (other frames per slot): the descriptors are rebuilt
        fleet.adopt(opt, tr[::-1], slot)
        _eq(fleet.check(slot, 0.0, None), opt.check(tr[::-1], 0.0, None), tag + " check, re-adopted")
        _eq(fleet.extent(slot, 0.0, 30.0, t0=1.0)["box"], opt.extent(tr[::-1], 0.0, 30.0, t0=1.0)["box"], tag + " extent")


# ---- F6 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_release_and_empty_slots(hill):
    import uneven_planner_amd as U
    m, src, res, ok = hill["m"], hill["src"], hill["res"], hill["ok"]
    E = U._lib.UnevenHipError
    fleet = U.TrajFleet(m, 4)
    fleet.adopt(src, ok[:3], [0, 1, 2], t0=[1.0, 2.0, 3.0])
    fleet.release([1])
    fleet.release([1, 3])                                    # idempotent, and an empty slot stays empty
    assert fleet.occupied.tolist() == [True, False, True, False] and fleet.t0.tolist() == [1.0, 0.0, 3.0, 0.0]
    g = fleet.get([1])
    assert (g["n_xy"][0], g["n_yaw"][0], g["ret"][0], g["T_xy"][0]) == (0, 0, U._lib.UPH_RET_UNSUPPORTED, 0.0)
    offs = fleet.rollout_plan(0.05, True)
    assert offs[2] == offs[1] and offs[4] == offs[3] and offs[1] > 0 and offs[3] > offs[2]
    calls = dict(traj_states=lambda s: fleet.traj_states(s, [0.5]), check=lambda s: fleet.check(s), locate=lambda s: fleet.locate(s, [0.0, 0.0, 0.0]),
                 within=lambda s: fleet.within(s, [-1.0, 1.0, -1.0, 1.0]), extent=lambda s: fleet.extent(s, 0.0, 5.0),
                 separation=lambda s: fleet.separation([0], s, 0.0, 5.0, 0.5), separation_a=lambda s: fleet.separation(s, [0], 0.0, 5.0, 0.5),
                 other=lambda s: src.separation([int(ok[0])], s, 0.0, 5.0, 0.5, other=fleet),
                 footprint_separation=lambda s: fleet.footprint_separation([0], s, 0.0, 5.0, [0.4, 0.1, 0.15], [0.4, 0.1, 0.15], 0.1),
                 conflicts=lambda s: fleet.conflicts([0] + s, 0.3, 0.0, 5.0), footprint_conflicts=lambda s: fleet.footprint_conflicts([0] + s, [0.4, 0.1, 0.15], 0.1, 0.0, 5.0),
                 delay_sweep=lambda s: fleet.delay_sweep([0], s, 0.0, 5.0, 0.5, 0.0, 0.5, 4), delay_extent=lambda s: fleet.delay_extent(s, 0.0, 5.0, 0.0, 0.5, 4),
                 delays=lambda s: fleet.delays([0] + s, 0.3, 0.0, 5.0, 0.0, 0.5, 4),
                 footprint_delay_sweep=lambda s: fleet.footprint_delay_sweep([0], s, 0.0, 5.0, [0.4, 0.1, 0.15], [0.4, 0.1, 0.15], 0.1, 0.0, 0.5, 4),
                 footprint_delays=lambda s: fleet.footprint_delays([0] + s, [0.4, 0.1, 0.15], 0.1, 0.0, 5.0, 0.0, 0.5, 4),
                 refine=lambda s: U.ALMTrajOpt(m).refine_upload(fleet, s, [0.5]))
    for name, call in calls.items():
        for s in (1, 3):
            with pytest.raises(E, match="empty slot"):
                call([s])
        call([2])                                            # the same call on an occupied slot runs
    with pytest.raises(E, match="getTraj"):
        fleet.getTraj(1)
    # re-adopting works, and the other slots were never touched
    fleet.adopt(src, [ok[5]], [1], t0=9.0)
    _holds(fleet, [0, 1, 2], [res[ok[0]], res[ok[5]], res[ok[2]]], "re-adopted")
    assert fleet.occupied.tolist() == [True, True, True, False] and fleet.t0.tolist() == [1.0, 9.0, 3.0, 0.0]
    _eq(fleet.traj_states([1], [0.5]), src.traj_states([ok[5]], [0.5]))


# ---- F7 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hill):
    import uneven_planner_amd as U
    L = U._lib.load()
    m, ka, src, res, ok = hill["m"], hill["ka"], hill["src"], hill["res"], hill["ok"]
    fleet = U.TrajFleet(m, 4, 128, 256)
    fleet.adopt(src, ok[:2], [0, 1], t0=[1.0, 2.0])
    state = lambda: (fleet.get([0, 1, 2, 3]), fleet.occupied.copy(), fleet.t0.copy())
    before = state()
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(U._lib.DP)

    def refused(rc, code, *words):
        msg = L.uph_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, msg, words)
        now = state()
        _eq(now[0], before[0], msg)
        assert np.array_equal(now[1], before[1]) and np.array_equal(now[2], before[2]), msg

    adopt = lambda f, s, n, tr, sl, t0=None: L.uph_fleet_adopt(f, s, n, ip(tr), ip(sl), None if t0 is None else dp(t0))
    other_map = _hill_map()
    alien = U.ALMTrajOpt(other_map)
    unsolved = U.ALMTrajOpt(m)
    unsolved.upload([dict(init_xy=np.array([[0.0, 0.05, 0.0], [0.0, 0.0, 0.0]]), end_xy=np.array([[0.6, 0.05, 0.0], [0.0, 0.0, 0.0]]), inner_xy=np.array([[0.3], [0.0]]),
                          init_yaw=np.zeros(3), end_yaw=np.zeros(3), inner_yaw=np.zeros(1), total_time=1.44)])
    empty_fleet = U.TrajFleet(m, 2)
    refused(adopt(src.h, src.h, 1, [0], [2]), INVALID, "uph_fleet_adopt", "not a fleet")
    refused(adopt(fleet.h, fleet.h, 1, [0], [2]), INVALID, "uph_fleet_adopt", "the fleet itself")
    refused(adopt(fleet.h, alien.h, 1, [0], [2]), INVALID, "uph_fleet_adopt", "different maps")
    refused(adopt(fleet.h, unsolved.h, 1, [0], [2]), INVALID, "uph_fleet_adopt", "no resident trajectory")
    blank = U.ALMTrajOpt(m)                                  # (kept alive: its context must outlive the call)
    refused(adopt(fleet.h, blank.h, 1, [0], [2]), INVALID, "uph_fleet_adopt", "no resident trajectory")
    refused(adopt(fleet.h, src.h, 2, [ok[0], len(res)], [2, 3]), INVALID, "uph_fleet_adopt", "query 1", "no trajectory of the source")
    refused(adopt(fleet.h, src.h, 2, [ok[0], -1], [2, 3]), INVALID, "uph_fleet_adopt", "query 1")
    refused(adopt(fleet.h, empty_fleet.h, 1, [0], [2]), INVALID, "uph_fleet_adopt", "empty slot")
    refused(adopt(fleet.h, src.h, 2, ok[:2], [2, 4]), INVALID, "uph_fleet_adopt", "query 1", "no slot")
    refused(adopt(fleet.h, src.h, 2, ok[:2], [2, -1]), INVALID, "uph_fleet_adopt", "query 1", "no slot")
    refused(adopt(fleet.h, src.h, 3, ok[:3], [2, 3, 2]), INVALID, "uph_fleet_adopt", "query 2", "second time")
    refused(adopt(fleet.h, src.h, 2, ok[:2], [2, 3], [0.0, np.nan]), INVALID, "uph_fleet_adopt", "query 1", "non-finite t0")
    refused(adopt(fleet.h, src.h, 2, ok[:2], [2, 3], [np.inf, 0.0]), INVALID, "uph_fleet_adopt", "query 0", "non-finite t0")
    refused(adopt(fleet.h, src.h, 0, ok[:1], [2]), INVALID, "uph_fleet_adopt", "bad arguments")
    refused(adopt(fleet.h, src.h, -2, ok[:1], [2]), INVALID, "uph_fleet_adopt", "bad arguments")
    refused(L.uph_fleet_adopt(fleet.h, src.h, 1, None, ip([2]), None), INVALID, "uph_fleet_adopt", "bad arguments")
    refused(L.uph_fleet_adopt(fleet.h, src.h, 1, ip([0]), None, None), INVALID, "uph_fleet_adopt", "bad arguments")
    refused(L.uph_fleet_adopt(fleet.h, None, 1, ip([0]), ip([2]), None), INVALID, "uph_fleet_adopt", "bad arguments")
    # an unsupported slot of the source
    mixed = U.ALMTrajOpt(m)
    good = dict(init_xy=np.array([[0.0, 0.05, 0.0], [0.0, 0.0, 0.0]]), end_xy=np.array([[0.6, 0.05, 0.0], [0.0, 0.0, 0.0]]), inner_xy=np.array([[0.3], [0.0]]),
                init_yaw=np.zeros(3), end_yaw=np.zeros(3), inner_yaw=np.zeros(1), total_time=1.44)
    wrong = dict(good, inner_xy=np.array([[0.2, 0.4], [0.0, 0.0]]))           # fewer yaw pieces than position pieces
    out = mixed.optimize_batch([good, wrong])
    assert out[1]["ret"] == U._lib.UPH_RET_UNSUPPORTED
    refused(adopt(fleet.h, mixed.h, 2, [0, 1], [2, 3]), INVALID, "uph_fleet_adopt", "query 1", "UPH_RET_UNSUPPORTED")
    # an asynchronous solve in flight on the source
    mixed.upload([good])
    mixed.solve_async()
    refused(adopt(fleet.h, mixed.h, 1, [0], [2]), INVALID, "uph_fleet_adopt", "asynchronous solve")
    mixed.wait()
    # more pieces than the caps: UPH_ERR_LIMIT, the query named
    small = U.TrajFleet(m, 2, 1, 1)
    assert adopt(small.h, src.h, 1, ok[:1], [0]) == LIMIT and "query 0" in L.uph_last_error().decode() and not small.occupied.any()
    # the other fleet calls: not on a context that is no fleet, and their own arguments
    for rc in (L.uph_fleet_release(src.h, 1, ip([0])), L.uph_fleet_info(src.h, None, None, None, None, None),
               L.uph_fleet_get(src.h, 1, ip([0]), None, None, None, None, None, None, None), L.uph_fleet_kernel_ms(src.h, C.byref(C.c_double()))):
        refused(rc, INVALID, "uph_fleet_", "not a fleet")
    refused(L.uph_fleet_release(fleet.h, 2, ip([0, 4])), INVALID, "uph_fleet_release", "query 1")
    refused(L.uph_fleet_release(fleet.h, 0, ip([0])), INVALID, "uph_fleet_release")
    refused(L.uph_fleet_get(fleet.h, 1, ip([-1]), None, None, None, None, None, None, None), INVALID, "uph_fleet_get", "query 0")
    refused(L.uph_fleet_kernel_ms(fleet.h, None), INVALID, "uph_fleet_kernel_ms")
    # what uploads into, solves, evaluates, reports on or downloads a batch, or sets its state: "is a fleet"
    h = fleet.h
    arr, keep = U.alm_traj_opt.pack_problems([good])
    resu = (U._lib.Result * 4)()
    one, four = np.zeros(64), np.zeros(4, dtype=np.int32)
    mp = U.ALMTrajOpt._manager_params("test", MK)
    ctxs = (C.c_void_p * 1)(h.value)
    S3, G3 = np.zeros((1, 3)), np.ones((1, 3))
    plan_out = lambda: (ip(four), ip(four), ip(four), ip(four))
    refusing = dict(
        uph_batch_upload=lambda: L.uph_batch_upload(h, 1, arr), uph_optimize_batch=lambda: L.uph_optimize_batch(h, 1, arr, resu),
        uph_optimize_batch_multi=lambda: L.uph_optimize_batch_multi(ctxs, 1, 1, arr, resu),
        uph_plan_upload=lambda: L.uph_plan_upload(ka.h, h, C.byref(mp), 1, dp(S3), dp(G3), 0, *plan_out()),
        uph_replan_upload=lambda: L.uph_replan_upload(ka.h, src.h, h, C.byref(mp), 1, ip([ok[0]]), dp([0.5]), None, 0, None, *plan_out()),
        uph_refine_upload=lambda: L.uph_refine_upload(src.h, h, 1, ip([ok[0]]), dp([0.5]), None, *plan_out()),
        uph_batch_solve=lambda: L.uph_batch_solve(h), uph_batch_solve_async=lambda: L.uph_batch_solve_async(h), uph_batch_wait=lambda: L.uph_batch_wait(h),
        uph_batch_download=lambda: L.uph_batch_download(h, resu), uph_eval_batch=lambda: L.uph_eval_batch(h, None, dp(one), None, 1),
        uph_penalty_batch=lambda: L.uph_penalty_batch(h, 1, 0, dp(one), None, None, None), uph_init_scaling_batch=lambda: L.uph_init_scaling_batch(h),
        uph_report_batch=lambda: L.uph_report_batch(h, dp(one)), uph_batch_set_state=lambda: L.uph_batch_set_state(h, None, None, None, None, dp(one)),
        uph_batch_set_x=lambda: L.uph_batch_set_x(h, dp(one)), uph_batch_alm_passes=lambda: L.uph_batch_alm_passes(h, 1),
        uph_batch_lbfgs_resume=lambda: L.uph_batch_lbfgs_resume(h, 1, 0), uph_batch_get_lbfgs_state=lambda: L.uph_batch_get_lbfgs_state(h, None, None, None, None, None, None, None),
        uph_plan_staged=lambda: L.uph_plan_staged(h, 1, 1, dp(one), dp(one), dp(one), dp(one), dp(one), dp(one), ip(four), ip(four), dp(one)),
        uph_batch_origin=lambda: L.uph_batch_origin(h, ip(four)), uph_batch_stats=lambda: L.uph_batch_stats(h, None, None, None, None, None),
        uph_ctx_set_lanes=lambda: L.uph_ctx_set_lanes(h, 64), uph_ctx_set_wps=lambda: L.uph_ctx_set_wps(h, 1), uph_ctx_set_rho=lambda: L.uph_ctx_set_rho(h, 2.0),
        uph_ctx_set_sample_precision=lambda: L.uph_ctx_set_sample_precision(h, 32), uph_ctx_set_trial_abandon=lambda: L.uph_ctx_set_trial_abandon(h, 0),
        uph_ctx_set_xcd_locality=lambda: L.uph_ctx_set_xcd_locality(h, 16), uph_ctx_set_trace=lambda: L.uph_ctx_set_trace(h, 4))
    for name, call in refusing.items():
        refused(call(), INVALID, name, "is a fleet")
    assert (four == 0).all() and not one.any()
    # ... and the wrapper raises before it gets there
    for name in ("upload", "solve", "download", "eval_batch", "refine", "plan_goals", "set_rho"):
        with pytest.raises(U._lib.UnevenHipError, match="TrajFleet"):
            getattr(fleet, name)()
    # the source is as it was: the fleet still equals it
    _holds(fleet, [0, 1], [res[ok[0]], res[ok[1]]], "after the refusals")


# ---- F8 ---------------------------------------------------------------------------------------------------------------------------------------------------
CPP = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
#include <cstdio>
using namespace uneven_hip;
int main(int argc, char** argv) {
    // in: {ncell, B}, cells, B x {start, goal, start time on the common clock, radius}
    FILE* f = std::fopen(argv[1], "rb");
    long long hdr[2];
    if (!f || fread(hdr, 8, 2, f) != 2) return 2;
    std::vector<double> cells((size_t)hdr[0] * 4), sg((size_t)hdr[1] * 8);
    if (fread(cells.data(), 8, cells.size(), f) != cells.size() || fread(sg.data(), 8, sg.size(), f) != sg.size()) return 2;
    std::fclose(f);
    uph_map_params mp = {2, 10.0, 10.0, 0.2, 0.1, 0.1, 0.05, 0.1, 0.8, 0.05, 9.81};
    UnevenMapHandle map(mp, 0);
    map.setCells(cells.data());
    KinoAstar kino;
    kino.setEnvironment(&map);
    ALMTrajOpt opt;
    opt.setEnvironment(&map);
    std::vector<std::array<double, 3>> starts((size_t)hdr[1]), goals((size_t)hdr[1]);
    for (long long b = 0; b < hdr[1]; b++) for (int k = 0; k < 3; k++) { starts[b][k] = sg[8 * b + k]; goals[b][k] = sg[8 * b + 3 + k]; }
    uph_manager_params mgr{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5};
    ALMTrajOpt::GoalPlan p = opt.planSE2TrajBatch(kino, starts, goals, mgr);
    std::vector<int> traj, slot;
    std::vector<double> t0, rad, tf, tt;
    for (long long b = 0; b < hdr[1]; b++)
        if (p.traj_of[b] >= 0 && p.ret[b] != UPH_RET_UNSUPPORTED) {
            traj.push_back(p.traj_of[b]); t0.push_back(sg[8 * b + 6]); rad.push_back(sg[8 * b + 7]);
            tf.push_back(sg[8 * b + 6] - 0.5); tt.push_back(sg[8 * b + 6] + 12.0);
        }
    const size_t n = traj.size();
    for (size_t k = 0; k < n; k++) slot.push_back((int)(n - k));          // slot 0 stays empty
    TrajFleet fleet;
    fleet.setEnvironment(&map, (int)n + 1, 64, 128);
    fleet.adoptSE2TrajBatch(opt, traj, slot, t0);
    const std::vector<double> starts_kept = fleet.startTimes();
    const std::vector<int32_t> occ = fleet.occupied();
    std::vector<double> tk;
    for (size_t k = 0; k < n; k++) tk.push_back(starts_kept[(size_t)slot[k]]);
    const ALMTrajOpt::TrajExtent e = fleet.extentSE2TrajBatch(slot, tk, tf, tt);
    const ALMTrajOpt::TrajConflicts c = fleet.conflictsSE2TrajBatch(slot, tk, rad, 99.0, 130.0);
    const ALMTrajOpt::TrajSeparation x = opt.separationSE2TrajBatch(traj, slot, t0, tk, tf, tt, rad, 0.05, &fleet);
    const std::vector<double> st = fleet.trajStates(slot, std::vector<double>(n, 0.75));
    int refused = 0;
    try { fleet.getMaxVxAxAyCurAttSigBatch(); } catch (const std::runtime_error&) { refused++; }
    try { fleet.getTraj(0); } catch (const std::runtime_error&) { refused++; }
    FILE* o = std::fopen(argv[2], "wb");
    double head[4] = {(double)n, (double)fleet.slots(), (double)occ[0], (double)refused};
    fwrite(head, 8, 4, o);
    for (size_t k = 0; k < n; k++) { double q = (double)traj[k]; fwrite(&q, 8, 1, o); }
    for (size_t q = 0; q < n; q++) { double h[6] = {e.box[4 * q], e.box[4 * q + 1], e.box[4 * q + 2], e.box[4 * q + 3], (double)e.counts[2 * q], (double)e.counts[2 * q + 1]}; fwrite(h, 8, 6, o); }
    for (size_t q = 0; q < n; q++) { double h[6] = {x.min_d2[q], x.min_t[q], x.first_t[q], x.last_t[q], (double)x.counts[2 * q], (double)x.counts[2 * q + 1]}; fwrite(h, 8, 6, o); }
    fwrite(st.data(), 8, st.size(), o);
    double h3[3] = {(double)c.n_conflicts, (double)c.n_candidates, (double)c.pairs.size()};
    fwrite(h3, 8, 3, o);
    for (size_t k = 0; k < c.pairs.size(); k++) {
        double w[7] = {(double)c.pairs[k][0], (double)c.pairs[k][1], c.min_d2[k], c.min_t[k], c.first_t[k], c.last_t[k], (double)c.below[k]};
        fwrite(w, 8, 7, o);
    }
    // the trajectory of the last slot as the reference's pieces: durations and coefficients, highest order first
    const SE2Trajectory t = fleet.getTraj(slot[0]);
    double np2[2] = {(double)t.pos_traj.getPieceNum(), (double)t.yaw_traj.getPieceNum()};
    fwrite(np2, 8, 2, o);
    for (const Piece<2>& pc : t.pos_traj) { double d = pc.getDuration(); fwrite(&d, 8, 1, o); fwrite(&pc.coeff[0][0], 8, 12, o); }
    for (const Piece<1>& pc : t.yaw_traj) { double d = pc.getDuration(); fwrite(&d, 8, 1, o); fwrite(&pc.coeff[0][0], 8, 6, o); }
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_matches_ctypes_bit_for_bit(tmp_path, analytic_cells):
    import uneven_planner_amd as U
    from uneven_planner_amd import scenes
    m = U.UnevenMap()
    m.set_cells(analytic_cells)
    ka = U.KinoAstar(m)
    S, G = scenes.random_queries(24, seed0=9900)
    t0 = 100.0 + 0.5 * np.arange(S.shape[0])
    rad = 0.2 + 0.05 * (np.arange(S.shape[0]) % 5)
    opt = U.ALMTrajOpt(m)
    opt.set_rho(1.0)
    plan = opt.plan_goals(ka, S, G, **MK)
    src_ = tmp_path / "fleet.cpp"
    src_.write_text(CPP)
    exe = str(tmp_path / "fleet")
    libdir = os.path.join(ROOT, "uneven_planner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src_), "-o", exe, "-L", libdir, "-lunevenhip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    cells = np.ascontiguousarray(analytic_cells, dtype=np.float64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2q", cells.shape[0], S.shape[0]))
        f.write(cells.tobytes())
        f.write(np.ascontiguousarray(np.concatenate([S, G, t0[:, None], rad[:, None]], axis=1), dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, dtype=np.float64)
    live = [b for b in range(S.shape[0]) if plan[b]["status"] == 0 and plan[b]["ret"] != 4]
    tr = np.array([plan[b]["traj_of"] for b in live], dtype=np.int32)
    n = tr.size
    assert raw[:4].tolist() == [n, n + 1, 0.0, 2.0] and n >= 10 and raw[4:4 + n].astype(int).tolist() == tr.tolist()
    t0, rad = t0[live], rad[live]
    tf, tt = t0 - 0.5, t0 + 12.0
    slot = (n - np.arange(n)).astype(np.int32)
    fleet = U.TrajFleet(m, n + 1, 64, 128)
    fleet.adopt(opt, tr, slot, t0=t0)
    at = 4 + n
    ext = raw[at:at + 6 * n].reshape(n, 6)
    _eq(dict(box=ext[:, :4], counts=ext[:, 4:].astype(np.int32)), fleet.extent(slot, tf, tt), "adapter extent")
    at += 6 * n
    sep = raw[at:at + 6 * n].reshape(n, 6)
    want = opt.separation(tr, slot, tf, tt, rad, t0_a=t0, t0_b=t0, other=fleet, dt=0.05)
    _eq(dict(min_d2=sep[:, 0], min_t=sep[:, 1], first_t=sep[:, 2], last_t=sep[:, 3], counts=sep[:, 4:].astype(np.int32)), want, "adapter separation")
    assert (sep[:, 0] == 0.0).all()                          # each trajectory against its own copy in the fleet
    at += 6 * n
    _eq(raw[at:at + 10 * n].reshape(n, 10), fleet.traj_states(slot, np.full(n, 0.75)), "adapter states")
    at += 10 * n
    want = fleet.conflicts(slot, rad, 99.0, 130.0)
    nc, nk, m_ = (int(v) for v in raw[at:at + 3])
    rows = raw[at + 3:at + 3 + 7 * m_].reshape(m_, 7)
    at += 3 + 7 * m_
    assert nc == want["n_conflicts"] and nk == want["n_candidates"] and m_ == want["pairs"].shape[0] >= 1
    assert np.array_equal(rows[:, :2].astype(np.int32), want["pairs"]) and np.array_equal(rows[:, 2:6], want["rows"], equal_nan=True)
    assert np.array_equal(rows[:, 6].astype(np.int32), want["below"])
    npx, npy = int(raw[at]), int(raw[at + 1])
    at += 2
    t = fleet.getTraj(int(slot[0]))
    px = raw[at:at + 13 * npx].reshape(npx, 13)
    at += 13 * npx
    py = raw[at:at + 7 * npy].reshape(npy, 7)
    at += 7 * npy
    assert at == raw.size
    assert np.array_equal(px[:, 0], t.pos_durations) and np.array_equal(px[:, 1:].reshape(npx, 2, 6), t.pos_coeffs)
    assert np.array_equal(py[:, 0], t.yaw_durations) and np.array_equal(py[:, 1:].reshape(npy, 1, 6), t.yaw_coeffs)
