"""CPU tier of the goals -> resident trajectories chain (uph_plan_upload, PlanManager::rcvWpsCallBack plan_manager.cpp:43-134 with every stage on
the device): the C-ABI and its binding, argument refusals that need no device, the C++ adapter's planSE2TrajBatch, and the shared comb walk
(csrc/resample_walk.hpp) built by g++ on its own against uph_resample_batch.  The GPU tier is tests/test_gpu_plan_chain.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from uneven_planner_amd import _lib
from uneven_planner_amd import resample as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uneven_planner_amd", "csrc")


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_new_symbols_are_exported_with_the_binding_signatures():
    L = _lib.load()
    assert _lib.SYMBOLS["uph_plan_upload"][1][:3] == [C.c_void_p, C.c_void_p, C.POINTER(_lib.ManagerParams)]
    assert len(_lib.SYMBOLS["uph_plan_upload"][1]) == 11 and len(_lib.SYMBOLS["uph_plan_staged"][1]) == 12
    for name in ("uph_plan_upload", "uph_plan_staged"):
        fn = getattr(L, name)
        assert fn.restype == C.c_int and fn.argtypes == _lib.SYMBOLS[name][1]
    hdr = open(os.path.join(ROOT, "include", "uneven_hip.h")).read()
    assert "#define UPH_PLAN_PATH_CAP %d" % _lib.UPH_PLAN_PATH_CAP in hdr


def test_refusals_need_no_device():
    """null handles, negative counts / capacities and bad manager parameters are refused before any HIP call: UPH_ERR_INVALID, no CPU fall-back"""
    L = _lib.load()
    mp = _lib.ManagerParams(**R.MANAGER_PARAMS)
    s, g = np.zeros((4, 3)), np.ones((4, 3))
    st, to, nx, ny = (np.full(4, 7, dtype=np.int32) for _ in range(4))
    dp = lambda a: a.ctypes.data_as(_lib.DP)
    fake = C.c_void_p(0x1000)            # never dereferenced: every call below fails its argument check first
    cases = [(None, None, C.byref(mp), 4, 0), (fake, None, C.byref(mp), 4, 0), (None, fake, C.byref(mp), 4, 0), (fake, fake, None, 4, 0),
             (fake, fake, C.byref(mp), 0, 0), (fake, fake, C.byref(mp), -3, 0), (fake, fake, C.byref(mp), 4, -1)]
    for k, c, m, B, cap in cases:
        assert L.uph_plan_upload(k, c, m, B, dp(s), dp(g), cap, _ip(st), _ip(to), _ip(nx), _ip(ny)) == -1
        assert b"uph_plan_upload" in L.uph_last_error()
    # a null output array, null starts
    assert L.uph_plan_upload(fake, fake, C.byref(mp), 4, dp(s), dp(g), 0, None, _ip(to), _ip(nx), _ip(ny)) == -1
    assert L.uph_plan_upload(fake, fake, C.byref(mp), 4, None, dp(g), 0, _ip(st), _ip(to), _ip(nx), _ip(ny)) == -1
    # manager parameters the stage cannot walk with (piece_len 0; test mode without a max_vel)
    for kw in (dict(piece_len=0.0), dict(yaw_piece_times=-1.0), dict(mean_vel=0.0), dict(test_mode=1, test_max_vel=0.0)):
        q = dict(R.MANAGER_PARAMS)
        q.update(kw)
        bad = _lib.ManagerParams(**q)
        assert L.uph_plan_upload(fake, fake, C.byref(bad), 4, dp(s), dp(g), 0, _ip(st), _ip(to), _ip(nx), _ip(ny)) == -1
    assert (st == 7).all() and (to == 7).all()       # refused before anything was written
    z = np.zeros(8)
    n = np.zeros(1, dtype=np.int32)
    assert L.uph_plan_staged(None, 4, 4, dp(z), dp(z), dp(z), dp(z), dp(z), dp(z), _ip(n), _ip(n), dp(z)) == -1
    assert L.uph_plan_staged(fake, -1, 4, dp(z), dp(z), dp(z), dp(z), dp(z), dp(z), _ip(n), _ip(n), dp(z)) == -1
    assert L.uph_plan_staged(fake, 4, 4, dp(z), None, dp(z), dp(z), dp(z), dp(z), _ip(n), _ip(n), dp(z)) == -1


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
#include <array>
int plan_goals(uneven_hip::UnevenMapHandle* map) {
    uneven_hip::KinoAstar kino;
    kino.setEnvironment(map);
    uneven_hip::ALMTrajOpt opt;
    opt.setEnvironment(map);
    std::vector<std::array<double, 3>> starts(2, std::array<double, 3>{{0.0, 0.0, 0.0}}), goals(2, std::array<double, 3>{{2.0, 1.0, 0.5}});
    uph_manager_params mgr{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5};
    uneven_hip::ALMTrajOpt::GoalPlan p = opt.planSE2TrajBatch(kino, starts, goals, mgr);
    int n = 0;
    for (size_t b = 0; b < p.ret.size(); b++) {
        if (p.traj_of[b] < 0) { n += p.status[b] == UPH_KINO_OK ? 100 : 0; continue; }
        n += p.ret[b] == 0 ? 1 : 0;
        n += p.traj[b].getTotalDuration() > 0.0 ? 1 : 0;
    }
    std::vector<std::vector<uneven_hip::SE3Pose>> path = opt.getSE3PathBatch(0.03);
    return n + (int)path.size();
}
"""


def test_adapter_plan_se2_traj_batch_compiles(tmp_path):
    src = tmp_path / "goals.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "goals.o")])


WALK_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "resample_walk.hpp"
// stdin-free driver: argv[1] = binary file {int32 B, int32 cap_xy, int32 cap_yaw, ManagerParams as 7 doubles (test_mode as a double),
// int64 offsets[B + 1], double poses[offsets[B]][3]}; argv[2] = output: per path {int32 nxy, nyw; double init_xy[6], end_xy[6], init_yaw[3],
// end_yaw[3], total_time, inner_xy[2 cap_xy], inner_yaw[cap_yaw]}
struct P { const double* p; double operator()(int64_t k, int j) const { return p[3 * k + j]; } };
struct S {
    double *oxy, *oyw; int cx, cy, nxy = 0, nyw = 0;
    void xy(double x, double y) { if (nxy < cx) { oxy[2 * nxy] = x; oxy[2 * nxy + 1] = y; } nxy++; }
    void yaw(double v) { if (nyw < cy) oyw[nyw] = v; nyw++; }
    void unwrapped(int64_t, double) {}
};
int main(int argc, char** argv) {
    FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[3]; double mpd[7];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(mpd, 8, 7, f) != 7) return 2;
    const int B = hdr[0], cx = hdr[1], cy = hdr[2];
    uph_manager_params mp{mpd[0], mpd[1], mpd[2], mpd[3], mpd[4], (int32_t)mpd[5], mpd[6]};
    std::vector<int64_t> off(B + 1);
    if (std::fread(off.data(), 8, B + 1, f) != (size_t)B + 1) return 2;
    std::vector<double> poses(3 * off[B]);
    if (std::fread(poses.data(), 8, poses.size(), f) != poses.size()) return 2;
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb");
    const uph::WalkSetup ws = uph::walkSetup(mp);
    std::vector<double> oxy(2 * cx), oyw(cy);
    for (int b = 0; b < B; b++) {
        const double* p = poses.data() + 3 * off[b];
        const int64_t m = off[b + 1] - off[b];
        std::fill(oxy.begin(), oxy.end(), 0.0); std::fill(oyw.begin(), oyw.end(), 0.0);
        S s{oxy.data(), oyw.data(), cx, cy};
        const uph::WalkEnd e = uph::resampleWalk(ws, P{p}, m, s);
        double ixy[6] = {p[0], p[1], ws.sig_vel * std::cos(e.yaw_first), ws.sig_vel * std::sin(e.yaw_first), 0.0, 0.0};
        double exy[6] = {p[3 * (m - 1)], p[3 * (m - 1) + 1], ws.sig_vel * std::cos(e.yaw_last), ws.sig_vel * std::sin(e.yaw_last), 0.0, 0.0};
        double iyw[3] = {e.yaw_first, 0.0, 0.0}, eyw[3] = {e.yaw_last, 0.0, 0.0};
        const double tt = uph::walkTotalTime(ws, mp, e.len);
        int32_t n2[2] = {s.nxy, s.nyw};
        std::fwrite(n2, 4, 2, o); std::fwrite(ixy, 8, 6, o); std::fwrite(exy, 8, 6, o); std::fwrite(iyw, 8, 3, o); std::fwrite(eyw, 8, 3, o);
        std::fwrite(&tt, 8, 1, o); std::fwrite(oxy.data(), 8, oxy.size(), o); std::fwrite(oyw.data(), 8, oyw.size(), o);
    }
    std::fclose(o);
    return 0;
}
"""


def _walk_paths(n, seed):
    """front-end style paths: Hermite curves at several sample spacings, yaw columns wrapped with 2 pi jumps, repeated poses, long jumps"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = np.array([rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(-math.pi, math.pi)])
        g = np.array([rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(-math.pi, math.pi)])
        p = R.hermite_path(s, g, interval=rng.choice([0.03, 0.06, 0.11]))
        if i % 3 == 0:
            p[:, 2] = np.arctan2(np.sin(p[:, 2]), np.cos(p[:, 2])) + 2 * math.pi * rng.integers(-2, 3, size=p.shape[0])
        if i % 4 == 1:
            p = np.concatenate([p[:5], p[4:5], p[4:5], p[5::7]])
        out.append(p)
    return out


def test_shared_walk_built_by_gpp_reproduces_the_host_stage(tmp_path):
    """csrc/resample_walk.hpp is the comb walk of both the host routine and the device kernel: compiled alone by g++ it must reproduce
    uph_resample_batch bit for bit -- counts, way-points, boundary states, total_time -- in both producers' variants"""
    drv = tmp_path / "walk.cpp"
    drv.write_text(WALK_DRIVER)
    exe = tmp_path / "walk"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(drv), "-o", str(exe)])
    ps = _walk_paths(48, 77)
    cx, cy = 512, 1024
    for kw in (dict(), dict(piece_len=0.2, yaw_piece_times=3.0, mean_vel=0.7, init_time_times=1.4, init_sig_vel=0.08), dict(test_mode=1, test_max_vel=0.6)):
        mk = dict(R.MANAGER_PARAMS)
        mk.update(kw)
        off = np.zeros(len(ps) + 1, dtype=np.int64)
        off[1:] = np.cumsum([p.shape[0] for p in ps])
        inp = tmp_path / "in.bin"
        with open(inp, "wb") as f:
            f.write(np.array([len(ps), cx, cy], dtype=np.int32).tobytes())
            f.write(np.array([mk[k] for k in ("piece_len", "mean_vel", "init_time_times", "yaw_piece_times", "init_sig_vel", "test_mode", "test_max_vel")],
                             dtype=np.float64).tobytes())
            f.write(off.tobytes())
            f.write(np.ascontiguousarray(np.concatenate(ps), dtype=np.float64).tobytes())
        outp = tmp_path / "out.bin"
        subprocess.check_call([str(exe), str(inp), str(outp)])
        raw = outp.read_bytes()
        rec = np.dtype([("n", "<i4", 2), ("ixy", "<f8", 6), ("exy", "<f8", 6), ("iyw", "<f8", 3), ("eyw", "<f8", 3), ("tt", "<f8"),
                        ("oxy", "<f8", 2 * cx), ("oyw", "<f8", cy)])
        got = np.frombuffer(raw, dtype=rec)
        native = R.resample_batch(ps, cap_xy=cx, cap_yaw=cy, **kw)
        n_nodes = 0
        for b, nat in enumerate(native):
            r = got[b]
            nxy, nyw = int(r["n"][0]), int(r["n"][1])
            assert (nxy, nyw) == (nat["inner_xy"].shape[1], nat["inner_yaw"].shape[0]), (kw, b)
            assert np.array_equal(r["ixy"], nat["init_xy"].T.ravel()) and np.array_equal(r["exy"], nat["end_xy"].T.ravel())
            assert np.array_equal(r["iyw"], nat["init_yaw"]) and np.array_equal(r["eyw"], nat["end_yaw"]) and r["tt"] == nat["total_time"]
            assert np.array_equal(r["oxy"][:2 * nxy], nat["inner_xy"].T.ravel()) and np.array_equal(r["oyw"][:nyw], nat["inner_yaw"])
            n_nodes += nxy + nyw
        assert n_nodes > 1000


def test_header_constants_match_the_binding():
    hdr = open(os.path.join(ROOT, "include", "uneven_hip.h")).read()
    assert "#define UPH_MAX_PIECE_XY %d " % _lib.UPH_MAX_PIECE_XY in hdr and "#define UPH_MAX_PIECE_YAW %d " % _lib.UPH_MAX_PIECE_YAW in hdr
    assert (_lib.PLAN_STAGE_XY, _lib.PLAN_STAGE_YAW) == (_lib.UPH_MAX_PIECE_XY - 1, _lib.UPH_MAX_PIECE_YAW - 1)
    assert "#define UPH_ERR_INVALID (%d)" % _lib.UPH_ERR_INVALID in hdr and "#define UPH_ERR_LIMIT (%d)" % _lib.UPH_ERR_LIMIT in hdr
    assert "#define UPH_KINO_OK %d" % _lib.UPH_KINO_OK in hdr


class _FakeLib:
    """stands in for the library behind ALMTrajOpt.plan_goals_upload: returns `rc` and, when `write` is given, writes those statuses (the way
    uph_plan_upload writes its outputs: all together, traj_of -1 for goals without a path)"""

    def __init__(self, rc, write=None, count=0):
        self.rc, self.write, self.count = rc, write, count

    def uph_plan_upload(self, kh, h, mp, B, s, g, cap, st, to, nx, ny):
        if self.write is not None:
            for b, v in enumerate(self.write):
                st[b], to[b], nx[b], ny[b] = v, (b if v == 0 else -1), 0, 0
        return self.rc

    def uph_batch_count(self, h):
        return self.count

    def uph_last_error(self):
        return _lib.load().uph_last_error()


def _fake_opt(fake):
    import uneven_planner_amd as U
    opt = U.ALMTrajOpt.__new__(U.ALMTrajOpt)      # (no device: the context is never touched, only the return code and the outputs are read)
    opt.L, opt.h, opt.int_K = fake, None, 16
    return opt


def test_plan_goals_raises_on_every_failure_but_no_path():
    """plan_goals_upload treats ONLY "no goal produced a path" (UPH_ERR_INVALID with the outputs written, no UPH_KINO_OK among them) as an empty
    batch; a HIP failure inside the search (outputs untouched), bad arguments, or a batch whose found problems were all refused must raise"""
    import pytest
    import types
    kino = types.SimpleNamespace(h=None)
    S, G = np.zeros((3, 3)), np.ones((3, 3))
    plan = _fake_opt(_FakeLib(-1, write=[3, 1, 2])).plan_goals_upload(kino, S, G)
    assert plan["status"].tolist() == [3, 1, 2] and (plan["traj_of"] == -1).all()
    out = _fake_opt(_FakeLib(-1, write=[3, 6, 6])).plan_goals(kino, S, G)      # (statuses of failed searches, UPH_KINO_INTERNAL included)
    assert [r["status"] for r in out] == [3, 6, 6]
    for fake in (_FakeLib(-2), _FakeLib(-1), _FakeLib(-4, write=[0, 3, 0]), _FakeLib(-1, write=[0, 3, 0]), _FakeLib(-2, write=[3, 3, 3])):
        with pytest.raises(_lib.UnevenHipError):
            _fake_opt(fake).plan_goals_upload(kino, S, G)
