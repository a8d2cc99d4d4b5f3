"""CPU tier of the map update (uph_map_update_rect, the adapter's new methods): no device needed.

uph_map_update_rect is held to the rule of the ABI header written literally in numpy (map_update_cases.rect_rule).  The GPU tier
(tests/test_gpu_map_update.py) holds uph_map_update itself to a fresh build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from map_update_cases import BOX, rect_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELLIPSOIDS = [dict(), dict(ellipsoid_x=0.45, ellipsoid_y=0.25, ellipsoid_z=0.2)]
BOXES = [BOX,                                     # inside
         (0.0, 1.0, 0.0, 1.0), (-0.25, 0.25, -2.0, -1.5),
         (1.3, 1.3, -0.7, -0.7),                  # degenerate: one point
         (2.025, 2.025, 2.0, 2.6),                # degenerate in x, on a cell centre
         (4.6, 5.4, -5.8, -4.7),                  # straddles two borders
         (-9.0, 9.0, -0.1, 0.1), (-7.0, -4.9, 4.9, 12.0),
         (4.679, 4.7, 0.0, 0.1),                  # the margin reaches the last column or not, depending on the ellipsoid
         (5.7, 6.0, 0.0, 1.0), (0.0, 1.0, -8.0, -5.7), (-30.0, -20.0, -30.0, -20.0),      # outside: empty
         (-np.inf, np.inf, 0.0, 0.0)]


def _params(extra):
    from uneven_planner_amd.uneven_map import HILL_MAP_PARAMS
    return dict(HILL_MAP_PARAMS, **extra)


def _rect(prm, box):
    import uneven_planner_amd as U
    L = U._lib.load()
    mp = U._lib.MapParams(**{k: (int(v) if k == "iter_num" else float(v)) for k, v in prm.items()})
    b = np.asarray(box, dtype=np.float32)
    r = (C.c_int32 * 4)(7, 7, 7, 7)
    rc = L.uph_map_update_rect(C.byref(mp), b.ctypes.data_as(C.POINTER(C.c_float)), r)
    return rc, tuple(int(v) for v in r)


@pytest.mark.parametrize("ell", [0, 1])
def test_update_rect_equals_the_rule(ell):
    prm = _params(ELLIPSOIDS[ell])
    seen_empty = seen_clipped = 0
    for box in BOXES:
        rc, got = _rect(prm, box)
        want = rect_rule(prm, box)
        assert rc == 0 and got == want, (box, got, want)
        seen_empty += want == (0, 0, 0, 0)
        seen_clipped += want != (0, 0, 0, 0) and (want[0] == 0 or want[1] == 200 or want[2] == 0 or want[3] == 200)
    assert seen_empty >= 3 and seen_clipped >= 3
    # the documented case: y columns 87-116 for the box of the GPU tier's one-update test (88-115 without the extra cell of margin)
    if ell == 0:
        assert _rect(prm, BOX)[1][2:] == (87, 117)
        assert _rect(prm, (1.3, 1.3, -0.7, -0.7))[1] == rect_rule(prm, (1.3, 1.3, -0.7, -0.7)) != (0, 0, 0, 0)
    # a non-square grid with another resolution
    prm2 = dict(prm, map_size_x=7.3, map_size_y=4.1, xy_resolution=0.07)
    for box in BOXES:
        assert _rect(prm2, box) == (0, rect_rule(prm2, box)), box


def test_update_rect_refuses_nan_and_reversed_boxes():
    prm = _params({})
    for box in [(np.nan, 1.0, 0.0, 1.0), (0.0, np.nan, 0.0, 1.0), (0.0, 1.0, np.nan, 1.0), (0.0, 1.0, 0.0, np.nan), (1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 1.0, 0.0)]:
        rc, got = _rect(prm, box)
        assert rc == -1 and got == (7, 7, 7, 7), (box, rc, got)
    import uneven_planner_amd as U
    L = U._lib.load()
    assert L.uph_map_update_rect(None, None, None) == -1


def test_update_info_layout_matches_the_header():
    import uneven_planner_amd as U
    I = U._lib.MapUpdateInfo
    assert C.sizeof(I) == 8 * 4 + 4 * 4 + 3 * 8 and I.n_refit.offset == 32 and I.n_removed.offset == 48


ADAPTER_USER = r"""
#include "uneven_hip_adapter.hpp"
using namespace uneven_hip;
// a scan callback: the box and its points go to the map, the changed rect comes back
int on_scan(UnevenMapHandle& map, const std::vector<float>& filtered, const float box[4], const std::vector<float>& scan) {
    map.buildFilteredMap(filtered.data(), (long)(filtered.size() / 3));
    uph_map_update_info info;
    map.updateMap(box, scan, info);
    map.updateMap(box, nullptr, 0, info);                       // remove only
    int32_t rect[4];
    uph_map_params mp{};
    if (uph_map_update_rect(&mp, box, rect) != UPH_OK) return -1;
    return info.full_refit ? -2 : (info.changed[1] - info.changed[0]) * (info.changed[3] - info.changed[2]) + info.n_refit + (int)info.n_cloud;
}
"""


def test_adapter_update_methods_compile(tmp_path):
    src = tmp_path / "scan_user.cpp"
    src.write_text(ADAPTER_USER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "s.o")])
