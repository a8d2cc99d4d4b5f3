"""CPU tier of the clearance layer (include/uneven_hip.h uph_clearance_*, uneven_planner_amd/clearance.py): the rule's two numpy forms against each
other and against scipy, both polarities, the guarantee a value gives, the rect arithmetic, the query's mirror on hand-made rows, the bindings and the adapter.
No device is needed: everything here is host arithmetic or text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from uneven_planner_amd import _lib, clearance as CL
from uneven_planner_amd.clearance import (CLEAR_FAR, CLEAR_MAX_R, CLEAR_TO_FREE, CLEAR_TO_OCCUPIED, clearance_brute, clearance_check_rows, clearance_rows,
                                          grow_rect, grow_rect_rows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = ((40, 30, 63), (37, 53, 32))
DENSITIES = (0.0, 0.002, 0.05, 0.5, 1.0)
NAN = float("nan")


def _body(dims, density, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=dims) < density).astype(np.int8)


def _header():
    return open(os.path.join(ROOT, "include", "uneven_hip.h")).read()


def test_symbols_signatures_and_header_text():
    L = _lib.load()
    hdr = _header()
    names = ("uph_body_layer_writes", "uph_clearance_grow_rect", "uph_clearance_create", "uph_clearance_build", "uph_clearance_update", "uph_clearance_get",
             "uph_clearance_info", "uph_clearance_kernel_ms", "uph_clearance_destroy", "uph_clearance_check_batch", "uph_clearance_check_kernel_ms")
    for n in names:
        assert n in _lib.SYMBOLS and hasattr(L, n) and re.search(r"\bint %s\(" % n, hdr), n
    # the number of arguments the binding passes is the number the header declares
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in names:
        args = re.search(r"\bint %s\((.*?)\);" % n, flat, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib.SYMBOLS[n][1]), n
    for name, val in (("UPH_CLEAR_TO_OCCUPIED", 0), ("UPH_CLEAR_TO_FREE", 1), ("UPH_CLEAR_MAX_R", 254), ("UPH_CLEAR_FAR", 65535)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr) and getattr(_lib, name) == val, name
    assert (CLEAR_TO_OCCUPIED, CLEAR_TO_FREE, CLEAR_MAX_R, CLEAR_FAR) == (0, 1, 254, 65535)
    # the contract: the rule, the guarantee, the rect update and the freshness are stated where the ABI is
    for phrase in ("res * (sqrt(D) - sqrt(2))", "sqrt(rmax^2 + 1) for sqrt(D)","grown by rmax and clipped", "exactly one write behind", "never features",
                   "equals a fresh build bit for bit", "earliest", "samples, below, outside, far"):
        assert phrase.lower() in hdr.lower(), phrase
    import uneven_planner_amd as U
    assert U.ClearanceLayer is CL.ClearanceLayer and U.grow_rect is CL.grow_rect and U.CLEAR_FAR == 65535
    assert callable(U.ALMTrajOpt.clearance) and callable(U.ALMTrajOpt.clearance_kernel_ms) and callable(U.BodyLayer.writes)
    assert callable(U.TrajFleet.clearance)


@pytest.mark.parametrize("dims", DIMS, ids=["40x30x63", "37x53x32"])
@pytest.mark.parametrize("polarity", [CLEAR_TO_OCCUPIED, CLEAR_TO_FREE])
def test_the_separable_form_equals_the_disc(dims, polarity):
    seen_far = seen_near = 0
    for k, density in enumerate(DENSITIES):
        body = _body(dims, density, 100 * dims[0] + k)
        for rmax in (1, 5, 13):
            a, b = clearance_rows(body, rmax, polarity), clearance_brute(body, rmax, polarity)
            assert a.dtype == np.uint16 and a.shape == dims and np.array_equal(a, b), (dims, density, rmax, int((a != b).sum()))
            feat = (body == 1) if polarity == CLEAR_TO_OCCUPIED else (body == 0)
            assert np.array_equal(a == 0, feat)
            near = a[a != CLEAR_FAR]
            assert near.size == 0 or near.max() <= rmax * rmax
            seen_far += int((a == CLEAR_FAR).sum())
            seen_near += int(((a > 0) & (a != CLEAR_FAR)).sum())
    assert seen_far > 0 and seen_near > 0


def test_both_polarities_are_each_others_complement():
    """a layer's field under one polarity is the complemented layer's under the other; together a signed field: never both positive"""
    body = _body((37, 53, 32), 0.3, 5)
    for rmax in (3, 64):
        occ, free = clearance_rows(body, rmax, CLEAR_TO_OCCUPIED), clearance_rows(body, rmax, CLEAR_TO_FREE)
        assert np.array_equal(free, clearance_rows(1 - body, rmax, CLEAR_TO_OCCUPIED))
        assert np.array_equal(occ == 0, body == 1) and np.array_equal(free == 0, body == 0)
        assert not ((occ > 0) & (free > 0)).any()
    for bad in (0, 255, -1):
        with pytest.raises(_lib.UnevenHipError, match="rmax"):
            clearance_rows(body, bad)
    with pytest.raises(_lib.UnevenHipError, match="polarity"):
        clearance_rows(body, 3, 2)


@pytest.mark.parametrize("dims", DIMS, ids=["40x30x63", "37x53x32"])
def test_radii_wider_than_the_grid_against_scipy(dims):
    """rmax 64 and 254 reach beyond either side of both grids: every feature of a slice is in range, and the field is scipy's exact transform, squared"""
    ndi = pytest.importorskip("scipy.ndimage")
    for k, density in enumerate(DENSITIES):
        body = _body(dims, density, 7 + k)
        for polarity in (CLEAR_TO_OCCUPIED, CLEAR_TO_FREE):
            feat = (body == 1) if polarity == CLEAR_TO_OCCUPIED else (body == 0)
            want = np.zeros(dims, dtype=np.int64)
            for iw in range(dims[2]):
                if feat[:, :, iw].any():
                    want[:, :, iw] = np.rint(ndi.distance_transform_edt(~feat[:, :, iw]) ** 2).astype(np.int64)
                else:
                    want[:, :, iw] = CLEAR_FAR
            for rmax in (64, 254):
                got = clearance_rows(body, rmax, polarity).astype(np.int64)
                assert np.array_equal(got, np.where(want <= rmax * rmax, want, CLEAR_FAR)), (dims, density, polarity, rmax)


def test_what_a_value_guarantees():
    """a position in column (ix, iy) moved by less than res * (sqrt(D) - sqrt(2)) lands in a column that is not a feature; D = FAR counts as rmax^2 + 1.
    120 000 random in-cell positions, a tenth of them on cell corners, the moves drawn up to the bound"""
    # why FAR is rmax^2 + 1 and not (rmax + 1)^2: the feature at offset (rmax, 1) is beyond the disc, and a corner of the cell is rmax - 1 cells from it
    one = np.zeros((8, 4, 1), dtype=np.int8)
    one[6, 2, 0] = 1
    assert clearance_rows(one, 5)[1, 1, 0] == CLEAR_FAR and clearance_rows(one, 6)[1, 1, 0] == 26
    assert np.hypot(6.01 - 2.0, 2.01 - 2.0) < (5 + 1) - np.sqrt(2.0) and np.hypot(6.0 - 2.0, 0.0) > np.sqrt(26.0) - np.sqrt(2.0)
    rng = np.random.default_rng(41)
    nx, ny, res, rmax = 48, 40, 0.05, 9
    n, tried, moved = 120000, 0, 0
    for density in (0.004, 0.03):
        feat = rng.uniform(size=(nx, ny)) < density
        D = clearance_rows(feat[:, :, None].astype(np.int8), rmax)[:, :, 0].astype(np.float64)
        root = np.where(D == CLEAR_FAR, np.sqrt(rmax * rmax + 1.0), np.sqrt(D))
        ix, iy = rng.integers(0, nx, n // 2), rng.integers(0, ny, n // 2)
        frac = rng.uniform(size=(n // 2, 2))
        corner = np.arange(n // 2) % 10 == 0
        frac[corner] = rng.integers(0, 2, (int(corner.sum()), 2))           # exactly on a corner of the cell (the closed cell: the worst case of the proof)
        bound = res * (root[ix, iy] - np.sqrt(2.0))
        ok = bound > 0.0
        ang = rng.uniform(0.0, 2.0 * np.pi, n // 2)
        length = bound * np.where(rng.uniform(size=n // 2) < 0.5, 1.0 - 1e-9, rng.uniform(size=n // 2))
        px = (ix + frac[:, 0]) * res + length * np.cos(ang)
        py = (iy + frac[:, 1]) * res + length * np.sin(ang)
        # a landing point on a cell edge belongs to every cell that touches it: none of them may be a feature
        for ex in (-1e-12, 1e-12):
            for ey in (-1e-12, 1e-12):
                jx, jy = np.floor((px + ex) / res).astype(np.int64), np.floor((py + ey) / res).astype(np.int64)
                inside = ok & (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny)
                assert not feat[jx[inside], jy[inside]].any(), density
        tried += n // 2
        moved += int(ok.sum())
    assert tried >= 100000 and moved > 20000
    print("guarantee: %d positions, %d with a positive bound, no violation" % (tried, moved))


def test_grow_rect_and_its_refusals():
    L = _lib.load()
    cases = (((40, 30), (17, 18, 11, 12), 5), ((40, 30), (0, 6, 9, 21), 13), ((40, 30), (31, 40, 22, 30), 64), ((40, 30), (0, 40, 0, 30), 1),
             ((40, 30), (3, 3, 0, 5), 7), ((40, 30), (3, 9, 5, 5), 7), ((200, 200), (60, 90, 60, 90), 0), ((37, 53), (36, 37, 0, 1), 254))
    for dims, rect, r in cases:
        got = grow_rect(dims, rect, r)
        assert got == grow_rect_rows(dims, rect, r), (dims, rect, r, got)
        if rect[0] < rect[1] and rect[2] < rect[3]:
            assert got == (max(0, rect[0] - r), min(dims[0], rect[1] + r), max(0, rect[2] - r), min(dims[1], rect[3] + r))
        else:
            assert got == tuple(rect)               # an empty rect stays empty
    # the chain: the map's changed rect grown by the body layer's R, then by rmax, is the rect grown by R + rmax
    assert grow_rect((200, 200), grow_rect((200, 200), (60, 90, 60, 90), 13), 20) == grow_rect((200, 200), (60, 90, 60, 90), 33)
    for dims, rect, r in (((40, 30), (5, 4, 0, 3), 1), ((40, 30), (0, 3, 7, 6), 1), ((40, 30), (-1, 3, 0, 3), 1), ((40, 30), (0, 41, 0, 3), 1), ((40, 30), (0, 3, -2, 3), 1),
                          ((40, 30), (0, 3, 0, 31), 1), ((40, 30), (0, 3, 0, 3), -1), ((0, 30), (0, 0, 0, 3), 1)):
        with pytest.raises(_lib.UnevenHipError):
            grow_rect(dims, rect, r)
        with pytest.raises(_lib.UnevenHipError):
            grow_rect_rows(dims, rect, r)
    out = (C.c_int32 * 4)(9, 9, 9, 9)
    assert L.uph_clearance_grow_rect(None, (C.c_int32 * 4)(0, 1, 0, 1), 1, out) == _lib.UPH_ERR_INVALID and list(out) == [9, 9, 9, 9]
    assert L.uph_clearance_grow_rect((C.c_int32 * 2)(4, 4), (C.c_int32 * 4)(0, 5, 0, 1), 1, out) == _lib.UPH_ERR_INVALID and list(out) == [9, 9, 9, 9]
    assert b"uph_clearance_grow_rect" in L.uph_last_error()


def test_null_handles_are_refused():
    L = _lib.load()
    h = C.c_void_p()
    assert L.uph_clearance_create(None, 5, 0, C.byref(h)) == _lib.UPH_ERR_INVALID and not h.value
    assert L.uph_clearance_build(None) == _lib.UPH_ERR_INVALID and L.uph_clearance_update(None, (C.c_int32 * 4)(0, 1, 0, 1)) == _lib.UPH_ERR_INVALID
    assert L.uph_clearance_get(None, None) == _lib.UPH_ERR_INVALID and L.uph_clearance_info(None, None, None, None, None) == _lib.UPH_ERR_INVALID
    ms = C.c_double(-9.0)
    assert L.uph_clearance_kernel_ms(None, C.byref(ms)) == _lib.UPH_ERR_INVALID and ms.value == -9.0
    assert L.uph_clearance_check_kernel_ms(None, C.byref(ms)) == _lib.UPH_ERR_INVALID and ms.value == -9.0
    w = C.c_uint64(77)
    assert L.uph_body_layer_writes(None, C.byref(w)) == _lib.UPH_ERR_INVALID and w.value == 77
    assert L.uph_clearance_check_batch(None, None, 1, None, None, None, 0.01, 1, None, None, None, None, None, None, None) == _lib.UPH_ERR_INVALID
    assert b"uph_clearance_check_batch" in L.uph_last_error()
    assert L.uph_clearance_destroy(None) == 0


def test_the_query_mirror_on_hand_made_rows():
    dims = (6, 5, 4)
    D = np.full(dims, CLEAR_FAR, dtype=np.uint16)
    D[1, 1, 0], D[2, 1, 0], D[3, 1, 1], D[4, 1, 1], D[4, 2, 1] = 9, 4, 4, 25, 0
    t = np.array([0.0, 0.1, 0.2, 0.3, 0.4])
    ok = np.ones(5, dtype=bool)
    # a tie on the min: the earliest wins
    cells = np.array([[1, 1, 0], [2, 1, 0], [3, 1, 1], [4, 1, 1], [0, 0, 3]])
    r = clearance_check_rows(t, cells, ok, D, dims, 10)
    assert r["min_d2"] == 4 and r["min_t"] == 0.1 and r["min_cell"].tolist() == [2, 1, 0] and r["v"].tolist() == [9, 4, 4, 25, CLEAR_FAR]
    assert r["first_t"] == 0.0 and r["last_t"] == 0.2 and r["counts"].tolist() == [5, 3, 0, 1]
    assert clearance_check_rows(t, cells, ok, D, dims, 4)["counts"].tolist() == [5, 0, 0, 1] and np.isnan(clearance_check_rows(t, cells, ok, D, dims, 4)["first_t"])
    assert clearance_check_rows(t, cells, ok, D, dims, CLEAR_FAR)["counts"].tolist() == [5, 4, 0, 1]
    # an empty window
    e = clearance_check_rows(np.zeros(0), np.zeros((0, 3)), np.zeros(0, dtype=bool), D, dims, 10)
    assert e["min_d2"] == -1 and np.isnan(e["min_t"]) and e["min_cell"].tolist() == [-1, -1, -1] and np.isnan(e["first_t"]) and np.isnan(e["last_t"])
    assert e["counts"].tolist() == [0, 0, 0, 0]
    # all far: the min is FAR at the first sample, nothing below a threshold that is not beyond FAR
    far = np.array([[0, 0, 0], [5, 4, 3], [0, 4, 2]])
    f = clearance_check_rows(t[:3], far, ok[:3], D, dims, CLEAR_FAR)
    assert f["min_d2"] == CLEAR_FAR and f["min_t"] == 0.0 and f["min_cell"].tolist() == [0, 0, 0] and np.isnan(f["first_t"]) and f["counts"].tolist() == [3, 0, 0, 3]
    # outside samples: each index beyond its side, a negative one, and a degenerate pose (ok False; its cell reads (0, 0, -1)) -- value 0, counted, no cell
    out = np.array([[1, 1, 0], [6, 1, 0], [1, 5, 0], [1, 1, 4], [-1, 1, 0], [0, 0, -1]])
    oks = np.array([True, True, True, True, True, False])
    tt = np.arange(6) * 0.5
    o = clearance_check_rows(tt, out, oks, D, dims, 1)
    assert o["v"].tolist() == [9, 0, 0, 0, 0, 0] and o["min_d2"] == 0 and o["min_t"] == 0.5 and o["min_cell"].tolist() == [-1, -1, -1]
    assert o["first_t"] == 0.5 and o["last_t"] == 2.5 and o["counts"].tolist() == [6, 5, 5, 0]
    # a feature cell inside and an outside sample both give 0: the earliest decides whether there is a cell
    both = clearance_check_rows(t[:2], np.array([[4, 2, 1], [9, 9, 9]]), ok[:2], D, dims, 1)
    assert both["min_d2"] == 0 and both["min_cell"].tolist() == [4, 2, 1] and both["counts"].tolist() == [2, 2, 1, 0]
    # metres to squared cells
    assert CL.below2_of(0.2, 0.05).tolist() == 16 and CL.below2_of(0.12, 0.05).tolist() == 6 and CL.below2_of(0.0, 0.05).tolist() == 0
    with pytest.raises(_lib.UnevenHipError):
        CL.below2_of(-0.1, 0.05)


CONSUMER = r"""
#include "uneven_hip_adapter.hpp"
int main() {
    uneven_hip::BodyLayer* b = nullptr;
    uneven_hip::ALMTrajOpt* o = nullptr;
    uneven_hip::TrajFleet* f = nullptr;
    if (b && o && f) {
        uneven_hip::ClearanceLayer layer(*b, 20);
        uneven_hip::ClearanceLayer depth(*b, 64, UPH_CLEAR_TO_FREE);
        layer.build();
        const uneven_hip::ClearanceLayer::Info i = layer.info();
        const std::array<int32_t, 4> body_rect = uneven_hip::ClearanceLayer::growRect(i.dims, {60, 90, 60, 90}, b->info().R);
        layer.update(body_rect);
        std::vector<uint16_t> d = layer.get();
        const int32_t b2 = uneven_hip::ClearanceLayer::below2(0.2, 0.05);
        uneven_hip::ALMTrajOpt::TrajClearance c = o->clearanceSE2TrajBatch(layer, {0}, {0.0}, {}, {b2});
        uneven_hip::ALMTrajOpt::TrajClearance g = f->clearanceSE2TrajBatch(depth, {0}, {0.0}, {1.0}, {b2}, 0.05, false);
        return (int)d.size() + i.rmax + i.polarity + i.behind + (i.fresh() ? 1 : 0) + (int)layer.kernelMs() + (int)b->writes() + c.min_d2[0] + c.min_cell[0][2] +
               (int)c.metres(0, 0.05) + (int)c.first_t[0] + (int)c.last_t[0] + (int)c.min_t[0] + c.counts[3] + g.counts[0];
    }
    return 0;
}
"""


def test_adapter_offers_the_clearance_layer(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "a.o")])
