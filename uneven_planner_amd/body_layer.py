"""The body layer (include/uneven_hip.h uph_body_*, csrc/body_occ.hip): the map's occupancy dilated by the vehicle's rectangle, one slice per
yaw bin, built on the device and read by the front-end search (KinoAstar.set_body_layer) where it reads occ_r2 by default.

`BodyLayer` binds the device object.  `body_stencil`, `body_layer_rows` and `body_layer_margin` are numpy mirrors of the rule, for tests and for callers who
want the layer of a hypothetical map on the host; they need no device."""
import ctypes as C
import math

import numpy as np

from . import _lib

FOOT_OCC_XY, FOOT_OUTSIDE = _lib.UPH_FOOT_OCC_XY, _lib.UPH_FOOT_OUTSIDE


def _dp(a):
    return a.ctypes.data_as(_lib.DP)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def map_nyaw(yaw_resolution):
    """yaw bins of a map (uneven_map.cpp:96-110) and the yaw origin"""
    size = 2.0 * math.pi + 5e-2
    return int(math.ceil(size / yaw_resolution)), -size / 2.0


def inflated(shape, margin):
    """(hl', o, w') of the rule: footCheckShape"""
    f, r, w = (float(v) for v in shape)
    return 0.5 * (f + r) + float(margin), 0.5 * (f - r), w + float(margin)


def stencil_radius(res, shape, margin):
    f, r, w = (float(v) for v in shape)
    reach = float(np.hypot(max(f, r) + float(margin), w + float(margin))) * (1.0 + 2.0 ** -40)
    return int(math.floor(reach / float(res))) + 1


def covered(cs, res, shape, margin, R=None):
    """the covered offsets pointwise: bool [nyaw][2R + 1][2R + 1] indexed (iw, dx + R, dy + R); every product and sum rounded on its own, in the rule's order"""
    cs = np.asarray(cs, dtype=np.float64).reshape(-1, 2)
    hl, o, w = inflated(shape, margin)
    if R is None:
        R = stencil_radius(res, shape, margin)
    d = np.arange(-R, R + 1, dtype=np.float64) * float(res)
    c, s = cs[:, 0][:, None, None], cs[:, 1][:, None, None]
    qx = d[None, :, None] - o * c
    qy = d[None, None, :] - o * s
    along = qx * c + qy * s
    across = qx * (-s) + qy * c
    return (np.abs(along) <= hl) & (np.abs(across) <= w)


def body_stencil(cs, res, shape, margin):
    """R, lo [nyaw][2R + 1], hi: smallest and largest covered dy of every row dx (an empty row: lo = 1, hi = 0), from the table cs [nyaw][2] that
    uph_body_stencil returned -- so the mirror does not depend on whose cosine it is"""
    R = stencil_radius(res, shape, margin)
    cov = covered(cs, res, shape, margin, R)
    dy = np.arange(-R, R + 1, dtype=np.int32)
    any_ = cov.any(axis=2)
    lo = np.where(any_, np.where(cov, dy[None, None, :], R + 1).min(axis=2), 1).astype(np.int32)
    hi = np.where(any_, np.where(cov, dy[None, None, :], -R - 1).max(axis=2), 0).astype(np.int32)
    return R, lo, hi


def body_layer_rows(occ_r2, lo, hi, layers):
    """the layer [nx][ny][nyaw] (int8) of occ_r2 [nx][ny] under the stencil rows lo, hi [nyaw][2R + 1]: prefix sums along iy make a row one subtraction"""
    occ_r2 = np.asarray(occ_r2)
    nx, ny = occ_r2.shape
    lo, hi = np.asarray(lo), np.asarray(hi)
    nyaw, W = lo.shape
    R = (W - 1) // 2
    pred = np.full((nx + 2 * R, ny + 2 * R), 1 if (layers & FOOT_OUTSIDE) else 0, dtype=np.int32)
    pred[R:R + nx, R:R + ny] = (occ_r2 != 0) if (layers & FOOT_OCC_XY) else 0
    cnt = np.zeros((nx + 2 * R, ny + 2 * R + 1), dtype=np.int32)
    np.cumsum(pred, axis=1, out=cnt[:, 1:])
    out = np.zeros((nx, ny, nyaw), dtype=np.int8)
    for iw in range(nyaw):
        hit = np.zeros((nx, ny), dtype=bool)
        for k in range(W):
            l, h = int(lo[iw, k]), int(hi[iw, k])
            if l > h:
                continue
            rows = cnt[k:k + nx]                     # rows ix + dx of the padded array, dx = k - R
            hit |= rows[:, R + h + 1:R + h + 1 + ny] != rows[:, R + l:R + l + ny]
        out[:, :, iw] = hit
    return out


def body_layer_margin(res, yaw_res, shape):
    """(res sqrt(2) / 2 + 2 hypot(max(front, rear), half_width) sin(yaw_res / 4)) (1 + 2^-40): with it a 0 of the layer holds for every pose inside the cell"""
    f, r, w = (float(v) for v in shape)
    reach = float(np.hypot(max(f, r), w))
    return (float(res) * math.sqrt(2.0) / 2.0 + 2.0 * reach * math.sin(float(yaw_res) / 4.0)) * (1.0 + 2.0 ** -40)


def _map_params(params):
    from .uneven_map import HILL_MAP_PARAMS
    q = dict(HILL_MAP_PARAMS)
    if params:
        q.update(params)
    return _lib.MapParams(**{k: (int(v) if k == "iter_num" else float(v)) for k, v in q.items()})


def stencil(params, shape, margin):
    """uph_body_stencil for a map with these parameters (host only): dict(R, nyaw, cs [nyaw][2], lo, hi [nyaw][2R + 1])"""
    L = _lib.load()
    mp = _map_params(params)
    sh = np.ascontiguousarray(shape, dtype=np.float64).reshape(3)
    R, nyaw = C.c_int32(0), C.c_int32(0)
    _lib.check(L.uph_body_stencil(C.byref(mp), _dp(sh), float(margin), C.byref(R), C.byref(nyaw), None, None, None), "uph_body_stencil")
    cs = np.zeros((nyaw.value, 2))
    lo = np.zeros((nyaw.value, 2 * R.value + 1), dtype=np.int32)
    hi = np.zeros_like(lo)
    _lib.check(L.uph_body_stencil(C.byref(mp), _dp(sh), float(margin), None, None, _dp(cs), _ip(lo), _ip(hi)), "uph_body_stencil")
    return dict(R=R.value, nyaw=nyaw.value, cs=cs, lo=lo, hi=hi)


def layer_margin(params, shape):
    """uph_body_layer_margin for a map with these parameters (host only)"""
    L = _lib.load()
    mp = _map_params(params)
    sh = np.ascontiguousarray(shape, dtype=np.float64).reshape(3)
    m = C.c_double(0)
    _lib.check(L.uph_body_layer_margin(C.byref(mp), _dp(sh), C.byref(m)), "uph_body_layer_margin")
    return m.value


class BodyLayer:
    def __init__(self, uneven_map, shape, margin=None, layers=FOOT_OCC_XY | FOOT_OUTSIDE):
        """shape = (front, rear, half_width); margin None: the conservative margin (uph_body_layer_margin).  Builds from the map's occupancy as it is now."""
        self.L = _lib.load()
        self.h = None
        self.uneven_map = uneven_map
        self.shape = np.ascontiguousarray(shape, dtype=np.float64).reshape(3)
        self.margin = layer_margin(uneven_map.params, self.shape) if margin is None else float(margin)
        self.layers = int(layers)
        h = C.c_void_p()
        _lib.check(self.L.uph_body_layer_create(uneven_map.h, _dp(self.shape), self.margin, self.layers, C.byref(h)), "uph_body_layer_create")
        self.h = h
        self.dims = tuple(self.info()["dims"])

    def build(self):
        _lib.check(self.L.uph_body_layer_build(self.h), "uph_body_layer_build")
        return self

    def update(self, rect):
        """rect = (x0, x1, y0, y1), half-open, of the columns whose occupancy changed (UnevenMap.update's info["changed"])"""
        r = (C.c_int32 * 4)(*[int(v) for v in rect])
        _lib.check(self.L.uph_body_layer_update(self.h, r), "uph_body_layer_update")
        return self

    def get(self):
        out = np.zeros(self.dims, dtype=np.int8)
        _lib.check(self.L.uph_body_layer_get(self.h, out.ctypes.data_as(C.c_char_p)), "uph_body_layer_get")
        return out

    def set(self, layer_bytes):
        """the caller's own layer [nx][ny][nyaw]: every byte 0 (free) or 1 (occupied), anything else is refused"""
        b = np.ascontiguousarray(layer_bytes, dtype=np.int8)
        assert b.size == int(np.prod(self.dims)), "a layer has nx * ny * nyaw bytes"
        _lib.check(self.L.uph_body_layer_set(self.h, b.ctypes.data_as(C.c_char_p)), "uph_body_layer_set")
        return self

    def stencil(self):
        return stencil(self.uneven_map.params, self.shape, self.margin)

    def info(self):
        sh = np.zeros(3)
        m = C.c_double(0)
        lay, R, behind = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        d = (C.c_int32 * 3)()
        _lib.check(self.L.uph_body_layer_info(self.h, _dp(sh), C.byref(m), C.byref(lay), C.byref(R), d, C.byref(behind)), "uph_body_layer_info")
        return dict(shape=sh, margin=m.value, layers=lay.value, R=R.value, dims=[int(v) for v in d], behind=behind.value, fresh=behind.value == 0)

    def writes(self):
        """how often the layer's bytes have been written: build (the one of the constructor included), update and set count one each -- the stamp of a
        ClearanceLayer"""
        w = C.c_uint64(0)
        _lib.check(self.L.uph_body_layer_writes(self.h, C.byref(w)), "uph_body_layer_writes")
        return int(w.value)

    def kernel_ms(self):
        ms = C.c_double(0)
        _lib.check(self.L.uph_body_layer_kernel_ms(self.h, C.byref(ms)), "uph_body_layer_kernel_ms")
        return ms.value

    def close(self):
        """raises while a search context still names the layer"""
        if getattr(self, "h", None):
            _lib.check(self.L.uph_body_layer_destroy(self.h), "uph_body_layer_destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
