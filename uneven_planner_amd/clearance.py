"""The clearance layer (include/uneven_hip.h uph_clearance_*, csrc/clearance.hip): the exact, truncated, squared Euclidean distance transform of a
body layer, one field per yaw slice, built and updated in a rect on the device and read along resident trajectories by ALMTrajOpt.clearance.

`ClearanceLayer` binds the device object.  `clearance_rows`, `clearance_brute`, `clearance_check_rows` and `grow_rect_rows` are numpy mirrors written from the
rule, for tests and for callers who want the field of a hypothetical layer on the host; they need no device."""
import ctypes as C

import numpy as np

from . import _lib

CLEAR_TO_OCCUPIED, CLEAR_TO_FREE = _lib.UPH_CLEAR_TO_OCCUPIED, _lib.UPH_CLEAR_TO_FREE
CLEAR_MAX_R, CLEAR_FAR = _lib.UPH_CLEAR_MAX_R, _lib.UPH_CLEAR_FAR


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _admit(rmax, polarity, who):
    rmax, polarity = int(rmax), int(polarity)
    if not 1 <= rmax <= CLEAR_MAX_R:
        raise _lib.UnevenHipError(who + ": rmax must lie in 1 .. CLEAR_MAX_R (254) cells")
    if polarity not in (CLEAR_TO_OCCUPIED, CLEAR_TO_FREE):
        raise _lib.UnevenHipError(who + ": polarity must be CLEAR_TO_OCCUPIED or CLEAR_TO_FREE")
    return rmax, polarity


def features(body, polarity=CLEAR_TO_OCCUPIED):
    """bool [nx][ny][nyaw]: the cells the distance is measured to -- bytes that are 1 under CLEAR_TO_OCCUPIED, bytes that are 0 under CLEAR_TO_FREE"""
    b = np.asarray(body)
    return (b == 0) if int(polarity) == CLEAR_TO_FREE else (b == 1)


def clearance_rows(body, rmax, polarity=CLEAR_TO_OCCUPIED):
    """The rule in its separable form: D [nx][ny][nyaw] (uint16) of the body layer's bytes.  Pass 1 along iy: g = |dy| to the nearest feature of the row within
    rmax (255: none), as the smaller of a forward and a backward count of the columns since the last feature.  Pass 2 along ix: the min over |dx| <= rmax of
    dx^2 + g(ix + dx)^2, kept when it is at most rmax^2 and CLEAR_FAR otherwise."""
    rmax, polarity = _admit(rmax, polarity, "clearance_rows")
    f = features(body, polarity)
    nx, ny, nyaw = f.shape
    big = np.int64(1) << 40
    iy = np.arange(ny, dtype=np.int64)[None, :, None]
    last = np.maximum.accumulate(np.where(f, iy, -big), axis=1)                      # the last feature at or before iy
    nxt = np.minimum.accumulate(np.where(f, iy, big)[:, ::-1], axis=1)[:, ::-1]      # the next one at or after iy
    g = np.minimum(iy - last, nxt - iy)
    g = np.where(g <= rmax, g, 255)
    lim = rmax * rmax + 1
    best = np.full(f.shape, lim, dtype=np.int64)
    g2 = np.where(g == 255, big, g * g)
    for dx in range(0, min(rmax, nx - 1) + 1):
        d2 = dx * dx
        # outputs ix read row ix + dx (ix < nx - dx) and row ix - dx (ix >= dx)
        best[:nx - dx] = np.minimum(best[:nx - dx], g2[dx:] + d2)
        best[dx:] = np.minimum(best[dx:], g2[:nx - dx] + d2)
    return np.where(best < lim, best, CLEAR_FAR).astype(np.uint16)


def clearance_brute(body, rmax, polarity=CLEAR_TO_OCCUPIED):
    """The rule as the loop over the offsets of the disc dx^2 + dy^2 <= rmax^2: a second, independent form for small rmax"""
    rmax, polarity = _admit(rmax, polarity, "clearance_brute")
    f = features(body, polarity)
    nx, ny, nyaw = f.shape
    pad = np.zeros((nx + 2 * rmax, ny + 2 * rmax, nyaw), dtype=bool)                 # cells outside the grid are never features
    pad[rmax:rmax + nx, rmax:rmax + ny] = f
    out = np.full(f.shape, CLEAR_FAR, dtype=np.int64)
    for dx in range(-rmax, rmax + 1):
        for dy in range(-rmax, rmax + 1):
            d2 = dx * dx + dy * dy
            if d2 > rmax * rmax:
                continue
            hit = pad[rmax + dx:rmax + dx + nx, rmax + dy:rmax + dy + ny]
            out = np.where(hit & (d2 < out), d2, out)
    return out.astype(np.uint16)


def grow_rect_rows(dims2, rect, r):
    """uph_clearance_grow_rect in numpy: rect = (x0, x1, y0, y1) grown by r and clipped to dims2 = (nx, ny); an empty rect stays as it is"""
    nx, ny = (int(v) for v in dims2)
    x0, x1, y0, y1 = (int(v) for v in rect)
    if nx <= 0 or ny <= 0 or int(r) < 0:
        raise _lib.UnevenHipError("grow_rect: the dimensions must be positive and r must not be negative")
    if x0 < 0 or x1 > nx or x0 > x1 or y0 < 0 or y1 > ny or y0 > y1:
        raise _lib.UnevenHipError("grow_rect: rect = (x0, x1, y0, y1) must be half-open, ordered and inside the grid")
    if x0 == x1 or y0 == y1:
        return (x0, x1, y0, y1)
    return (max(0, x0 - int(r)), min(nx, x1 + int(r)), max(0, y0 - int(r)), min(ny, y1 + int(r)))


def grow_rect(dims2, rect, r):
    """uph_clearance_grow_rect (host only): the rect grown by r and clipped.  The map's `changed` rect grown by the body layer's R is what BodyLayer.update
    rewrote; that rect grown by rmax is what ClearanceLayer.update rewrites."""
    L = _lib.load()
    d = (C.c_int32 * 2)(*[int(v) for v in dims2])
    rc = (C.c_int32 * 4)(*[int(v) for v in rect])
    out = (C.c_int32 * 4)()
    _lib.check(L.uph_clearance_grow_rect(d, rc, int(r), out), "uph_clearance_grow_rect")
    return tuple(int(v) for v in out)


def clearance_check_rows(t, cells, ok, D, dims, below2):
    """Host mirror of one uph_clearance_check_batch query, written from the rule: t (n,) the window's sample times, cells (n, 3) = ix, iy, iw of the samples'
    points and ok (n,) -- footprint_cover's `point`, `iw` and `ok` --, D the layer's values, dims = (nx, ny, nyaw).  A sample inside the grid has v = D[cell];
    any other (a degenerate pose included) has v = 0 and counts as outside.  Returns min_d2 (-1: empty window), min_t and min_cell (3,) of the earliest sample
    that attains the min (the cell (-1, -1, -1) when it is outside), first_t / last_t of the samples with v < below2 (NaN: none), counts (4,) = samples, below,
    outside, far, and v (n,)."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    n = t.shape[0]
    nx, ny, nyaw = (int(v) for v in dims)
    c = np.asarray(cells, dtype=np.int64).reshape(n, 3)
    D = np.asarray(D).reshape(nx, ny, nyaw)
    inside = np.asarray(ok, dtype=bool).reshape(n) & (c >= 0).all(axis=1) & (c[:, 0] <= nx - 1) & (c[:, 1] <= ny - 1) & (c[:, 2] <= nyaw - 1)
    cc = np.where(inside[:, None], c, 0)
    v = np.where(inside, D[cc[:, 0], cc[:, 1], cc[:, 2]].astype(np.int64), 0)
    below = np.nonzero(v < int(below2))[0]
    out = dict(min_d2=-1, min_t=np.nan, min_cell=np.full(3, -1, dtype=np.int32), first_t=np.nan, last_t=np.nan, v=v,
               counts=np.array([n, below.size, int(np.count_nonzero(~inside)), int(np.count_nonzero(v == CLEAR_FAR))], dtype=np.int32))
    if n:
        j = int(np.argmin(v))                   # the first of equal values
        out["min_d2"], out["min_t"] = int(v[j]), t[j]
        if inside[j]:
            out["min_cell"] = c[j].astype(np.int32)
    if below.size:
        out["first_t"], out["last_t"] = t[below[0]], t[below[-1]]
    return out


def below2_of(below, res):
    """the threshold in squared cells of a distance in metres: ceil((below / res)^2), so that v < below2 holds for every v with res * sqrt(v) < below"""
    b = np.asarray(below, dtype=np.float64)
    if not (np.isfinite(b).all() and (b >= 0.0).all()):
        raise _lib.UnevenHipError("clearance: below must be finite and not negative")
    return np.minimum(np.ceil((b / float(res)) ** 2), 2.0 ** 31 - 1).astype(np.int32)


class ClearanceLayer:
    def __init__(self, body_layer, rmax, polarity=CLEAR_TO_OCCUPIED):
        """the distance transform of body_layer truncated at rmax cells (1 .. CLEAR_MAX_R), built from the body layer's bytes as they are now.  The body layer
        must outlive it: BodyLayer.close raises while a clearance layer names it."""
        self.L = _lib.load()
        self.h = None
        self.body_layer = body_layer
        self.rmax, self.polarity = int(rmax), int(polarity)
        h = C.c_void_p()
        _lib.check(self.L.uph_clearance_create(body_layer.h, self.rmax, self.polarity, C.byref(h)), "uph_clearance_create")
        self.h = h
        self.dims = tuple(self.info()["dims"])

    def build(self):
        _lib.check(self.L.uph_clearance_build(self.h), "uph_clearance_build")
        return self

    def update(self, rect):
        """rect = (x0, x1, y0, y1), half-open, of the columns whose body bytes changed: for a BodyLayer.update(changed) it is grow_rect(dims, changed, R)"""
        r = (C.c_int32 * 4)(*[int(v) for v in rect])
        _lib.check(self.L.uph_clearance_update(self.h, r), "uph_clearance_update")
        return self

    def get(self):
        out = np.zeros(self.dims, dtype=np.uint16)
        _lib.check(self.L.uph_clearance_get(self.h, out.ctypes.data_as(C.POINTER(C.c_uint16))), "uph_clearance_get")
        return out

    def info(self):
        rmax, pol, behind = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        d = (C.c_int32 * 3)()
        _lib.check(self.L.uph_clearance_info(self.h, C.byref(rmax), C.byref(pol), d, C.byref(behind)), "uph_clearance_info")
        return dict(rmax=rmax.value, polarity=pol.value, dims=[int(v) for v in d], behind=behind.value, fresh=behind.value == 0)

    def kernel_ms(self):
        ms = C.c_double(0)
        _lib.check(self.L.uph_clearance_kernel_ms(self.h, C.byref(ms)), "uph_clearance_kernel_ms")
        return ms.value

    def close(self):
        if getattr(self, "h", None):
            _lib.check(self.L.uph_clearance_destroy(self.h), "uph_clearance_destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
