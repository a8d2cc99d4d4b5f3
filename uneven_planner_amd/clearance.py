"""The clearance layer (include/uneven_hip.h uph_clearance_*, csrc/clearance.hip): the exact, truncated, squared Euclidean distance transform of a
body layer, one field per yaw slice, built and updated in a rect on the device and read along resident trajectories by ALMTrajOpt.clearance.

`ClearanceLayer` binds the device object.  `clearance_rows`, `clearance_brute`, `clearance_check_rows` and `grow_rect_rows` are numpy mirrors written from the
rule, for tests and for callers who want the field of a hypothetical layer on the host; they need no device.  `clearance_field` and `clearance_term_rows`
mirror the continuous field made of the values and the clearance term of the objective that reads it."""
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


def layer_geometry(uneven_map):
    """the `geometry` the field's mirrors take, of a map: (origin (3,), xy_resolution, yaw_resolution)"""
    return (np.asarray(uneven_map.map_origin, dtype=np.float64).copy(), float(uneven_map.xy_resolution), float(uneven_map.yaw_resolution))


def _norm_so2(yaw):
    """UnevenMap::normSO2 as the device runs it: + / - 2 pi until the angle lies in [-pi, pi], at most 4096 times each way; a NaN or an infinity stays"""
    y = np.array(yaw, dtype=np.float64).reshape(-1)
    two_pi = 2 * 3.14159265358979323846
    with np.errstate(invalid="ignore"):
        for _ in range(4096):
            m = y < -3.14159265358979323846
            if not m.any():
                break
            y[m] += two_pi
        for _ in range(4096):
            m = y > 3.14159265358979323846
            if not m.any():
                break
            y[m] -= two_pi
    return y


def clearance_field(D, geometry, rmax, pos):
    """Host mirror of uph_clearance_field (csrc/clearance_dev.hpp), written from the rule: the continuous clearance c in metres and its gradient (dc/dx, dc/dy)
    at pos (n, 3) = x, y, yaw from the values D [nx][ny][nyaw] of a layer of polarity CLEAR_TO_OCCUPIED; geometry = layer_geometry(map).
      yaw slice   iw = floor((normSO2(yaw) - origin_w) / yaw_res): piecewise constant in yaw, no yaw gradient
      cell value  d = res * sqrt(min(D, rmax^2 + 1)): CLEAR_FAR reads as the first distance beyond the disc
      in xy       bilinear between the four nearest cell centres, u = (x - origin_x) / res - 0.5, i0 = floor(u), fx = u - i0; indices clamped to the grid
      degenerate  a pose that is not finite or whose index reaches 2^30: value and gradient 0
    The quotients are products with 1 / res and 1 / yaw_res, the reciprocals the grid holds, and every operation is the device's in its order.
    Returns (c (n,), grad (n, 2))."""
    origin, res, yaw_res = geometry
    D = np.asarray(D)
    nx, ny, nyaw = D.shape
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    x, y, w = p[:, 0], p[:, 1], _norm_so2(p[:, 2])
    xy_inv, yaw_inv = 1.0 / res, 1.0 / yaw_res
    with np.errstate(invalid="ignore", over="ignore"):
        u, v = (x - origin[0]) * xy_inv - 0.5, (y - origin[1]) * xy_inv - 0.5
        fu, fv, fw = np.floor(u), np.floor(v), np.floor((w - origin[2]) * yaw_inv)
        lim30 = 1073741824.0
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(w) & (np.abs(fu) < lim30) & (np.abs(fv) < lim30) & (np.abs(fw) < lim30)
        fx, fy = np.where(ok, u - fu, 0.0), np.where(ok, v - fv, 0.0)
    i0, j0, k0 = (np.where(ok, f, 0.0).astype(np.int64) for f in (fu, fv, fw))
    xa, xb = np.clip(i0, 0, nx - 1), np.clip(i0 + 1, 0, nx - 1)
    ya, yb = np.clip(j0, 0, ny - 1), np.clip(j0 + 1, 0, ny - 1)
    iw = np.clip(k0, 0, nyaw - 1)
    lim = int(rmax) * int(rmax) + 1
    m = [res * np.sqrt(np.minimum(D[a, b, iw].astype(np.int64), lim).astype(np.float64)) for a, b in ((xa, ya), (xb, ya), (xa, yb), (xb, yb))]
    lo, hi = m[0] * (1.0 - fx) + m[1] * fx, m[2] * (1.0 - fx) + m[3] * fx
    c = lo * (1.0 - fy) + hi * fy
    gx = ((m[1] - m[0]) * (1.0 - fy) + (m[3] - m[2]) * fy) * xy_inv
    gy = (hi - lo) * xy_inv
    return np.where(ok, c, 0.0), np.stack([np.where(ok, gx, 0.0), np.where(ok, gy, 0.0)], axis=1)


def clearance_term_rows(D, geometry, rmax, d_safe, weight, c_xy, c_yaw, T_xy, T_yaw, K, scale_fx=1.0):
    """Host mirror of what the clearance term (uph_ctx_set_clearance_term) adds to calConstrainCostGrad for ONE trajectory, from its downloaded piece
    coefficients c_xy (6 Nxy, 2), c_yaw (6 Nyaw,) and piece durations, at the reference's own sample times: piece i, sample j = 0 .. K sits at the running sums
    s1 (s1 += T_xy / K) and base (base += T_xy); its yaw comes from yaw piece min(int((s1 + base) / T_yaw), Nyaw - 1).  With g = d_safe - c(pos, yaw) and
    om = (0.5 at j = 0 and j = K, else 1) * weight * (T_xy / K) * scale_fx, a sample with g > 0 adds om g^2 to the cost and grad_p = -2 om g grad c.
    Returns a dict: cost; gdCxy (6 Nxy, 2) = per piece sum_j beta0(s1_j) (x) grad_p_j; gdT = the added sum of the time gradients of the xy pieces, sum_j
    om g^2 / K + (grad_p . vel) j / K (the yaw pieces get none); c (Nxy, K + 1) the field at the samples; below (Nxy, K + 1) = g > 0."""
    c_xy = np.asarray(c_xy, dtype=np.float64).reshape(-1, 2)
    c_yaw = np.asarray(c_yaw, dtype=np.float64).reshape(-1)
    Nxy, Nyaw, K = c_xy.shape[0] // 6, c_yaw.shape[0] // 6, int(K)
    step = T_xy / K
    s1 = np.zeros(K + 1)
    for j in range(1, K + 1):
        s1[j] = s1[j - 1] + step
    base = np.zeros(Nxy)
    for i in range(1, Nxy):
        base[i] = base[i - 1] + T_xy
    pw = np.stack([s1 ** 0, s1, s1 * s1, (s1 * s1) * s1, (s1 * s1) * (s1 * s1), ((s1 * s1) * (s1 * s1)) * s1], axis=1)       # (K + 1, 6): beta0
    dpw = np.stack([0 * s1, s1 ** 0, 2.0 * s1, 3.0 * (s1 * s1), 4.0 * ((s1 * s1) * s1), 5.0 * ((s1 * s1) * (s1 * s1))], axis=1)
    cx = c_xy.reshape(Nxy, 6, 2)
    pos, vel = np.zeros((Nxy, K + 1, 2)), np.zeros((Nxy, K + 1, 2))
    for k in range(6):                                          # the device's summation order
        pos += cx[:, None, k, :] * pw[None, :, k, None]
        vel += cx[:, None, k, :] * dpw[None, :, k, None]
    now = s1[None, :] + base[:, None]
    yi = np.clip((now / T_yaw).astype(np.int64), 0, Nyaw - 1)      # (the device's quotient from the stored reciprocal is the rounded quotient as well)
    u = now - yi * T_yaw
    cy = c_yaw.reshape(Nyaw, 6)[yi]
    yaw = np.zeros_like(now)
    up = np.ones_like(now)
    for k in range(6):
        yaw += cy[..., k] * up
        up = up * u
    pose = np.concatenate([pos.reshape(-1, 2), yaw.reshape(-1, 1)], axis=1)
    c, gc = clearance_field(D, geometry, rmax, pose)
    c, gc = c.reshape(Nxy, K + 1), gc.reshape(Nxy, K + 1, 2)
    g = d_safe - c
    below = g > 0.0
    half = np.where((np.arange(K + 1) == 0) | (np.arange(K + 1) == K), 0.5, 1.0)
    om = half * weight * step * scale_fx
    cc = np.where(below, om[None, :] * g * g, 0.0)
    gp = np.where(below[..., None], -(2.0 * om[None, :, None] * g[..., None] * gc), 0.0)
    alpha = (1.0 / K) * np.arange(K + 1)
    gdT = float(np.sum(cc / K + (gp * vel).sum(axis=2) * alpha[None, :]))
    gdC = np.einsum("jk,ijd->ikd", pw, gp).reshape(6 * Nxy, 2)
    return dict(cost=float(cc.sum()), gdCxy=gdC, gdT=gdT, c=c, below=below)


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

    def field(self, pos):
        """uph_clearance_field: the continuous clearance c (n,) in metres and its gradient (n, 2) at pos (n, 3) = x, y, yaw, on the device -- the field the
        clearance term of the objective reads (ALMTrajOpt.set_clearance_term).  See clearance_field for the rule."""
        p = np.ascontiguousarray(np.asarray(pos, dtype=np.float64).reshape(-1, 3))
        n = p.shape[0]
        c, g = np.zeros(n), np.zeros((n, 2))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        _lib.check(self.L.uph_clearance_field(self.h, n, dp(p), dp(c), dp(g)), "uph_clearance_field")
        return c, g

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
