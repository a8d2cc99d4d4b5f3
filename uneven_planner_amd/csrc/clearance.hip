// libunevenhip.so -- the clearance layer: the exact, truncated, squared Euclidean distance transform of a body layer, one field per yaw slice
// (include/uneven_hip.h uph_clearance_*).  D[ix][iy][iw] = min dx^2 + dy^2 over the features of slice iw within rmax cells, UPH_CLEAR_FAR when
// there is none: how much room the cell has, where the body layer (body_occ.hip) says only whether it has any.  uph_clearance_check_batch (traj_query.hip)
// reads it along resident trajectories.
//
// Reference: there is none.  UnevenMap keeps occupancy bits only (uneven_map.h:471-500) and the optimiser has no obstacle term; this is the field such a term
// would read.
//
// Two parts: the two kernels of the separable evaluation (integers only), the layer object with its freshness stamp towards the body layer.  And the
// continuous field made of the values (clearance_dev.hpp), which the clearance term of the solve kernel reads: uph_clearance_field evaluates it at poses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/uneven_hip.h"
#include "clearance_dev.hpp"
#include "uph_internal.hpp"

using namespace uph;

#define CHIPCHK(call)                                                                              \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            setError(std::string(#call) + ": " + hipGetErrorString(_e));                           \
            return UPH_ERR_HIP;                                                                    \
        }                                                                                          \
    } while (0)

namespace {

constexpr int CLEAR_NT = 256;
constexpr int CLEAR_NONE = 255;             // g: no feature of the row within rmax (why UPH_CLEAR_MAX_R is 254)
constexpr int CLEAR_SEG_MIN = 16;           // columns of one lane's scan in pass 1, at least

// ---- the kernels --------------------------------------------------------------------------------------------------------------------------------------
// The layer's bytes are laid out [ix][iy][iw], iw fastest: a row ix is one run of ny * nyaw bytes, and so are the rows of g and D.  Both kernels put consecutive
// lanes on consecutive bytes of such a run, so that the byte loads of a wave are one or two lines and the 16-bit stores of D are consecutive; nyaw need not
// be a multiple of anything.
struct ClearArgs {
    const char* body;           // [nx][ny][nyaw], bytes 0 / 1
    unsigned char* g;           // [nx][ny][nyaw]: |dy| to the nearest feature of the row within rmax, CLEAR_NONE: none
    unsigned short* D;          // [nx][ny][nyaw]
    int nx, ny, nyaw, rmax, polarity;
    int x0, x1, y0, y1;         // half-open, inside the grid, not empty: the entries of g (pass 1) or of D (pass 2) that are written
    int seg, nseg;              // pass 1: columns of one lane's scan, and how many of them cover [y0, y1)
};

// Pass 1, along iy: a lane owns (row, segment of `seg` columns, yaw bin) and scans it twice with a saturating count of the columns since the last feature --
// forward from rmax columns before the segment, backward from rmax columns behind it, so that every feature within rmax of a column of the segment is met.
// The forward scan stores its count; the backward scan reads it back (the lane's own store), takes the smaller and stores CLEAR_NONE for one beyond rmax.
__global__ __launch_bounds__(CLEAR_NT) void uph_clearance_rows_kernel(ClearArgs a) {
    const size_t per_row = (size_t)a.nseg * (size_t)a.nyaw;
    const size_t t = (size_t)blockIdx.x * CLEAR_NT + threadIdx.x;
    if (t >= (size_t)(a.x1 - a.x0) * per_row) return;
    const int r = (int)(t / per_row);
    const unsigned rem = (unsigned)(t - (size_t)r * per_row);
    const int s = (int)(rem / (unsigned)a.nyaw), iw = (int)(rem - (unsigned)s * (unsigned)a.nyaw);
    const int ya = a.y0 + s * a.seg, yb = min(a.y1, ya + a.seg);
    const size_t row = (size_t)(a.x0 + r) * a.ny;
    const char feature = a.polarity == UPH_CLEAR_TO_FREE ? 0 : 1;
    int cnt = CLEAR_NONE;
    for (int y = max(0, ya - a.rmax); y < yb; y++) {
        const size_t k = (row + y) * a.nyaw + iw;
        cnt = a.body[k] == feature ? 0 : min(cnt + 1, CLEAR_NONE);
        if (y >= ya) a.g[k] = (unsigned char)cnt;
    }
    cnt = CLEAR_NONE;
    for (int y = min(a.ny, yb + a.rmax) - 1; y >= ya; y--) {
        const size_t k = (row + y) * a.nyaw + iw;
        cnt = a.body[k] == feature ? 0 : min(cnt + 1, CLEAR_NONE);
        if (y < yb) {
            const int v = min(cnt, (int)a.g[k]);
            a.g[k] = (unsigned char)(v > a.rmax ? CLEAR_NONE : v);
        }
    }
}

// Pass 2, along ix: a lane owns one output and walks dx outward from 0 over g of the rows ix - dx and ix + dx, keeping the smallest dx^2 + g^2; it stops once
// dx^2 reaches the running min, which starts at rmax^2 + 1 -- so dx never passes rmax and a min above rmax^2 never replaces the start.
__global__ __launch_bounds__(CLEAR_NT) void uph_clearance_cols_kernel(ClearArgs a) {
    const unsigned run = (unsigned)(a.y1 - a.y0) * (unsigned)a.nyaw, bpr = (run + CLEAR_NT - 1) / CLEAR_NT;
    const unsigned r = blockIdx.x / bpr, k = (blockIdx.x - r * bpr) * CLEAR_NT + threadIdx.x;
    if (k >= run) return;
    const int ix = a.x0 + (int)r;
    const size_t stride = (size_t)a.ny * a.nyaw, col = (size_t)a.y0 * a.nyaw + k;
    const int lim = a.rmax * a.rmax + 1;
    int best = lim;
    for (int dx = 0; dx * dx < best; dx++) {
        const int lo = ix - dx, hi = ix + dx;
        if (lo < 0 && hi >= a.nx) break;
        if (lo >= 0) {
            const int g = a.g[(size_t)lo * stride + col];
            if (g != CLEAR_NONE) best = min(best, dx * dx + g * g);
        }
        if (dx > 0 && hi < a.nx) {
            const int g = a.g[(size_t)hi * stride + col];
            if (g != CLEAR_NONE) best = min(best, dx * dx + g * g);
        }
    }
    a.D[(size_t)ix * stride + col] = (unsigned short)(best < lim ? best : UPH_CLEAR_FAR);
}

// the continuous field at n poses (clearance_dev.hpp clearanceField): one lane per pose, the yaw normalised as the solve kernel normalises it (normSO2)
__global__ __launch_bounds__(CLEAR_NT) void uph_clearance_field_kernel(ClearGeom g, const unsigned short* __restrict__ D, const double* __restrict__ pos, int n,
                                                                       double* __restrict__ value, double* __restrict__ grad) {
    const int i = blockIdx.x * CLEAR_NT + threadIdx.x;
    if (i >= n) return;
    double c, gx, gy;
    clearanceField(g, D, pos[3 * (size_t)i], pos[3 * (size_t)i + 1], normSO2(pos[3 * (size_t)i + 2]), c, gx, gy);
    value[i] = c;
    grad[2 * (size_t)i] = gx; grad[2 * (size_t)i + 1] = gy;
}

// the rect grown by r and clipped (the rect is ordered, inside the grid and not empty)
void growRect(int nx, int ny, const int32_t rect[4], int r, int32_t out[4]) {
    out[0] = std::max(0, rect[0] - r); out[1] = (int32_t)std::min<int64_t>(nx, (int64_t)rect[1] + r);
    out[2] = std::max(0, rect[2] - r); out[3] = (int32_t)std::min<int64_t>(ny, (int64_t)rect[3] + r);
}
bool rectBad(int nx, int ny, const int32_t rect[4]) {
    return rect[0] < 0 || rect[1] > nx || rect[0] > rect[1] || rect[2] < 0 || rect[3] > ny || rect[2] > rect[3];
}

}  // namespace

struct uph_clearance {
    uph_body_layer* body = nullptr;
    int device = 0;
    int rmax = 0, polarity = 0;
    int nx = 0, ny = 0, nyaw = 0;
    size_t ncell = 0;
    unsigned char* d_g = nullptr;
    unsigned short* d_D = nullptr;
    unsigned long long stamp = 0;       // the body layer's write count the values were made from
    bool stamped = false;
    int users = 0;                      // optimiser contexts that name the layer in a clearance term
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double last_ms = 0.0;
};

// both passes, blocking: g of rows [rect[0], rect[1]) and the columns of the rect grown by rmax, then D inside the rect grown by rmax (the rect is ordered, inside
// the grid and not empty; the whole grid makes a build)
static int clearLaunch(uph_clearance* l, const int32_t rect[4]) {
    int32_t grown[4];
    growRect(l->nx, l->ny, rect, l->rmax, grown);
    ClearArgs a;
    a.body = uphBodyLayerBytes(l->body); a.g = l->d_g; a.D = l->d_D;
    a.nx = l->nx; a.ny = l->ny; a.nyaw = l->nyaw; a.rmax = l->rmax; a.polarity = l->polarity;
    a.x0 = rect[0]; a.x1 = rect[1]; a.y0 = grown[2]; a.y1 = grown[3];
    a.seg = std::max(CLEAR_SEG_MIN, l->rmax);
    a.nseg = (a.y1 - a.y0 + a.seg - 1) / a.seg;
    const size_t lanes1 = (size_t)(a.x1 - a.x0) * a.nseg * l->nyaw;
    ClearArgs b = a;
    b.x0 = grown[0]; b.x1 = grown[1]; b.seg = b.nseg = 0;
    const size_t run = (size_t)(b.y1 - b.y0) * l->nyaw;
    const size_t blocks1 = (lanes1 + CLEAR_NT - 1) / CLEAR_NT, blocks2 = (size_t)(b.x1 - b.x0) * ((run + CLEAR_NT - 1) / CLEAR_NT);
    if (blocks1 > 0x7fffffffull || blocks2 > 0x7fffffffull) { setError("uph_clearance: the layer is too large for one launch"); return UPH_ERR_LIMIT; }
    CHIPCHK(hipEventRecord(l->e0, 0));
    hipLaunchKernelGGL(uph_clearance_rows_kernel, dim3((unsigned)blocks1), dim3(CLEAR_NT), 0, 0, a);
    CHIPCHK(hipGetLastError());
    hipLaunchKernelGGL(uph_clearance_cols_kernel, dim3((unsigned)blocks2), dim3(CLEAR_NT), 0, 0, b);
    CHIPCHK(hipGetLastError());
    CHIPCHK(hipEventRecord(l->e1, 0));
    CHIPCHK(hipDeviceSynchronize());
    float ms = 0.f;
    CHIPCHK(hipEventElapsedTime(&ms, l->e0, l->e1));
    l->last_ms = ms;
    return UPH_OK;
}

// writes of the body layer the values are behind (0: fresh); a layer that was never built is behind by everything
static unsigned long long clearBehind(const uph_clearance* l) {
    if (!l->stamped) return ~0ull;
    return uphBodyLayerWrites(l->body) - l->stamp;
}

const uph_body_layer* uphClearanceBody(const uph_clearance* l) { return l->body; }
const unsigned short* uphClearanceValues(const uph_clearance* l) { return l->d_D; }
bool uphClearanceFresh(const uph_clearance* l) { return clearBehind(l) == 0; }
void uphClearanceUse(uph_clearance* l, int delta) { l->users += delta; }

extern "C" {

int uph_clearance_grow_rect(const int32_t dims2[2], const int32_t rect[4], int32_t r, int32_t out[4]) {
    const std::string who = "uph_clearance_grow_rect";
    if (!dims2 || !rect || !out) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    if (dims2[0] <= 0 || dims2[1] <= 0 || r < 0) { setError(who + ": the dimensions must be positive and r must not be negative"); return UPH_ERR_INVALID; }
    if (rectBad(dims2[0], dims2[1], rect)) { setError(who + ": rect = (x0, x1, y0, y1) must be half-open, ordered and inside the grid"); return UPH_ERR_INVALID; }
    int32_t g[4] = {rect[0], rect[1], rect[2], rect[3]};
    if (rect[0] < rect[1] && rect[2] < rect[3]) growRect(dims2[0], dims2[1], rect, r, g);
    for (int k = 0; k < 4; k++) out[k] = g[k];
    return UPH_OK;
}

int uph_clearance_create(uph_body_layer* body, int32_t rmax, int32_t polarity, uph_clearance** out) {
    const std::string who = "uph_clearance_create";
    if (!body || !out) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    if (rmax < 1 || rmax > UPH_CLEAR_MAX_R) { setError(who + ": rmax must lie in 1 .. UPH_CLEAR_MAX_R (254) cells"); return UPH_ERR_INVALID; }
    if (polarity != UPH_CLEAR_TO_OCCUPIED && polarity != UPH_CLEAR_TO_FREE) { setError(who + ": polarity must be UPH_CLEAR_TO_OCCUPIED or UPH_CLEAR_TO_FREE"); return UPH_ERR_INVALID; }
    int dims[3];
    uphBodyLayerDims(body, dims);
    if ((size_t)dims[1] * (size_t)dims[2] > 0x7fffffffull) { setError(who + ": a row of the layer (ny * nyaw) exceeds 2^31 - 1 bytes"); return UPH_ERR_LIMIT; }
    CHIPCHK(hipSetDevice(uphBodyLayerDevice(body)));
    uph_clearance* l = new uph_clearance();
    l->body = body; l->device = uphBodyLayerDevice(body);
    l->rmax = rmax; l->polarity = polarity;
    l->nx = dims[0]; l->ny = dims[1]; l->nyaw = dims[2];
    l->ncell = (size_t)dims[0] * dims[1] * dims[2];
    uphBodyLayerDepend(body, 1);
    if (hipMalloc((void**)&l->d_g, l->ncell) != hipSuccess || hipMalloc((void**)&l->d_D, 2 * l->ncell) != hipSuccess || hipEventCreate(&l->e0) != hipSuccess ||
        hipEventCreate(&l->e1) != hipSuccess) {
        setError(who + ": allocating the layer failed");
        (void)hipGetLastError();
        uph_clearance_destroy(l);
        return UPH_ERR_HIP;
    }
    const int r = uph_clearance_build(l);
    if (r != UPH_OK) { uph_clearance_destroy(l); return r; }
    *out = l;
    return UPH_OK;
}

int uph_clearance_build(uph_clearance* l) {
    if (!l) { setError("uph_clearance_build: bad arguments"); return UPH_ERR_INVALID; }
    CHIPCHK(hipSetDevice(l->device));
    const unsigned long long w = uphBodyLayerWrites(l->body);
    l->stamped = false;
    const int32_t all[4] = {0, l->nx, 0, l->ny};
    const int r = clearLaunch(l, all);
    if (r != UPH_OK) return r;
    l->stamp = w; l->stamped = true;
    return UPH_OK;
}

int uph_clearance_update(uph_clearance* l, const int32_t rect[4]) {
    const std::string who = "uph_clearance_update";
    if (!l || !rect) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    if (rectBad(l->nx, l->ny, rect)) { setError(who + ": rect = (x0, x1, y0, y1) must be half-open, ordered and inside the grid"); return UPH_ERR_INVALID; }
    if (clearBehind(l) > 1) { setError(who + ": the layer is more than one write behind its body layer: rebuild (uph_clearance_build)"); return UPH_ERR_INVALID; }
    CHIPCHK(hipSetDevice(l->device));
    const unsigned long long w = uphBodyLayerWrites(l->body);
    if (rect[0] < rect[1] && rect[2] < rect[3]) {
        l->stamped = false;
        const int r = clearLaunch(l, rect);
        if (r != UPH_OK) return r;
    } else l->last_ms = 0.0;
    l->stamp = w; l->stamped = true;
    return UPH_OK;
}

int uph_clearance_get(uph_clearance* l, uint16_t* d) {
    if (!l || !d) { setError("uph_clearance_get: bad arguments"); return UPH_ERR_INVALID; }
    CHIPCHK(hipSetDevice(l->device));
    CHIPCHK(hipMemcpy(d, l->d_D, 2 * l->ncell, hipMemcpyDeviceToHost));
    return UPH_OK;
}

int uph_clearance_info(const uph_clearance* l, int32_t* rmax, int32_t* polarity, int32_t* dims3, int32_t* behind) {
    if (!l) { setError("uph_clearance_info: bad arguments"); return UPH_ERR_INVALID; }
    if (rmax) *rmax = l->rmax;
    if (polarity) *polarity = l->polarity;
    if (dims3) { dims3[0] = l->nx; dims3[1] = l->ny; dims3[2] = l->nyaw; }
    if (behind) { const unsigned long long b = clearBehind(l); *behind = b > 0x7fffffffull ? 0x7fffffff : (int32_t)b; }
    return UPH_OK;
}

int uph_clearance_kernel_ms(const uph_clearance* l, double* kernel_ms) {
    if (!l || !kernel_ms) { setError("uph_clearance_kernel_ms: bad arguments"); return UPH_ERR_INVALID; }
    *kernel_ms = l->last_ms;
    return UPH_OK;
}

int uph_clearance_field(uph_clearance* l, int32_t n, const double* pos, double* value, double* grad) {
    const std::string who = "uph_clearance_field";
    if (!l || n < 0 || (n > 0 && (!pos || !value || !grad))) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    if (l->polarity != UPH_CLEAR_TO_OCCUPIED) { setError(who + ": the field is defined for a layer of polarity UPH_CLEAR_TO_OCCUPIED"); return UPH_ERR_INVALID; }
    if (l->ncell > 0x7fffffffull) { setError(who + ": the layer has more than 2^31 - 1 entries (the field addresses it with 32-bit offsets)"); return UPH_ERR_LIMIT; }
    if (n == 0) return UPH_OK;
    CHIPCHK(hipSetDevice(l->device));
    const ClearGeom g = clearGeom(uphMapGrid(uphBodyLayerMap(l->body)), l->rmax);
    UphDevTmp dp, dv, dg;
    if (hipMalloc(&dp.p, 24 * (size_t)n) != hipSuccess || hipMalloc(&dv.p, 8 * (size_t)n) != hipSuccess || hipMalloc(&dg.p, 16 * (size_t)n) != hipSuccess) {
        setError(who + ": allocating the pose buffers failed");
        (void)hipGetLastError();
        return UPH_ERR_HIP;
    }
    CHIPCHK(hipMemcpy(dp.p, pos, 24 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(uph_clearance_field_kernel, dim3((unsigned)(((size_t)n + CLEAR_NT - 1) / CLEAR_NT)), dim3(CLEAR_NT), 0, 0, g, l->d_D, dp.as<double>(), (int)n,
                       dv.as<double>(), dg.as<double>());
    CHIPCHK(hipGetLastError());
    CHIPCHK(hipDeviceSynchronize());
    CHIPCHK(hipMemcpy(value, dv.p, 8 * (size_t)n, hipMemcpyDeviceToHost));
    CHIPCHK(hipMemcpy(grad, dg.p, 16 * (size_t)n, hipMemcpyDeviceToHost));
    return UPH_OK;
}

int uph_clearance_destroy(uph_clearance* l) {
    if (!l) return UPH_OK;
    if (l->users > 0) { setError("uph_clearance_destroy: a context still names the layer in its clearance term (uph_ctx_set_clearance_term(c, NULL, 0, 0) or destroy it first)"); return UPH_ERR_INVALID; }
    hipSetDevice(l->device);
    hipFree(l->d_g); hipFree(l->d_D);
    if (l->e0) hipEventDestroy(l->e0);
    if (l->e1) hipEventDestroy(l->e1);
    uphBodyLayerDepend(l->body, -1);
    delete l;
    return UPH_OK;
}

}  // extern "C"
