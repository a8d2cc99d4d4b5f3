// libunevenhip.so -- the body layer: the map's occupancy dilated by the vehicle's rectangle, one slice per yaw bin (include/uneven_hip.h uph_body_*,
// DESIGN.md 7u).  body[ix][iy][iw] = 1 iff the rectangle posed at the centre of cell (ix, iy, iw) covers a column that is occupied in occ_r2 or lies
// outside the grid: the configuration-space obstacle of the rectangle on the search's own lattice.  The front-end search (kino_search.hip) reads it where
// it reads occ_r2 by default (uph_kino_set_body_layer).
//
// Reference: UnevenMap::isOccupancy / isOccupancyXY (uneven_map.h:471-500) are the reads the layer stands in for; kino_astar.cpp:178 carries the per-yaw
// read `// occ = uneven_map->isOccupancy(xt);` that the reference tried and left commented out.  The rectangle is the footprint check's (traj_query.hip
// footCentreIn), posed at a cell centre and written in offsets.
//
// Three parts: the stencil (host arithmetic, exported), the kernel (integer only), the layer object with its freshness stamp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uneven_hip.h"
#include "uph_internal.hpp"

using namespace uph;

#define BHIPCHK(call)                                                                              \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            setError(std::string(#call) + ": " + hipGetErrorString(_e));                           \
            return UPH_ERR_HIP;                                                                    \
        }                                                                                          \
    } while (0)

namespace {

constexpr int BODY_MAX_R = 64;              // stencil radius in columns the kernel's LDS tile is sized for (UPH_BODY_MAX_R)
// output columns of one workgroup.  A lane's outputs are a serial chain of stencil rows (a 16-bit load from the L2-resident stencil, then two LDS reads), so the
// tile is small: 8 x 8 columns x 64 yaw bins are 16 outputs per lane, and the hill grid gives 625 workgroups.  At the largest R the tile's counts are
// (8 + 128) x 138 x 2 B = 37.5 KB: four workgroups per compute unit.
constexpr int BODY_TX = 8, BODY_TY = 8;
constexpr int BODY_NT = 256;

// ---- the stencil --------------------------------------------------------------------------------------------------------------------------------------
struct BodyShape { double hl, o, w; };      // footCheckShape's: hl and w inflated by the margin, one rounded add each
BodyShape bodyShape(const double* s3, double margin) {
#pragma clang fp contract(off)
    BodyShape s;
    s.hl = 0.5 * (s3[0] + s3[1]) + margin; s.o = 0.5 * (s3[0] - s3[1]); s.w = s3[2] + margin;
    return s;
}
// whether offset (dx, dy) is covered at heading (c, s): footCentreIn with the pose at a cell centre, every product and sum rounded on its own
bool bodyCovered(int dx, int dy, double res, double c, double s, const BodyShape& b) {
#pragma clang fp contract(off)
    const double qx = (double)dx * res - b.o * c, qy = (double)dy * res - b.o * s;
    return std::fabs(qx * c + qy * s) <= b.hl && std::fabs(qx * (-s) + qy * c) <= b.w;
}
// the yaw axis of a map with these parameters (map_build.hip createMap: uneven_map.cpp:96-110)
void bodyYawAxis(const uph_map_params* mp, double& origin_w, int& nyaw) {
    const double size = 2.0 * 3.14159265358979323846 + 5e-2;
    origin_w = -size / 2.0;
    nyaw = (int)std::ceil(size / mp->yaw_resolution);
}
// admission shared by the exported stencil call and the layer: footAdmit's refusals and the 2^14 column bound through uph_footprint_check_columns,
// then R and its own limit
int bodyAdmit(const std::string& who, const uph_map_params* mp, const double* shape, double margin, int& R) {
#pragma clang fp contract(off)
    if (!(mp->yaw_resolution > 0.0) || !std::isfinite(mp->yaw_resolution)) { setError(who + ": the map's yaw_resolution must be positive and finite"); return UPH_ERR_INVALID; }
    int64_t cols = 0;
    const int r = uph_footprint_check_columns(mp, 1, shape, &margin, &cols);
    if (r != UPH_OK) return r;
    if (cols > ((int64_t)1 << 14)) { setError(who + ": the shape and margin can cover more than 2^14 columns (uph_footprint_check_columns)"); return UPH_ERR_LIMIT; }
    const double reach = std::hypot(std::max(shape[0], shape[1]) + margin, shape[2] + margin) * (1.0 + 0x1p-40);
    const double Rd = std::floor(reach / mp->xy_resolution) + 1.0;
    if (!(Rd <= (double)BODY_MAX_R)) { setError(who + ": the stencil radius exceeds UPH_BODY_MAX_R columns (a long one-sided shape: front or rear far beyond the other)"); return UPH_ERR_LIMIT; }
    R = (int)Rd;
    return UPH_OK;
}
void bodyStencil(const uph_map_params* mp, const BodyShape& b, int R, int nyaw, double origin_w, double* cs, int32_t* lo, int32_t* hi) {
#pragma clang fp contract(off)
    const int W = 2 * R + 1;
    for (int iw = 0; iw < nyaw; iw++) {
        const double psi = origin_w + ((double)iw + 0.5) * mp->yaw_resolution;
        const double c = std::cos(psi), s = std::sin(psi);
        if (cs) { cs[2 * iw] = c; cs[2 * iw + 1] = s; }
        if (!lo && !hi) continue;
        for (int dx = -R; dx <= R; dx++) {
            int l = 1, h = 0;
            for (int dy = -R; dy <= R; dy++) if (bodyCovered(dx, dy, mp->xy_resolution, c, s, b)) { if (l > h) l = dy; h = dy; }
            if (lo) lo[(size_t)iw * W + (dx + R)] = l;
            if (hi) hi[(size_t)iw * W + (dx + R)] = h;
        }
    }
}

// ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------------
// One workgroup per tile of BODY_TX x BODY_TY output columns, all yaw bins.  occ_r2 of the tile and a halo of R columns is staged in LDS as running counts
// along iy of "this column makes a hit" (occupied inside the grid / outside the grid, by `layers`), so that a stencil row lo..hi is the difference of two
// counts.  Outputs of one tile row are consecutive bytes (iy, then iw fastest): a lane forms four of them and writes one aligned dword; the ragged ends
// of a run are byte stores.  Every result is an OR of integer comparisons: the tiling cannot show in it.
struct BodyArgs {
    const char* occ2;           // [nx][ny]
    char* out;                  // [nx][ny][nyaw]
    const signed char* st;      // [nyaw][2R + 1][2]: lo, hi
    int nx, ny, nyaw, R, layers;
    int ox0, ox1, oy0, oy1;     // the outputs written: a half-open rect of columns inside the grid
    int stride;                 // halves per staged row: >= BODY_TY + 2R + 1, an odd number of dwords
};

__global__ __launch_bounds__(BODY_NT) void uph_body_layer_kernel(BodyArgs a) {
    extern __shared__ unsigned short cnt[];
    const int R = a.R, S = a.stride;
    const int tx0 = a.ox0 + (int)blockIdx.x * BODY_TX, ty0 = a.oy0 + (int)blockIdx.y * BODY_TY;
    const int txn = min(BODY_TX, a.ox1 - tx0), tyn = min(BODY_TY, a.oy1 - ty0);
    const int Hd = BODY_TX + 2 * R, Wd = BODY_TY + 2 * R;
    // the predicate of every staged column, consecutive threads on consecutive iy
    for (int t = threadIdx.x; t < Hd * Wd; t += BODY_NT) {
        const int r = t / Wd, j = t - r * Wd;
        const int gx = tx0 - R + r, gy = ty0 - R + j;
        const bool in = gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny;
        bool p;
        if (in) p = (a.layers & UPH_FOOT_OCC_XY) != 0 && a.occ2[(size_t)gx * a.ny + gy] != 0;
        else p = (a.layers & UPH_FOOT_OUTSIDE) != 0;
        cnt[r * S + j + 1] = p ? 1 : 0;
    }
    __syncthreads();
    // running counts per row: cnt[r][j] = hits among the row's first j columns
    for (int r = threadIdx.x; r < Hd; r += BODY_NT) {
        unsigned short* row = cnt + r * S;
        unsigned acc = 0;
        row[0] = 0;
        for (int j = 1; j <= Wd; j++) { acc += row[j]; row[j] = (unsigned short)acc; }
    }
    __syncthreads();
    const int W = 2 * R + 1;
    const unsigned run_len = (unsigned)tyn * (unsigned)a.nyaw;
    const int ndw = (int)((run_len + 3u) / 4u) + 1;          // aligned dwords a run can touch
    for (int item = threadIdx.x; item < txn * ndw; item += BODY_NT) {
        const int rx = item / ndw, k = item - rx * ndw;
        const size_t run0 = ((size_t)(tx0 + rx) * a.ny + ty0) * a.nyaw, run1 = run0 + run_len;
        const size_t b0 = (run0 & ~(size_t)3) + 4 * (size_t)k;
        if (b0 >= run1) continue;
        unsigned word = 0, mask = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const size_t b = b0 + q;
            if (b < run0 || b >= run1) continue;
            const unsigned off = (unsigned)(b - run0);
            const int ly = (int)(off / (unsigned)a.nyaw), iw = (int)(off - (unsigned)ly * (unsigned)a.nyaw);
            const signed char* st = a.st + (size_t)iw * W * 2;
            const unsigned short* base = cnt + (rx + R) * S + (ly + R);
            bool hit = false;
            for (int dx = -R; dx <= R && !hit; dx++) {
                const int l = st[2 * (dx + R)], h = st[2 * (dx + R) + 1];
                if (l <= h) {
                    const unsigned short* row = base + dx * S;
                    hit = row[h + 1] != row[l];
                }
            }
            word |= (hit ? 1u : 0u) << (8 * q);
            mask |= 1u << q;
        }
        if (mask == 15u) *(unsigned*)(a.out + b0) = word;
        else {
#pragma unroll
            for (int q = 0; q < 4; q++) if (mask & (1u << q)) a.out[b0 + q] = (char)((word >> (8 * q)) & 0xffu);
        }
    }
}

int bodyStride(int R) {
    int s = BODY_TY + 2 * R + 1;
    if (s & 1) s++;
    if (((s / 2) & 1) == 0) s += 2;
    return s;
}

}  // namespace

struct uph_body_layer {
    uph_map* map = nullptr;
    int device = 0;
    double shape[3] = {0.0, 0.0, 0.0}, margin = 0.0;
    int layers = 0, R = 0;
    int nx = 0, ny = 0, nyaw = 0;
    size_t ncell = 0;
    char* d_bytes = nullptr;
    signed char* d_st = nullptr;
    unsigned long long version = 0;     // the map's occupancy version the bytes were made from
    bool stamped = false;
    int users = 0;                      // search contexts that name the layer
    int dependants = 0;                 // clearance layers made from the layer
    unsigned long long writes = 0;      // build, update and set count one each: the stamp of a clearance layer
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double last_ms = 0.0;
};

// the kernel over the outputs [x0, x1) x [y0, y1) (inside the grid, not empty), blocking
static int bodyLaunch(uph_body_layer* l, int x0, int x1, int y0, int y1) {
    const char *occ = nullptr, *occ2 = nullptr;
    uphMapOcc(l->map, &occ, &occ2);
    BodyArgs a;
    a.occ2 = occ2; a.out = l->d_bytes; a.st = l->d_st;
    a.nx = l->nx; a.ny = l->ny; a.nyaw = l->nyaw; a.R = l->R; a.layers = l->layers;
    a.ox0 = x0; a.ox1 = x1; a.oy0 = y0; a.oy1 = y1;
    a.stride = bodyStride(l->R);
    const size_t lds = (size_t)(BODY_TX + 2 * l->R) * a.stride * sizeof(unsigned short);
    const dim3 grid((unsigned)((x1 - x0 + BODY_TX - 1) / BODY_TX), (unsigned)((y1 - y0 + BODY_TY - 1) / BODY_TY));
    BHIPCHK(hipEventRecord(l->e0, 0));
    hipLaunchKernelGGL(uph_body_layer_kernel, grid, dim3(BODY_NT), lds, 0, a);
    BHIPCHK(hipGetLastError());
    BHIPCHK(hipEventRecord(l->e1, 0));
    BHIPCHK(hipDeviceSynchronize());
    float ms = 0.f;
    BHIPCHK(hipEventElapsedTime(&ms, l->e0, l->e1));
    l->last_ms = ms;
    return UPH_OK;
}

// versions of the map's occupancy the layer is behind (0: fresh); a layer that was never built is behind by everything
static unsigned long long bodyBehind(const uph_body_layer* l) {
    if (!l->stamped) return ~0ull;
    return uphMapOccVersion(l->map) - l->version;
}

const uph_map* uphBodyLayerMap(const uph_body_layer* l) { return l->map; }
const char* uphBodyLayerBytes(const uph_body_layer* l) { return l->d_bytes; }
bool uphBodyLayerFresh(const uph_body_layer* l) { return bodyBehind(l) == 0; }
void uphBodyLayerUse(uph_body_layer* l, int delta) { l->users += delta; }
int uphBodyLayerDevice(const uph_body_layer* l) { return l->device; }
void uphBodyLayerDims(const uph_body_layer* l, int dims3[3]) { dims3[0] = l->nx; dims3[1] = l->ny; dims3[2] = l->nyaw; }
unsigned long long uphBodyLayerWrites(const uph_body_layer* l) { return l->writes; }
void uphBodyLayerDepend(uph_body_layer* l, int delta) { l->dependants += delta; }

extern "C" {

int uph_body_stencil(const uph_map_params* mp, const double* shape, double margin, int32_t* R, int32_t* nyaw, double* cs, int32_t* lo, int32_t* hi) {
    const std::string who = "uph_body_stencil";
    if (!mp || !shape) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    int r_ = 0;
    const int r = bodyAdmit(who, mp, shape, margin, r_);
    if (r != UPH_OK) return r;
    double ow; int nw;
    bodyYawAxis(mp, ow, nw);
    if (R) *R = r_;
    if (nyaw) *nyaw = nw;
    if (cs || lo || hi) bodyStencil(mp, bodyShape(shape, margin), r_, nw, ow, cs, lo, hi);
    return UPH_OK;
}

int uph_body_layer_margin(const uph_map_params* mp, const double* shape, double* margin) {
#pragma clang fp contract(off)
    const std::string who = "uph_body_layer_margin";
    if (!mp || !shape || !margin) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    if (!(mp->yaw_resolution > 0.0) || !std::isfinite(mp->yaw_resolution)) { setError(who + ": the map's yaw_resolution must be positive and finite"); return UPH_ERR_INVALID; }
    int64_t cols = 0;
    const int r = uph_footprint_check_columns(mp, 1, shape, nullptr, &cols);      // the refusals of the resolution and the shape
    if (r != UPH_OK) return r;
    const double reach = std::hypot(std::max(shape[0], shape[1]), shape[2]);
    *margin = (mp->xy_resolution * std::sqrt(2.0) / 2.0 + 2.0 * reach * std::sin(mp->yaw_resolution / 4.0)) * (1.0 + 0x1p-40);
    return UPH_OK;
}

int uph_body_layer_create(uph_map* m, const double* shape, double margin, int32_t layers, uph_body_layer** out) {
    const std::string who = "uph_body_layer_create";
    if (!m || !shape || !out) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    const GridDev g = uphMapGrid(m);
    if (g.nx_hold != g.nx) { setError(who + ": tile maps carry no body layer (the halo needs rows the tile does not hold)"); return UPH_ERR_INVALID; }
    if (layers != UPH_FOOT_OCC_XY && layers != UPH_FOOT_OUTSIDE && layers != (UPH_FOOT_OCC_XY | UPH_FOOT_OUTSIDE)) {
        setError(who + ": layers must be UPH_FOOT_OCC_XY, UPH_FOOT_OUTSIDE or both (occ_r2 is already the OR of occ over yaw)"); return UPH_ERR_INVALID;
    }
    uph_map_params mp;
    std::memset(&mp, 0, sizeof(mp));
    mp.xy_resolution = g.xy_res; mp.yaw_resolution = g.yaw_res;
    int R = 0;
    int r = bodyAdmit(who, &mp, shape, margin, R);
    if (r != UPH_OK) return r;
    const int W = 2 * R + 1;
    std::vector<int32_t> lo((size_t)g.nyaw * W), hi((size_t)g.nyaw * W);
    bodyStencil(&mp, bodyShape(shape, margin), R, g.nyaw, g.origin[2], nullptr, lo.data(), hi.data());
    std::vector<signed char> st((size_t)g.nyaw * W * 2);
    for (size_t i = 0; i < lo.size(); i++) { st[2 * i] = (signed char)lo[i]; st[2 * i + 1] = (signed char)hi[i]; }
    BHIPCHK(hipSetDevice(uphMapDevice(m)));
    uph_body_layer* l = new uph_body_layer();
    l->map = m; l->device = uphMapDevice(m);
    for (int k = 0; k < 3; k++) l->shape[k] = shape[k];
    l->margin = margin; l->layers = layers; l->R = R;
    l->nx = g.nx; l->ny = g.ny; l->nyaw = g.nyaw;
    l->ncell = (size_t)g.nx * g.ny * g.nyaw;
    if (hipMalloc((void**)&l->d_bytes, l->ncell) != hipSuccess || hipMalloc((void**)&l->d_st, st.size()) != hipSuccess ||
        hipMemcpy(l->d_st, st.data(), st.size(), hipMemcpyHostToDevice) != hipSuccess || hipEventCreate(&l->e0) != hipSuccess || hipEventCreate(&l->e1) != hipSuccess) {
        setError(who + ": allocating the layer failed");
        (void)hipGetLastError();
        uph_body_layer_destroy(l);
        return UPH_ERR_HIP;
    }
    r = uph_body_layer_build(l);
    if (r != UPH_OK) { uph_body_layer_destroy(l); return r; }
    *out = l;
    return UPH_OK;
}

int uph_body_layer_build(uph_body_layer* l) {
    if (!l) { setError("uph_body_layer_build: bad arguments"); return UPH_ERR_INVALID; }
    BHIPCHK(hipSetDevice(l->device));
    const unsigned long long v = uphMapOccVersion(l->map);
    l->stamped = false;
    l->writes++;
    const int r = bodyLaunch(l, 0, l->nx, 0, l->ny);
    if (r != UPH_OK) return r;
    l->version = v; l->stamped = true;
    return UPH_OK;
}

int uph_body_layer_update(uph_body_layer* l, const int32_t rect[4]) {
    const std::string who = "uph_body_layer_update";
    if (!l || !rect) { setError(who + ": bad arguments"); return UPH_ERR_INVALID; }
    if (rect[0] < 0 || rect[1] > l->nx || rect[0] > rect[1] || rect[2] < 0 || rect[3] > l->ny || rect[2] > rect[3]) {
        setError(who + ": rect = (x0, x1, y0, y1) must be half-open, ordered and inside the grid"); return UPH_ERR_INVALID;
    }
    if (bodyBehind(l) > 1) { setError(who + ": the layer is more than one occupancy version behind the map: rebuild (uph_body_layer_build)"); return UPH_ERR_INVALID; }
    BHIPCHK(hipSetDevice(l->device));
    const unsigned long long v = uphMapOccVersion(l->map);
    l->writes++;
    if (rect[0] < rect[1] && rect[2] < rect[3]) {
        const int x0 = std::max(0, rect[0] - l->R), x1 = std::min(l->nx, rect[1] + l->R), y0 = std::max(0, rect[2] - l->R), y1 = std::min(l->ny, rect[3] + l->R);
        l->stamped = false;
        const int r = bodyLaunch(l, x0, x1, y0, y1);
        if (r != UPH_OK) return r;
    } else l->last_ms = 0.0;
    l->version = v; l->stamped = true;
    return UPH_OK;
}

int uph_body_layer_get(uph_body_layer* l, char* bytes) {
    if (!l || !bytes) { setError("uph_body_layer_get: bad arguments"); return UPH_ERR_INVALID; }
    BHIPCHK(hipSetDevice(l->device));
    BHIPCHK(hipMemcpy(bytes, l->d_bytes, l->ncell, hipMemcpyDeviceToHost));
    return UPH_OK;
}

int uph_body_layer_set(uph_body_layer* l, const char* bytes) {
    if (!l || !bytes) { setError("uph_body_layer_set: bad arguments"); return UPH_ERR_INVALID; }
    // the search takes a byte for occupied when it is 1 (isOccupancy's `== 1`, as for occ): another value would read as free there and as occupied elsewhere
    for (size_t i = 0; i < l->ncell; i++)
        if (bytes[i] != 0 && bytes[i] != 1) { setError("uph_body_layer_set: layer bytes must be 0 (free) or 1 (occupied)"); return UPH_ERR_INVALID; }
    BHIPCHK(hipSetDevice(l->device));
    l->stamped = false;
    l->writes++;
    BHIPCHK(hipMemcpy(l->d_bytes, bytes, l->ncell, hipMemcpyHostToDevice));
    l->version = uphMapOccVersion(l->map); l->stamped = true;
    return UPH_OK;
}

int uph_body_layer_info(const uph_body_layer* l, double* shape3, double* margin, int32_t* layers, int32_t* R, int32_t* dims3, int32_t* behind) {
    if (!l) { setError("uph_body_layer_info: bad arguments"); return UPH_ERR_INVALID; }
    if (shape3) for (int k = 0; k < 3; k++) shape3[k] = l->shape[k];
    if (margin) *margin = l->margin;
    if (layers) *layers = l->layers;
    if (R) *R = l->R;
    if (dims3) { dims3[0] = l->nx; dims3[1] = l->ny; dims3[2] = l->nyaw; }
    if (behind) { const unsigned long long b = bodyBehind(l); *behind = b > 0x7fffffffull ? 0x7fffffff : (int32_t)b; }
    return UPH_OK;
}

int uph_body_layer_kernel_ms(const uph_body_layer* l, double* kernel_ms) {
    if (!l || !kernel_ms) { setError("uph_body_layer_kernel_ms: bad arguments"); return UPH_ERR_INVALID; }
    *kernel_ms = l->last_ms;
    return UPH_OK;
}

int uph_body_layer_writes(const uph_body_layer* l, uint64_t* writes) {
    if (!l || !writes) { setError("uph_body_layer_writes: bad arguments"); return UPH_ERR_INVALID; }
    *writes = l->writes;
    return UPH_OK;
}

int uph_body_layer_destroy(uph_body_layer* l) {
    if (!l) return UPH_OK;
    if (l->users > 0) { setError("uph_body_layer_destroy: a search context still names the layer (uph_kino_set_body_layer(k, NULL) or destroy it first)"); return UPH_ERR_INVALID; }
    if (l->dependants > 0) { setError("uph_body_layer_destroy: a clearance layer is still made from the layer (uph_clearance_destroy it first)"); return UPH_ERR_INVALID; }
    hipSetDevice(l->device);
    hipFree(l->d_bytes); hipFree(l->d_st);
    if (l->e0) hipEventDestroy(l->e0);
    if (l->e1) hipEventDestroy(l->e1);
    delete l;
    return UPH_OK;
}

}  // extern "C"
