// libunevenhip.so -- the fleet: a long-lived context whose resident batch is a fixed number of SLOTS that solved trajectories of other contexts are adopted into
// (include/uneven_hip.h uph_fleet_*).  A slot owns 12 cap_xy doubles of the fleet's c_xy array and 6 cap_yaw doubles of its c_yaw array, so replacing the
// trajectory of a slot by one of any admissible piece counts moves nothing else and cannot run out of space.  Every query on resident trajectories
// (traj_query.hip) reads a fleet as it reads any batch: TrajDesc / TrajState rows, coefficients, the per-slot frame, rejected[] (here: the slot is EMPTY).
// The adoption is one kernel launch on the device; no coefficient crosses the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uneven_hip.h"
#include "uph_ctx.hpp"

static_assert(sizeof(TrajDesc) + sizeof(TrajState) == UPH_FLEET_SLOT_ROW_BYTES, "the per-slot figure include/uneven_hip.h documents");
static_assert(sizeof(TrajDesc) % 8 == 0 && sizeof(TrajState) % 8 == 0, "the rows are copied as 8-byte words");

// ------------------------------------------------------------------------------------------------ device side
struct AdoptRec {               // one adoption of a launch (formed on the host); every offset counts doubles and is even: the coefficients move as 16-byte words
    int64_t src_cxy, src_cyaw;  // the source trajectory's offsets into its context's c_xy / c_yaw
    int64_t dst_cxy, dst_cyaw;  // the slot's: slot * 12 cap_xy, slot * 6 cap_yaw
    int32_t src_b, dst_b;       // the rows: trajectory of the source, slot of the fleet
    int32_t w_xy, w_yaw;        // 16-byte words to copy: 6 Nxy, 3 Nyaw
};
struct AdoptArgs {
    const TrajDesc* sdesc;
    const TrajState* sstate;
    const double* scxy;
    const double* scyaw;
    TrajDesc* ddesc;
    TrajState* dstate;
    double* dcxy;
    double* dcyaw;
    const AdoptRec* recs;
};
constexpr int ADOPT_NT = 256;

// One workgroup per adopted trajectory.  The record is indexed by blockIdx only (scalar loads); lanes stride over the 6 Nxy + 3 Nyaw 16-byte words of the
// coefficients; lane 0 copies the two rows and then rewrites what of the descriptor names the SOURCE's packed arrays: the coefficient offsets become the slot's, and
// the offsets into arrays a fleet does not have (x, samples, history) and the operator indices become 0 / -1.  No LDS, no scratch.
__global__ __launch_bounds__(ADOPT_NT) void uph_fleet_adopt_kernel(AdoptArgs a) {
    const AdoptRec r = a.recs[blockIdx.x];
    const double2* sx = reinterpret_cast<const double2*>(a.scxy + r.src_cxy);
    const double2* sy = reinterpret_cast<const double2*>(a.scyaw + r.src_cyaw);
    double2* dx = reinterpret_cast<double2*>(a.dcxy + r.dst_cxy);
    double2* dy = reinterpret_cast<double2*>(a.dcyaw + r.dst_cyaw);
    for (int i = (int)threadIdx.x; i < r.w_xy; i += ADOPT_NT) dx[i] = sx[i];
    for (int i = (int)threadIdx.x; i < r.w_yaw; i += ADOPT_NT) dy[i] = sy[i];
    if (threadIdx.x != 0) return;
    const unsigned long long* sd = reinterpret_cast<const unsigned long long*>(a.sdesc + r.src_b);
    unsigned long long* dd = reinterpret_cast<unsigned long long*>(a.ddesc + r.dst_b);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(TrajDesc) / 8); i++) dd[i] = sd[i];
    const unsigned long long* ss = reinterpret_cast<const unsigned long long*>(a.sstate + r.src_b);
    unsigned long long* ds = reinterpret_cast<unsigned long long*>(a.dstate + r.dst_b);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(TrajState) / 8); i++) ds[i] = ss[i];
    TrajDesc& t = a.ddesc[r.dst_b];
    t.op_xy = -1; t.op_yaw = -1;
    t.off_x = 0; t.off_s = 0; t.off_hist = 0;
    t.off_cxy = r.dst_cxy; t.off_cyaw = r.dst_cyaw;
}

// ------------------------------------------------------------------------------------------------ host side
constexpr int FLEET_EMPTY = UPH_ERR_INVALID;       // rejected[] of an empty slot (any value but 0)

static bool sameGeometry(const GridDev& a, const GridDev& b) {     // what syncGridMem compares: the geometry the frames were formed from
    return a.nx == b.nx && a.ny == b.ny && a.nyaw == b.nyaw && a.xy_res == b.xy_res && a.origin[0] == b.origin[0] && a.origin[1] == b.origin[1] && a.lo[0] == b.lo[0] &&
           a.hi[0] == b.hi[0] && a.lo[1] == b.lo[1] && a.hi[1] == b.hi[1];
}
static bool framedMap(const GridDev& g) {           // admitBatch's FRAME_EXTENT rule
    return std::max(std::max(std::fabs(g.minb[0]), std::fabs(g.maxb[0])), std::max(std::fabs(g.minb[1]), std::fabs(g.maxb[1]))) > FRAME_EXTENT;
}
// the frame of an empty slot: the map's corner (no query reads it; its descriptor is formed like any other)
static TrajFrame cornerFrame(const GridDev& g) {
    TrajFrame f;
    for (int d = 0; d < 2; d++) { f.ioff[d] = 0; f.shift[d] = g.origin[d]; f.fo[d] = 0.0; f.lo[d] = g.lo[d] - f.shift[d]; f.hi[d] = g.hi[d] - f.shift[d]; }
    return f;
}
static void emptySlot(uph_ctx* f, int s, const GridDev& g) {
    std::memset(&f->desc[(size_t)s], 0, sizeof(TrajDesc));
    std::memset(&f->state_host[(size_t)s], 0, sizeof(TrajState));
    f->rejected[(size_t)s] = FLEET_EMPTY;
    f->fleet_t0[(size_t)s] = 0.0;
    for (int k = 0; k < 3; k++) f->end_pose[(size_t)3 * s + k] = 0.0;
    for (int k = 0; k < 9; k++) f->end_bnd[(size_t)9 * s + k] = 0.0;
    if (!f->frames.empty()) f->frames[(size_t)s] = cornerFrame(g);
}
static void countEmpty(uph_ctx* f) {
    f->n_rejected = 0;
    for (int r : f->rejected) f->n_rejected += r ? 1 : 0;
}
static int needFleet(const uph_ctx* f, const char* who) {
    if (!f) { setError(std::string(who) + ": bad arguments (null fleet)"); return UPH_ERR_INVALID; }
    if (!f->is_fleet) { setError(std::string(who) + ": the context is not a fleet (uph_fleet_create makes one)"); return UPH_ERR_INVALID; }
    return UPH_OK;
}
static int fleetShape(int32_t slots, int32_t cap_xy, int32_t cap_yaw, const char* who) {
    if (slots < 1 || cap_xy < 1 || cap_xy > UPH_MAX_PIECE_XY || cap_yaw < 1 || cap_yaw > UPH_MAX_PIECE_YAW) {
        setError(std::string(who) + ": slots >= 1, 1 <= cap_xy <= UPH_MAX_PIECE_XY and 1 <= cap_yaw <= UPH_MAX_PIECE_YAW"); return UPH_ERR_INVALID;
    }
    return UPH_OK;
}
// exactly `bytes` of zeroed device memory (no slack: uph_fleet_bytes is what a fleet takes)
static int exactBuf(DevBuf& b, size_t bytes) {
    b.release();
    if (hipMalloc(&b.p, bytes) != hipSuccess) { b.p = nullptr; setError("uph_fleet_create: hipMalloc failed"); return UPH_ERR_HIP; }
    b.cap = bytes;
    if (hipMemset(b.p, 0, bytes) != hipSuccess) { setError("uph_fleet_create: hipMemset failed"); return UPH_ERR_HIP; }
    return UPH_OK;
}

extern "C" {

int uph_fleet_bytes(int32_t slots, int32_t cap_xy, int32_t cap_yaw, int64_t* bytes) {
    if (!bytes) { setError("uph_fleet_bytes: bad arguments"); return UPH_ERR_INVALID; }
    const int r = fleetShape(slots, cap_xy, cap_yaw, "uph_fleet_bytes");
    if (r != UPH_OK) return r;
    *bytes = (int64_t)slots * (8 * (12 * (int64_t)cap_xy + 6 * (int64_t)cap_yaw) + UPH_FLEET_SLOT_ROW_BYTES);
    return UPH_OK;
}

int uph_fleet_create(uph_map* m, const uph_opt_params* p, int32_t slots, int32_t cap_xy, int32_t cap_yaw, uph_ctx** out) {
    if (!m || !p || !out) { setError("uph_fleet_create: null argument"); return UPH_ERR_INVALID; }
    int r = fleetShape(slots, cap_xy, cap_yaw, "uph_fleet_create");
    if (r != UPH_OK) return r;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { setError("uph_fleet_create: no HIP device visible"); return UPH_ERR_NO_DEVICE; }
    uph_ctx* f = nullptr;
    r = uph_ctx_create(m, p, &f);
    if (r != UPH_OK) return r;
    const GridDev tg = uphMapGrid(m);
    const size_t S = (size_t)slots;
    f->is_fleet = true; f->fleet_cap_xy = cap_xy; f->fleet_cap_yaw = cap_yaw;
    f->sum_cxy = (int64_t)S * 12 * cap_xy; f->sum_cyaw = (int64_t)S * 6 * cap_yaw;
    if ((r = exactBuf(f->d_cxy, 8 * (size_t)f->sum_cxy)) != UPH_OK || (r = exactBuf(f->d_cyaw, 8 * (size_t)f->sum_cyaw)) != UPH_OK ||
        (r = exactBuf(f->d_desc, sizeof(TrajDesc) * S)) != UPH_OK || (r = exactBuf(f->d_state, sizeof(TrajState) * S)) != UPH_OK) {
        uph_ctx_destroy(f);
        return r;
    }
    f->desc.assign(S, TrajDesc());
    f->state_host.assign(S, TrajState());
    f->rejected.assign(S, FLEET_EMPTY);
    f->fleet_t0.assign(S, 0.0);
    f->end_pose.assign(3 * S, 0.0);
    f->end_bnd.assign(9 * S, 0.0);
    f->frames.clear();
    f->frames_grid = tg;
    if (framedMap(tg)) f->frames.assign(S, cornerFrame(tg));
    for (int s = 0; s < slots; s++) emptySlot(f, s, tg);
    f->n_rejected = slots;
    f->framed_valid = false;
    f->B = slots;
    f->traj_resident = true;        // the slots ARE the resident batch: an empty fleet answers every query with "empty slot", the rollout with no rows
    *out = f;
    return UPH_OK;
}

int uph_fleet_adopt(uph_ctx* fleet, uph_ctx* src, int32_t n, const int32_t* src_traj, const int32_t* slot, const double* t0) {
    const char* who = "uph_fleet_adopt";
    int r = needFleet(fleet, who);
    if (r != UPH_OK) return r;
    if (!src || n <= 0 || !src_traj || !slot) { setError("uph_fleet_adopt: bad arguments (null pointer or n <= 0)"); return UPH_ERR_INVALID; }
    if (src == fleet) { setError("uph_fleet_adopt: the source is the fleet itself"); return UPH_ERR_INVALID; }
    if (src->map != fleet->map) { setError("uph_fleet_adopt: the source and the fleet are bound to different maps"); return UPH_ERR_INVALID; }
    if (src->pending || fleet->pending) { setError("uph_fleet_adopt: an asynchronous solve is in flight (uph_batch_wait first)"); return UPH_ERR_INVALID; }
    if (src->B <= 0 || !src->traj_resident) { setError("uph_fleet_adopt: the source holds no resident trajectory (uph_batch_solve / uph_eval_batch after the upload first)"); return UPH_ERR_INVALID; }
    std::vector<char> taken((size_t)fleet->B, 0);
    for (int32_t q = 0; q < n; q++) {
        const std::string qn = std::string(who) + ": query " + std::to_string(q);
        const int32_t b = src_traj[q], s = slot[q];
        if (b < 0 || b >= src->B) { setError(qn + " names no trajectory of the source's resident batch"); return UPH_ERR_INVALID; }
        if (!src->rejected.empty() && src->rejected[(size_t)b]) {
            setError(qn + (src->is_fleet ? " names an empty slot of the source fleet (no trajectory)" : " names an UPH_RET_UNSUPPORTED slot of the source (no trajectory)")); return UPH_ERR_INVALID;
        }
        if (s < 0 || s >= fleet->B) { setError(qn + " names no slot of the fleet"); return UPH_ERR_INVALID; }
        if (taken[(size_t)s]) { setError(qn + " names slot " + std::to_string(s) + " a second time in one call"); return UPH_ERR_INVALID; }
        taken[(size_t)s] = 1;
        if (t0 && !std::isfinite(t0[q])) { setError(qn + " has a non-finite t0"); return UPH_ERR_INVALID; }
    }
    const GridDev tg = uphMapGrid(fleet->map);
    if (src->frames.empty() != fleet->frames.empty() || (!src->frames.empty() && (!sameGeometry(src->frames_grid, tg) || !sameGeometry(fleet->frames_grid, tg)))) {
        setError("uph_fleet_adopt: the map's geometry changed since the source's batch was uploaded or the fleet was created (their local frames were formed from another one)");
        return UPH_ERR_INVALID;
    }
    for (int32_t q = 0; q < n; q++) {
        const TrajDesc& t = src->desc[(size_t)src_traj[q]];
        if (t.Nxy > fleet->fleet_cap_xy || t.Nyaw > fleet->fleet_cap_yaw) {
            setError(std::string(who) + ": query " + std::to_string(q) + " has " + std::to_string(t.Nxy) + " / " + std::to_string(t.Nyaw) + " pieces, more than the fleet's caps " +
                     std::to_string(fleet->fleet_cap_xy) + " / " + std::to_string(fleet->fleet_cap_yaw));
            return UPH_ERR_LIMIT;
        }
    }
    // admitted as a whole: the records, one launch, the wait
    std::vector<AdoptRec> rec((size_t)n);
    for (int32_t q = 0; q < n; q++) {
        const TrajDesc& t = src->desc[(size_t)src_traj[q]];
        AdoptRec& k = rec[(size_t)q];
        k.src_cxy = t.off_cxy; k.src_cyaw = t.off_cyaw;
        k.dst_cxy = (int64_t)slot[q] * 12 * fleet->fleet_cap_xy; k.dst_cyaw = (int64_t)slot[q] * 6 * fleet->fleet_cap_yaw;
        k.src_b = src_traj[q]; k.dst_b = slot[q];
        k.w_xy = 6 * t.Nxy; k.w_yaw = 3 * t.Nyaw;
        if ((k.src_cxy | k.src_cyaw | k.dst_cxy | k.dst_cyaw) & 1) { setError("uph_fleet_adopt: a coefficient offset is not a multiple of 16 bytes"); return UPH_ERR_INVALID; }     // (not reached: multiples of 12 and 6 doubles)
        if (k.src_cxy < 0 || k.src_cxy + 12 * (int64_t)t.Nxy > src->sum_cxy || k.src_cyaw < 0 || k.src_cyaw + 6 * (int64_t)t.Nyaw > src->sum_cyaw) {
            setError("uph_fleet_adopt: a source trajectory does not lie inside the source's coefficient arrays"); return UPH_ERR_INVALID;                                      // (not reached)
        }
    }
    HIPCHK(hipSetDevice(uphMapDevice(fleet->map)));
    if (fleet->d_adopt_rec.ensure(sizeof(AdoptRec) * (size_t)n)) return UPH_ERR_HIP;
    HIPCHK(hipMemcpyAsync(fleet->d_adopt_rec.p, rec.data(), sizeof(AdoptRec) * (size_t)n, hipMemcpyHostToDevice, fleet->stream));
    AdoptArgs a;
    a.sdesc = src->d_desc.as<TrajDesc>(); a.sstate = src->d_state.as<TrajState>(); a.scxy = src->d_cxy.as<double>(); a.scyaw = src->d_cyaw.as<double>();
    a.ddesc = fleet->d_desc.as<TrajDesc>(); a.dstate = fleet->d_state.as<TrajState>(); a.dcxy = fleet->d_cxy.as<double>(); a.dcyaw = fleet->d_cyaw.as<double>();
    a.recs = fleet->d_adopt_rec.as<AdoptRec>();
    HIPCHK(hipEventRecord(fleet->ev0, fleet->stream));
    hipLaunchKernelGGL(uph_fleet_adopt_kernel, dim3((unsigned)n), dim3(ADOPT_NT), 0, fleet->stream, a);
    const hipError_t le = hipGetLastError();
    HIPCHK(hipEventRecord(fleet->ev1, fleet->stream));
    const hipError_t se = hipStreamSynchronize(fleet->stream);
    HIPCHK(le); HIPCHK(se);
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, fleet->ev0, fleet->ev1));
    fleet->last_adopt_ms = ms;
    // the host copies of what the kernel wrote, and what lives on the host only
    for (int32_t q = 0; q < n; q++) {
        const size_t b = (size_t)src_traj[q], s = (size_t)slot[q];
        TrajDesc& t = fleet->desc[s];
        t = src->desc[b];
        t.op_xy = -1; t.op_yaw = -1; t.off_x = 0; t.off_s = 0; t.off_hist = 0;
        t.off_cxy = rec[(size_t)q].dst_cxy; t.off_cyaw = rec[(size_t)q].dst_cyaw;
        fleet->rejected[s] = 0;
        fleet->fleet_t0[s] = t0 ? t0[q] : 0.0;
        for (int k = 0; k < 3; k++) fleet->end_pose[3 * s + k] = src->end_pose[3 * b + k];
        for (int k = 0; k < 9; k++) fleet->end_bnd[9 * s + k] = src->end_bnd[9 * b + k];
        if (!fleet->frames.empty()) fleet->frames[s] = src->frames[b];
    }
    countEmpty(fleet);
    fleet->framed_valid = false;
    return refreshStates(fleet);
}

int uph_fleet_release(uph_ctx* fleet, int32_t n, const int32_t* slot) {
    int r = needFleet(fleet, "uph_fleet_release");
    if (r != UPH_OK) return r;
    if (n <= 0 || !slot) { setError("uph_fleet_release: bad arguments (null pointer or n <= 0)"); return UPH_ERR_INVALID; }
    for (int32_t q = 0; q < n; q++) if (slot[q] < 0 || slot[q] >= fleet->B) { setError("uph_fleet_release: query " + std::to_string(q) + " names no slot of the fleet"); return UPH_ERR_INVALID; }
    HIPCHK(hipSetDevice(uphMapDevice(fleet->map)));
    const GridDev tg = uphMapGrid(fleet->map);
    for (int32_t q = 0; q < n; q++) {
        const int s = slot[q];
        if (fleet->rejected[(size_t)s]) continue;
        emptySlot(fleet, s, tg);
        HIPCHK(hipMemsetAsync(fleet->d_desc.as<TrajDesc>() + s, 0, sizeof(TrajDesc), fleet->stream));
        HIPCHK(hipMemsetAsync(fleet->d_state.as<TrajState>() + s, 0, sizeof(TrajState), fleet->stream));
    }
    HIPCHK(hipStreamSynchronize(fleet->stream));
    countEmpty(fleet);
    fleet->framed_valid = false;
    return UPH_OK;
}

int uph_fleet_info(const uph_ctx* fleet, int32_t* slots, int32_t* cap_xy, int32_t* cap_yaw, int32_t* occupied, double* t0) {
    const int r = needFleet(fleet, "uph_fleet_info");
    if (r != UPH_OK) return r;
    if (slots) *slots = fleet->B;
    if (cap_xy) *cap_xy = fleet->fleet_cap_xy;
    if (cap_yaw) *cap_yaw = fleet->fleet_cap_yaw;
    for (int s = 0; s < fleet->B; s++) {
        if (occupied) occupied[s] = fleet->rejected[(size_t)s] ? 0 : 1;
        if (t0) t0[s] = fleet->fleet_t0[(size_t)s];
    }
    return UPH_OK;
}

int uph_fleet_get(uph_ctx* fleet, int32_t n, const int32_t* slot, int32_t* n_xy, int32_t* n_yaw, double* T_xy, double* T_yaw, int32_t* ret_code, double* c_xy, double* c_yaw) {
    int r = needFleet(fleet, "uph_fleet_get");
    if (r != UPH_OK) return r;
    if (n <= 0 || !slot) { setError("uph_fleet_get: bad arguments (null pointer or n <= 0)"); return UPH_ERR_INVALID; }
    for (int32_t q = 0; q < n; q++) if (slot[q] < 0 || slot[q] >= fleet->B) { setError("uph_fleet_get: query " + std::to_string(q) + " names no slot of the fleet"); return UPH_ERR_INVALID; }
    HIPCHK(hipSetDevice(uphMapDevice(fleet->map)));
    const size_t wx = 12 * (size_t)fleet->fleet_cap_xy, wy = 6 * (size_t)fleet->fleet_cap_yaw;
    // many slots: the arrays in one copy each through pinned staging; few: the slots' own regions
    const bool whole = (size_t)n * 4 >= (size_t)fleet->B;
    struct Pull { double* out; HostBuf* h; DevBuf* d; size_t w; };
    const Pull pulls[2] = {{c_xy, &fleet->h_cxy, &fleet->d_cxy, wx}, {c_yaw, &fleet->h_cyaw, &fleet->d_cyaw, wy}};
    for (const Pull& p : pulls) {
        if (!p.out) continue;
        if (whole) {
            if (p.h->ensure(8 * p.w * (size_t)fleet->B)) return UPH_ERR_HIP;
            HIPCHK(hipMemcpyAsync(p.h->p, p.d->p, 8 * p.w * (size_t)fleet->B, hipMemcpyDeviceToHost, fleet->stream));
        } else {
            for (int32_t q = 0; q < n; q++)
                HIPCHK(hipMemcpyAsync(p.out + p.w * (size_t)q, p.d->as<double>() + p.w * (size_t)slot[q], 8 * p.w, hipMemcpyDeviceToHost, fleet->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(fleet->stream));
    if (whole) for (const Pull& p : pulls) {
        if (!p.out) continue;
        for (int32_t q = 0; q < n; q++) std::memcpy(p.out + p.w * (size_t)q, p.h->as<double>() + p.w * (size_t)slot[q], 8 * p.w);
    }
    for (int32_t q = 0; q < n; q++) {
        const size_t s = (size_t)slot[q];
        const bool empty = fleet->rejected[s] != 0;
        const TrajDesc& t = fleet->desc[s];
        const TrajState& st = fleet->state_host[s];
        if (n_xy) n_xy[q] = empty ? 0 : t.Nxy;
        if (n_yaw) n_yaw[q] = empty ? 0 : t.Nyaw;
        if (T_xy) T_xy[q] = empty ? 0.0 : st.T_xy;
        if (T_yaw) T_yaw[q] = empty ? 0.0 : st.T_yaw;
        if (ret_code) ret_code[q] = empty ? UPH_RET_UNSUPPORTED : st.ret_code;
        // back into map coordinates, as uph_batch_download: every piece's constant coefficient
        if (c_xy && !empty && !fleet->frames.empty())
            for (int i = 0; i < t.Nxy; i++) for (int d = 0; d < 2; d++) c_xy[wx * (size_t)q + 12 * (size_t)i + d] += fleet->frames[s].shift[d];
    }
    return UPH_OK;
}

int uph_fleet_kernel_ms(const uph_ctx* fleet, double* kernel_ms) {
    const int r = needFleet(fleet, "uph_fleet_kernel_ms");
    if (r != UPH_OK) return r;
    if (!kernel_ms) { setError("uph_fleet_kernel_ms: bad arguments"); return UPH_ERR_INVALID; }
    *kernel_ms = fleet->last_adopt_ms;
    return UPH_OK;
}

}  // extern "C"
