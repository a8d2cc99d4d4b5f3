// The optimiser context and what the translation units that work on it share (unevenhip.hip: uploads, solves, plan / re-plan / refine; traj_query.hip: the
// queries on resident trajectories): device / pinned buffers, the admission header of a problem, uph_ctx itself, HIPCHK and the functions that cross the boundary.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "clearance_dev.hpp"
#include "uph_internal.hpp"

using namespace uph;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        if (hipMalloc(&p, want) != hipSuccess) { setError("hipMalloc failed"); return -1; }
        cap = want;
        return 0;
    }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() { return (T*)p; }
};

// grow-only pinned host staging (downloads run at the PCIe rate instead of the pageable-copy rate)
struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) hipHostFree(p);
        p = nullptr; cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { setError("hipHostMalloc failed"); return -1; }
        cap = want;
        return 0;
    }
    void release() { if (p) hipHostFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() { return (T*)p; }
};

// What the admission of a batch reads of a problem: its scalars, the bounding box of its initial path and the heading changes of its yaw way-points --
// not the way-points themselves.  uph_batch_upload forms it from the caller's uph_problem, uph_plan_upload from the headers the device staged.
struct ProblemHead {
    int32_t n_inner_xy = 0, n_inner_yaw = 0;
    int refused = 0;                // != 0: refused before the limit checks (that UPH_ERR_* reason, message `why`)
    const char* why = nullptr;
    double init_xy[6], end_xy[6], init_yaw[3], end_yaw[3], total_time = 0.0;
    double lo[2], hi[2];            // bounding box of the inner way-points together with the init / end positions
    double turn = 0.0, kink = 0.0;  // yawTurnKink
};
struct uph_ctx {
    uph_map* map = nullptr;
    int device = 0;                         // copied at creation: the context must never dereference the map during teardown
    OptParams P;
    double rho = 1.0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // MINCO operator cache
    std::map<int, int> op_index;            // N -> index
    std::vector<MincoOp> ops_host;          // device pointers inside
    std::vector<void*> op_allocs;
    DevBuf d_ops;
    bool ops_dirty = false;
    // batch
    int B = 0;
    std::vector<TrajDesc> desc;
    std::vector<int> order;
    int64_t sum_n = 0, sum_S = 0, sum_cxy = 0, sum_cyaw = 0, sum_hist = 0;
    size_t lds_bytes = 0;                   // dynamic LDS of the main launch (largest footprint among the trajectories below the residency limit)
    size_t lds_big = 0;                     // ... and of the oversize class, launched concurrently on stream2 (0 = no such class)
    int n_main = 0;                         // order[0, n_main) main class, order[n_main, B) oversize class
    std::vector<int> rejected;              // per problem: 0, or the status code that made it unsupported (solved as a placeholder, reported as UPH_RET_UNSUPPORTED)
    int n_rejected = 0;
    bool all_rejected = false;              // the last upload failed because EVERY problem was unsupported (not because of a misuse or a resource limit)
    std::vector<TrajFrame> frames;          // per-trajectory local frames of the uploaded batch (empty: the map's own frame, uph_common.hpp TrajFrame)
    std::vector<GridDev> grid_host_framed;  // ... and the per-trajectory grid descriptors made from them (source of the asynchronous copy)
    GridDev frames_grid;                    // the map's descriptor the frames were formed from (geometry check at launch)
    GridDev framed_from;                    // the map's descriptor the resident per-trajectory descriptors were made from
    bool framed_valid = false;              // d_gridmem holds the framed descriptors of the current batch
    std::vector<int> origin;                // batch loaded by uph_optimize_batch_multi: the caller's index of each problem of this context's share (empty: identity)
    bool sample_f32 = false;                // fp32 sample arithmetic (uph_ctx_set_sample_precision)
    uph_clearance* clear_layer = nullptr;   // the clearance term (uph_ctx_set_clearance_term): its layer (nullptr: off; counted on the layer while set) ...
    double clear_d_safe = 0.0, clear_weight = 0.0;      // ... its safe distance in metres and its weight
    unsigned char param_block[sizeof(OptParams) + sizeof(ClearTermDev)];   // source of the per-launch copy into d_parammem: the parameters, the term's descriptor behind them
    int xcd_group = 0;                      // experiment knob (uph_ctx_set_xcd_locality): > 0 = permute the launch order inside groups of that many workgroups for per-XCD L2 locality
    hipStream_t stream2 = nullptr;
    hipEvent_t evp0 = nullptr, evp1 = nullptr;      // prepare launch of an asynchronous solve
    bool pending = false;                   // uph_batch_solve_async issued, uph_batch_wait not yet called
    hipEvent_t ev2 = nullptr;
    std::vector<size_t> fp_bytes;           // per-trajectory LDS footprint
    int lanes = 64;                         // lanes per trajectory of the current batch (64 or 256)
    int lanes_forced = 0;                   // 0 = choose from the batch size
    int wps = 1;                            // workgroups of 256 lanes per CU the kernel is compiled for (1 or 2)
    int wps_forced = 0;                     // experiment knob: register-capped (2) or uncapped (1) build regardless of batch size
    DevBuf d_thomas, d_rsd, d_rs, d_gridmem, d_parammem;
    GridDev grid_host;                      // source of the descriptor copy (outlives the asynchronous copy)
    DevBuf d_desc, d_state, d_x, d_x0, d_gout, d_dual, d_res, d_scl, d_cxy, d_cyaw, d_hist, d_report, d_order, d_trace;
    DevBuf d_pen_gxy, d_pen_gyaw, d_pen_out;      // uph_penalty_batch outputs (allocated at its first call)
    DevBuf d_roll_tt, d_roll_traj, d_roll_stage;  // uph_rollout_*: time table, launch records, staging of the host variant (allocated at the first call)
    bool traj_resident = false;             // the resident coefficients / durations are those of a solve or evaluation of the current batch (rollout input)
    // uph_plan_upload: staging indexed by goal (PlanHead, way-points), re-searched goals' indices, scatter records; the resident problems as staged
    DevBuf d_plan_head, d_plan_xy, d_plan_yaw, d_plan_goal, d_plan_rec;
    bool planned = false;                   // the resident batch came from uph_plan_upload (uph_plan_staged may read the staging)
    std::vector<ProblemHead> plan_probs;   // [B] the staged problems in resident order, boundary velocities formed on the host
    std::vector<double> end_pose;          // [B][3] each problem's end position (map coordinates) and end yaw as uploaded (uph_replan_upload, goals == NULL)
    std::vector<double> end_bnd;           // [B][9] each problem's whole end boundary as uploaded: end_xy {P, V, A} (map coordinates), end_yaw (uph_refine_upload)
    DevBuf d_sw_q, d_sw_out;               // uph_replan_upload / uph_traj_states / uph_refine_upload: state queries and states (allocated at the first call)
    DevBuf d_refine_rec;                   // uph_refine_upload: staging records
    DevBuf d_win_q, d_win_out;             // uph_check_batch / uph_locate_batch / uph_within_batch and the common-clock queries: query records and result rows (allocated at the first call)
    double last_check_ms = 0.0;            // uph_check_kernel of the last uph_check_batch (events on the context's stream)
    double last_locate_ms = 0.0;           // the kernel(s) of the last uph_locate_batch or uph_within_batch (events on the context's stream)
    double last_sep_ms = 0.0;              // the kernels of the last uph_extent_batch, uph_separation_batch or uph_conflicts_batch (events on the context's stream)
    DevBuf d_delay;                        // uph_delay_sweep_batch / uph_delay_extent_batch / uph_delays_batch: the table of start delays (allocated at the first call)
    double last_delay_ms = 0.0;            // the kernels of the last of those three calls (events on the context's stream)
    double last_foot_ms = 0.0;             // the kernels of the last uph_footprint_separation_batch or uph_footprint_conflicts_batch (events on the context's stream)
    double last_foot_check_ms = 0.0;       // the kernel(s) of the last uph_footprint_check_batch (events on the context's stream)
    double last_clear_check_ms = 0.0;      // the kernel(s) of the last uph_clearance_check_batch (events on the context's stream)
    int trace_cap = 0;                      // requested for the next upload
    int trace_cap_up = 0;                   // what the uploaded batch's trace buffer was sized for
    std::vector<TrajState> state_host;
    HostBuf h_x, h_cxy, h_cyaw, h_dual, h_res, h_scl;      // download staging
    // stats of the last solve
    double last_ms = 0.0, last_prepare_ms = 0.0;
    int64_t last_evals = 0, last_sample_evals = 0, last_iters = 0, last_hist_bytes = 0;
    int64_t last_abandon[5] = {0, 0, 0, 0, 0};   // line-search trial counters of the last solve (uph_batch_abandon_stats): rejected, guarded, abandoned, chunks skipped, adjoints skipped
    // fleet (uph_fleet_create, fleet.hip): the resident batch is B slots of fixed stride -- slot s owns 12 cap_xy doubles of d_cxy and 6 cap_yaw of d_cyaw --, filled by
    // uph_fleet_adopt from other contexts; rejected[s] != 0 marks an EMPTY slot.  Never uploaded into, never solved.
    bool is_fleet = false;
    int fleet_cap_xy = 0, fleet_cap_yaw = 0;
    std::vector<double> fleet_t0;          // [B] each slot's start on the common clock (0 for an empty slot)
    DevBuf d_adopt_rec;                    // uph_fleet_adopt: the launch's records
    double last_adopt_ms = 0.0;            // uph_fleet_adopt_kernel of the last uph_fleet_adopt (events on the fleet's stream)
};
// the refusal of an entry point that uploads into, solves, evaluates, reports on, downloads or sets the state of a batch, on a fleet (`who`: the call's own name)
inline bool refusedOnFleet(const uph_ctx* c, const char* who) {
    if (!c || !c->is_fleet) return false;
    setError(std::string(who) + ": the context is a fleet (its slots are filled by uph_fleet_adopt; it takes no upload, solve, evaluation, report, download or batch state)");
    return true;
}
#define NOT_ON_FLEET(c, who)                                  \
    do {                                                      \
        if (refusedOnFleet((c), (who))) return UPH_ERR_INVALID; \
    } while (0)

#define HIPCHK(call)                                                                               \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            setError(std::string(#call) + ": " + hipGetErrorString(_e));                           \
            return UPH_ERR_HIP;                                                                    \
        }                                                                                          \
    } while (0)

// ---- unevenhip.hip
int refreshStates(uph_ctx* c);                  // the resident TrajState rows (T_xy, T_yaw, ...) into c->state_host
// the map's grid descriptor -> grid, and the descriptors the kernels read from memory (BatchDev::grid_mem) brought up to date on the context's stream
int syncGridMem(uph_ctx* c, uph::GridDev& grid);

// ---- traj_query.hip
struct SwitchQuery {            // one state query (uph_switch_state_kernel), formed on the host
    int32_t b, framed;          // resident trajectory; framed: the batch solves in local frames (add shift, as the rollout does)
    double t;                   // switch time (finite)
    double shift[2];
};
constexpr int SWITCH_COLS = 9, TRAJ_STATE_COLS = 10;
// the check every query on resident trajectories passes: no asynchronous solve is in flight on c, c holds resident trajectories and every query names one of
// them at a finite time (`who` opens the message)
int checkTrajQueries(const uph_ctx* c, int32_t n, const int32_t* traj, const double* t, const char* who);
SwitchQuery trajQuery(const uph_ctx* c, int32_t b, double t);
// the states of queries sq on c's resident trajectories into c->d_sw_out [n][cols] (enqueued on c's stream, not waited for); cols = SWITCH_COLS or TRAJ_STATE_COLS
int launchTrajStates(uph_ctx* c, const std::vector<SwitchQuery>& sq, int cols = TRAJ_STATE_COLS);
