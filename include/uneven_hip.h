/*
 * uneven_hip.h -- C-ABI of libunevenhip.so, the MI355X (gfx950) back-end that drops in behind the reference's
 * ALMTrajOpt::optimizeSE2Traj and UnevenMap interfaces (ZJU-FAST-Lab/uneven_planner).
 *
 * Plain C: opaque handles, caller-owned arrays, int status returns (0 = ok, <0 = error, text via uph_last_error()).
 * Nothing throws across this boundary.  A context is not thread-safe (one solve at a time, like the reference's
 * in_opt flag, back_end/src/alm_traj_opt.cpp:61,178,275); distinct contexts may be used concurrently.
 *
 * Reference interfaces replaced (paths relative to /root/reference/src/uneven_planner):
 *   uph_optimize_batch      <- ALMTrajOpt::optimizeSE2Traj  back_end/include/back_end/alm_traj_opt.h:92-98,
 *                              back_end/src/alm_traj_opt.cpp:168-278 (B = 1 reproduces one call)
 *   uph_result              <- ALMTrajOpt::getTraj / MINCO_SE2::getTraj / getTrajJerkCost
 *                              alm_traj_opt.h:165-168, back_end/include/utils/se2traj.hpp:682-695,844-855
 *   uph_opt_params          <- ALMTrajOpt public parameter members  alm_traj_opt.h:29-53 (rosparam, alm_traj_opt.cpp:7-29)
 *   uph_map_build           <- UnevenMap::constructMap  uneven_map/src/uneven_map.cpp:317-417 (+ crop/voxel filter :130-144)
 *   uph_map_set_cells       <- UnevenMap::constructMapInput  uneven_map.cpp:270-315 (cells from the .map cache)
 *   uph_map_save_csv / uph_map_load_csv / uph_map_save_cache / uph_map_load_cache
 *                           <- the `.map` cache: written at the end of UnevenMap::constructMap (uneven_map.cpp:400-412), read by constructMapInput (:270-315)
 *   uph_map_get_cells       -> fills UnevenMap::map_buffer / c_buffer / occ_buffer / occ_r2_buffer
 *                              uneven_map/include/uneven_map/uneven_map.h:91-94, occupancy rule uneven_map.cpp:170-179
 *   uph_terrain_query       <- UnevenMap::getAllWithGrad  uneven_map.h:318-377 (device-side twin, exposed for parity tests)
 *   uph_terrain_pose_query  <- UnevenMap::getTerrainPos  uneven_map.h:203-218 (batched)
 *   uph_map_filter_cloud    <- pcl::CropBox + pcl::VoxelGrid as UnevenMap::init applies them  uneven_map.cpp:133-143
 *   uph_frontend_query      <- UnevenMap::getTerrainSig / isOccupancy / isOccupancyXY  uneven_map.h:389-396, 471-498 (batched)
 *   uph_eval_batch          <- innerCallback  alm_traj_opt.cpp:280-347 (one objective+gradient evaluation; test/bench hook)
 *   uph_penalty_batch       <- ALMTrajOpt::calConstrainCostGrad  alm_traj_opt.cpp:663-991 (the penalty kernel alone; test/bench hook)
 *   uph_init_scaling_batch  <- ALMTrajOpt::initScaling  alm_traj_opt.cpp:349-661 (test hook)
 *   uph_report_batch        <- ALMTrajOpt::getMaxVxAxAyCurAttSig alm_traj_opt.h:170-229 + SE2Trajectory::getNonHolError
 *                              se2traj.hpp:551-561
 *   uph_rollout_batch / uph_rollout_batch_dev
 *                           <- ALMTrajOpt::visSE3Traj  back_end/src/alm_traj_opt.cpp:1102-1135 (SE2Trajectory::getNormSE2Pos every dt, then
 *                              UnevenMap::getTerrainPos, + the end point) and the per-sample terms behind getMaxVxAxAyCurAttSig
 *                              (alm_traj_opt.h:170-229): the resident batch sampled on the device
 *   uph_rollout_sizes / uph_rollout_plan
 *                           <- the sample count of their `for (t = 0; t < total; t += dt)` loops (total: se2traj.hpp getTotalDuration)
 *   uph_map_build_multi     <- UnevenMap::constructMap (as above) sharded over the GPUs of one node from ONE host process -- the reference
 *                              is a single process (plan_manager/src/manager_node.cpp): x-slabs + one RCCL all-gather (BASELINE.json configs[3])
 *   uph_optimize_batch_multi<- B x ALMTrajOpt::optimizeSE2Traj split over per-device contexts (BASELINE.json configs[2], [4])
 *   uph_kino_plan_batch     <- KinoAstar::plan  front_end/src/kino_astar.cpp:67-236 (one call per query; B = 1 reproduces one call), the caller of
 *                              the map's query interface and the producer of the front-end path PlanManager resamples (plan_manager.cpp:59-60)
 *   uph_plan_upload         <- PlanManager::rcvWpsCallBack's chain up to the optimiser (plan_manager.cpp:43-134): kino_astar->plan (:59-60), the
 *                              initial-guess stage (:62-132) and the arguments of optimizeSE2Traj, for a batch of goals with the paths kept on the device
 *   uph_replan_upload       <- the same chain for a vehicle in motion: the start of each plan is a resident trajectory's state at a switch time
 *                              (getPos / getVel / getAcc of SE2Trajectory, se2traj.hpp:343-361, 106-140) instead of plan_manager.cpp:86-94's start
 *   uph_traj_states         <- getPos / getVel / getAcc of resident trajectories at given (trajectory, time) pairs
 *   uph_refine_upload       <- receding-horizon refinement: the rest of each resident trajectory as the initial guess of a new problem from its
 *                              state at a switch time, no search
 *   uph_check_batch         <- ALMTrajOpt::getMaxVxAxAyCurAttSig (alm_traj_opt.h:170-229) + SE2Trajectory::getNonHolError (se2traj.hpp:551-561) + UnevenMap::isOccupancy
 *                              (uneven_map.h:471-488) per sample, over time windows of chosen resident trajectories, held against the optimiser's
 *                              limits (alm_traj_opt.h:29-53) instead of printed
 *   uph_check_window        <- the part of their `for (t = 0; t < total; t += dt)` loop a time window holds
 *   uph_check_limits        <- the limits among ALMTrajOpt's parameter members  alm_traj_opt.h:33-38
 *   uph_locate_batch        <- the time on a trajectory that traj_anal.hpp:490-491 takes from the wall clock (t_cur = now - start_time), here from the
 *                              odometry pose PlanManager::rcvOdomCallBack holds (plan_manager.cpp:31-41), with the tracking error at that time
 *   uph_within_batch        <- which resident trajectories enter a rect of the map (a changed region) and when
 *   uph_separation_batch    <- how close two resident trajectories come at the same moment of a clock they share (each starts at its own t0 on it)
 *   uph_conflicts_batch     <- the pairs of a fleet on one map that come closer than their radii allow: extents, a host broad phase, separation
 *   uph_footprint_separation_batch / uph_footprint_conflicts_batch  <- the same two with the vehicles as oriented rectangles (front, rear, half width)
 *                              turned by the trajectory's yaw instead of discs
 *   uph_footprint_check_batch  <- UnevenMap::isOccupancy / isOccupancyXY (uneven_map.h:471-488) at every column the vehicle's rectangle covers, not only the one
 *                              under the trajectory's point, over time windows of chosen resident trajectories
 *   uph_clearance_* / uph_clearance_check_batch  <- no counterpart (UnevenMap keeps occupancy bits only): the squared distance transform of a body layer per yaw
 *                              slice, and its value along time windows of chosen resident trajectories -- how close, when and where
 *   uph_delays_batch        <- the smallest start delay that clears each vehicle of a fleet against all vehicles ahead of it in priority order
 *   uph_footprint_delay_sweep_batch / uph_footprint_delays_batch  <- the delay sweep and the schedule with the vehicles as oriented rectangles
 *   uph_kino_params         <- rosparam kino_astar/...  kino_astar.cpp:7-20, values of plan_manager/params/run_hill.yaml:16-30
 */
#ifndef UNEVEN_HIP_H
#define UNEVEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct uph_map uph_map;   /* device-resident SE(2) -> R x S2+ terrain grid            */
typedef struct uph_ctx uph_ctx;   /* optimiser context bound to one map, one device, one stream */
typedef struct uph_kino uph_kino; /* front-end search context bound to one map: per-query workspaces (node pools, open heaps) in HBM */
typedef struct uph_body_layer uph_body_layer; /* the occupancy of one map dilated by a vehicle rectangle, one byte per (ix, iy, iyaw), in HBM */

/* ---- status codes */
#define UPH_OK 0
#define UPH_ERR_INVALID (-1)   /* bad argument                                   */
#define UPH_ERR_HIP (-2)       /* a HIP runtime call failed (see uph_last_error) */
#define UPH_ERR_NO_DEVICE (-3) /* no gfx950 device visible                        */
#define UPH_ERR_LIMIT (-4)     /* problem exceeds a compiled limit (UPH_MAX_*)    */
#define UPH_ERR_NO_CACHE (-5)  /* uph_map_load_cache only: neither cache file is readable -- build the map (uneven_map.cpp:166-167); any other code is a real failure */

/* uph_result.ret_code beyond the reference's 0 / 1 / 2: */
#define UPH_RET_STOPPED 3      /* test hook only: the ALM loop was stopped by uph_batch_alm_passes' pass cap                          */
#define UPH_RET_UNSUPPORTED 4  /* the problem lies outside the compiled limits (more than UPH_MAX_PIECE_* pieces; piece_yaw < piece_xy):
                                  not solved, outputs untouched, last_lbfgs_ret = the UPH_ERR_* reason.  The other problems of the
                                  batch are solved normally.  (A goal closer than one piece length -- n_inner_* = 0, a single quintic
                                  piece per block -- IS solved, as the reference does.)                                               */

#define UPH_RET_LEFT_TILE 5    /* tile maps only: the solved path reached the border of the rows the tile holds (lookups were clamped there) */
#define UPH_TILE_MARGIN 2.0    /* [m] a problem is accepted by a tile map when its initial path keeps this distance from the tile's border */

#define UPH_MAX_PIECE_XY 128   /* Nxy  <= 128 (38 m at piece_len 0.3)  */
#define UPH_MAX_PIECE_YAW 256  /* Nyaw <= 256                          */
#define UPH_MAX_MEM 256        /* L-BFGS history length                */
#define UPH_MAX_PAST 8

/* ---- map parameters: rosparam uneven_map/... (uneven_map.cpp:75-88), values of plan_manager/params/run_hill.yaml:2-14 */
typedef struct uph_map_params {
    int32_t iter_num;           /* 2     */
    double map_size_x;          /* 10.0  */
    double map_size_y;          /* 10.0  */
    double ellipsoid_x;         /* 0.2   */
    double ellipsoid_y;         /* 0.1   */
    double ellipsoid_z;         /* 0.1   */
    double xy_resolution;       /* 0.05  */
    double yaw_resolution;      /* 0.1   */
    double min_cnormal;         /* 0.8   */
    double max_rho;             /* 0.05  */
    double gravity;             /* 9.81  */
} uph_map_params;

/* ---- analytic fractal terrain of BASELINE.json configs[4] ("synthetic 1 km^2 fractal terrain ... fp32").  No reference
 *      counterpart: the reference only loads .pcd clouds (uneven_map.cpp:121-128); the cell fit applied to the analytic surface is
 *      constructMap's (uneven_map.cpp:329-391).  Values of tools / bench: seed 7, H 0.8, 2..512 m, 15 m, 35 deg, 32 waves */
#define UPH_FBM_MAX_WAVES 48
#define UPH_FBM_TABLE_DOUBLES (4 * UPH_FBM_MAX_WAVES + 12 + 9)
typedef struct uph_fbm_params {
    uint64_t seed;
    double hurst;               /* amplitude ~ wavelength^hurst                                             */
    double lambda_min, lambda_max;   /* band limits of the fBm sum [m]                                       */
    double amplitude;           /* bound on the sum of the wave amplitudes [m]                               */
    double max_slope_deg;       /* bound on the sum of amplitude x wavenumber (worst-case slope)             */
    int32_t n_waves;            /* <= UPH_FBM_MAX_WAVES                                                      */
    double rough_amp;           /* ripple amplitude inside rough patches [m]                                 */
    double rough_lambda;        /* ripple wavelength [m] (x 0.8..1.2)                                        */
    double patch_lambda;        /* envelope wavelength [m] (x 1..3)                                          */
    double rough_threshold;     /* envelope level above which ripples appear (0..1)                          */
} uph_fbm_params;

/* ---- optimiser parameters: alm_traj_opt.h:29-53, values of run_hill.yaml:32-55 */
typedef struct uph_opt_params {
    double rho_T, rho_ter, max_vel, max_acc_lon, max_acc_lat, max_kap, min_cxi, max_sig;
    int32_t use_scaling;
    double rho, beta, gamma, epsilon_con, max_iter;            /* max_iter is a double in the reference */
    double g_epsilon, min_step, inner_max_iter, delta;
    int32_t mem_size, past, int_K;
} uph_opt_params;

/* ---- PlanManager parameters of the initial-guess stage: rosparam manager/... (plan_manager.cpp:9-13), values of run_hill.yaml:57-62 */
typedef struct uph_manager_params {
    double piece_len;           /* 0.3  */
    double mean_vel;            /* 0.5  */
    double init_time_times;     /* 1.2  */
    double yaw_piece_times;     /* 2.0  */
    double init_sig_vel;        /* 0.05 */
    /* test_mode != 0 selects the OTHER producer of optimizeSE2Traj's arguments in the reference, the back-end's stand-alone test node
     * ALMTrajOpt::rcvWpsCallBack (back_end/src/alm_traj_opt.cpp:73-144): its literals replace the five parameters above (piece_len 0.3, yaw
     * pitch piece_len / 2, end velocities 0.05, total time = length / max_vel * 1.2 with the optimiser's max_vel), each comb emits AT MOST ONE
     * node per path segment (`if`, :122,128, where PlanManager loops with `while`), and every position node also contributes its interpolated
     * yaw to the yaw way-points (:132).  Zero-initialised aggregates ({0.3, 0.5, 1.2, 2.0, 0.05}) keep selecting PlanManager's stage. */
    int32_t test_mode;          /* 0    */
    double test_max_vel;        /* ALMTrajOpt::max_vel, run_hill.yaml:35 (0.5); read in test mode only */
} uph_manager_params;

/* ---- KinoAstar parameters: rosparam kino_astar/... (front_end/src/kino_astar.cpp:7-19), values of run_hill.yaml:16-30 */
typedef struct uph_kino_params {
    double yaw_resolution;      /* 3.15 : lattice yaw bin of the search (NOT the map's yaw_resolution) */
    double lambda_heu;          /* 1.0  */
    double weight_r2;           /* 1.0  */
    double weight_so2;          /* 0.5  */
    double weight_v_change;     /* 0.0  */
    double weight_delta_change; /* 0.0  */
    double weight_sigma;        /* 10.0 */
    double time_interval;       /* 0.3  */
    double collision_interval;  /* 0.06 */
    double oneshot_range;       /* 1.0  */
    double wheel_base;          /* 0.26 */
    double max_steer;           /* 0.5  */
    double max_vel;             /* 0.5  */
} uph_kino_params;

/* uph_kino_plan_batch status per query (the reference prints a message and returns an empty path for 1-4, kino_astar.cpp:86-95, 212-216, 233) */
#define UPH_KINO_OK 0
#define UPH_KINO_START_OCCUPIED 1
#define UPH_KINO_GOAL_OCCUPIED 2
#define UPH_KINO_NO_PATH 3
#define UPH_KINO_POOL_EXHAUSTED 4
#define UPH_KINO_EXPANSION_CAP 5   /* test hook: stopped by max_expand */
#define UPH_KINO_INTERNAL 6

/* ---- one optimizeSE2Traj call.  Matrices are column-major like Eigen::MatrixXd:
 *      init_xy/end_xy = 2x3 {P,V,A columns} -> [Px,Py,Vx,Vy,Ax,Ay]; inner_xy = 2 x n_inner_xy -> [x0,y0,x1,y1,...] */
typedef struct uph_problem {
    int32_t n_inner_xy;         /* piece_xy  - 1 */
    int32_t n_inner_yaw;        /* piece_yaw - 1 */
    double init_xy[6], end_xy[6];
    double init_yaw[3], end_yaw[3];
    const double* inner_xy;
    const double* inner_yaw;
    double total_time;
} uph_problem;

/* ---- result of one solve.  Pointer members are caller-owned (may be NULL to skip);
 *      sizes: x_final[n], n = 2*n_inner_xy + n_inner_yaw + 1 (alm_traj_opt.cpp:188);
 *      c_xy[6*piece_xy*2] row-major (row 6i+k = t^k coefficient of piece i, se2traj.hpp:570), c_yaw[6*piece_yaw];
 *      hx[S], gx[6*S], lambda[S], mu[6*S] in the reference's constraint order (alm_traj_opt.cpp:705-708), S = piece_xy*(int_K+1) */
typedef struct uph_result {
    int32_t ret_code;           /* 0 ok, 1 L-BFGS hard error, 2 ALM hit max_iter (alm_traj_opt.cpp:176,252,267); UPH_RET_* above */
    int32_t alm_iters, lbfgs_iters, evals, last_lbfgs_ret;
    double cost;                /* inner_cost of the last L-BFGS call */
    double jerk_cost;           /* minco_se2.getTrajJerkCost() of the last evaluated trajectory */
    double piece_T_xy, piece_T_yaw;   /* uniform piece durations of the last evaluated trajectory */
    double rho_final;
    double scale_fx;
    double* x_final;
    double* c_xy;
    double* c_yaw;
    double* hx;
    double* gx;
    double* lambda;
    double* mu;
    double* scale_cx;           /* [7*S] */
} uph_result;

/* ---- library */
const char* uph_last_error(void);
int uph_device_count(void);
const char* uph_version(void);
/* hash (16 hex digits) of the sources this library was built from: every .hip / .hpp / .cpp file of csrc and this header, in sorted order (csrc/Makefile) --
 * `uneven_planner_amd._lib.sources_id()` computes the same over the tree, so a run can tell whether the library it loaded is a build of the tree next to it */
const char* uph_build_id(void);

/* ---- initial guess: PlanManager::rcvWpsCallBack between kino_astar->plan and traj_opt.optimizeSE2Traj (plan_manager.cpp:62-132) -- or, with
 *      mp->test_mode, the test node's ALMTrajOpt::rcvWpsCallBack (alm_traj_opt.cpp:73-144) --, for a
 *      batch of front-end paths.  paths = concatenated poses [x, y, yaw]; path b is poses offsets[b] .. offsets[b+1]-1.  Outputs are the
 *      optimizeSE2Traj arguments in uph_problem's layout, problem b at init_xy + 6b, init_yaw + 3b, inner_xy + 2*cap_xy*b ([x0,y0,x1,y1,..]),
 *      inner_yaw + cap_yaw*b; n_inner_* receive the way-point counts.  unwrapped (may be NULL) receives the yaw column after :62-78.
 *      UPH_ERR_LIMIT when a path needs more than cap_xy / cap_yaw way-points (the counts are still written). */
int uph_resample_batch(const uph_manager_params* mp, int32_t B, const double* paths, const int64_t* offsets, int32_t cap_xy, int32_t cap_yaw,
                       double* init_xy, double* end_xy, double* init_yaw, double* end_yaw, double* inner_xy, double* inner_yaw,
                       int32_t* n_inner_xy, int32_t* n_inner_yaw, double* total_time, double* unwrapped);

/* ---- terrain map */
int uph_map_create(const uph_map_params* mp, int device, uph_map** out);
/* the same grid with its cells stored as four floats (16 bytes) instead of four doubles: BASELINE.json configs[4]'s fp32 mode.  Lookups widen
 * to double on load and all arithmetic stays fp64; uph_map_build is refused, the cells come from uph_map_fill_fbm / uph_map_set_cells / import */
int uph_map_create_f32(const uph_map_params* mp, int device, uph_map** out);
int uph_map_storage_bytes(const uph_map* m);                                                    /* 8 or 4: bytes per stored field */
/* a TILE of the grid: only the x-rows [x0, x1) of the whole grid (uph_map_dims keeps reporting the whole grid) are held in memory -- for
 * grids that do not fit one GPU (1 km^2 at 0.05 m is 410 GB).  Index arithmetic is the whole grid's, so every lookup
 * inside the tile is bit-identical to the replicated grid; lookups outside are clamped to the tile.  Problems are routed on the host to the
 * tile that owns them (x-slab + halo); uph_batch_upload rejects (UPH_RET_UNSUPPORTED) a path closer than UPH_TILE_MARGIN to the border and
 * uph_batch_download flags one that ended there (UPH_RET_LEFT_TILE).  Filled by uph_map_fill_fbm / uph_map_set_cells (held rows only);
 * uph_map_get_cells / get_window / occupancy cover the held rows. */
int uph_map_create_tile(const uph_map_params* mp, int device, int32_t x0, int32_t x1, int32_t f32, uph_map** out);
int uph_map_tile(const uph_map* m, int32_t* x0, int32_t* x1);                                  /* the rows held: whole grid -> [0, nx) */
/* fill the x-slab [x0, x1) (x1 <= 0: whole map) with the analytic fractal terrain: one constructMap-style plane fit per cell on a 5 x 3
 * body-frame lattice of surface samples; then commit.  uph_fbm_table returns the wave table a checker needs to restate the surface:
 * [UPH_FBM_MAX_WAVES][a, kx, ky, phase], ripples [4][kx, ky, phase], envelope [3][kx, ky, phase] */
int uph_map_fill_fbm(uph_map* m, const uph_fbm_params* fp, int32_t x0, int32_t x1);
int uph_fbm_table(const uph_fbm_params* fp, double* table);
/* cells of the xy window [x0, x1) x [y0, y1) (all yaw bins) as doubles, whatever the storage: rxs2[(x1-x0)*(y1-y0)*nyaw*4] */
int uph_map_get_window(uph_map* m, int32_t x0, int32_t x1, int32_t y0, int32_t y1, double* rxs2);
void uph_map_destroy(uph_map* m);
int uph_map_dims(const uph_map* m, int32_t dims3[3]);                       /* voxel_num (uneven_map.cpp:108-110) */
/* cells: ncell x 4 {z, sigma, zb.x, zb.y} in the reference's address order (uneven_map.h:427-435); recomputes c and occupancy */
int uph_map_set_cells(uph_map* m, const double* rxs2);
/* any pointer may be NULL.  rxs2: ncell x 4, c: ncell, occ: ncell chars, occ_r2: nx*ny chars */
int uph_map_get_cells(uph_map* m, double* rxs2, double* c, char* occ, char* occ_r2);
/* ---- the `.map` cache: the CSV UnevenMap::constructMap writes at its end (uneven_map.cpp:400-412: one line
 * `x,y,yaw,z,sigma,zb.x,zb.y` per cell in address order, ostream default format = six significant digits) and constructMapInput reads
 * (uneven_map.cpp:270-315: cells not mentioned stay RXS2() zeros, indices through atoi, values through stold narrowed to double, lines with an
 * index outside the grid dropped), plus a binary side-car that holds the cells bit for bit.  Host functions, no device needed:
 * rxs2 = ncell x 4 doubles in address order, dims3 = voxel_num; c (may be NULL) receives c_buffer = sqrt(1 - |zb|^2) of the cells read, 1 for
 * the others (uneven_map.cpp:117-119, 307); n_lines (may be NULL) the number of lines used.  load_*: UPH_ERR_INVALID when the file cannot be
 * opened (the reference then builds the map, uneven_map.cpp:166-167), load_bin UPH_ERR_LIMIT when it was written for another grid. */
int uph_map_save_csv(const char* path, const double* rxs2, const int32_t dims3[3]);
int uph_map_load_csv(const char* path, const int32_t dims3[3], double* rxs2, double* c, int64_t* n_lines);
int uph_map_save_bin(const char* path, const double* rxs2, const int32_t dims3[3]);
int uph_map_load_bin(const char* path, const int32_t dims3[3], double* rxs2);
/* the same against a device map: save = download the cells and write the CSV and / or the side-car (either path may be NULL); load =
 * constructMapInput: the side-car if bin_path names a readable one for this grid that is not older than the CSV (the CSV is the reference's own
 * cache and the source of truth: one regenerated later wins), else the CSV, then uph_map_set_cells (commit: c, occupancy).
 * A named CSV that does not exist means NO cache even when a side-car lies next to it (the reference rebuilds whenever map_file is absent,
 * uneven_map.cpp:166-167, 270-277); the side-car alone is used only with csv_path == NULL.
 * source (may be NULL): 2 side-car, 1 CSV.  UPH_ERR_NO_CACHE when no cache can be read: build the map then (every other error code -- a tile
 * map, a grid that does not fit host memory, a HIP failure -- is a failure, not a reason to rebuild and overwrite the cache). */
int uph_map_save_cache(uph_map* m, const char* csv_path, const char* bin_path);
int uph_map_load_cache(uph_map* m, const char* csv_path, const char* bin_path, int32_t* source);
/* constructMap on the x-slab [x0, x1): crop box + 1 cm voxel filter, xy bucketing and plane fits all on the device (the host uploads the cloud).
 * xyz: n x 3 float32 (what pcl::PCDReader delivers).  Cells outside the slab are untouched.  Blocking. */
int uph_map_build(uph_map* m, const float* xyz, int64_t n, int32_t x0, int32_t x1);
/* uph_map_build with the VoxelGrid stage skipped: the cloud passes the crop box and keeps its order -- for callers that hold a filtered cloud already
 * (uph_map_filter_cloud's output, or uph_map_built_cloud's).  Refusals as uph_map_build. */
int uph_map_build_filtered(uph_map* m, const float* xyz, int64_t n, int32_t x0, int32_t x1);
/* ---- the map from a new scan in a box (csrc/map_build.hip).  After a uph_map_build / uph_map_build_filtered of the WHOLE grid, or a
 * uph_map_update, the map owns the filtered cloud W its cells derive from ("resident"; uph_map_built_cloud reads it).  uph_map_set_cells,
 * uph_map_import_cells_dev, uph_map_load_cache, uph_map_fill_fbm and uph_map_commit end the residency: the cells then no longer derive from W.
 * uph_map_update: box = {x_min, x_max, y_min, y_max}, closed, compared in float.  The new resident cloud is
 *     W' = (W without the points whose (x, y) lie in the box, order kept) ++ cropAndVoxel(points of xyz that are finite and lie in the box, input order)
 * (crop box and 1 cm voxel grid of uph_map_build, applied to the new points alone; n = 0 with xyz = NULL removes only), and afterwards cells, c and both
 * occupancy layers equal uph_map_build_filtered(W') on a fresh map bit for bit.  Only the columns of uph_map_update_rect plus those whose last fit took
 * the global nearest-neighbour search are refitted -- unless the minimum x or y of W' differs from W's (the bucket origin moves): then every column is
 * (full_refit = 1, dirty = the whole grid).  Blocking, on the build's stream.  Refused with UPH_ERR_INVALID, cells, occupancy and W as they were: an
 * fp32 or tile map, no resident cloud, a reversed box or one with a NaN, n < 0, n > 0 with xyz = NULL, an update that would leave W' empty;
 * UPH_ERR_LIMIT: a disc of W' too dense for the staging window (as uph_map_build).  info may be NULL. */
typedef struct uph_map_update_info {
    int32_t dirty[4];     /* {x0, x1, y0, y1}, half-open column rect: uph_map_update_rect's, or the whole grid on a full refit */
    int32_t changed[4];   /* tight bounding rect (half-open) of the columns with a cell, c or occupancy byte that changed; zeros when none */
    int32_t n_refit;      /* columns refitted = area of dirty + n_far */
    int32_t n_far;        /* refitted columns OUTSIDE dirty: their last fit took the global nearest-neighbour search (0 on a full refit) */
    int32_t n_changed;    /* columns that changed */
    int32_t full_refit;
    int64_t n_removed, n_added, n_cloud;   /* points of W inside the box, filtered new points, size of W' */
} uph_map_update_info;
int uph_map_update(uph_map* m, const float box[4], const float* xyz, int64_t n, uph_map_update_info* info);
/* the columns whose fit can see a point of the box (host function: no device needed): column x belongs when
 *     box[0] - Rm <= (x + 0.5) res + origin_x <= box[1] + Rm     (in double; y alike),
 * Rm = (double)Rst + res, Rst = (float)(0.12 + max ellipsoid axis) + 1e-3f the fit's staging radius, origin = -map_size / 2, clipped to the grid.
 * rect = {x0, x1, y0, y1} half-open, all zeros when empty.  UPH_ERR_INVALID for a reversed box or one with a NaN. */
int uph_map_update_rect(const uph_map_params* mp, const float box[4], int32_t rect[4]);
/* stages of the last uph_map_update, milliseconds: out6 = upload of the new points, cloud edit + filter, bucketing + column list + LDS sizing,
 * fit kernel (HIP events), windowed commit, the whole call (wall) */
int uph_map_update_stages(uph_map* m, double* out6);
/* ---- several GPUs, one host process.  maps[g] = one map per device (same parameters and storage, whole-grid maps).  Device g produces the
 * x-slab [g per, min(nx, (g + 1) per)), per = ceil(nx / n_gpus), of the cell array -- all devices concurrently, one host thread each --, ONE
 * ncclAllGather over an in-process RCCL clique (ncclCommInitAll; in place on the cell arrays when n_gpus divides nx) leaves the complete array
 * on every device, every map commits.  Results are bit-identical to uph_map_build on one device.  RCCL is bound at first use (dlopen: an RCCL
 * the process already carries, else the system's); n_gpus = 1 needs none.  maps on the SAME device are accepted (single-GPU test
 * configuration: RCCL refuses a device twice, the slabs then move by device-to-device copies).  Blocking. */
int uph_map_build_multi(uph_map* const* maps, int32_t n_gpus, const float* xyz, int64_t n);
/* the host-side decisions of the two *_multi builds for a grid of nx rows over n_gpus devices, without a device (dry run of an 8-GPU node on
 * any box): x0[g], x1[g] = the x-slab device g fits (per = ceil(nx / n_gpus) rows; the last slabs shorter or empty), *in_place = 1 when the
 * all-gather runs in place on the cell arrays (n_gpus divides nx), 0 when it goes through zero-padded staging of n_gpus x per rows */
int uph_multi_slab_plan(int32_t nx, int32_t n_gpus, int32_t* x0, int32_t* x1, int32_t* per, int32_t* in_place);
/* the analytic terrain (uph_map_fill_fbm) sharded the same way; fp32 maps exchange float slabs */
int uph_map_fill_fbm_multi(uph_map* const* maps, int32_t n_gpus, const uph_fbm_params* fp);
/* wall milliseconds of the last *_multi call led by `lead` (= maps[0]): slab fits, slab exchange, commit; HIP-event milliseconds of the
 * all-gather on device 0's stream; via_rccl = 1 if the exchange was an RCCL collective */
int uph_map_multi_stats(uph_map* lead, double* fit_ms, double* exchange_ms, double* commit_ms, double* exchange_device_ms, int32_t* via_rccl);
/* diagnostic: binds RCCL the way the sharded build does, forms the in-process clique of devices 0 .. n_devices-1 and all-gathers a known
 * pattern; info (may be NULL) receives which librccl was bound and its version.  UPH_OK = the collective path works in this process */
int uph_rccl_selftest(int32_t n_devices, char* info, int32_t info_cap);
/* releases the cached RCCL cliques (optional; they live until process exit otherwise) */
void uph_multi_shutdown(void);

/* device pointer / byte size of the AoS cell array (ncell x 4 doubles) so that the host framework can all-gather
 * x-slabs across GPUs (RCCL) in place; call uph_map_commit afterwards to refresh c and occupancy */
int uph_map_cells_device(uph_map* m, void** dptr, int64_t* nbytes);
int uph_map_commit(uph_map* m);
/* sharded build helpers (device pointers owned by the caller, e.g. torch tensors used with torch.distributed / RCCL):
 * export the x-slab [x0,x1) of the AoS cell array (contiguous: x is the slowest index), import a full gathered array + commit */
int uph_map_export_slab_dev(uph_map* m, int32_t x0, int32_t x1, void* dst_dev);
int uph_map_import_cells_dev(uph_map* m, const void* src_dev);
/* device twin of UnevenMap::getAllWithGrad: pos n x 3 (x, y, yaw already wrapped to [-pi,pi]) -> values n x 7, grads n x 21 */
int uph_terrain_query(uph_map* m, const double* pos, int32_t n, double* values7, double* grads21);
/* batched front-end cost queries (what kino_astar.cpp:86,91,179,193 and kino_astar.h:263 ask per expanded state):
 * pos n x 3 (x, y, yaw) -> sigma[n] = UnevenMap::getTerrainSig (uneven_map.h:389-396, zeros outside the map),
 * occ[n] = isOccupancy(pos), occ_xy[n] = isOccupancyXY(pos) (uneven_map.h:471-498; -1 outside).  Any output may be NULL. */
int uph_frontend_query(uph_map* m, const double* pos, int32_t n, double* sigma, int32_t* occ, int32_t* occ_xy);
/* kernel milliseconds of the last uph_frontend_query (HIP events) */
/* batched UnevenMap::getTerrainPos (uneven_map.h:203-218) served from the device grid: pose12[n][12] = rotation matrix column-major
 * (x_b, y_b, z_b), then the position (x, y, interpolated z) */
int uph_terrain_pose_query(uph_map* m, const double* pos, int32_t n, double* pose12);
int uph_frontend_query_ms(uph_map* m, double* kernel_ms);
/* the cloud uph_map_build fits planes to: UnevenMap::init's pcl::CropBox [-10,10]^2 x [-0.01,5] followed by pcl::VoxelGrid with a 1 cm
 * leaf (uneven_map.cpp:133-143), applied to xyz (n points).  out_xyz takes at most cap points (NULL: count only); returns the
 * number of filtered points, < 0 on error.  Host function: no device needed. */
int64_t uph_map_filter_cloud(const float* xyz, int64_t n, float* out_xyz, int64_t cap);
/* last uph_map_build timing: kernel milliseconds (HIP events) and number of cell-iterations processed */
int uph_map_build_stats(uph_map* m, double* kernel_ms, int64_t* cell_iters, int64_t* cloud_points);
/* stages of the last uph_map_build, milliseconds: out6 = cloud upload, crop box + voxel filter, bucketing + LDS sizing (all three on the device: the
 * host only launches), plane-fit kernel (HIP events), commit (c, occupancy), the whole call (wall) */
int uph_map_build_stages(uph_map* m, double* out6);
/* test hook: the cloud the last uph_map_build fitted planes to, as the DEVICE filtered it (must equal uph_map_filter_cloud, the host form, bit for bit);
 * at most cap points into out_xyz (NULL: count only); returns the count, < 0 on error */
int64_t uph_map_built_cloud(uph_map* m, float* out_xyz, int64_t cap);

/* ---- front end: KinoAstar::plan for a batch of queries, one wave64 per query (csrc/kino_search.hip).
 * uph_kino_create = KinoAstar::init + setEnvironment (kino_astar.cpp:5-43, kino_astar.h:170-178): parameters, the Dubins radius wheel_base / tan(max_steer),
 * a node pool of getXYNum() nodes per concurrent query.  slots = number of queries searched concurrently (each owns ~3.7 MB of HBM at 200 x 200 cells);
 * when the device cannot hold that many, as many as fit (uph_kino_slots tells).  slots = 0: automatic -- the workspaces follow the batches that
 * arrive (allocated by the first uph_kino_plan_batch for its B, at least 16; grown when a larger batch comes), up to one per wave slot of the default
 * kernel instantiation (16 per compute unit) and never beyond half of the HBM that was free at creation: a single plan() costs ~60 MB, not 16 GB.
 * UPH_ERR_LIMIT when the grid has more than 2^31 columns or (cells + 1) x yaw bins of the lattice does not fit 32-bit keys, or when not even one
 * workspace fits.  The map must stay alive and must not be rebuilt while a search runs. */
int uph_kino_create(uph_map* m, const uph_kino_params* kp, int32_t slots, uph_kino** out);
void uph_kino_destroy(uph_kino* k);
int uph_kino_slots(const uph_kino* k);           /* workspaces allocated (automatic context before its first search: the upper bound) */
/* experiment knob: waves per SIMD the search kernel is compiled for -- 2, 4 (default), 6 or 8 (register caps 256 / 128 / 80 / 64) */
int uph_kino_set_wps(uph_kino* k, int32_t wps);
/* experiment knob: bit 0 = queries handed out dynamically, longest first (default on); bit 1 = sincosFast instead of the device library's sin / cos (default on) */
int uph_kino_set_flags(uph_kino* k, int32_t flags);
int uph_kino_primitives(const uph_kino* k);   /* motion primitives per expansion produced by the reference's loops (kino_astar.cpp:138-145): 15 */
/* starts / goals [B][3] = (x, y, yaw): plan(start_state, end_state) per query.  paths [B][path_cap][3] receives front_end_path (the poses of the
 * node chain, then the Dubins shot samples, kino_astar.h:273-292), n_path[B] its length (may exceed path_cap: truncated), status[B] UPH_KINO_*;
 * iter_num / use_node_num [B] (may be NULL) the reference's counters.  max_expand > 0 stops a query after that many expansions (test hook).
 * expanded (may be NULL with exp_cap = 0): [B][exp_cap][3] lattice index (ix, iy, iyaw) of every expanded node in order.  Blocking. */
int uph_kino_plan_batch(uph_kino* k, int32_t B, const double* starts, const double* goals, int32_t path_cap, double* paths, int32_t* n_path, int32_t* status,
                        int32_t* iter_num, int32_t* use_node_num, int32_t max_expand, int32_t exp_cap, int32_t* expanded);
/* kernel milliseconds (HIP events) of the last uph_kino_plan_batch */
int uph_kino_stats(uph_kino* k, double* kernel_ms);

/* ---- goals -> resident trajectories in one call: PlanManager::rcvWpsCallBack (plan_manager.cpp:43-134) for a batch of goals with every stage on the device.
 * The search of uph_kino_plan_batch (kino_astar->plan, :59-60) runs into device memory; a path longer than path_cap (0: UPH_PLAN_PATH_CAP) is searched
 * again with room for all its poses, so no clipped path is resampled; the stage of uph_resample_batch (:62-132, or the test node's with mp->test_mode,
 * alm_traj_opt.cpp:73-144) runs on the device over the paths where the search left them, bit for bit the host routine's results (the boundary
 * velocities sig_vel * cos / sin of the end headings, :94-95, are formed on the host); only a header per goal crosses PCIe; the problems are uploaded
 * to c as uph_batch_upload uploads them (same limits: a problem beyond UPH_MAX_PIECE_* keeps its slot as UPH_RET_UNSUPPORTED).  k and c must be bound
 * to the same map.  The resident batch = the goals whose search succeeded, in goal order; uph_batch_origin returns each one's goal index.
 * Outputs [B]: status = UPH_KINO_*, traj_of = the goal's index in the resident batch or -1, n_inner_xy / n_inner_yaw = its way-point counts (0 for a
 * goal without a path): what sizes the uph_result arrays of uph_batch_download.  Then uph_batch_solve / _solve_async / _wait / _download,
 * uph_report_batch and uph_rollout_* work as after uph_batch_upload.  The four outputs are written together, once every search and the resampling
 * have run; a return before that point (bad arguments, contexts on different maps, a pending asynchronous solve, a HIP failure) leaves them
 * untouched.  No goal produced a path: UPH_ERR_INVALID WITH the outputs written and no status[b] == UPH_KINO_OK, the context holding no batch -- the
 * only UPH_ERR_INVALID with written outputs that has no UPH_KINO_OK in them (pre-fill status with a value that is no UPH_KINO_* code, e.g. -1,
 * to tell it apart).  A found path of fewer than two poses (not produced by the search) keeps its slot as UPH_RET_UNSUPPORTED with
 * last_lbfgs_ret UPH_ERR_INVALID, where uph_resample_batch refuses its whole batch.  Blocking. */
#define UPH_PLAN_PATH_CAP 1024
int uph_plan_upload(uph_kino* k, uph_ctx* c, const uph_manager_params* mp, int32_t B, const double* starts, const double* goals, int32_t path_cap,
                    int32_t* status, int32_t* traj_of, int32_t* n_inner_xy, int32_t* n_inner_yaw);
/* ---- re-plan from states on resident trajectories: uph_plan_upload for a vehicle that follows trajectory src_traj[q] of src's resident batch and
 * switches to a new plan at t_switch[q] (seconds from that trajectory's start, the clock of uph_rollout_batch; t <= 0 is the start, t >= its duration
 * the end, the duration as the rollout forms it).  The switch state (x, y in map coordinates, dx, dy, ddx, ddy, normSO2(yaw), dyaw, ddyaw) is
 * evaluated on the device from src's coefficients, as the rollout evaluates its rows; the search runs from (x, y, yaw) to goals[q] (NULL: the
 * source problem's end pose -- end position, normSO2 of its end yaw: "the map changed, same goal"); the resampling is uph_plan_upload's; the problem's
 * start boundary is init_xy = {x, y, dx, dy, ddx, ddy} and init_yaw = {yaw of the path's first pose, dyaw, ddyaw} (the yaw way-points unwrap from
 * that pose as in PlanManager), its end boundary, way-points and total_time uph_plan_upload's.  Upload, admission, uph_batch_origin (= the query
 * index), uph_plan_staged and the four outputs [B] follow uph_plan_upload, into dst; switch_states [B][9] (or NULL) is written together with them.
 * dst == src is allowed (every state is taken before dst is reset).  Refused with UPH_ERR_INVALID, outputs untouched and dst's batch as it was:
 * bad arguments, src holding no resident trajectory (uph_rollout_batch's rule), an src_traj[q] out of range or naming an UPH_RET_UNSUPPORTED slot,
 * a non-finite t_switch[q], k / src / dst bound to different maps, an asynchronous solve pending on src or dst.  Blocking. */
int uph_replan_upload(uph_kino* k, uph_ctx* src, uph_ctx* dst, const uph_manager_params* mp, int32_t B, const int32_t* src_traj, const double* t_switch,
                      const double* goals, int32_t path_cap, double* switch_states, int32_t* status, int32_t* traj_of, int32_t* n_inner_xy, int32_t* n_inner_yaw);
/* ---- resident trajectories at given times: row q of out10 [n][10] is trajectory traj[q] of c's resident batch at t[q] seconds from its start, clamped
 * to [0, duration] (the duration as uph_rollout_batch forms it: running sums of the piece durations, the smaller of the two).  Columns 0-8 are
 * uph_replan_upload's switch-state columns -- x, y (map coordinates), dx, dy, ddx, ddy, normSO2(yaw), dyaw, ddyaw -- and column 9 is the raw
 * (unwrapped) yaw.  At a rollout row's t, columns 0-7 equal that row bit for bit.  Refused with UPH_ERR_INVALID, out10 untouched: bad arguments, no
 * resident trajectory (uph_rollout_batch's rule), a traj[q] out of range or naming an UPH_RET_UNSUPPORTED slot, a non-finite t[q], an asynchronous
 * solve pending on c.  Blocking. */
int uph_traj_states(uph_ctx* c, int32_t n, const int32_t* traj, const double* t, double* out10);
/* ---- refine resident trajectories from a switch time without a new search: query q continues trajectory b = src_traj[q] of src's resident batch
 * from its state at tc = t_switch[q] clamped to [0, D] (D: the duration as above) to the end boundary of b's problem as it was uploaded, with the
 * rest of b as the initial guess.  With R = D - tc and b's piece durations T_xy / T_yaw: N' = max(1, nearbyint(R / T_xy)) position pieces and
 * M' = max(N', nearbyint(R / T_yaw)) yaw pieces (tc = 0 gives back b's counts); the xy way-points are b's (x, y) at tc + k (R / N'), k = 1 .. N' - 1,
 * the yaw way-points its raw yaw at tc + k (R / M'), k = 1 .. M' - 1 (the times formed without contraction, the values those of uph_traj_states at
 * the same times bit for bit); init_xy = {x, y, dx, dy, ddx, ddy} and init_yaw = {raw yaw, dyaw, ddyaw} of the state at tc; end_xy / end_yaw b's
 * uploaded end boundary; total_time = R.  R <= 0: status[q] = UPH_REFINE_AT_END and nothing is uploaded for q.  The other queries are uploaded to
 * dst in query order as uph_plan_upload uploads its goals (same admission and local frames; uph_batch_origin = the query index; uph_plan_staged).
 * Outputs [B]: status (UPH_KINO_OK or UPH_REFINE_AT_END), traj_of, n_inner_xy, n_inner_yaw, and switch_states [B][10] (may be NULL: uph_traj_states'
 * columns at tc), written together once the device work has run.  No query left to refine: UPH_ERR_INVALID WITH the outputs written, dst holding
 * no batch.  dst == src is allowed.  Refused with UPH_ERR_INVALID, outputs untouched and dst's batch as it was: bad arguments, src holding no resident
 * trajectory, an src_traj[q] out of range or naming an UPH_RET_UNSUPPORTED slot, a non-finite t_switch[q] or piece duration of b, src / dst bound to
 * different maps, an asynchronous solve pending on src or dst.  Blocking. */
#define UPH_REFINE_AT_END 7     /* t_switch at or past the end: nothing left to refine (not uploaded) */
int uph_refine_upload(uph_ctx* src, uph_ctx* dst, int32_t B, const int32_t* src_traj, const double* t_switch, double* switch_states /* B x 10, may be NULL */,
                      int32_t* status, int32_t* traj_of, int32_t* n_inner_xy, int32_t* n_inner_yaw);
/* test hook: the resident problems of a batch uploaded by uph_plan_upload exactly as the device staged them, in uph_resample_batch's output layout
 * and the resident order (boundary velocities included).  UPH_ERR_LIMIT when a problem has more way-points than cap_xy / cap_yaw or than the staging
 * holds (UPH_MAX_PIECE_* - 1; the counts are still written); UPH_ERR_INVALID when the resident batch did not come from uph_plan_upload or
 * uph_replan_upload. */
int uph_plan_staged(uph_ctx* c, int32_t cap_xy, int32_t cap_yaw, double* init_xy, double* end_xy, double* init_yaw, double* end_yaw, double* inner_xy,
                    double* inner_yaw, int32_t* n_inner_xy, int32_t* n_inner_yaw, double* total_time);

/* ---- optimiser */
int uph_ctx_create(uph_map* m, const uph_opt_params* p, uph_ctx** out);
void uph_ctx_destroy(uph_ctx* c);
/* rho is a member that persists across solves in the reference (alm_traj_opt.cpp:16, alm_traj_opt.h:137): every problem of a
 * batch starts from the context's rho.  After a solve of ONE problem the context's rho is that problem's final rho (the reference's
 * behaviour over consecutive calls); a batch of B > 1 independent problems leaves it unchanged (each result carries its rho_final). */
/* lanes of one workgroup that cooperate on ONE trajectory: 64, 128, 256 or 512 (one, two, four or eight wave64); 0 = automatic (default):
 * 128 lanes with up to four workgroups per CU from 2304 problems (throughput), 256 lanes below, 512 lanes up to 256 problems (latency).  Takes effect at the next
 * upload.  Results do not depend on the choice beyond the summation order of the block reductions. */
int uph_ctx_set_lanes(uph_ctx* c, int32_t lanes);
/* experiment knob (takes effect at the next upload): group >= 16 permutes the launch order inside groups of `group` workgroups of similar predicted
 * cost so that the workgroups dispatched to one XCD (workgroup index mod 8) work in one octant of the map (per-XCD L2 locality); 0 = off (default).
 * Placement never changes results. */
int uph_ctx_set_xcd_locality(uph_ctx* c, int32_t group);
/* experiment knob: 2 = register-capped kernel build (two waves per SIMD), 1 = uncapped, 0 = choose from the batch size */
int uph_ctx_set_wps(uph_ctx* c, int32_t wps);
/* BASELINE.json configs[4] "fp32": bits = 32 makes the sample phase of the objective (polynomial evaluation, terrain lookup, penalties and
 * their chain rule: alm_traj_opt.cpp:716-988) compute in fp32 -- MINCO, the gradient reduction, L-BFGS and ALM stay fp64.  The reference is
 * double-only: results are then NOT comparable at 1e-9, only through cost / feasibility statistics (tests/test_gpu_km2.py).  64 = default.
 * Applies to the solve and evaluation kernels of 128 / 256 / 512 lanes (every automatic selection); a forced 64-lane context stays fp64. */
int uph_ctx_set_sample_precision(uph_ctx* c, int32_t bits);
int uph_ctx_set_rho(uph_ctx* c, double rho);
int uph_ctx_get_rho(uph_ctx* c, double* rho);
/* on = 1 (default): a line-search trial stops as soon as its rejection by the Armijo test is certain and no exit of the search can follow it --
 * before its first constraint sample when a lower bound of the cost already exceeds the threshold, or before the adjoint once the cost is known.
 * Results are the same bit for bit with on = 0 (every trial evaluated in full), except on a map with cells that make a sample non-finite: there a
 * trial abandoned before that sample is bisected where the reference returns LBFGSERR_INVALID_FUNCVAL. */
int uph_ctx_set_trial_abandon(uph_ctx* c, int32_t on);

/* diagnostic: keep the first `cap` entries of each trajectory's cost trace of the next solves (cost after every accepted
 * L-BFGS iteration, -1 at the start of an ALM pass); cap = 0 switches it off.  uph_ctx_get_trace: out[B][cap]. */
int uph_ctx_set_trace(uph_ctx* c, int32_t cap);
int uph_ctx_get_trace(uph_ctx* c, double* out);

/* blocking: upload + solve + download.  B = 1 is one ALMTrajOpt::optimizeSE2Traj call.  A problem outside the compiled limits does not fail
 * the batch: its result carries ret_code UPH_RET_UNSUPPORTED and the others are solved; only a batch without any supported problem
 * returns UPH_ERR_INVALID / UPH_ERR_LIMIT. */
int uph_optimize_batch(uph_ctx* c, int32_t B, const uph_problem* probs, uph_result* results);
/* the same call over several GPUs of this process: ctxs[g] = one context per device (each bound to its device's copy of the map, e.g. from
 * uph_map_build_multi).  The problems are dealt to the contexts in descending predicted cost, round-robin; one host thread per device runs
 * upload -> solve -> download on its share; results[] comes back in the caller's order.  No collective: trajectories are independent.
 * Contexts on the same device are accepted (test configuration).  n_gpus = 1 is uph_optimize_batch. */
int uph_optimize_batch_multi(uph_ctx* const* ctxs, int32_t n_gpus, int32_t B, const uph_problem* probs, uph_result* results);
/* the split uph_optimize_batch_multi makes, without a device: share_of[b] = index of the context problem b is dealt to (descending predicted
 * cost, round-robin); predicted_cost (may be NULL) [B] = the a-priori cost the split and every upload's launch order sort by */
int uph_multi_batch_plan(int32_t n_gpus, int32_t B, const uph_problem* probs, int32_t* share_of, double* predicted_cost);
/* number of problems of the uploaded batch (0: none) */
int uph_batch_count(const uph_ctx* c);
/* after uph_optimize_batch_multi every context holds ITS SHARE of the batch (uph_batch_count problems, in share order): idx[k] = the caller's index
 * of problem k of this context -- what maps the rows of uph_report_batch / uph_batch_cycles of a context back to the caller's problems.  Identity
 * after uph_batch_upload / uph_optimize_batch; after uph_plan_upload the goal index of each resident problem. */
int uph_batch_origin(const uph_ctx* c, int32_t* idx);
/* split form (inputs resident in HBM before the timed region): upload -> solve (kernel only, blocking) -> download */
int uph_batch_upload(uph_ctx* c, int32_t B, const uph_problem* probs);
int uph_batch_solve(uph_ctx* c);
/* the same solve split into enqueue and completion: uph_batch_solve_async returns after queuing the two kernels on the context's own HIP
 * stream, uph_batch_wait blocks until they are done and collects the statistics (uph_batch_solve = the two back to back).  Contexts are
 * independent, so two of them driven alternately keep the GPU full across batch boundaries (the tail of one launch overlaps the head of
 * the next).  One asynchronous solve per context at a time; upload / download / hooks require a waited context. */
int uph_batch_solve_async(uph_ctx* c);
int uph_batch_wait(uph_ctx* c);
int uph_batch_download(uph_ctx* c, uph_result* results);
/* timing / work counters of the last uph_batch_solve: kernel ms (HIP events on the context's stream), total objective
 * evaluations, total constraint-sample evaluations, total L-BFGS iterations, bytes streamed from the L-BFGS history */
int uph_batch_stats(uph_ctx* c, double* kernel_ms, int64_t* evals, int64_t* sample_evals, int64_t* lbfgs_iters, int64_t* hist_bytes);
/* line-search trial counters of the last solve, summed over the batch: out5 = trials rejected by the Armijo test; of those, trials that an exit of the
 * search could follow (always evaluated in full); trials abandoned before their first sample; sample chunks those did not run; adjoints not run.
 * sample_evals of uph_batch_stats counts the samples actually evaluated. */
int uph_batch_abandon_stats(uph_ctx* c, int64_t* out5);

/* uph_batch_solve = two launches: reset+initScaling, then the ALM/L-BFGS solve kernel (uph_batch_stats reports the latter);
 * this returns the kernel milliseconds of the former */
int uph_batch_prepare_ms(uph_ctx* c, double* ms);

/* diagnostic: shader-clock cycles per phase of the last uph_batch_solve, out[B][16]:
 * 0 MINCO generate, 1 constraint samples, 2 per-piece scatter, 3 adjoint, 4 L-BFGS two-loop, 5 initScaling, 6 whole solve.
 * All zero in the shipped library: the in-kernel timers are compiled out (they cost 1.7 % of a solve launch); build with -DUPH_CYC=1 for them
 * (tools/build_variants.sh cyc="-DUPH_CYC=1"). */
int uph_batch_cycles(uph_ctx* c, long long* out);

/* test / bench hooks on the uploaded batch (state = duals, scales, rho as currently resident):
 * one innerCallback evaluation at x (packed [sum n]); outputs f[B], grad (packed), and refreshes hx/gx/c on the device.
 * `repeat` >= 1 re-runs the same evaluation that many times inside one launch per trajectory (roofline measurement). */
int uph_eval_batch(uph_ctx* c, const double* x_packed, double* f, double* grad_packed, int32_t repeat);
/* A5 ALONE -- ALMTrajOpt::calConstrainCostGrad (back_end/src/alm_traj_opt.cpp:663-991) and nothing else of innerCallback: the coefficients and piece
 * durations RESIDENT on the device (those of the last uph_eval_batch / solve of this batch), the resident duals, scales, rho and scale_fx in ->
 * cost[B], gdCxy (packed [sum 12 Nxy]: per trajectory the reference's 6 Nxy x 2 block, row 6 i + k, row-major), gdCyaw (packed [sum 6 Nyaw]),
 * gdT2[B][2] = (sum_i gdTxy(i), sum_i gdTyaw(i)) -- the pieces share one duration (alm_traj_opt.h:257-261), only the sums enter the gradient
 * (alm_traj_opt.cpp:341-344) -- out.  store_residuals != 0: hx / gx are written by every call as the reference's function writes them (:835, 846 ...;
 * read them with uph_batch_download).  `repeat` >= 1 calls inside one launch per trajectory: this is SURVEY.md 8d's "penalty kernel" measured as
 * north_star defines it (bench.py roofline.penalty_kernel.frac_a5_only).  Any output pointer may be NULL. */
int uph_penalty_batch(uph_ctx* c, int32_t repeat, int32_t store_residuals, double* cost, double* gdcxy_packed, double* gdcyaw_packed, double* gdT2);
int uph_init_scaling_batch(uph_ctx* c);
/* diagnostic: measures the workgroup primitives (barrier, reductions, dependent global load, ...) on the uploaded batch;
 * per-trajectory results via uph_batch_cycles (a -DUPH_CYC=1 build) */
int uph_microbench_batch(uph_ctx* c, int32_t reps);
/* overwrite resident duals / scales (packed in the reference's order; any pointer may be NULL) */
int uph_batch_set_state(uph_ctx* c, const double* lambda, const double* mu, const double* scale_cx, const double* scale_fx, const double* rho);
/* ---- test hooks of the teacher-forced late-state tests (tests/test_gpu_forced.py): drive the device state machine from a state the
 * CPU oracle dumped, one L-BFGS iteration / one ALM pass at a time */
/* overwrite the resident x (packed like x_final) */
int uph_batch_set_x(uph_ctx* c, const double* x_packed);
/* the ALM loop of optimizeSE2Traj (alm_traj_opt.cpp:234-271) from the RESIDENT x, duals, scales and rho -- no reset, no initScaling --
 * for at most max_passes passes (0 = until it ends); a solve stopped by the cap reports ret_code 3 */
int uph_batch_alm_passes(uph_ctx* c, int32_t max_passes);
/* L-BFGS state at the top of the iteration loop (lbfgs.hpp:555): g, d packed like x; pf [B][UPH_MAX_PAST]; the history as the
 * reference holds it (lm_s / lm_y column j of trajectory b at off_b + j*n, off_b = mem * sum of the n before b; lm_ys [B][mem]);
 * scal5 [B][5] = step, fx, k, end, bound */
int uph_batch_set_lbfgs_state(uph_ctx* c, const double* g, const double* d, const double* pf, const double* lm_s, const double* lm_y, const double* lm_ys, const double* scal5);
/* continue from that state for at most `budget` iterations (< 0: until the loop ends); finish_pass: then react as the ALM loop does */
int uph_batch_lbfgs_resume(uph_ctx* c, int32_t budget, int32_t finish_pass);
/* state afterwards; scal8 [B][8] = step, fx, k, end, bound, L-BFGS code (999 = budget ran out), accepted, converged */
int uph_batch_get_lbfgs_state(uph_ctx* c, double* g, double* d, double* pf, double* lm_s, double* lm_y, double* lm_ys, double* scal8);
/* post-solve feasibility report per trajectory: out[B][7] = max vx, ax, ay, cur, att(-cos xi), sigma, non-holonomic error; B = uph_batch_count */
int uph_report_batch(uph_ctx* c, double* out7);

/* ---- trajectory rollout: the resident batch (coefficients and piece durations of the last solve / evaluation, what uph_report_batch reads)
 * sampled on the device.  Sample q of a trajectory sits at t_q = the value after q additions of dt to 0.0 (the reference's running sum
 * `for (t = 0; t < total; t += dt)`, not q * dt); a trajectory has the first q with t_q >= total samples, total = min(Nxy x T_xy, Nyaw x T_yaw)
 * as running sums piece by piece; with_end != 0 appends one row at t = total (visSE3Traj's closing pose).  Columns per row, in this order,
 * only the groups selected by `channels`: */
#define UPH_ROLLOUT_STATE 1     /* 9:  t, x, y, yaw (normSO2, as getNormSE2Pos), dx, dy, ddx, ddy, dyaw                                         */
#define UPH_ROLLOUT_TERRAIN 2   /* 7:  vx, ax, ay, cur, att (-1 / cos xi), sigma, non-holonomic error: the terms uph_report_batch reduces       */
#define UPH_ROLLOUT_POSE 4      /* 12: UnevenMap::getTerrainPos at (x, y, yaw), the layout of uph_terrain_pose_query (R column-major, then p)   */
#define UPH_ROLLOUT_ALL 7
#define UPH_ROLLOUT_MAX_SAMPLES 262144   /* samples of one trajectory (>= the 200 000 of the report's own loop)                      */
/* host only, no device needed: offsets[B + 1] = exclusive prefix sum of the row counts of B trajectories of n_xy[b] pieces of T_xy[b] and
 * n_yaw[b] pieces of T_yaw[b].  UPH_ERR_INVALID for dt <= 0 / not finite, a negative piece count or a null pointer; UPH_ERR_LIMIT when a
 * trajectory needs more than UPH_ROLLOUT_MAX_SAMPLES samples (or the running sum stops growing before it reaches the total). */
int uph_rollout_sizes(int32_t B, const int32_t* n_xy, const double* T_xy, const int32_t* n_yaw, const double* T_yaw, double dt, int32_t with_end,
                      int64_t* offsets);
/* the same for the resident batch of c (B = uph_batch_count): what uph_rollout_batch writes.  A problem with ret_code UPH_RET_UNSUPPORTED has
 * no rows.  UPH_ERR_INVALID when no trajectory is resident (after uph_batch_upload and before a solve / uph_eval_batch). */
int uph_rollout_plan(uph_ctx* c, double dt, int32_t with_end, int64_t* offsets);
/* rows of trajectories [b0, b1) of the resident batch, row-major [row][column], positions in map coordinates (as uph_batch_download's):
 * out holds offsets[b1] - offsets[b0] rows.  Staged through a bounded device buffer (a few hundred MB) in chunks of trajectories. */
int uph_rollout_batch(uph_ctx* c, double dt, int32_t with_end, int32_t channels, int32_t b0, int32_t b1, double* out);
/* the same rows written straight into device memory of the context's device (e.g. a torch tensor's data_ptr()), on the context's stream;
 * returns after the stream has synchronised */
int uph_rollout_batch_dev(uph_ctx* c, double dt, int32_t with_end, int32_t channels, int32_t b0, int32_t b1, void* out_dev);

/* ---- check resident trajectories against the map as it is now: query q reduces the samples of trajectory traj[q] of c's resident batch whose t lies in
 * [t_from[q], t_to[q]] (t_from <= t and t <= t_to, literally; t_to == NULL: to the end).  The samples are exactly the rows uph_rollout_batch(dt, with_end)
 * has for that trajectory -- same time table, same evaluation, the end row at t = total included when with_end is set.  Per sample a mask: bit k
 * (k = 0..6, the UPH_ROLLOUT_TERRAIN columns vx, ax, ay, cur, att, sigma, non-holonomic error) is set when !(fabs(v) <= lim7[k]) for k < 4 and when
 * !(v <= lim7[k]) for k >= 4, so a NaN term violates; bit UPH_CHECK_OCC_BIT is set when the map's occupancy at the row's (x, y, yaw) -- what
 * uph_frontend_query returns as occ -- is not 0 (-1, outside the map, counts as occupied).  Outputs per query, any of them may be NULL:
 *   first_t [n]      t of the first sample with a non-zero mask (NaN: none), first_mask [n] its mask (0: none)
 *   counts  [n][3]   samples in the window, samples with a non-zero mask, samples with the occupancy bit
 *   worst   [n][7]   per term the largest fabs(v) (k < 4) or v (k >= 4) over the window; a non-finite term counts as +inf; -inf for an empty window
 *   worst_t [n][7]   t of the sample that set worst[k], the earliest one among equals (NaN for an empty window)
 * lim7 == NULL: uph_check_limits(c).  The same trajectory may be named by several queries.  Deterministic: no floating-point atomics, a selection whose
 * result does not depend on the order of the reduction.  Blocking, on the context's stream.  Refused with UPH_ERR_INVALID, outputs untouched: bad
 * arguments, dt <= 0 or not finite, no resident trajectory (uph_rollout_batch's rule), a traj[q] out of range or naming an UPH_RET_UNSUPPORTED slot, a
 * non-finite t_from[q], a NaN t_to[q] (+-inf is allowed), an asynchronous solve pending on c.  UPH_ERR_LIMIT as uph_rollout_plan. */
#define UPH_CHECK_OCC_BIT 7
/* host only: lim7 = { max_vel, max_acc_lon, max_acc_lat, max_kap, -min_cxi, max_sig, +inf } of the context's uph_opt_params */
int uph_check_limits(const uph_ctx* c, double* lim7);
/* host only, no device needed: the samples of a trajectory of duration `total` that the window [t_from, t_to] holds -- table samples [q_lo, q_hi) of the
 * running sum t += dt, and end_row != 0 when with_end is set and the end row (t = total) lies in the window.  UPH_ERR_INVALID for dt <= 0 / not finite,
 * a NaN bound or a null pointer; UPH_ERR_LIMIT as uph_rollout_sizes. */
int uph_check_window(double dt, int32_t with_end, double total, double t_from, double t_to, int32_t* q_lo, int32_t* q_hi, int32_t* end_row);
int uph_check_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t_from, const double* t_to /* NULL: to the end */, double dt, int32_t with_end,
                    const double* lim7 /* NULL: defaults */, double* first_t /* [n], NaN: none */, int32_t* first_mask /* [n] */,
                    int32_t* counts /* [n][3]: samples, violating, occupied */, double* worst /* [n][7] */, double* worst_t /* [n][7] */);
/* milliseconds of uph_check_kernel in the last uph_check_batch of c (events on the context's stream) */
int uph_check_kernel_ms(const uph_ctx* c, double* kernel_ms);

/* ---- locate poses on resident trajectories, and find where resident trajectories cross a rect.  Both reduce the STATE samples of (trajectory, time
 * window) pairs of c's resident batch: query q names trajectory traj[q] and the window [t_from[q], t_to[q]] (t_to == NULL: to the end), and its samples
 * tau_0 .. tau_{n-1} are, in table order, exactly the rows uph_rollout_batch(dt, with_end) has for that trajectory inside the window (uph_check_batch's
 * rule, uph_check_window).  X, Y below are a STATE row's x, y: map coordinates.  No terrain is read.
 *
 * uph_locate_batch: poses [n][3] = x, y, yaw in map coordinates.
 *   coarse stage (exact): d2 = ex ex + ey ey with ex = X - x, ey = Y - y and both products rounded before the add.  The smallest d2 wins, a NaN d2
 *   counts as +inf, equal keys go to the smaller sample index j*.   near_t [n] = tau_j*,  near_d2 [n],  count [n] = samples in the window.
 *   refinement (continuous): bracket lo = tau_max(j*-1, 0), hi = tau_min(j*+1, n-1).  With e = p(t) + shift - (x, y), g(t) = e . v and
 *   h(t) = v . v + e . a: start at t = tau_j* with [a, b] = [lo, hi]; at most 8 iterations of -- evaluate at t; g > 0: b = t, g < 0: a = t, g == 0: stop;
 *   the next t is t - g / h when h > 0 and that point lies in [a, b], else (a + b) / 2; stop when the next t equals t.  The state at the candidate and
 *   its d2 (as above) are evaluated; !(d2 <= near_d2): the result is the coarse sample itself and refined = 0, otherwise the candidate and refined = 1.
 *   t [n], refined [n], d2 [n];  state [n][10] in uph_traj_states' columns, equal to uph_traj_states(traj, t) bit for bit;
 *   err [n][3] = e_lon, e_lat, e_yaw: with psi the raw yaw of the state (column 9) and r = (x, y) - (X, Y):  r . (cos psi, sin psi),
 *   r . (-sin psi, cos psi),  normSO2(yaw - psi).
 *   An empty window: count 0, near_t = t = NaN, near_d2 = d2 = +inf, refined 0, state and err NaN.
 * uph_within_batch: rects [n][4] = x0, x1, y0, y1 in map coordinates, closed.  A sample is inside when x0 <= X && X <= x1 && y0 <= Y && Y <= y1 (a NaN
 *   position is not inside; a reversed rect is empty, not an error).   enter_t [n] / leave_t [n] = t of the first / last sample inside (NaN: none),
 *   counts [n][2] = samples in the window, samples inside.
 * Any output may be NULL.  The same trajectory may be named by several queries.  Deterministic: selections under a total order, no floating-point
 * atomics; the result does not depend on how lanes and waves are combined.  Blocking, on the context's stream.  Refused with UPH_ERR_INVALID, outputs
 * untouched: bad arguments, dt <= 0 or not finite, no resident trajectory (uph_rollout_batch's rule), a traj[q] out of range or naming an
 * UPH_RET_UNSUPPORTED slot, a non-finite t_from[q], a NaN t_to[q] (+-inf is allowed), a non-finite pose component, a NaN rect bound (+-inf is allowed),
 * an asynchronous solve pending on c.  UPH_ERR_LIMIT as uph_rollout_plan. */
int uph_locate_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* poses /* [n][3] */, const double* t_from, const double* t_to /* NULL: to the end */,
                     double dt, int32_t with_end, double* near_t /* [n] */, double* near_d2 /* [n] */, int32_t* count /* [n] */, double* t /* [n] */,
                     int32_t* refined /* [n] */, double* state /* [n][10] */, double* d2 /* [n] */, double* err /* [n][3]: e_lon, e_lat, e_yaw */);
int uph_within_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* rects /* [n][4] */, const double* t_from, const double* t_to /* NULL: to the end */,
                     double dt, int32_t with_end, double* enter_t /* [n], NaN: none */, double* leave_t /* [n] */, int32_t* counts /* [n][2]: samples, inside */);
/* milliseconds of the kernel(s) of the last uph_locate_batch or uph_within_batch of c, whichever came last (events on the context's stream) */
int uph_locate_kernel_ms(const uph_ctx* c, double* kernel_ms);

/* ---- resident trajectories against each other on a common clock.  Every resident trajectory counts time from its own start; a vehicle here is a trajectory
 * and the time t0 on the common clock at which it starts.
 *   sample times   a query has a window [t_from, t_to] on the common clock (both finite) and a step dt > 0 (finite).  Sample k sits at
 *                  tau_k = t_from + k * dt -- the product rounded, then the sum rounded, never one fused operation.  K = the number of k >= 0 with tau_k <= t_to
 *                  (0 when t_to < t_from).  The rollout's additive time table is not used.  A query with K > 2^22 is refused with UPH_ERR_LIMIT.
 *   a vehicle at tau   its own time is u = tau - t0 (one rounded subtraction), clamped as uph_traj_states clamps it (u <= 0: 0, u >= total: total); its position
 *                  X, Y is columns 0 and 1 of uph_traj_states(traj, u), bit for bit.  Before t0 it stands at its start, after its end at its goal.
 *   separation     d2 = ex ex + ey ey with ex = X_a - X_b, ey = Y_a - Y_b and both products rounded before the add (uph_locate_batch's d2).  A sample is
 *                  BELOW when d2 < R2, strictly, R2 = R * R rounded; a NaN d2 is never below.  For the minimum a NaN d2 reads +inf and the smaller k wins
 *                  among equals.
 *   extent         (xmin, xmax, ymin, ymax) over the samples whose X and Y are both not NaN; (+inf, -inf, +inf, -inf) when there is none.
 *   candidates     the pair (i, j), i < j, of boxes box_i, box_j with radii r_i, r_j has R = r_i + r_j (one rounded add) and is DROPPED iff
 *                  xmin_i - xmax_j > R || xmin_j - xmax_i > R || ymin_i - ymax_j > R || ymin_j - ymax_i > R.  Rounding is monotone and `below` is strict, so a
 *                  dropped pair has d2 >= R2 at every sample of the window its boxes were taken over: the pruning loses nothing and needs no epsilon.
 * Deterministic as uph_locate_batch: selections under a total order and integer sums.  The device calls are blocking, on the (first) context's stream; any
 * output may be NULL; every refusal leaves the outputs untouched: UPH_ERR_INVALID for bad arguments, dt <= 0 or not finite, a non-finite window bound or start
 * time, a negative or non-finite radius, no resident trajectory, a trajectory index out of range or naming an UPH_RET_UNSUPPORTED slot, an asynchronous solve
 * pending; UPH_ERR_LIMIT for K > 2^22. */
/* host only, no device needed: K of the window by the rule above */
int uph_separation_times(double t_from, double t_to, double dt, int64_t* K);
/* query q: the extent of vehicle (traj[q], t0[q]) of c's resident batch over the window [t_from[q], t_to[q]] */
int uph_extent_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* t_from, const double* t_to, double dt,
                     double* box /* [n][4]: xmin, xmax, ymin, ymax */, int32_t* counts /* [n][2]: samples, NaN samples */);
/* query q: vehicle (traj_a[q], t0_a[q]) of ca against vehicle (traj_b[q], t0_b[q]) of cb over [t_from[q], t_to[q]], radius[q] = R itself.  min_t, first_t and
 * last_t are tau on the common clock: of the minimum, of the first and of the last sample below (NaN: no such sample); min_d2 is +inf for K = 0.  The two
 * contexts may differ (a refined batch against the fleet it came from): both on the same device, both with solved trajectories and no solve in flight; cb's
 * stream is waited for before the launch on ca's stream, and each side applies its own context's frame shift.  The kernel time is kept on ca. */
int uph_separation_batch(uph_ctx* ca, uph_ctx* cb /* NULL: ca */, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, const double* t0_b,
                         const double* t_from, const double* t_to, double dt, const double* radius, double* min_d2 /* [n] */, double* min_t /* [n] */,
                         double* first_t /* [n], NaN: none */, double* last_t /* [n] */, int32_t* counts /* [n][2]: samples, below */);
/* host only, no device needed: the pairs of n boxes (uph_extent_batch's rows; +-inf allowed, NaN refused) with per-box radii that the rule does not drop, by a
 * sort on xmin and a sweep.  pairs holds the first cap of them in (i, j) order, *n_pairs is their full number. */
int uph_conflict_candidates(int32_t n, const double* box /* [n][4] */, const double* radius /* [n] */, int64_t cap, int32_t* pairs /* [cap][2] */, int64_t* n_pairs);
/* the fleet: vehicles (traj[i], t0[i]) of c's resident batch with radius[i] each, one window for all.  Extents on the device, candidates on the host, then the
 * separation of every candidate (a = i, b = j, R = radius[i] + radius[j]) on the device in launches of bounded size.  The pairs with below > 0 -- indices into
 * the vehicle list, in (i, j) order, the first cap of them -- with rows = min_d2, min_t, first_t, last_t and below = their number of samples below;
 * *n_conflicts is the full number of such pairs, *n_candidates the number of pairs the broad phase kept. */
int uph_conflicts_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* radius /* [n]: per vehicle */, double t_from, double t_to, double dt,
                        int64_t cap, int32_t* pairs /* [cap][2] */, double* rows /* [cap][4]: min_d2, min_t, first_t, last_t */, int32_t* below /* [cap] */,
                        int64_t* n_conflicts, int64_t* n_candidates);
/* milliseconds of the kernels of the last uph_extent_batch, uph_separation_batch or uph_conflicts_batch of c (events on the context's stream) */
int uph_separation_kernel_ms(const uph_ctx* c, double* kernel_ms);

/* ---- the same with oriented rectangles for the vehicles.  Sample times, the clamp of a vehicle's own time and its position X, Y are uph_separation_batch's
 * above, unchanged; its heading psi is column 9 of uph_traj_states(traj, u), the raw yaw, at the same u.
 *   shape          front, rear, half_width in metres, all finite and >= 0: in the body frame the rectangle spans [-rear, front] x [-half_width, half_width]
 *                  around the trajectory's point.  Zeros are allowed and give a segment or a point.  hl = (front + rear) / 2, o = (front - rear) / 2 and
 *                  w = half_width are formed on the host.
 *   pose at tau    c = cos psi, s = sin psi by sincosFast (csrc/uph_common.hpp, < 0.8 ulp each); u = (c, s), v = (-s, c).  Coordinates are taken relative to
 *                  vehicle a's point, so that no rounding grows with the place on the map: D = (X_b - X_a, Y_b - Y_a), the centres C_a = (o_a c_a, o_a s_a)
 *                  and C_b = (D_x + o_b c_b, D_y + o_b s_b), d = C_b - C_a.  Every product and every sum of this block is rounded on its own, in the order
 *                  written; a dot product p . q is p_x q_x + p_y q_y.
 *   overlap        for each axis n of u_a, v_a, u_b, v_b:
 *                      gap_n = |d . n| - ((hl_a |n . u_a| + w_a |n . v_a|) + (hl_b |n . u_b| + w_b |n . v_b|))
 *                  and g is the largest gap_n.  The rectangles OVERLAP iff g <= 0: touching counts.  For two rectangles these four axes decide overlap
 *                  exactly, the crossed configuration in which no corner lies inside the other rectangle included.
 *   clearance      c2 = 0 when the rectangles overlap.  Otherwise c2 is the smallest of the eight values ex ex + ey ey, one for each corner
 *                  (C_x +- hl u_x) +- w v_x, (C_y +- hl u_y) +- w v_y of one rectangle against the other rectangle: with e = corner - C_other,
 *                  ex = max(|e . u_other| - hl_other, 0) and ey = max(|e . v_other| - w_other, 0).  Two disjoint rectangles are closest at a corner of one
 *                  of them, so this is the exact squared Euclidean distance between them.  A pose with a value that is not finite gives c2 = NaN: the
 *                  sample is neither overlapping nor below, and reads +inf for the minimum, as a NaN d2 does in `separation`.
 *   below          a sample is BELOW when it overlaps or when c2 < M2, strictly, M2 = M * M rounded; M >= 0 is the pair's margin.  With M = 0, "below"
 *                  means "overlapping".
 *   minimum        the smallest c2, the smaller k among equals: a selection under the total order of the other queries, no floating-point atomics.
 *   radii          every point of rectangle i lies within rho_i = hypot(max(front_i, rear_i), half_width_i) of (X_i, Y_i).  uph_footprint_radii gives
 *                  r_i = (rho_i + m_i) * (1 + 2^-40) for margins m_i: if two boxes of uph_extent_batch are further apart than r_i + r_j along an axis, the
 *                  two points are at every sample, the rectangles' clearance exceeds m_i + m_j by the share of 2^-40 that the roundings of hypot, of the
 *                  sums and of the device's c2 (a few 1e-16 of the distance) do not use up, and no sample is below M = m_i + m_j.  uph_conflict_candidates
 *                  with these radii therefore drops no pair that is below at any sample.
 * Not bit for bit against numpy -- a sine is involved -- but deterministic as the other queries: no answer depends on the launch width, on how samples are
 * split over lanes or on the query's place in the batch.  The device calls follow uph_separation_batch / uph_conflicts_batch unchanged: two contexts, cb == NULL,
 * any output NULL, blocking, each side's frame shift, K = 0 rows (+inf, NaN, NaN, NaN, 0), every refusal with the outputs untouched, UPH_ERR_LIMIT for K > 2^22;
 * and UPH_ERR_INVALID for a shape component that is negative or not finite and for a margin that is negative or not finite. */
/* host only, no device needed: the broad-phase radii r[n] by the rule above */
int uph_footprint_radii(int32_t n, const double* shape /* [n][3]: front, rear, half_width */, const double* margin /* [n] */, double* r /* [n] */);
/* query q: vehicle (traj_a[q], t0_a[q]) of ca with shape_a[q] against vehicle (traj_b[q], t0_b[q]) of cb with shape_b[q] over [t_from[q], t_to[q]],
 * margin[q] = M itself.  min_t, first_t and last_t are tau on the common clock: of the minimum, of the first and of the last sample below (NaN: no such
 * sample); min_c2 is +inf for K = 0.  The kernel time is kept on ca. */
int uph_footprint_separation_batch(uph_ctx* ca, uph_ctx* cb /* NULL: ca */, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a,
                                   const double* t0_b, const double* t_from, const double* t_to, double dt, const double* shape_a /* [n][3] */,
                                   const double* shape_b /* [n][3] */, const double* margin /* [n] */, double* min_c2 /* [n] */, double* min_t /* [n] */,
                                   double* first_t /* [n], NaN: none */, double* last_t /* [n] */, int32_t* counts /* [n][3]: samples, below, overlapping */);
/* the fleet, as uph_conflicts_batch: vehicles (traj[i], t0[i]) of c's resident batch with shape[i] and margin[i] each, one window for all.  Extents on the
 * device, candidates on the host with uph_footprint_radii's radii, then the footprint separation of every candidate (a = i, b = j, M = margin[i] + margin[j],
 * one rounded add) on the device in launches of bounded size.  The pairs with below > 0, in (i, j) order, the first cap of them, with rows = min_c2, min_t,
 * first_t, last_t and below = their number of samples below; *n_conflicts is the full number of such pairs, *n_candidates the number the broad phase kept. */
int uph_footprint_conflicts_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* shape /* [n][3] */,
                                  const double* margin /* [n]: per vehicle */, double t_from, double t_to, double dt, int64_t cap, int32_t* pairs /* [cap][2] */,
                                  double* rows /* [cap][4]: min_c2, min_t, first_t, last_t */, int32_t* below /* [cap] */, int64_t* n_conflicts,
                                  int64_t* n_candidates);
/* milliseconds of the kernels of the last uph_footprint_separation_batch or uph_footprint_conflicts_batch of c (events on the context's stream) */
int uph_footprint_kernel_ms(const uph_ctx* c, double* kernel_ms);

/* ---- footprint check: the vehicle's rectangle swept over the map's occupancy layers as they are now.  uph_check_batch reads the occupancy at ONE place per
 * sample, the column under the trajectory's point; this query reads every column the body covers and answers "does the body touch an occupied column, when
 * first, and where".
 *   samples        query q names trajectory traj[q] and the window [t_from[q], t_to[q]] (t_to == NULL: to the end): exactly uph_check_batch's samples (same
 *                  time table, the end row at t = total when with_end is set; uph_check_window).
 *   pose           per sample the STATE row at t: X, Y in map coordinates (uph_traj_states' columns 0, 1), psi the raw yaw (column 9), yawn the normalised yaw
 *                  (column 6).  c = cos psi, s = sin psi by sincosFast, as the footprint metric above takes them; u = (c, s), v = (-s, c).
 *   rectangle      hl = (front + rear) / 2, o = (front - rear) / 2, w = half_width, formed on the host as above.  The margin m >= 0 inflates both half extents:
 *                  hl' = hl + m, w' = w + m, one rounded add each, on the host.  Centre C = (X + o c, Y + o s).
 *   covered        column (ix, iy) is COVERED by the pose iff it is the column of the point itself -- ix = floor((X - origin_x) * xy_inv), iy the same in y,
 *                  uph_check_batch's own statements -- or its centre P = (origin_x + (ix + 0.5) res, origin_y + (iy + 0.5) res) has
 *                      |(P - C) . u| <= hl'   and   |(P - C) . v| <= w'
 *                  with every product and every sum rounded on its own, in the order written (a dot product p . q is p_x q_x + p_y q_y; v's first component
 *                  is the negated s).  The point's column makes an all-zero shape exactly uph_check_batch's occupancy read.  The test is on CELL CENTRES: a
 *                  caller who wants "any part of the cell" adds res * sqrt(2) / 2 to the margin.
 *   kinds          of a covered column, with iw = floor((yawn - origin_yaw) * yaw_inv), uph_check_batch's yaw bin:
 *                      UPH_FOOT_OUTSIDE  ix, iy or iw outside the grid, or the row ix - x_off outside the rows a tile map holds (uph_check_batch's -1);
 *                      UPH_FOOT_OCC_XY   otherwise, the byte of occ_r2 (uph_map_get_cells) at (ix, iy) is not 0;
 *                      UPH_FOOT_OCC_YAW  otherwise, the byte of occ at (ix, iy, iw) is not 0.
 *   hits           a column is a HIT when its kinds intersect `layers`, a non-empty subset of UPH_FOOT_ALL; a sample is a hit when any covered column is.
 *   degenerate     a pose with X, Y, psi or yawn not finite, or with |ix|, |iy| or |iw| of its point at or above 2^30 (an index that would not fit 31 bits once
 *                  the box's extent and pad are added), covers nothing and is of kind UPH_FOOT_OUTSIDE: a hit iff layers holds that bit, with no hit column.
 *                  No float-to-int conversion of such a value is executed.
 *   enumeration    the kernel tests the columns of the box floor((C_x -+ ex - origin_x) * xy_inv) -+ 1 by floor((C_y -+ ey - origin_y) * xy_inv) -+ 1 with
 *                  ex = hl'|c| + w'|s|, ey = hl'|s| + w'|c|: the rectangle's hull and one column of pad -- 0.05 m on the reference's grids against roundings
 *                  of about 1e-14 m.  The rule is the membership test; the box is the implementation.  A query whose box can exceed 2^14 columns is refused
 *                  with UPH_ERR_LIMIT; the bound is uph_footprint_check_columns': side = floor(2 hypot(hl', w') (1 + 2^-40) / res) + 4, cols = side * side.
 * Outputs per query, any of them may be NULL:
 *   first_t, last_t [n]   t of the first and of the last hit sample (NaN: none)
 *   first_mask [n]        OR of the kinds within `layers` over the hit columns of the first hit sample (0: none)
 *   first_cell [n][2]     the lexicographically smallest (ix, iy) among the hit columns of the first hit sample: where the obstacle is.  (-1, -1): none (no
 *                         hit sample, or a degenerate first one)
 *   counts [n][5]         samples, hit samples, then samples with a covered column of kind XY, of kind YAW, of kind OUTSIDE -- these three regardless of layers
 *   cells [n][2]          covered columns and hit columns, summed over the window's samples
 * An empty window gives NaN, NaN, 0, (-1, -1) and zeros.  Not bit for bit against numpy where a centre lies within a rounding of the rectangle's edge -- a sine
 * is involved -- but deterministic: every output is an integer sum or a selection under a total order, so no answer depends on the launch width, on how samples
 * and columns are split over lanes or on the query's place in the batch.  Reads the occupancy layers on the map's own grid and no terrain cell.  Blocking, on the
 * context's stream.  Refusals, all before anything is written: uph_check_batch's; a shape component or a margin that is negative or not finite; layers outside
 * 1 .. UPH_FOOT_ALL; UPH_ERR_LIMIT as above and as uph_rollout_plan. */
#define UPH_FOOT_OCC_XY 1
#define UPH_FOOT_OCC_YAW 2
#define UPH_FOOT_OUTSIDE 4
#define UPH_FOOT_ALL 7
/* host only, no device needed: cols[q] = the bound on the columns of one sample's box for shape[q] inflated by margin[q] on a map of mp's resolution (the rule
 * above; saturates at 2^62).  UPH_ERR_INVALID: a NULL argument (margin == NULL: 0), n < 0, a resolution that is not positive and finite, a shape component or
 * margin that is negative or not finite, a reach that is not finite. */
int uph_footprint_check_columns(const uph_map_params* mp, int32_t n, const double* shape /* [n][3]: front, rear, half_width */, const double* margin /* [n], NULL: 0 */,
                                int64_t* cols /* [n] */);
int uph_footprint_check_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t_from, const double* t_to /* NULL: to the end */, double dt, int32_t with_end,
                              const double* shape /* [n][3] */, const double* margin /* [n], NULL: 0 */, int32_t layers, double* first_t /* [n], NaN: none */,
                              double* last_t /* [n] */, int32_t* first_mask /* [n] */, int32_t* first_cell /* [n][2] */, int32_t* counts /* [n][5] */,
                              int64_t* cells /* [n][2] */);
/* milliseconds of the kernel(s) of the last uph_footprint_check_batch of c (events on the context's stream) */
int uph_footprint_check_kernel_ms(const uph_ctx* c, double* kernel_ms);

/* ---- body layer: the map's occupancy dilated by the vehicle's rectangle, one slice per yaw bin (csrc/body_occ.hip).  The front-end search tests a
 * POINT: every collision sample, the goal and every one-shot sample read one byte of occ_r2 (isOccupancyXY).  The body layer is the configuration-space obstacle
 * of the rectangle on the map's own lattice: body[ix][iy][iw] = 1 iff the rectangle posed at the centre of cell (ix, iy, iw) covers an occupied column or one
 * outside the grid.  uph_kino_set_body_layer makes the search read it where it reads occ_r2, so that a path is searched in the space where the body fits.  The
 * reference marks the place: kino_astar.cpp:178 carries `// occ = uneven_map->isOccupancy(xt);`, a per-yaw read tried and left commented out.
 *   shape          (front, rear, half_width) and a margin m >= 0, admitted as uph_footprint_check_columns admits them.  Inflated as the footprint check does:
 *                  hl' = (front + rear) / 2 + m, o = (front - rear) / 2, w' = half_width + m, one rounded add each.
 *   bin pose       psi_iw = origin_yaw + (iw + 0.5) * yaw_resolution (one multiply, one add), c = cos(psi_iw), s = sin(psi_iw) by the host's libm.  The table
 *                  cs [nyaw][2] is an OUTPUT of uph_body_stencil; the numpy mirror (uneven_planner_amd/body_layer.py) takes it as input.
 *   covered        the integer offset (dx, dy) is COVERED in bin iw iff, with qx = dx * res - o * c and qy = dy * res - o * s,
 *                      |qx * c + qy * s| <= hl'   and   |qx * (-s) + qy * c| <= w'
 *                  with every product and every sum rounded on its own, in the order written: the footprint check's centre test with the pose at a cell centre,
 *                  written in offsets, so that it is translation-invariant by definition.
 *   stencil        R = floor(hypot(max(front, rear) + m, half_width + m) * (1 + 2^-40) / res) + 1.  For every iw and every row dx in [-R, R]: lo[iw][dx + R] and
 *                  hi[iw][dx + R] are the smallest and the largest covered dy in [-R, R]; an empty row has lo = 1, hi = 0.  The rule IS the interval per row (a
 *                  convex rectangle gives an interval; tests/test_body_layer_cpu.py shows that rounding never breaks one).
 *   limits         UPH_ERR_LIMIT when uph_footprint_check_columns' bound for the shape and margin exceeds 2^14 (the footprint check's own limit), or when R
 *                  exceeds UPH_BODY_MAX_R: the column bound is on (front + rear) / 2, R on max(front, rear), so a one-sided shape (front = 6 m, rear = 0 at res = 0.05) can
 *                  pass the first and not the second.
 *   layer          body[(ix * ny + iy) * nyaw + iw], one byte, laid out as occ (uph_map_get_cells), is 1 iff some covered (dx, dy) names a column
 *                  (ix + dx, iy + dy) that is inside the grid with occ_r2 != 0, when `layers` holds UPH_FOOT_OCC_XY, or outside [0, nx) x [0, ny), when `layers`
 *                  holds UPH_FOOT_OUTSIDE.  layers: UPH_FOOT_OCC_XY, UPH_FOOT_OUTSIDE or both; UPH_FOOT_OCC_YAW is refused (occ_r2 is already the OR of occ over
 *                  yaw).  An all-zero shape with m = 0 and layers = UPH_FOOT_OCC_XY makes every yaw slice equal to occ_r2.
 *   margin         uph_body_layer_margin = (res * sqrt(2) / 2 + 2 * hypot(max(front, rear), half_width) * sin(yaw_resolution / 4)) * (1 + 2^-40).  With this margin
 *                  a 0 at (ix, iy, iw) says of EVERY pose in that cell -- any position in the column, any yaw in the bin -- that the rectangle at margin 0, as
 *                  the footprint check defines it, covers no occupied column centre: such a pose is within res * sqrt(2) / 2 of the cell's centre pose, a body
 *                  point at radius r moves at most 2 r sin(e / 2) under a yaw change e <= yaw_resolution / 2, and inflating both half extents by d contains
 *                  everything within d of the rectangle.
 *   freshness      the map counts the writes of its occupancy (every commit: uph_map_set_cells, uph_map_build*, uph_map_update, uph_map_load_cache,
 *                  uph_map_commit, uph_map_import_cells_dev, uph_map_fill_fbm and the multi-GPU calls).  build and set stamp the layer with that count;
 *                  update is accepted only from a layer that is fresh or exactly one write behind -- the rect is the caller's statement of what that write
 *                  changed, normally uph_map_update_info.changed -- and otherwise refused with UPH_ERR_INVALID ("rebuild").  A search with a stale layer is
 *                  refused before anything is launched.  The layer does not follow the map by itself.
 * Every byte is an OR of integer comparisons on the stencil and occ_r2: neither the kernel's tiling nor the launch width can show, and update(rect) equals a
 * fresh build bit for bit when the rect holds every column whose occ_r2 changed.  Refusals, all before any device write: a tile map (uph_map_tile not the whole
 * grid); the shape, margin and layers as above; a rect that is reversed or leaves the grid (an empty rect is accepted and writes nothing); uph_body_layer_destroy
 * while a search context still names the layer.  Maps with fp32 cell storage are accepted: occupancy is bytes either way. */
#define UPH_BODY_MAX_R 64
/* host only, no device needed.  *R and *nyaw (the map's yaw bins, ceil((2 pi + 0.05) / yaw_resolution)) first, then cs [nyaw][2], lo and hi [nyaw][2R + 1];
 * any output may be NULL, so that R and nyaw can be asked first. */
int uph_body_stencil(const uph_map_params* mp, const double* shape /* [3]: front, rear, half_width */, double margin, int32_t* R, int32_t* nyaw, double* cs, int32_t* lo,
                     int32_t* hi);
int uph_body_layer_margin(const uph_map_params* mp, const double* shape /* [3] */, double* margin);
/* allocates nx * ny * nyaw bytes on the map's device, uploads the stencil and builds.  The map must outlive the layer. */
int uph_body_layer_create(uph_map* m, const double* shape /* [3] */, double margin, int32_t layers, uph_body_layer** out);
int uph_body_layer_build(uph_body_layer* l);                            /* the whole grid, from the map's occ_r2 as it is now.  Blocking. */
/* rect = (x0, x1, y0, y1), half-open, of the columns whose occ_r2 changed: rewrites exactly the outputs inside the rect grown by R and clipped.  Blocking. */
int uph_body_layer_update(uph_body_layer* l, const int32_t rect[4]);
int uph_body_layer_get(uph_body_layer* l, char* bytes /* [nx * ny * nyaw] */);
int uph_body_layer_set(uph_body_layer* l, const char* bytes);           /* the caller's own layer, every byte 0 (free) or 1 (occupied), else UPH_ERR_INVALID and nothing written: stamped fresh */
/* any output may be NULL.  behind: occupancy writes of the map since the layer was made (0: fresh; saturates at 2^31 - 1) */
int uph_body_layer_info(const uph_body_layer* l, double* shape3, double* margin, int32_t* layers, int32_t* R, int32_t* dims3, int32_t* behind);
int uph_body_layer_kernel_ms(const uph_body_layer* l, double* kernel_ms);   /* HIP-event milliseconds of the last build or update kernel */
int uph_body_layer_destroy(uph_body_layer* l);                          /* UPH_ERR_INVALID while a search context names the layer; NULL is accepted */
/* the search reads `layer` (of the same map as k) wherever it reads occ_r2 by default: the goal test, the one-shot samples and the collision samples of the
 * primitives, each at its own yaw bin as isOccupancy forms it.  The start test stays on occ (the vehicle is where it is), and everything else is the
 * reference's, its sampling gaps included: end states are not sampled, v = 0 primitives have no samples.  layer = NULL: back to occ_r2.  uph_plan_upload and
 * uph_replan_upload search through k and follow it.  Results with an all-zero-shape layer (m = 0, UPH_FOOT_OCC_XY) are the default search's. */
int uph_kino_set_body_layer(uph_kino* k, uph_body_layer* layer);
/* how often the layer's bytes have been written: uph_body_layer_build (the one inside create included), uph_body_layer_update (an empty rect too) and
 * uph_body_layer_set count one each.  The stamp of a clearance layer (below). */
int uph_body_layer_writes(const uph_body_layer* l, uint64_t* writes);

/* ---- clearance layer: the exact, truncated, squared Euclidean distance transform of a body layer, one field per yaw slice (csrc/clearance.hip).
 * A body layer answers one bit per cell at one margin chosen in advance; the clearance layer says how much room a cell has, and uph_clearance_check_batch reads it
 * along resident trajectories: how close, when and where.
 *   source         a body layer body[(ix * ny + iy) * nyaw + iw], bytes 0 / 1.  An all-zero-shape layer is occ_r2 per slice: the point case needs nothing extra.
 *   feature        under polarity UPH_CLEAR_TO_OCCUPIED (0) a cell is a FEATURE when its byte is 1; under UPH_CLEAR_TO_FREE (1) when its byte is 0 -- the depth
 *                  inside the obstacle, and with the other polarity a signed field.  Cells outside [0, nx) x [0, ny) are never features: the border enters through
 *                  the body layer's own UPH_FOOT_OUTSIDE bit.
 *   value          with the truncation radius rmax in cells, 1 <= rmax <= UPH_CLEAR_MAX_R:
 *                      m(ix, iy, iw) = min{ dx^2 + dy^2 : |dx| <= rmax, |dy| <= rmax, (ix + dx, iy + dy) inside the grid and a feature in slice iw }
 *                      D = m if such a feature exists and m <= rmax^2, else UPH_CLEAR_FAR
 *                  D is a uint16 laid out as the body layer.  A feature cell has D = 0; slices never mix.  In metres: res * sqrt(D).  The min over the square
 *                  window filtered by <= rmax^2 equals the min over the disc, so the separable evaluation is the rule and not an approximation: pass 1 along iy
 *                  finds g, the distance to the nearest feature of the row within rmax (255: none -- why rmax <= 254); pass 2 along ix takes min dx^2 + g^2.
 *   guarantee      a position in column (ix, iy) moved by any vector shorter than res * (sqrt(D) - sqrt(2)) lands in a column whose byte in slice iw is not a
 *                  feature: both positions are within res * sqrt(2) / 2 of their columns' centres, so a feature column reached that way would have its centre
 *                  nearer than res * sqrt(D).  For D = UPH_CLEAR_FAR take sqrt(rmax^2 + 1) for sqrt(D): every feature lies beyond the disc, and
 *                  the nearest place beyond it is that far, not rmax + 1 (the offset (rmax, 1)).  Under UPH_CLEAR_TO_OCCUPIED, with the body
 *                  layer built at uph_body_layer_margin, this is a statement about the real rectangle at every pose of those cells.
 *   rect update    when the body layer's bytes changed only inside rect (x0, x1, y0, y1), D can change only inside the rect grown by rmax and clipped:
 *                  uph_clearance_update rewrites exactly those outputs and equals a fresh build bit for bit.  uph_clearance_grow_rect serves both steps of the
 *                  chain: the map's `changed` rect grown by the body layer's R is what uph_body_layer_update rewrote; that rect grown by rmax is what
 *                  uph_clearance_update rewrites.
 *   freshness      create and build stamp the layer with the body layer's write count (uph_body_layer_writes).  update is accepted from a layer that is fresh or
 *                  exactly one write behind -- the rect is the caller's statement of what that write changed -- and otherwise refused with UPH_ERR_INVALID
 *                  ("rebuild"): the rule the body layer has towards the map.  uph_body_layer_destroy is refused while a clearance layer names the body layer.
 * Every value is a min of integer sums: neither tiling nor launch width can show.  Refusals, before any device write: rmax outside 1 .. UPH_CLEAR_MAX_R, a polarity
 * other than the two, a rect that is reversed or leaves the grid (an empty rect is accepted and writes nothing). */
#define UPH_CLEAR_TO_OCCUPIED 0
#define UPH_CLEAR_TO_FREE 1
#define UPH_CLEAR_MAX_R 254
#define UPH_CLEAR_FAR 65535
typedef struct uph_clearance uph_clearance;
/* host only, no device needed: out = rect = (x0, x1, y0, y1) grown by r >= 0 on every side and clipped to dims2 = (nx, ny).  An empty rect stays empty (out = rect).
 * UPH_ERR_INVALID: a NULL argument, r < 0, dims not positive, a rect that is reversed or leaves the grid. */
int uph_clearance_grow_rect(const int32_t dims2[2], const int32_t rect[4], int32_t r, int32_t out[4]);
/* allocates nx * ny * nyaw uint16 and as many scratch bytes on the body layer's device, and builds.  The body layer must outlive the clearance layer. */
int uph_clearance_create(uph_body_layer* body, int32_t rmax, int32_t polarity, uph_clearance** out);
int uph_clearance_build(uph_clearance* l);                              /* the whole grid, from the body layer's bytes as they are now.  Blocking. */
/* rect = (x0, x1, y0, y1), half-open, of the columns whose body bytes changed: rewrites exactly the outputs inside the rect grown by rmax and clipped.  Blocking. */
int uph_clearance_update(uph_clearance* l, const int32_t rect[4]);
int uph_clearance_get(uph_clearance* l, uint16_t* d /* [nx * ny * nyaw] */);
/* any output may be NULL.  behind: writes of the body layer since the clearance layer was made (0: fresh; saturates at 2^31 - 1) */
int uph_clearance_info(const uph_clearance* l, int32_t* rmax, int32_t* polarity, int32_t* dims3, int32_t* behind);
int uph_clearance_kernel_ms(const uph_clearance* l, double* kernel_ms);    /* HIP-event milliseconds of the two passes of the last build or update */
int uph_clearance_destroy(uph_clearance* l);                            /* NULL is accepted */
/* The query: the clearance along resident trajectories.  c is a context or a fleet bound to the layer's map (anything else: UPH_ERR_INVALID).
 *   samples        exactly uph_check_batch's: the same time table, end row and uph_check_window.
 *   cell           per sample (ix, iy, iw) by the footprint check's own floor statements on X, Y and the normalised yaw, with the same degenerate rule: a value
 *                  not finite or an index at or above 2^30 means that no float-to-int conversion is executed, and the sample counts as outside.
 *   value          a sample inside the grid has v = D[cell]; a sample outside has v = 0 and is counted as outside.
 * Outputs per query, any of them may be NULL:
 *   min_d2 [n]            the smallest v; -1 for an empty window
 *   min_t [n], min_cell [n][3]   t and cell of the EARLIEST sample that attains the min; NaN and (-1, -1, -1) for an empty window, the cell (-1, -1, -1) when that
 *                         sample is outside
 *   first_t, last_t [n]   t of the first and of the last sample with v < below2[q] (NaN: none)
 *   counts [n][4]         samples, below, outside, far (v == UPH_CLEAR_FAR)
 * Every output is an integer sum or a selection under the total order (value, sample index): launch width and lane split cannot show.  Reads no terrain cell.
 * Blocking, on the context's stream.  Refusals, all before any launch: uph_check_batch's; below2[q] < 0; a clearance layer behind its body layer; a body layer
 * behind the map; a context on another map. */
int uph_clearance_check_batch(uph_ctx* c, uph_clearance* layer, int32_t n, const int32_t* traj, const double* t_from, const double* t_to /* NULL: to the end */,
                              double dt, int32_t with_end, const int32_t* below2 /* [n] */, int32_t* min_d2 /* [n] */, double* min_t /* [n] */,
                              int32_t* min_cell /* [n][3] */, double* first_t /* [n] */, double* last_t /* [n] */, int32_t* counts /* [n][4] */);
/* milliseconds of the kernel(s) of the last uph_clearance_check_batch of c (events on the context's stream) */
int uph_clearance_check_kernel_ms(const uph_ctx* c, double* kernel_ms);

/* ---- the clearance term: a soft cost in the optimiser's objective that keeps the solve off obstacles.  The check reports a hit and the body search
 * finds a path where the body fits; without this term the solve that follows has point terms only and pulls the path back onto the obstacle.
 *   the field      c(x, y, yaw) in metres, from a clearance layer of polarity UPH_CLEAR_TO_OCCUPIED:
 *                    yaw slice   iw by the footprint check's floor statement on the NORMALISED yaw.  The field is piecewise constant in yaw: it has no yaw gradient.
 *                    cell value  d(cell) = res * sqrt(min(D, rmax^2 + 1)): UPH_CLEAR_FAR reads as the first distance beyond the disc, so the truncated field is
 *                                continuous and bounded
 *                    in xy       bilinear between the four nearest cell centres: u = (x - origin_x) / res - 0.5, i0 = floor(u), fx = u - i0, the same in y; the four
 *                                corner indices are clamped to the grid (the border itself enters through the body layer's UPH_FOOT_OUTSIDE bit)
 *                    gradient    (dc/dx, dc/dy): the exact gradient of the bilinear patch
 *                    degenerate  a pose that is not finite or whose index is at or above 2^30: value and gradient 0, no float-to-int conversion is executed
 *                  uph_clearance_field evaluates it at n poses (one lane per pose; UPH_ERR_INVALID for a layer of polarity UPH_CLEAR_TO_FREE).
 *   the term       at every sample j of a piece (the K + 1 quadrature samples the surface-variation cost rho_ter * sigma^2 is summed over, with its weights):
 *                  g = d_safe - c(position, yaw); where g > 0 the sample adds  om * g^2  to the cost, with om = (j == 0 or j == K ? 0.5 : 1) * weight * step * scale_fx,
 *                  and -2 om g grad c to the position gradient; everything behind that (time gradient, way-point gradient) is the objective's own machinery.
 *                  It is a cost, not a constraint: no multiplier, no residual, nothing in the stop rule; scale_fx and the constraint scales of initScaling do not see
 *                  it.  It says nothing between samples, and nothing about yaw within a slice.
 * uph_ctx_set_clearance_term persists on the context and applies to every later evaluation (uph_batch_eval), solve and uph_penalty_batch of it, whoever uploaded the
 * batch (uph_optimize_batch, uph_plan_upload, uph_replan_upload, uph_refine_upload as dst); layer == NULL switches it off, and off is the code without the term.
 * uph_clearance_destroy is refused while a context names the layer.  Refused with UPH_ERR_INVALID and a message, when the term is set or -- for what depends on the
 * batch -- at the launch, before anything is launched: a layer of polarity UPH_CLEAR_TO_FREE; a layer on another map; d_safe <= 0, weight < 0 or a value that is not
 * finite; d_safe > res * rmax (a cell with no obstacle within rmax must never be penalised); a clearance layer behind its body layer or a body layer behind the
 * map ("rebuild"); 64 lanes per trajectory; the fp32 sample mode; the L-BFGS resume hook; a batch with per-trajectory local frames (tile / km^2 maps). */
int uph_ctx_set_clearance_term(uph_ctx* c, uph_clearance* layer /* NULL: off */, double d_safe, double weight);
int uph_ctx_clearance_term(const uph_ctx* c, uph_clearance** layer, double* d_safe, double* weight);     /* any output may be NULL; layer NULL: off */
int uph_clearance_field(uph_clearance* l, int32_t n, const double* pos /* [n][3]: x, y, yaw */, double* value /* [n] */, double* grad /* [n][2] */);

/* ---- start delays: clearing conflicts between resident trajectories without a new solve.  A vehicle that starts later drives the very same trajectory, so
 * every terrain term uph_check_batch has passed stays passed; only its start on the common clock moves.  Every number below is one uph_separation_batch /
 * uph_extent_batch returns for the shifted start, bit for bit.
 *   delay table    delay0 (finite), delay_step (finite, > 0) and a count D >= 1 give delta_j = delay0 + j * delay_step, 0 <= j < D -- the product rounded, then
 *                  the sum, as tau_k above.  The table is formed once on the host (uph_delay_times) and the device reads delta_j from it: a delayed vehicle
 *                  starts at t0 + delta_j, one rounded add, and there is no multiply on the device that could be fused into it.
 *   sweep row      row (q, j) holds min_d2, min_t and below (the number of samples below) of uph_separation_batch for vehicle a (traj_a[q], t0_a[q]) against
 *                  vehicle b (traj_b[q], t0_b[q] + delta_j) over the same window, dt and radius, its NaN and tie rules included; K = 0 gives +inf, NaN, 0.
 *                  first_clear[q] is the smallest j with below == 0 (-1: none), taken on the host from the rows.
 *   swept extent   per vehicle and window the hull over j of uph_extent_batch(traj, t0 + delta_j)'s boxes -- min and max are exact, the order of the fold cannot
 *                  matter --, with K and the number of (j, k) samples whose position is NaN.  Every position the vehicle takes at any sample under any
 *                  delay of the table lies in this box, so uph_conflict_candidates on swept boxes drops no pair that is below at any sample for any
 *                  combination of delays: the proof of `candidates` above, unchanged, with no epsilon.
 *   schedule       vehicles (traj[i], t0[i], radius[i]) in priority order, the smaller index first.  n_delays[i] in [1, D] (NULL: D for all) is the number of
 *                  delays vehicle i may use; a vehicle already under way has 1.  The swept boxes are taken over the whole table.  Vehicle i is compared with
 *                  every h < i the broad phase keeps, R = r_h + r_i, h at its EFFECTIVE start t0_h + delta_max(choice[h], 0) and i swept.  choice[i] is the
 *                  smallest j < n_delays[i] with below == 0 against every such h (0 without a partner); -1 when there is none, and the vehicle then stays at
 *                  j = 0 for all behind it, with blocker[i] the smallest h that is below at j = 0 (-1 otherwise).  start[i] is the effective start.  The
 *                  result is the sequential greedy's; the vehicles whose kept partners of smaller index are all placed -- the levels of the candidate
 *                  graph (uph_delay_levels) -- are swept in one round, since a choice depends on the choices of those partners alone.
 * The sweep kernel takes the samples in tiles of UPH_DELAY_TILE; no result depends on the tile, on the launch width or on how a tile is split over lanes.
 * The device calls are blocking, on the (first) context's stream; any output may be NULL; the two-context rules are uph_separation_batch's.  Every refusal of
 * uph_separation_batch / uph_extent_batch / uph_conflicts_batch applies unchanged, outputs untouched, and so do: UPH_ERR_INVALID for a delay_step that is not
 * positive and finite, a non-finite delay0, D < 1, a start t0 + delta_j that is not finite, an n_delays[i] outside [1, D], a pair of uph_delay_levels without
 * 0 <= i < j < n; UPH_ERR_LIMIT for D > 4096 and for a query with K * D > 2^26 (one workgroup's serial work is then at most that of 16 separation queries
 * of the largest length).  At most 2^20 sweep rows are on the device at a time: longer launches are split. */
#define UPH_DELAY_TILE 128
/* host only, no device needed: the table delta[D] by the rule above */
int uph_delay_times(double delay0, double delay_step, int32_t D, double* delta);
/* host only, no device needed: level[j] of n vehicles among pairs (i, j), i < j: 0 for a vehicle without a smaller partner, else 1 + the largest level of
 * its smaller partners */
int uph_delay_levels(int32_t n, int64_t n_pairs, const int32_t* pairs /* [n_pairs][2] */, int32_t* level /* [n] */);
/* query q: vehicle (traj_a[q], t0_a[q]) of ca against vehicle (traj_b[q], t0_b[q] + delta_j) of cb for every delay of the table; counts[q] = K.  The kernel
 * time is kept on ca. */
int uph_delay_sweep_batch(uph_ctx* ca, uph_ctx* cb /* NULL: ca */, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a, const double* t0_b,
                          const double* t_from, const double* t_to, double dt, const double* radius, double delay0, double delay_step, int32_t D,
                          double* min_d2 /* [n][D] */, double* min_t /* [n][D] */, int32_t* below /* [n][D] */, int32_t* first_clear /* [n] */,
                          int32_t* counts /* [n]: K */);
/* query q: the swept extent of vehicle (traj[q], t0[q]) over the window [t_from[q], t_to[q]] */
int uph_delay_extent_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* t_from, const double* t_to, double dt, double delay0,
                           double delay_step, int32_t D, double* box /* [n][4] */, int32_t* counts /* [n][2]: K, NaN samples over all delays */);
/* the fleet, one window for all as uph_conflicts_batch: swept extents on the device, candidates and their levels on the host, a sweep launch (or a few of
 * bounded size) per level.  *n_candidates is the number of pairs the broad phase kept, *n_rounds the number of levels that were swept, *n_unresolved the
 * number of vehicles with choice == -1. */
int uph_delays_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* radius, const int32_t* n_delays /* may be NULL */, double t_from,
                     double t_to, double dt, double delay0, double delay_step, int32_t D, int32_t* choice /* [n] */, double* start /* [n] */,
                     int32_t* blocker /* [n] */, int64_t* n_candidates, int32_t* n_rounds, int32_t* n_unresolved);

/* ---- start delays with oriented rectangles: the sweep and the schedule above with the footprint rule for the pair, so that a fleet whose conflicts were
 * reported by uph_footprint_conflicts_batch is cleared by the same metric and no vehicle waits for a pass side by side or nose to tail that the rectangles allow.
 *   footprint sweep row   row (q, j) holds min_c2, min_t, below and overlapping of uph_footprint_separation_batch for vehicle a (traj_a[q], t0_a[q], shape_a[q])
 *                  against vehicle b (traj_b[q], t0_b[q] + delta_j, shape_b[q]) over the same window, dt and margin, bit for bit, its NaN and tie rules
 *                  included; K = 0 gives +inf, NaN, 0, 0.  delta_j is uph_delay_times' table and the device performs only the add t0_b + delta_j.
 *                  first_clear[q] is the smallest j with below == 0 (-1: none), taken on the host from the rows; counts[q] = K.  Vehicle a does not move
 *                  with the delay: the kernel takes its pose and the sine and cosine of its heading once per sample and b's once per (delay, sample), by
 *                  the same sincosFast and the same statements of the rule as uph_footprint_separation_batch, which is why the bits agree.
 *   footprint schedule   the schedule above, unchanged in every rule -- priority order, n_delays, the effective start of the vehicles ahead, choice, start,
 *                  blocker, the levels as rounds -- with the footprint sweep for the narrow phase: vehicle h at its effective start with shape[h] is a,
 *                  vehicle i with shape[i] is b and is swept, M = margin[h] + margin[i], one rounded add as in uph_footprint_conflicts_batch.  The broad
 *                  phase is uph_conflict_candidates on the swept boxes of uph_delay_extent_batch with uph_footprint_radii's radii r_i.
 *   why the footprint broad phase loses nothing   every position a vehicle takes at any sample under any delay of the table lies in its swept box (swept
 *                  extent, above).  If two swept boxes are further apart than r_h + r_i along an axis, then so are the two points at every sample under
 *                  every combination of delays, and the argument of `radii` above applies to each such sample as it stands: the rectangles' clearance
 *                  exceeds m_h + m_i by the share of 2^-40 that the roundings do not use up, and the sample is not below M = m_h + m_i.  No new epsilon.
 * The two-context rules, NULL outputs and blocking are those of uph_delay_sweep_batch / uph_delays_batch.  The refusals are the union of the refusals of
 * uph_footprint_separation_batch / uph_footprint_conflicts_batch and of uph_delay_sweep_batch / uph_delays_batch -- UPH_ERR_LIMIT for D > 4096 and for a query
 * with K * D > 2^26 among them --, each before any output is written; the shape and margin checks come first, as in the footprint calls, then the delay
 * table's and n_delays', all before a context is read.  A footprint sweep row is 32 bytes: 2^20 of them, the most on the device at a time, are 32 MB. */
/* query q: vehicle (traj_a[q], t0_a[q]) of ca with shape_a[q] against vehicle (traj_b[q], t0_b[q] + delta_j) of cb with shape_b[q] for every delay of the
 * table, margin[q] = M itself.  The kernel time is kept on ca. */
int uph_footprint_delay_sweep_batch(uph_ctx* ca, uph_ctx* cb /* NULL: ca */, int32_t n, const int32_t* traj_a, const int32_t* traj_b, const double* t0_a,
                                    const double* t0_b, const double* t_from, const double* t_to, double dt, const double* shape_a /* [n][3] */,
                                    const double* shape_b /* [n][3] */, const double* margin /* [n] */, double delay0, double delay_step, int32_t D,
                                    double* min_c2 /* [n][D] */, double* min_t /* [n][D] */, int32_t* below /* [n][D] */, int32_t* overlapping /* [n][D] */,
                                    int32_t* first_clear /* [n] */, int32_t* counts /* [n]: K */);
/* the fleet with rectangles, as uph_delays_batch: vehicles (traj[i], t0[i]) with shape[i] and margin[i] in priority order, one window for all.  Swept extents
 * on the device, candidates (uph_footprint_radii's radii) and their levels on the host, a footprint sweep launch (or a few of bounded size) per level. */
int uph_footprint_delays_batch(uph_ctx* c, int32_t n, const int32_t* traj, const double* t0, const double* shape /* [n][3] */, const double* margin /* [n] */,
                               const int32_t* n_delays /* may be NULL */, double t_from, double t_to, double dt, double delay0, double delay_step, int32_t D,
                               int32_t* choice /* [n] */, double* start /* [n] */, int32_t* blocker /* [n] */, int64_t* n_candidates, int32_t* n_rounds,
                               int32_t* n_unresolved);
/* milliseconds of the kernels of the last uph_delay_sweep_batch, uph_delay_extent_batch or uph_delays_batch of c (events on the context's stream); also of the
 * last uph_footprint_delay_sweep_batch or uph_footprint_delays_batch, which keep their kernel time in the same place */
int uph_delay_kernel_ms(const uph_ctx* c, double* kernel_ms);

/* ---- a fleet of resident trajectories: a long-lived uph_ctx whose resident batch is `slots` SLOTS, filled by adopting solved trajectories of other contexts
 * on the device.  Every call that looks at a whole fleet (uph_conflicts_batch, uph_delays_batch, their footprint forms, check / locate / within over the live
 * vehicles) takes ONE context, while the trajectories a fleet drives are solved in several and every upload replaces the batch of its context: a fleet is the
 * one context that holds what every vehicle drives NOW.  Solve anywhere, adopt the result into the vehicle's slot, ask the fleet.
 *   layout       slot s owns 12 cap_xy doubles of the fleet's c_xy array and 6 cap_yaw doubles of its c_yaw array (fixed stride), one TrajDesc row (208 B) and
 *                one TrajState row (232 B): 96 cap_xy + 48 cap_yaw + UPH_FLEET_SLOT_ROW_BYTES bytes of device memory per slot, all allocated at creation and
 *                zeroed.  At the largest caps (128 / 256) that is 24 KiB of coefficients + 440 B per slot: 4096 slots take 96 MiB + 1.7 MiB.  Replacing a slot's
 *                trajectory by one of any piece counts within the caps moves no other slot and cannot fail for lack of space.  uph_fleet_bytes is that figure
 *                (pure host arithmetic; the query calls allocate their own small record / row buffers at their first use, as on any context).
 *   empty slot   is to every call what an UPH_RET_UNSUPPORTED slot of a batch is: a query that names it is refused ("... names an empty slot"), the rollout
 *                gives it no rows (uph_rollout_plan: offsets[s + 1] == offsets[s]).
 *   per slot     the fleet keeps what queries and re-plans read of a batch: the TrajDesc / TrajState rows (piece counts, T_xy, T_yaw, ret_code, f, jerk_cost, ...),
 *                the local frame when the map is one that solves in local frames (the same rule as any batch on that map), the end boundary of the problem in map
 *                coordinates (uph_replan_upload with goals == NULL and uph_refine_upload work from a fleet), and a start time t0 on the common clock (host side).
 *   adoption     uph_fleet_adopt copies trajectory src_traj[q] of src's resident batch into slot[q], with start t0[q] (NULL: 0), in ONE kernel launch
 *                (uph_fleet_adopt_kernel: a workgroup per trajectory, 16-byte loads and stores over its 12 Nxy + 6 Nyaw coefficient doubles, one lane writes the
 *                two rows; no coefficient crosses the host) and returns when the copy has completed.  Bit for bit: the coefficients, the piece counts, the whole
 *                TrajState row, the frame, the end boundary.  src is unchanged, and later uploads into src do not touch the fleet.  src may itself be a fleet.
 *                All or nothing: everything is validated before the first device write; a refusal leaves the fleet as it was.  UPH_ERR_INVALID: fleet is not a
 *                fleet, src == fleet, different maps, an asynchronous solve pending on either, src holding no resident trajectory, an src_traj[q] out of range or
 *                naming an unsupported / empty slot, a slot[q] out of range or named twice in one call (the same src_traj twice is fine), a non-finite t0[q], a
 *                map whose geometry changed since src's frames or the fleet's were formed, n <= 0, a NULL pointer.  UPH_ERR_LIMIT, naming the query: Nxy > cap_xy
 *                or Nyaw > cap_yaw.
 *   the three classes of entry points that take a uph_ctx
 *     work on a fleet, their numbers unchanged: uph_batch_count, uph_traj_states, uph_rollout_plan, uph_rollout_batch, uph_rollout_batch_dev, uph_check_limits,
 *                uph_check_batch, uph_locate_batch, uph_within_batch, uph_extent_batch, uph_separation_batch and uph_footprint_separation_batch (the fleet as
 *                side a, side b or both), uph_conflicts_batch, uph_footprint_conflicts_batch, uph_delay_sweep_batch, uph_delay_extent_batch, uph_delays_batch,
 *                uph_footprint_delay_sweep_batch, uph_footprint_delays_batch, uph_footprint_check_batch, every uph_*_kernel_ms getter, uph_ctx_get_rho, uph_ctx_destroy, and
 *                uph_replan_upload / uph_refine_upload with the fleet as src.  The t0 arguments of these calls are the caller's: uph_fleet_info returns the stored
 *                starts to pass.
 *     refused with UPH_ERR_INVALID ("... the context is a fleet"), the fleet untouched: everything that uploads into, solves, evaluates, reports on or downloads
 *                a batch or sets its state -- uph_batch_upload, uph_optimize_batch, uph_optimize_batch_multi, uph_plan_upload into it, a fleet as dst of
 *                uph_replan_upload / uph_refine_upload, uph_batch_solve, uph_batch_solve_async, uph_batch_wait, uph_batch_download, uph_eval_batch,
 *                uph_penalty_batch, uph_init_scaling_batch, uph_microbench_batch, uph_report_batch, uph_batch_set_state, uph_batch_set_x, uph_batch_alm_passes,
 *                uph_batch_set_lbfgs_state, uph_batch_lbfgs_resume, uph_batch_get_lbfgs_state, uph_plan_staged, uph_batch_origin, uph_batch_stats, and the solve
 *                knobs uph_ctx_set_lanes, uph_ctx_set_xcd_locality, uph_ctx_set_wps, uph_ctx_set_sample_precision, uph_ctx_set_rho, uph_ctx_set_trial_abandon,
 *                uph_ctx_set_trace.
 *     fleet only: the uph_fleet_* calls below, refused with UPH_ERR_INVALID ("... is not a fleet") on any other context. */
#define UPH_FLEET_SLOT_ROW_BYTES 440   /* the TrajDesc + TrajState rows of one slot */
/* device memory of a fleet of that shape: slots * (96 cap_xy + 48 cap_yaw + UPH_FLEET_SLOT_ROW_BYTES).  UPH_ERR_INVALID: slots < 1, a cap outside
 * [1, UPH_MAX_PIECE_*], bytes NULL. */
int uph_fleet_bytes(int32_t slots, int32_t cap_xy, int32_t cap_yaw, int64_t* bytes);
/* a fleet of `slots` empty slots on the map's device; p is kept for uph_check_limits / uph_check_batch.  uph_ctx_destroy frees it, uph_batch_count returns slots.
 * UPH_ERR_INVALID: a NULL argument, slots < 1, a cap outside [1, UPH_MAX_PIECE_*]; UPH_ERR_NO_DEVICE: no HIP device visible (there is no host fall-back);
 * then uph_ctx_create's own refusals. */
int uph_fleet_create(uph_map* m, const uph_opt_params* p, int32_t slots, int32_t cap_xy, int32_t cap_yaw, uph_ctx** out);
int uph_fleet_adopt(uph_ctx* fleet, uph_ctx* src, int32_t n, const int32_t* src_traj, const int32_t* slot, const double* t0 /* [n], NULL: 0 */);
/* empties the slots (an empty one stays empty: idempotent); their coefficients stay where they lie until the next adoption overwrites them */
int uph_fleet_release(uph_ctx* fleet, int32_t n, const int32_t* slot);
/* every output may be NULL: the shape, occupied[s] = 1 / 0, t0[s] = the stored start (0 for an empty slot) */
int uph_fleet_info(const uph_ctx* fleet, int32_t* slots, int32_t* cap_xy, int32_t* cap_yaw, int32_t* occupied /* [slots], may be NULL */, double* t0 /* [slots], may be NULL */);
/* the trajectories of the named slots (any order, repeats allowed; every output may be NULL): counts, piece durations, ret_code, and the slot's whole coefficient
 * regions, of which the first 12 n_xy / 6 n_yaw doubles are the trajectory -- in map coordinates, exactly the doubles uph_batch_download gives for the source --
 * and the rest whatever earlier adoptions left (zeros at first).  An empty slot: counts 0, durations 0, ret_code UPH_RET_UNSUPPORTED, its regions as they lie. */
int uph_fleet_get(uph_ctx* fleet, int32_t n, const int32_t* slot, int32_t* n_xy, int32_t* n_yaw, double* T_xy, double* T_yaw, int32_t* ret_code,
                  double* c_xy /* [n][12*cap_xy] */, double* c_yaw /* [n][6*cap_yaw] */);
/* milliseconds of uph_fleet_adopt_kernel in the last uph_fleet_adopt (events on the fleet's stream) */
int uph_fleet_kernel_ms(const uph_ctx* fleet, double* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* UNEVEN_HIP_H */
