// uneven_hip_adapter.hpp -- header-only C++ adapter that gives libunevenhip.so the member names PlanManager uses on the
// reference's ALMTrajOpt and SE2Trajectory (plan_manager/src/plan_manager.cpp:17-22, 134-185), so that the goal callback compiles
// against it as it stands (INTEGRATION.md shows the swap).
//
// Mirrors (paths under /root/reference/src/uneven_planner):
//   ALMTrajOpt::optimizeSE2Traj   back_end/include/back_end/alm_traj_opt.h:92-98   (same argument list, same 0/1/2 return)
//   ALMTrajOpt::getTraj           alm_traj_opt.h:165-168  -> per-piece durations + D x 6 coefficient matrices, highest order first
//                                                            (MinJerkOpt::getTraj, back_end/include/utils/se2traj.hpp:682-695)
//   ALMTrajOpt::setEnvironment    alm_traj_opt.h:127-130
//   public parameter members      alm_traj_opt.h:29-53
//   getMaxVxAxAyCurAttSig         alm_traj_opt.h:170-229 (device report), init / setFrontend / visSE2Traj / visSE3Traj (no-ops here);
//   getSE3Path / getSE3PathBatch  visSE3Traj's path (alm_traj_opt.cpp:1102-1135) from the device rollout (uph_rollout_batch)
//   Piece / PolyTrajectory / SE2Trajectory   back_end/include/utils/se2traj.hpp:30-150, 253-406, 408-562 (evaluation members, getNonHolError)
//   mpc_controller/SE2Traj filler  plan_manager.cpp:150-182, mpc_controller/msg/SE2Traj.msg:1-9
//   KinoAstar::plan / setEnvironment / init   front_end/include/front_end/kino_astar.h:147-154, front_end/src/kino_astar.cpp:5-43, 67-236
//                                  (the batched device search, uph_kino_plan_batch; planBatch = many goals in one call)
//   planSE2TrajBatch               PlanManager::rcvWpsCallBack plan_manager.cpp:43-134 for many goals in one call, every stage on the device (uph_plan_upload)
//   replanSE2TrajBatch             the same from states on the last batch's trajectories: re-planning a vehicle in motion (uph_replan_upload)
//   refineSE2TrajBatch             the rest of the last batch's trajectories re-optimised from states at switch times, no search (uph_refine_upload)
//   checkSE2TrajBatch              time windows of the last batch's trajectories held against limits on the map as it is now (uph_check_batch)
//   footprintCheckSE2TrajBatch     the same windows with the vehicle's rectangle swept over the map's occupancy: first / last hit and where (uph_footprint_check_batch)
//   setClearanceTerm               a soft cost on the clearance field of a ClearanceLayer in every later solve (uph_ctx_set_clearance_term)
//   clearanceSE2TrajBatch          the same windows read in a ClearanceLayer, the distance transform of a BodyLayer: how close, when and where (uph_clearance_check_batch)
//
// The matrix/vector types are template parameters: anything with data(), rows(), cols()/size() and column-major storage works
// (Eigen::MatrixXd / Eigen::VectorXd in the ROS workspace; the tiny Mat/Vec below where Eigen is not installed, as in this
// repository's image).  No Eigen header is included here.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "uneven_hip.h"

namespace uneven_hip {

class KinoAstar;
class ClearanceLayer;

struct Mat {                       // minimal column-major stand-in with the Eigen accessors the adapter touches
    int r = 0, c = 0;
    std::vector<double> v;
    Mat() {}
    Mat(int rows_, int cols_) : r(rows_), c(cols_), v((size_t)rows_ * cols_, 0.0) {}
    const double* data() const { return v.data(); }
    double* data() { return v.data(); }
    int rows() const { return r; }
    int cols() const { return c; }
    int size() const { return r * c; }
    double& operator()(int i, int j) { return v[(size_t)j * r + i]; }
    double operator()(int i, int j) const { return v[(size_t)j * r + i]; }
};

// column vector of D doubles: Eigen's own type where Eigen is installed (so that `Eigen::Vector2d p = traj.pos_traj[i].getValue(0.0)`
// compiles unchanged), a minimal stand-in otherwise
#if __has_include(<Eigen/Core>)
}  // namespace uneven_hip
#include <Eigen/Core>
namespace uneven_hip {
template <int D> using VecN = Eigen::Matrix<double, D, 1>;
template <int D> inline VecN<D> vecZero() { return VecN<D>::Zero(); }
#else
template <int D>
struct VecN {
    double v[D];
    double operator[](int i) const { return v[i]; }
    double& operator[](int i) { return v[i]; }
    double operator()(int i) const { return v[i]; }
    double& operator()(int i) { return v[i]; }
    double x() const { return v[0]; }
    double y() const { return v[D > 1 ? 1 : 0]; }
};
template <int D> inline VecN<D> vecZero() { VecN<D> z; for (int d = 0; d < D; d++) z.v[d] = 0.0; return z; }
#endif

// Piece<Dim> (se2traj.hpp:30-150): duration + Dim x 6 coefficients, highest order first; the three evaluators follow the reference's loops
template <int Dim>
class Piece {
public:
    double duration = 0.0;
    double coeff[Dim][6];
    int getDim() const { return Dim; }
    int getOrder() const { return 5; }
    double getDuration() const { return duration; }
    VecN<Dim> getValue(const double& t) const {                         // :106-116
        VecN<Dim> value = vecZero<Dim>();
        double tn = 1.0;
        for (int i = 5; i >= 0; i--) { for (int d = 0; d < Dim; d++) value[d] += tn * coeff[d][i]; tn *= t; }
        return value;
    }
    VecN<Dim> getDotValue(const double& t) const {                      // :118-131
        VecN<Dim> value = vecZero<Dim>();
        double tn = 1.0;
        int n = 1;
        for (int i = 4; i >= 0; i--) { for (int d = 0; d < Dim; d++) value[d] += n * tn * coeff[d][i]; tn *= t; n++; }
        return value;
    }
    VecN<Dim> getDDotValue(const double& t) const {                     // :133-150
        VecN<Dim> value = vecZero<Dim>();
        double tn = 1.0;
        int m = 1, n = 2;
        for (int i = 3; i >= 0; i--) { for (int d = 0; d < Dim; d++) value[d] += m * n * tn * coeff[d][i]; tn *= t; m++; n++; }
        return value;
    }
};

// PolyTrajectory<Dim> (se2traj.hpp:253-406): the members PlanManager, the report and the MPC message filler use
template <int Dim>
class PolyTrajectory {
public:
    std::vector<Piece<Dim>> pieces;
    int getPieceNum() const { return (int)pieces.size(); }
    double getTotalDuration() const {                                   // :290-299
        double total = 0.0;
        for (const Piece<Dim>& p : pieces) total += p.getDuration();
        return total;
    }
    const Piece<Dim>& operator[](int i) const { return pieces[i]; }
    Piece<Dim>& operator[](int i) { return pieces[i]; }
    typename std::vector<Piece<Dim>>::const_iterator begin() const { return pieces.begin(); }
    typename std::vector<Piece<Dim>>::const_iterator end() const { return pieces.end(); }
    void clear() { pieces.clear(); }
    void emplace_back(const Piece<Dim>& p) { pieces.emplace_back(p); }
    int locatePieceIdx(double& t) const {                               // :343-361
        const int N = getPieceNum();
        int idx;
        double dur;
        for (idx = 0; idx < N && t > (dur = pieces[idx].getDuration()); idx++) t -= dur;
        if (idx == N) { idx--; t += pieces[idx].getDuration(); }
        return idx;
    }
    VecN<Dim> getValue(double t) const { const int i = locatePieceIdx(t); return pieces[i].getValue(t); }
    VecN<Dim> getDotValue(double t) const { const int i = locatePieceIdx(t); return pieces[i].getDotValue(t); }
    VecN<Dim> getDDotValue(double t) const { const int i = locatePieceIdx(t); return pieces[i].getDDotValue(t); }
};

class SE2Trajectory {              // se2traj.hpp:408-562
public:
    PolyTrajectory<2> pos_traj;
    PolyTrajectory<1> yaw_traj;
    double getTotalDuration() const { const double a = pos_traj.getTotalDuration(), b = yaw_traj.getTotalDuration(); return a < b ? a : b; }
    VecN<2> getPos(double t) const { return pos_traj.getValue(t); }
    VecN<2> getVel(double t) const { return pos_traj.getDotValue(t); }
    VecN<2> getAcc(double t) const { return pos_traj.getDDotValue(t); }
    double getAngle(double t) const { return yaw_traj.getValue(t)[0]; }
    double getAngleRate(double t) const { return yaw_traj.getDotValue(t)[0]; }
    double getNonHolError() const {                                     // :551-561
        double error = 0.0;
        for (double t = 0.0; t < getTotalDuration(); t += 0.01) {
            const VecN<2> v = getVel(t);
            const double yaw = getAngle(t);
            error += std::fabs(v[0] * std::sin(yaw) + v[1] * (-std::cos(yaw)));
        }
        return error;
    }
};

// mpc_controller/SE2Traj (mpc_controller/msg/SE2Traj.msg:1-9) as plain data, and the filler PlanManager runs before publishing
// (plan_manager.cpp:150-182): piece start points + the end point, piece durations, zero init_v / init_a.  fillSE2TrajMsg is a
// template, so the real ROS message type works as well as this stand-in (start_time is left to the caller: ros::Time::now()).
struct Point3 { double x = 0.0, y = 0.0, z = 0.0; };
struct SE2TrajMsg {
    double start_time = 0.0;
    std::vector<Point3> pos_pts, angle_pts;
    Point3 init_v, init_a;
    std::vector<double> posT_pts, angleT_pts;
};
template <class Msg>
inline void fillSE2TrajMsg(const SE2Trajectory& traj, Msg& msg) {
    typedef typename std::remove_reference<decltype(msg.pos_pts[0])>::type Pt;
    msg.init_v.x = 0.0; msg.init_v.y = 0.0; msg.init_v.z = 0.0;
    msg.init_a.x = 0.0; msg.init_a.y = 0.0; msg.init_a.z = 0.0;
    msg.pos_pts.clear(); msg.posT_pts.clear(); msg.angle_pts.clear(); msg.angleT_pts.clear();
    for (int i = 0; i < traj.pos_traj.getPieceNum(); i++) {
        Pt pt{};
        const VecN<2> pos = traj.pos_traj[i].getValue(0.0);
        pt.x = pos[0]; pt.y = pos[1];
        msg.pos_pts.push_back(pt);
        msg.posT_pts.push_back(traj.pos_traj[i].getDuration());
    }
    {
        Pt pt{};
        const VecN<2> pos = traj.pos_traj.getValue(traj.pos_traj.getTotalDuration());
        pt.x = pos[0]; pt.y = pos[1];
        msg.pos_pts.push_back(pt);
    }
    for (int i = 0; i < traj.yaw_traj.getPieceNum(); i++) {
        Pt pt{};
        pt.x = traj.yaw_traj[i].getValue(0.0)[0];
        msg.angle_pts.push_back(pt);
        msg.angleT_pts.push_back(traj.yaw_traj[i].getDuration());
    }
    {
        Pt pt{};
        pt.x = traj.yaw_traj.getValue(traj.yaw_traj.getTotalDuration())[0];
        msg.angle_pts.push_back(pt);
    }
}

// rosparam uneven_map/... as UnevenMap::init reads it (uneven_map/src/uneven_map.cpp:75-88; getParam: absent keys keep the value passed in,
// which starts as run_hill.yaml:2-14) -- for hosts that create the device grid without the reference's UnevenMap object.  INTEGRATION.md 1 builds
// the same block from UnevenMap's own members, which that very init has just loaded.  `mass`, `map_pcd`, `map_file` have no device side.
template <class NodeHandle>
inline uph_map_params loadMapParams(NodeHandle& nh, uph_map_params mp = uph_map_params{2, 10.0, 10.0, 0.2, 0.1, 0.1, 0.05, 0.1, 0.8, 0.05, 9.81}) {
    int iter_num = mp.iter_num;
    nh.getParam("uneven_map/iter_num", iter_num);
    mp.iter_num = iter_num;
    nh.getParam("uneven_map/map_size_x", mp.map_size_x);
    nh.getParam("uneven_map/map_size_y", mp.map_size_y);
    nh.getParam("uneven_map/ellipsoid_x", mp.ellipsoid_x);
    nh.getParam("uneven_map/ellipsoid_y", mp.ellipsoid_y);
    nh.getParam("uneven_map/ellipsoid_z", mp.ellipsoid_z);
    nh.getParam("uneven_map/xy_resolution", mp.xy_resolution);
    nh.getParam("uneven_map/yaw_resolution", mp.yaw_resolution);
    nh.getParam("uneven_map/min_cnormal", mp.min_cnormal);
    nh.getParam("uneven_map/max_rho", mp.max_rho);
    nh.getParam("uneven_map/gravity", mp.gravity);
    return mp;
}
// rosparam manager/... of PlanManager::init (plan_manager/src/plan_manager.cpp:9-13), for optimizeSE2TrajBatch's initial-guess stage
template <class NodeHandle>
inline uph_manager_params loadManagerParams(NodeHandle& nh, uph_manager_params mg = uph_manager_params{0.3, 0.5, 1.2, 2.0, 0.05, 0, 0.5}) {
    nh.getParam("manager/piece_len", mg.piece_len);
    nh.getParam("manager/mean_vel", mg.mean_vel);
    nh.getParam("manager/init_time_times", mg.init_time_times);
    nh.getParam("manager/yaw_piece_times", mg.yaw_piece_times);
    nh.getParam("manager/init_sig_vel", mg.init_sig_vel);
    return mg;
}

class UnevenMapHandle {            // owns a uph_map; what UnevenMap::Ptr is to the reference's optimiser
public:
    // fp32_cells: store the cells as four floats (16 bytes) instead of four doubles -- km^2-scale grids (BASELINE.json configs[4])
    explicit UnevenMapHandle(const uph_map_params& mp, int device = 0, bool fp32_cells = false) {
        if ((fp32_cells ? uph_map_create_f32(&mp, device, &m_) : uph_map_create(&mp, device, &m_)) != UPH_OK)
            throw std::runtime_error(std::string("uph_map_create: ") + uph_last_error());
    }
    ~UnevenMapHandle() { uph_map_destroy(m_); }
    UnevenMapHandle(const UnevenMapHandle&) = delete;
    UnevenMapHandle& operator=(const UnevenMapHandle&) = delete;
    // UnevenMap::constructMap replacement: xyz = the cloud pcl::PCDReader delivered (n x 3 float)
    void constructMap(const float* xyz, long n) {
        int32_t d[3];
        uph_map_dims(m_, d);
        if (uph_map_build(m_, xyz, n, 0, d[0]) != UPH_OK) throw std::runtime_error(std::string("uph_map_build: ") + uph_last_error());
    }
    // constructMap from a cloud that is filtered already (crop box only, order kept; uph_map_build_filtered)
    void buildFilteredMap(const float* xyz, long n) {
        int32_t d[3];
        uph_map_dims(m_, d);
        if (uph_map_build_filtered(m_, xyz, n, 0, d[0]) != UPH_OK) throw std::runtime_error(std::string("uph_map_build_filtered: ") + uph_last_error());
    }
    // a new scan of a box (no counterpart in the reference): the world inside box = {x_min, x_max, y_min, y_max} is now `cloud` (n x 3 float; n = 0 removes
    // only).  Refits the columns the box reaches on the device; info.changed is the rect of columns whose cells or occupancy changed -- the trajectories to
    // hand to ALMTrajOpt::checkSE2TrajBatch are those that cross it (uph_map_update)
    void updateMap(const float box[4], const float* cloud, long n, uph_map_update_info& info) {
        if (uph_map_update(m_, box, n > 0 ? cloud : nullptr, n, &info) != UPH_OK) throw std::runtime_error(std::string("uph_map_update: ") + uph_last_error());
    }
    void updateMap(const float box[4], const std::vector<float>& cloud, uph_map_update_info& info) { updateMap(box, cloud.data(), (long)(cloud.size() / 3), info); }
    // UnevenMap::constructMapInput replacement: cells from the `.map` cache (ncell x 4: z, sigma, zb.x, zb.y in the reference's address order)
    void setCells(const double* rxs2) {
        if (uph_map_set_cells(m_, rxs2) != UPH_OK) throw std::runtime_error(std::string("uph_map_set_cells: ") + uph_last_error());
    }
    // the `.map` cache (uneven_map.cpp:166-167, 270-315, 400-412).  loadMap = constructMapInput: false when no cache can be read (build the map
    // then); it prefers the bit-exact side-car `<map_file>.bin` and falls back to the reference's CSV.  saveMap = the "to txt" block at the end of
    // constructMap -- the CSV the reference's own constructMapInput reads (six significant digits) -- plus the side-car.
    bool loadMap(const std::string& map_file) {
        int32_t src = 0;
        const int rc = uph_map_load_cache(m_, map_file.c_str(), (map_file + ".bin").c_str(), &src);
        if (rc == UPH_ERR_NO_CACHE) return false;      // build the map; every other failure surfaces instead of triggering a rebuild that overwrites the cache
        if (rc != UPH_OK) throw std::runtime_error(std::string("uph_map_load_cache: ") + uph_last_error());
        return true;
    }
    void saveMap(const std::string& map_file, bool with_sidecar = true) {
        const std::string bin = map_file + ".bin";
        if (uph_map_save_cache(m_, map_file.c_str(), with_sidecar ? bin.c_str() : nullptr) != UPH_OK) throw std::runtime_error(std::string("uph_map_save_cache: ") + uph_last_error());
    }
    // analytic fractal terrain instead of a cloud (configs[4]; no counterpart in the reference)
    void fillFractal(const uph_fbm_params& fp) {
        if (uph_map_fill_fbm(m_, &fp, 0, 0) != UPH_OK) throw std::runtime_error(std::string("uph_map_fill_fbm: ") + uph_last_error());
    }
    // fills the host members of the reference's UnevenMap (map_buffer as 4 doubles per cell, c_buffer, occ_buffer, occ_r2_buffer)
    void download(double* rxs2, double* c, char* occ, char* occ_r2) { uph_map_get_cells(m_, rxs2, c, occ, occ_r2); }
    uph_map* get() const { return m_; }
    // constructMap over several GPUs of this process: maps[g] lives on device g; x-slab fits on all devices at once, one RCCL all-gather inside
    // the library, every map ends up with the complete grid (uph_map_build_multi)
    static void constructMapMulti(const std::vector<UnevenMapHandle*>& maps, const float* xyz, long n) {
        std::vector<uph_map*> h;
        for (UnevenMapHandle* m : maps) h.push_back(m->get());
        if (uph_map_build_multi(h.data(), (int32_t)h.size(), xyz, n) != UPH_OK) throw std::runtime_error(std::string("uph_map_build_multi: ") + uph_last_error());
    }

private:
    uph_map* m_ = nullptr;
};

// one pose of the SE(3) path visSE3Traj publishes (UnevenMap::getTerrainPos, uneven_map.h:203-218): R column-major (x_b, y_b, z_b), then p
struct SE3Pose {
    double R[9];
    double p[3];
};

class ALMTrajOpt {
public:
    // ---- the reference's public parameter members (alm_traj_opt.h:29-53); defaults = plan_manager/params/run_hill.yaml:32-55
    double rho_T = 100000.0, rho_ter = 10.0, max_vel = 0.5, max_acc_lon = 5.0, max_acc_lat = 10.0, max_kap = 2.1, min_cxi = 0.8, max_sig = 0.05;
    bool use_scaling = true;
    double rho = 1.0, beta = 1000.0, gamma = 1.0, epsilon_con = 0.001, max_iter = 10.0;
    double g_epsilon = 1.0e-3, min_step = 1.0e-32, inner_max_iter = 10000.0, delta = 1.0e-4;
    int mem_size = 256, past = 3, int_K = 16;
    bool in_opt = false;
    bool in_test = false, in_debug = false;   // alm_traj_opt.h:56-57: loaded like the reference does; the test node's topics and the debug drawing stay on the host

    ALMTrajOpt() = default;
    ~ALMTrajOpt() { if (ctx_) uph_ctx_destroy(ctx_); }
    ALMTrajOpt(const ALMTrajOpt&) = delete;               // owns a device context (the reference's object is a value member that is never copied)
    ALMTrajOpt& operator=(const ALMTrajOpt&) = delete;

    // void ALMTrajOpt::init(ros::NodeHandle& nh)  (back_end/src/alm_traj_opt.cpp:5-29): the 21 optimiser keys + in_test / in_debug, read with
    // getParam exactly as the reference does -- a key the parameter server does not hold leaves the member as it was.  NodeHandle is a template
    // parameter (ros::NodeHandle in the workspace; anything with getParam(const std::string&, T&) elsewhere).  The publishers / subscribers of
    // :31-44 (RViz paths, the test node's goal topic) stay with the host.  Call order as in PlanManager::init (plan_manager.cpp:20-22):
    // init, setFrontend, setEnvironment -- setEnvironment hands the members to the device context.
    template <class NodeHandle>
    void init(NodeHandle& nh) {
        nh.getParam("alm_traj_opt/rho_T", rho_T);
        nh.getParam("alm_traj_opt/rho_ter", rho_ter);
        nh.getParam("alm_traj_opt/max_vel", max_vel);
        nh.getParam("alm_traj_opt/max_acc_lon", max_acc_lon);
        nh.getParam("alm_traj_opt/max_acc_lat", max_acc_lat);
        nh.getParam("alm_traj_opt/max_kap", max_kap);
        nh.getParam("alm_traj_opt/min_cxi", min_cxi);
        nh.getParam("alm_traj_opt/max_sig", max_sig);
        nh.getParam("alm_traj_opt/use_scaling", use_scaling);
        nh.getParam("alm_traj_opt/rho", rho);
        nh.getParam("alm_traj_opt/beta", beta);
        nh.getParam("alm_traj_opt/gamma", gamma);
        nh.getParam("alm_traj_opt/epsilon_con", epsilon_con);
        nh.getParam("alm_traj_opt/max_iter", max_iter);
        nh.getParam("alm_traj_opt/g_epsilon", g_epsilon);
        nh.getParam("alm_traj_opt/min_step", min_step);
        nh.getParam("alm_traj_opt/inner_max_iter", inner_max_iter);
        nh.getParam("alm_traj_opt/delta", delta);
        nh.getParam("alm_traj_opt/mem_size", mem_size);
        nh.getParam("alm_traj_opt/past", past);
        nh.getParam("alm_traj_opt/int_K", int_K);
        nh.getParam("alm_traj_opt/in_test", in_test);
        nh.getParam("alm_traj_opt/in_debug", in_debug);
    }

    // the members as the C-ABI's parameter block (what setEnvironment hands to uph_ctx_create)
    uph_opt_params optParams() const {
        uph_opt_params p;
        p.rho_T = rho_T; p.rho_ter = rho_ter; p.max_vel = max_vel; p.max_acc_lon = max_acc_lon; p.max_acc_lat = max_acc_lat;
        p.max_kap = max_kap; p.min_cxi = min_cxi; p.max_sig = max_sig; p.use_scaling = use_scaling ? 1 : 0;
        p.rho = rho; p.beta = beta; p.gamma = gamma; p.epsilon_con = epsilon_con; p.max_iter = max_iter;
        p.g_epsilon = g_epsilon; p.min_step = min_step; p.inner_max_iter = inner_max_iter; p.delta = delta;
        p.mem_size = mem_size; p.past = past; p.int_K = int_K;
        return p;
    }

    void setEnvironment(UnevenMapHandle* env) {          // alm_traj_opt.h:127-130
        env_ = env;
        if (ctx_) { uph_ctx_destroy(ctx_); ctx_ = nullptr; }
        const uph_opt_params p = optParams();
        if (uph_ctx_create(env->get(), &p, &ctx_) != UPH_OK) throw std::runtime_error(std::string("uph_ctx_create: ") + uph_last_error());
    }
    uph_ctx* get() const { return ctx_; }                // the device context (nullptr before setEnvironment), as UnevenMapHandle::get() is the map's

    // int ALMTrajOpt::optimizeSE2Traj(initStateXY 2x3, endStateXY 2x3, innerPtsXY 2x(Nxy-1), initYaw 3, endYaw 3, innerPtsYaw, totalTime)
    template <class MatXY, class MatIn, class VecYaw, class VecIn>
    int optimizeSE2Traj(const MatXY& initStateXY, const MatXY& endStateXY, const MatIn& innerPtsXY, const VecYaw& initYaw, const VecYaw& endYaw,
                        const VecIn& innerPtsYaw, const double& totalTime) {
        in_opt = true;
        uph_problem pr;
        pr.n_inner_xy = (int32_t)innerPtsXY.cols();
        pr.n_inner_yaw = (int32_t)innerPtsYaw.size();
        for (int k = 0; k < 6; k++) { pr.init_xy[k] = initStateXY.data()[k]; pr.end_xy[k] = endStateXY.data()[k]; }   // column-major 2x3
        for (int k = 0; k < 3; k++) { pr.init_yaw[k] = initYaw.data()[k]; pr.end_yaw[k] = endYaw.data()[k]; }
        pr.inner_xy = innerPtsXY.data();
        pr.inner_yaw = innerPtsYaw.data();
        pr.total_time = totalTime;
        const int Nxy = pr.n_inner_xy + 1, Nyaw = pr.n_inner_yaw + 1;
        cxy_.assign((size_t)12 * Nxy, 0.0);
        cyaw_.assign((size_t)6 * Nyaw, 0.0);
        x_.assign((size_t)2 * pr.n_inner_xy + pr.n_inner_yaw + 1, 0.0);
        uph_result rs{};
        rs.x_final = x_.data(); rs.c_xy = cxy_.data(); rs.c_yaw = cyaw_.data();
        const int rc = uph_optimize_batch(ctx_, 1, &pr, &rs);
        in_opt = false;
        last_multi_ = false;
        if (rc != UPH_OK) return 1;                       // solver error, as the reference reports a hard L-BFGS failure
        last_ = rs;
        rho = rs.rho_final;                               // rho is a member that persists (alm_traj_opt.h:137)
        return rs.ret_code;
    }

    SE2Trajectory getTraj() const {                        // alm_traj_opt.h:165-168
        return makeTraj(cxy_.data(), (int)cxy_.size() / 12, last_.piece_T_xy, cyaw_.data(), (int)cyaw_.size() / 6, last_.piece_T_yaw);
    }

    // ---- batch form (no counterpart in the reference: many candidate goals in one call).  paths[b] = the poses (x, y, yaw) the front-end
    // returned for goal b (kino_astar->plan, plan_manager.cpp:56-60; any container of things indexable by [0..2], e.g.
    // std::vector<Eigen::Vector3d>).  Runs the stage of plan_manager.cpp:62-132 for all of them (uph_resample_batch), one
    // uph_optimize_batch, and returns one trajectory + return code per path.  ret[b] == UPH_RET_UNSUPPORTED marks a path outside the
    // compiled limits (its trajectory is empty); rho is left as it was (a batch has no "next call").
    struct BatchPlan {
        std::vector<int> ret;
        std::vector<SE2Trajectory> traj;
        std::vector<double> jerk_cost, total_time;
    };
    // peers: optimisers bound to the OTHER GPUs' copies of the map (setEnvironment done); the batch is then split over this object's device
    // and theirs (uph_optimize_batch_multi: one host thread per device, results in the caller's order)
    template <class Path>
    BatchPlan optimizeSE2TrajBatch(const std::vector<Path>& paths, const uph_manager_params& mgr, const std::vector<ALMTrajOpt*>& peers = {}) {
        const int32_t B = (int32_t)paths.size(), cap_xy = 2 * UPH_MAX_PIECE_XY, cap_yaw = 2 * UPH_MAX_PIECE_YAW;
        BatchPlan out;
        if (B == 0) return out;
        std::vector<int64_t> off((size_t)B + 1, 0);
        for (int32_t b = 0; b < B; b++) off[b + 1] = off[b] + (int64_t)paths[b].size();
        std::vector<double> flat((size_t)off[B] * 3);
        for (int32_t b = 0; b < B; b++)
            for (size_t i = 0; i < paths[b].size(); i++)
                for (int k = 0; k < 3; k++) flat[((size_t)off[b] + i) * 3 + k] = paths[b][i][k];
        std::vector<double> ixy((size_t)B * 6), exy((size_t)B * 6), iyw((size_t)B * 3), eyw((size_t)B * 3), oxy((size_t)B * 2 * cap_xy), oyw((size_t)B * cap_yaw), tt(B);
        std::vector<int32_t> nxy(B), nyw(B);
        const int rrc = uph_resample_batch(&mgr, B, flat.data(), off.data(), cap_xy, cap_yaw, ixy.data(), exy.data(), iyw.data(), eyw.data(), oxy.data(), oyw.data(),
                                           nxy.data(), nyw.data(), tt.data(), nullptr);
        if (rrc != UPH_OK && rrc != UPH_ERR_LIMIT) throw std::runtime_error(std::string("uph_resample_batch: ") + uph_last_error());
        // UPH_ERR_LIMIT: some path needs more way-points than the buffers hold (the counts are still reported).  Such a path is far beyond
        // the compiled piece limits anyway: clamp its counts to just above them so that the upload marks exactly that slot UNSUPPORTED and
        // the other goals are solved (the documented contract), instead of failing the whole batch
        for (int32_t b = 0; b < B; b++)
            if (nxy[b] > cap_xy || nyw[b] > cap_yaw) { nxy[b] = UPH_MAX_PIECE_XY; nyw[b] = UPH_MAX_PIECE_YAW; }
        std::vector<uph_problem> pr(B);
        std::vector<uph_result> rs(B);
        std::vector<size_t> ox(B), oc(B), oy(B);
        size_t sx = 0, sc = 0, sy = 0;
        for (int32_t b = 0; b < B; b++) {
            ox[b] = sx; oc[b] = sc; oy[b] = sy;
            sx += (size_t)2 * nxy[b] + nyw[b] + 1; sc += (size_t)12 * (nxy[b] + 1); sy += (size_t)6 * (nyw[b] + 1);
        }
        std::vector<double> xs(sx, 0.0), cx(sc, 0.0), cy(sy, 0.0);
        for (int32_t b = 0; b < B; b++) {
            uph_problem& p = pr[b];
            p.n_inner_xy = nxy[b]; p.n_inner_yaw = nyw[b];
            for (int k = 0; k < 6; k++) { p.init_xy[k] = ixy[(size_t)6 * b + k]; p.end_xy[k] = exy[(size_t)6 * b + k]; }
            for (int k = 0; k < 3; k++) { p.init_yaw[k] = iyw[(size_t)3 * b + k]; p.end_yaw[k] = eyw[(size_t)3 * b + k]; }
            p.inner_xy = oxy.data() + (size_t)2 * cap_xy * b;
            p.inner_yaw = oyw.data() + (size_t)cap_yaw * b;
            p.total_time = tt[b];
            rs[b] = uph_result{};
            rs[b].x_final = xs.data() + ox[b]; rs[b].c_xy = cx.data() + oc[b]; rs[b].c_yaw = cy.data() + oy[b];
        }
        in_opt = true;
        std::vector<uph_ctx*> cs(1, ctx_);
        for (ALMTrajOpt* q : peers) cs.push_back(q->ctx_);
        last_report_.clear(); last_multi_ = false; last_ctxs_ = cs; last_B_ = B;
        const int rc = uph_optimize_batch_multi(cs.data(), (int32_t)cs.size(), B, pr.data(), rs.data());
        in_opt = false;
        if (rc != UPH_OK) throw std::runtime_error(std::string("uph_optimize_batch_multi: ") + uph_last_error());
        if (cs.size() > 1) {
            // the batch now lives in shares on several devices.  The report rows are fetched HERE, while every context still holds its share
            // of THIS batch (a peer may be destroyed or run another solve before the caller asks), and go back to the caller's order through
            // uph_batch_origin
            last_report_.assign((size_t)7 * B, 0.0);
            for (uph_ctx* c : cs) {
                const int n = uph_batch_count(c);
                if (n <= 0) continue;                                                     // (a device whose share was empty or wholly unsupported)
                std::vector<double> part((size_t)7 * n);
                std::vector<int32_t> idx(n);
                if (uph_report_batch(c, part.data()) != UPH_OK) throw std::runtime_error(std::string("uph_report_batch: ") + uph_last_error());
                if (uph_batch_origin(c, idx.data()) != UPH_OK) throw std::runtime_error(std::string("uph_batch_origin: ") + uph_last_error());
                for (int k = 0; k < n; k++)
                    if (idx[k] >= 0 && idx[k] < B) for (int q = 0; q < 7; q++) last_report_[(size_t)7 * idx[k] + q] = part[(size_t)7 * k + q];
            }
            last_multi_ = true;
        }
        for (int32_t b = 0; b < B; b++) {
            out.ret.push_back(rs[b].ret_code);
            out.jerk_cost.push_back(rs[b].jerk_cost);
            out.total_time.push_back(tt[b]);
            out.traj.push_back(rs[b].ret_code == UPH_RET_UNSUPPORTED ? SE2Trajectory()
                                   : makeTraj(cx.data() + oc[b], nxy[b] + 1, rs[b].piece_T_xy, cy.data() + oy[b], nyw[b] + 1, rs[b].piece_T_yaw));
        }
        return out;
    }
    // ---- goals in, trajectories out: PlanManager::rcvWpsCallBack (plan_manager.cpp:43-134) for many goals in one call with every stage on the
    // device (uph_plan_upload: kino->plan, the resampling stage of plan_manager.cpp:62-132 with `mgr`, the upload; then one solve).  One entry
    // per goal: status[b] = UPH_KINO_* of its search; a goal without a path has ret[b] = -1 and an empty trajectory (as planBatch returns an empty
    // path), traj_of[b] = -1; otherwise traj_of[b] = its index in the resident batch (getSE3PathBatch / getMaxVxAxAyCurAttSigBatch rows).  The
    // search context must be bound to the same map.  total_time[b] is the solved trajectory's duration Nxy x T_xy (the initial guess stays on the
    // device).  Defined after KinoAstar.
    struct GoalPlan : BatchPlan {
        std::vector<int32_t> status, traj_of;
    };
    template <class V3>
    GoalPlan planSE2TrajBatch(KinoAstar& kino, const std::vector<V3>& starts, const std::vector<V3>& goals, const uph_manager_params& mgr, int32_t path_cap = 0);
    // the same for a vehicle in motion (PlanManager's goal callback while a trajectory is being followed; uph_replan_upload): query q starts where
    // trajectory traj[q] of this object's last batch (index in it, as traj_of / getSE3PathBatch rows) is at t_switch[q] seconds from its start, with
    // its velocity, acceleration, yaw rate and yaw acceleration; goals (one per query) or nullptr: each source trajectory's own end pose (the map
    // changed, same goal).  The new batch replaces the last one on this object.  Same GoalPlan as planSE2TrajBatch.  Defined after KinoAstar.
    template <class V3 = VecN<3>>
    GoalPlan replanSE2TrajBatch(KinoAstar& kino, const std::vector<int>& traj, const std::vector<double>& t_switch, const std::vector<V3>* goals,
                                const uph_manager_params& mgr, int32_t path_cap = 0);
    GoalPlan replanSE2TrajBatch(KinoAstar& kino, const std::vector<int>& traj, const std::vector<double>& t_switch, std::nullptr_t, const uph_manager_params& mgr,
                                int32_t path_cap = 0) {
        return replanSE2TrajBatch<VecN<3>>(kino, traj, t_switch, static_cast<const std::vector<VecN<3>>*>(nullptr), mgr, path_cap);
    }
    // receding-horizon refinement without a search (uph_refine_upload): query q re-optimises the rest of trajectory traj[q] of this object's last batch
    // from its state at t_switch[q] to its problem's end boundary, the old trajectory as the initial guess, on the current map.  status[q] =
    // UPH_KINO_OK, or UPH_REFINE_AT_END for a switch at or past the end (ret -1, empty trajectory).  The new batch replaces the last one on this
    // object.  Same GoalPlan as planSE2TrajBatch; replanSE2TrajBatch (a new search) is the fallback for a refined solve that fails.
    GoalPlan refineSE2TrajBatch(const std::vector<int>& traj, const std::vector<double>& t_switch) {
        if (t_switch.size() != traj.size()) throw std::runtime_error("refineSE2TrajBatch: traj and t_switch differ in number");
        if (last_multi_) throw std::runtime_error("refineSE2TrajBatch: the last batch was split over several devices");
        const int32_t B = (int32_t)traj.size();
        GoalPlan out;
        if (B == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end()), nxy(B), nyw(B);
        out.status.assign((size_t)B, -1); out.traj_of.assign((size_t)B, -1);
        in_opt = true;
        const int rc = uph_refine_upload(ctx_, ctx_, B, tr.data(), t_switch.data(), nullptr, out.status.data(), out.traj_of.data(), nxy.data(), nyw.data());
        if (rc == UPH_ERR_INVALID && out.status[0] < 0) {            // refused: the last batch is still resident, nothing of it changes
            in_opt = false;
            throw std::runtime_error(std::string("uph_refine_upload: ") + uph_last_error());
        }
        last_report_.clear(); last_multi_ = false; last_ctxs_.assign(1, ctx_); last_B_ = 0;
        return finishGoalPlan(rc, B, out, nxy, nyw, "uph_refine_upload", "refineSE2TrajBatch");
    }
    // the map changed: which trajectories of this object's last batch does it invalidate, from when on and by which constraint (uph_check_batch).
    // Query q reduces the samples (every dt, + the end point with with_end) of trajectory traj[q] with t in [t_from[q], t_to[q]] (t_to empty: to the
    // end) on the map as it is now against lim7 (nullptr: the optimiser's own limits, checkLimits()).  Feeds refineSE2TrajBatch / replanSE2TrajBatch:
    // refine the violators from a little before first_t, check again, re-plan what is still bad.
    struct TrajCheck {
        std::vector<double> first_t;        // [n] t of the first violating sample (NaN: none)
        std::vector<int32_t> first_mask;    // [n] bit k: term k (vx, ax, ay, cur, att, sigma, non-holonomic error), bit UPH_CHECK_OCC_BIT: occupied
        std::vector<int32_t> counts;        // [n][3] samples, violating, occupied
        std::vector<double> worst, worst_t; // [n][7]
        bool violates(size_t q) const { return first_mask[q] != 0; }
    };
    std::vector<double> checkLimits() const {
        std::vector<double> lim(7);
        if (uph_check_limits(ctx_, lim.data()) != UPH_OK) throw std::runtime_error(std::string("uph_check_limits: ") + uph_last_error());
        return lim;
    }
    TrajCheck checkSE2TrajBatch(const std::vector<int>& traj, const std::vector<double>& t_from, const std::vector<double>& t_to = std::vector<double>(),
                                double dt = 0.01, bool with_end = true, const double* lim7 = nullptr) {
        if (t_from.size() != traj.size() || (!t_to.empty() && t_to.size() != traj.size())) throw std::runtime_error("checkSE2TrajBatch: traj, t_from and t_to differ in number");
        if (last_multi_) throw std::runtime_error("checkSE2TrajBatch: the last batch was split over several devices");
        const int32_t n = (int32_t)traj.size();
        TrajCheck out;
        if (n == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end());
        out.first_t.assign((size_t)n, 0.0); out.first_mask.assign((size_t)n, 0); out.counts.assign((size_t)3 * n, 0);
        out.worst.assign((size_t)7 * n, 0.0); out.worst_t.assign((size_t)7 * n, 0.0);
        if (uph_check_batch(ctx_, n, tr.data(), t_from.data(), t_to.empty() ? nullptr : t_to.data(), dt, with_end ? 1 : 0, lim7, out.first_t.data(),
                            out.first_mask.data(), out.counts.data(), out.worst.data(), out.worst_t.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_check_batch: ") + uph_last_error());
        return out;
    }
    // where is each vehicle on its trajectory: pose poses[q] = (x, y, yaw) in map coordinates (odometry) located on trajectory traj[q] of this object's
    // last batch among its samples with t in [t_from[q], t_to[q]] (t_to empty: to the end) -- the nearest sample, then the time refined between its
    // neighbours, the state there and the tracking error (uph_locate_batch).  t is the t_now / t_switch of checkSE2TrajBatch / refineSE2TrajBatch /
    // replanSE2TrajBatch; a large error says: plan again from the pose instead.
    struct TrajLocate {
        std::vector<double> near_t, near_d2;    // [n] the nearest sample and its squared distance
        std::vector<int32_t> count;             // [n] samples in the window (0: t is NaN)
        std::vector<double> t, d2;              // [n] the located time and the squared distance there
        std::vector<int32_t> refined;           // [n] 0: the sample itself was kept
        std::vector<double> state;              // [n][10] uph_traj_states' columns at t
        std::vector<double> err;                // [n][3] e_lon, e_lat, e_yaw
    };
    TrajLocate locateSE2TrajBatch(const std::vector<int>& traj, const std::vector<std::array<double, 3>>& poses, const std::vector<double>& t_from,
                                  const std::vector<double>& t_to = std::vector<double>(), double dt = 0.01, bool with_end = true) {
        if (poses.size() != traj.size() || t_from.size() != traj.size() || (!t_to.empty() && t_to.size() != traj.size()))
            throw std::runtime_error("locateSE2TrajBatch: traj, poses, t_from and t_to differ in number");
        if (last_multi_) throw std::runtime_error("locateSE2TrajBatch: the last batch was split over several devices");
        const int32_t n = (int32_t)traj.size();
        TrajLocate out;
        if (n == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end());
        std::vector<double> ps((size_t)3 * n);
        for (int32_t q = 0; q < n; q++) for (int k = 0; k < 3; k++) ps[(size_t)3 * q + k] = poses[(size_t)q][k];
        out.near_t.assign((size_t)n, 0.0); out.near_d2.assign((size_t)n, 0.0); out.count.assign((size_t)n, 0); out.t.assign((size_t)n, 0.0);
        out.d2.assign((size_t)n, 0.0); out.refined.assign((size_t)n, 0); out.state.assign((size_t)10 * n, 0.0); out.err.assign((size_t)3 * n, 0.0);
        if (uph_locate_batch(ctx_, n, tr.data(), ps.data(), t_from.data(), t_to.empty() ? nullptr : t_to.data(), dt, with_end ? 1 : 0, out.near_t.data(),
                             out.near_d2.data(), out.count.data(), out.t.data(), out.refined.data(), out.state.data(), out.d2.data(), out.err.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_locate_batch: ") + uph_last_error());
        return out;
    }
    // a region of the map changed (UnevenMapHandle's update: `changed`): which trajectories of the last batch have samples inside the closed rect
    // rects[q] = (x0, x1, y0, y1) in map coordinates, with t in [t_from[q], t_to[q]], and when they enter and leave it (uph_within_batch).  Those are
    // the ones to hand to checkSE2TrajBatch.
    struct TrajWithin {
        std::vector<double> enter_t, leave_t;   // [n] t of the first / last sample inside (NaN: none)
        std::vector<int32_t> counts;            // [n][2] samples, inside
        bool enters(size_t q) const { return counts[2 * q + 1] > 0; }
    };
    TrajWithin withinSE2TrajBatch(const std::vector<int>& traj, const std::vector<std::array<double, 4>>& rects, const std::vector<double>& t_from,
                                  const std::vector<double>& t_to = std::vector<double>(), double dt = 0.01, bool with_end = true) {
        if (rects.size() != traj.size() || t_from.size() != traj.size() || (!t_to.empty() && t_to.size() != traj.size()))
            throw std::runtime_error("withinSE2TrajBatch: traj, rects, t_from and t_to differ in number");
        if (last_multi_) throw std::runtime_error("withinSE2TrajBatch: the last batch was split over several devices");
        const int32_t n = (int32_t)traj.size();
        TrajWithin out;
        if (n == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end());
        std::vector<double> rc((size_t)4 * n);
        for (int32_t q = 0; q < n; q++) for (int k = 0; k < 4; k++) rc[(size_t)4 * q + k] = rects[(size_t)q][k];
        out.enter_t.assign((size_t)n, 0.0); out.leave_t.assign((size_t)n, 0.0); out.counts.assign((size_t)2 * n, 0);
        if (uph_within_batch(ctx_, n, tr.data(), rc.data(), t_from.data(), t_to.empty() ? nullptr : t_to.data(), dt, with_end ? 1 : 0, out.enter_t.data(),
                             out.leave_t.data(), out.counts.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_within_batch: ") + uph_last_error());
        return out;
    }
    // ---- the trajectories of a fleet against each other.  Every trajectory counts time from its own start; on the clock the fleet shares, vehicle q starts
    // at t0[q].  A window [t_from, t_to] of that clock is sampled at tau_k = t_from + k dt; a vehicle stands at its start before t0 and at its goal after its
    // end.  The bounding box of each vehicle's positions over its window (uph_extent_batch): the input of a broad phase.
    struct TrajExtent {
        std::vector<double> box;                // [n][4] xmin, xmax, ymin, ymax in map coordinates ((+inf, -inf, +inf, -inf): no sample)
        std::vector<int32_t> counts;            // [n][2] samples, NaN samples
    };
    TrajExtent extentSE2TrajBatch(const std::vector<int>& traj, const std::vector<double>& t0, const std::vector<double>& t_from, const std::vector<double>& t_to,
                                  double dt = 0.01) {
        if (t0.size() != traj.size() || t_from.size() != traj.size() || t_to.size() != traj.size())
            throw std::runtime_error("extentSE2TrajBatch: traj, t0, t_from and t_to differ in number");
        if (last_multi_) throw std::runtime_error("extentSE2TrajBatch: the last batch was split over several devices");
        const int32_t n = (int32_t)traj.size();
        TrajExtent out;
        if (n == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end());
        out.box.assign((size_t)4 * n, 0.0); out.counts.assign((size_t)2 * n, 0);
        if (uph_extent_batch(ctx_, n, tr.data(), t0.data(), t_from.data(), t_to.data(), dt, out.box.data(), out.counts.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_extent_batch: ") + uph_last_error());
        return out;
    }
    // how close vehicle a = (traj_a[q], t0_a[q]) of this object's last batch and vehicle b = (traj_b[q], t0_b[q]) of `other`'s last batch (nullptr: this
    // object's; a refined batch against the fleet it came from is the main use) come over [t_from[q], t_to[q]], and when they are closer than radius[q]
    // (uph_separation_batch).  Before a refined or re-planned trajectory is handed to its vehicle.
    struct TrajSeparation {
        std::vector<double> min_d2, min_t;      // [n] the smallest squared distance and its time on the common clock (+inf, NaN: no sample)
        std::vector<double> first_t, last_t;    // [n] the first / last sample with d2 < radius^2 (NaN: none)
        std::vector<int32_t> counts;            // [n][2] samples, below
        bool conflicts(size_t q) const { return counts[2 * q + 1] > 0; }
    };
    TrajSeparation separationSE2TrajBatch(const std::vector<int>& traj_a, const std::vector<int>& traj_b, const std::vector<double>& t0_a, const std::vector<double>& t0_b,
                                          const std::vector<double>& t_from, const std::vector<double>& t_to, const std::vector<double>& radius, double dt = 0.01,
                                          const ALMTrajOpt* other = nullptr) {
        const size_t m = traj_a.size();
        pairCheck("separationSE2TrajBatch", m, {traj_b.size(), t0_a.size(), t0_b.size(), t_from.size(), t_to.size(), radius.size()}, other);
        const int32_t n = (int32_t)m;
        TrajSeparation out;
        if (n == 0) return out;
        std::vector<int32_t> ta(traj_a.begin(), traj_a.end()), tb(traj_b.begin(), traj_b.end());
        out.min_d2.assign(m, 0.0); out.min_t.assign(m, 0.0); out.first_t.assign(m, 0.0); out.last_t.assign(m, 0.0); out.counts.assign(2 * m, 0);
        if (uph_separation_batch(ctx_, other ? other->ctx_ : nullptr, n, ta.data(), tb.data(), t0_a.data(), t0_b.data(), t_from.data(), t_to.data(), dt, radius.data(),
                                 out.min_d2.data(), out.min_t.data(), out.first_t.data(), out.last_t.data(), out.counts.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_separation_batch: ") + uph_last_error());
        return out;
    }
    // the whole fleet at once: vehicles (traj[i], t0[i]) of this object's last batch, each a disc of radius[i], one window.  Every pair (i < j, indices into
    // traj) with a sample closer than radius[i] + radius[j], in (i, j) order (uph_conflicts_batch: extents, a host broad phase, separation of its candidates).
    struct TrajConflicts {
        std::vector<std::array<int32_t, 2>> pairs;      // [m]
        std::vector<double> min_d2, min_t, first_t, last_t;
        std::vector<int32_t> below;                     // [m] samples below
        int64_t n_conflicts = 0, n_candidates = 0;      // all conflicts (m of them are listed); pairs the broad phase kept
    };
    TrajConflicts conflictsSE2TrajBatch(const std::vector<int>& traj, const std::vector<double>& t0, const std::vector<double>& radius, double t_from, double t_to,
                                        double dt = 0.05, int64_t cap = -1) {
        if (t0.size() != traj.size() || radius.size() != traj.size()) throw std::runtime_error("conflictsSE2TrajBatch: traj, t0 and radius differ in number");
        if (last_multi_) throw std::runtime_error("conflictsSE2TrajBatch: the last batch was split over several devices");
        const int32_t n = (int32_t)traj.size();
        TrajConflicts out;
        if (n == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end());
        conflictList(out, out.min_d2, n, cap, "uph_conflicts_batch", [&](int64_t room, int32_t* pairs, double* rows, int32_t* below) {
            return uph_conflicts_batch(ctx_, n, tr.data(), t0.data(), radius.data(), t_from, t_to, dt, room, pairs, rows, below, &out.n_conflicts, &out.n_candidates);
        });
        return out;
    }
    // ---- the same two with the vehicles as oriented rectangles: shape = {front, rear, half_width} in metres around the trajectory's point, turned by its yaw.
    // For car-like vehicles in corridors, where the disc that covers a car reports vehicles passing side by side or following nose to tail.  margin[q] is the
    // clearance the pair must keep (0: only an overlap counts); a sample is below when the rectangles overlap or are closer than the margin
    // (uph_footprint_separation_batch).
    struct TrajFootprintSeparation {
        std::vector<double> min_c2, min_t;      // [n] the smallest squared distance between the rectangles (0: they overlap) and its time (+inf, NaN: no sample)
        std::vector<double> first_t, last_t;    // [n] the first / last sample below (NaN: none)
        std::vector<int32_t> counts;            // [n][3] samples, below, overlapping
        bool conflicts(size_t q) const { return counts[3 * q + 1] > 0; }
        bool overlaps(size_t q) const { return counts[3 * q + 2] > 0; }
    };
    TrajFootprintSeparation footprintSeparationSE2TrajBatch(const std::vector<int>& traj_a, const std::vector<int>& traj_b, const std::vector<double>& t0_a,
                                                            const std::vector<double>& t0_b, const std::vector<double>& t_from, const std::vector<double>& t_to,
                                                            const std::vector<std::array<double, 3>>& shape_a, const std::vector<std::array<double, 3>>& shape_b,
                                                            const std::vector<double>& margin, double dt = 0.01, const ALMTrajOpt* other = nullptr) {
        const size_t m = traj_a.size();
        pairCheck("footprintSeparationSE2TrajBatch", m, {traj_b.size(), t0_a.size(), t0_b.size(), t_from.size(), t_to.size(), shape_a.size(), shape_b.size(), margin.size()},
                  other);
        const int32_t n = (int32_t)m;
        TrajFootprintSeparation out;
        if (n == 0) return out;
        std::vector<int32_t> ta(traj_a.begin(), traj_a.end()), tb(traj_b.begin(), traj_b.end());
        out.min_c2.assign(m, 0.0); out.min_t.assign(m, 0.0); out.first_t.assign(m, 0.0); out.last_t.assign(m, 0.0); out.counts.assign(3 * m, 0);
        if (uph_footprint_separation_batch(ctx_, other ? other->ctx_ : nullptr, n, ta.data(), tb.data(), t0_a.data(), t0_b.data(), t_from.data(), t_to.data(), dt,
                                           shape_a[0].data(), shape_b[0].data(), margin.data(), out.min_c2.data(), out.min_t.data(), out.first_t.data(),
                                           out.last_t.data(), out.counts.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_footprint_separation_batch: ") + uph_last_error());
        return out;
    }
    // the whole fleet with rectangles: vehicles (traj[i], t0[i]) with shape[i] and margin[i], one window.  Every pair (i < j) with a sample that overlaps or is
    // closer than margin[i] + margin[j], in (i, j) order (uph_footprint_conflicts_batch: extents, a host broad phase on the circumscribed radii, the
    // footprint separation of its candidates).  footprintDelaysSE2TrajBatch clears these pairs with the same rectangles; delaysSE2TrajBatch with the radii
    // hypot(max(front, rear), half_width) + margin clears them too, but also postpones passes that the rectangles allow.
    struct TrajFootprintConflicts {
        std::vector<std::array<int32_t, 2>> pairs;      // [m]
        std::vector<double> min_c2, min_t, first_t, last_t;
        std::vector<int32_t> below;                     // [m] samples below
        int64_t n_conflicts = 0, n_candidates = 0;      // all conflicts (m of them are listed); pairs the broad phase kept
    };
    TrajFootprintConflicts footprintConflictsSE2TrajBatch(const std::vector<int>& traj, const std::vector<double>& t0, const std::vector<std::array<double, 3>>& shape,
                                                          const std::vector<double>& margin, double t_from, double t_to, double dt = 0.05, int64_t cap = -1) {
        if (t0.size() != traj.size() || shape.size() != traj.size() || margin.size() != traj.size())
            throw std::runtime_error("footprintConflictsSE2TrajBatch: traj, t0, shape and margin differ in number");
        if (last_multi_) throw std::runtime_error("footprintConflictsSE2TrajBatch: the last batch was split over several devices");
        const int32_t n = (int32_t)traj.size();
        TrajFootprintConflicts out;
        if (n == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end());
        conflictList(out, out.min_c2, n, cap, "uph_footprint_conflicts_batch", [&](int64_t room, int32_t* pairs, double* rows, int32_t* below) {
            return uph_footprint_conflicts_batch(ctx_, n, tr.data(), t0.data(), shape[0].data(), margin.data(), t_from, t_to, dt, room, pairs, rows, below, &out.n_conflicts,
                                                 &out.n_candidates);
        });
        return out;
    }
    // the map changed: does the BODY of a vehicle touch an occupied column, when first, and where (uph_footprint_check_batch).  checkSE2TrajBatch reads the
    // occupancy under the trajectory's point; this reads every column whose centre lies in the rectangle shape[q] = (front, rear, half_width) inflated by
    // margin[q] (empty: 0) and turned by the raw yaw, over the samples of trajectory traj[q] with t in [t_from[q], t_to[q]] (t_to empty: to the end).  layers:
    // the kinds (UPH_FOOT_OCC_XY, UPH_FOOT_OCC_YAW, UPH_FOOT_OUTSIDE) that make a column a hit.  The recipe after a map update: withinSE2TrajBatch with the
    // changed rect grown by uph_footprint_radii's radius, this on the trajectories that enter it, refineSE2TrajBatch / replanSE2TrajBatch from before first_t.
    struct TrajFootprintCheck {
        std::vector<double> first_t, last_t;            // [n] t of the first / last hit sample (NaN: none)
        std::vector<int32_t> first_mask;                // [n] the kinds within layers at the first hit sample
        std::vector<std::array<int32_t, 2>> first_cell; // [n] the smallest (ix, iy) among its hit columns ((-1, -1): none)
        std::vector<int32_t> counts;                    // [n][5] samples, hit samples, samples covering a column of kind XY / YAW / OUTSIDE
        std::vector<int64_t> cells;                     // [n][2] covered columns, hit columns, summed over the samples
        bool hits(size_t q) const { return counts[5 * q + 1] > 0; }
    };
    TrajFootprintCheck footprintCheckSE2TrajBatch(const std::vector<int>& traj, const std::vector<double>& t_from, const std::vector<double>& t_to,
                                                  const std::vector<std::array<double, 3>>& shape, const std::vector<double>& margin = std::vector<double>(),
                                                  int layers = UPH_FOOT_ALL, double dt = 0.01, bool with_end = true) {
        if (t_from.size() != traj.size() || (!t_to.empty() && t_to.size() != traj.size()) || shape.size() != traj.size() || (!margin.empty() && margin.size() != traj.size()))
            throw std::runtime_error("footprintCheckSE2TrajBatch: traj, t_from, t_to, shape and margin differ in number");
        if (last_multi_) throw std::runtime_error("footprintCheckSE2TrajBatch: the last batch was split over several devices");
        const int32_t n = (int32_t)traj.size();
        TrajFootprintCheck out;
        if (n == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end());
        out.first_t.assign((size_t)n, 0.0); out.last_t.assign((size_t)n, 0.0); out.first_mask.assign((size_t)n, 0);
        out.first_cell.assign((size_t)n, std::array<int32_t, 2>{-1, -1}); out.counts.assign((size_t)5 * n, 0); out.cells.assign((size_t)2 * n, 0);
        if (uph_footprint_check_batch(ctx_, n, tr.data(), t_from.data(), t_to.empty() ? nullptr : t_to.data(), dt, with_end ? 1 : 0, shape[0].data(),
                                      margin.empty() ? nullptr : margin.data(), layers, out.first_t.data(), out.last_t.data(), out.first_mask.data(),
                                      out.first_cell[0].data(), out.counts.data(), out.cells.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_footprint_check_batch: ") + uph_last_error());
        return out;
    }
    // how much room the body has along the last batch's trajectories (uph_clearance_check_batch): the ClearanceLayer's value at the cell of every sample's point
    // and yaw bin, over the samples of trajectory traj[q] with t in [t_from[q], t_to[q]] (t_to empty: to the end).  below2[q], in squared cells, marks the
    // samples that count as close (ClearanceLayer::below2 converts metres).  The layer must be fresh and of this optimiser's map.
    struct TrajClearance {
        std::vector<int32_t> min_d2;                    // [n] the smallest value (-1: empty window; UPH_CLEAR_FAR: nothing within rmax)
        std::vector<double> min_t;                      // [n] t of the earliest sample at the min (NaN: empty window)
        std::vector<std::array<int32_t, 3>> min_cell;   // [n] its cell (ix, iy, iw) ((-1, -1, -1): empty window, or that sample is outside the grid)
        std::vector<double> first_t, last_t;            // [n] t of the first / last sample with a value below below2[q] (NaN: none)
        std::vector<int32_t> counts;                    // [n][4] samples, below, outside, far
        double metres(size_t q, double res) const { return min_d2[q] < 0 ? std::nan("") : min_d2[q] == UPH_CLEAR_FAR ? HUGE_VAL : res * std::sqrt((double)min_d2[q]); }
    };
    TrajClearance clearanceSE2TrajBatch(const ClearanceLayer& layer, const std::vector<int>& traj, const std::vector<double>& t_from, const std::vector<double>& t_to,
                                        const std::vector<int32_t>& below2, double dt = 0.01, bool with_end = true);
    // ---- the clearance term of the objective (uph_ctx_set_clearance_term, no counterpart in the reference): every sample closer than d_safe metres to an
    // obstacle of `layer` (polarity UPH_CLEAR_TO_OCCUPIED, of this map, fresh) adds weight * step * scale_fx * (d_safe - c)^2 to the cost.  Persists on the
    // context -- until setEnvironment makes a new one -- and applies to every later solve, whoever uploaded the batch; nullptr switches it off.  The layer
    // must outlive the term: its destruction is refused while the context names it.
    struct ClearanceTerm {
        uph_clearance* layer = nullptr;     // nullptr: off
        double d_safe = 0.0, weight = 0.0;
    };
    void setClearanceTerm(const ClearanceLayer* layer, double d_safe = 0.0, double weight = 0.0);
    ClearanceTerm clearanceTerm() const {
        ClearanceTerm t;
        if (uph_ctx_clearance_term(ctx_, &t.layer, &t.d_safe, &t.weight) != UPH_OK) throw std::runtime_error(std::string("uph_ctx_clearance_term: ") + uph_last_error());
        return t;
    }
    // ---- clearing conflicts by starting later.  A delayed vehicle drives the same trajectory, so nothing the check has passed changes; the delays are
    // delta_j = delay0 + j * delay_step, 0 <= j < D.  separationSE2TrajBatch of a against b started at t0_b[q] + delta_j, for every j, in one call
    // (uph_delay_sweep_batch).
    struct TrajDelaySweep {
        int32_t D = 0;
        std::vector<double> min_d2, min_t;      // [n][D]
        std::vector<int32_t> below;             // [n][D] samples below
        std::vector<int32_t> first_clear;       // [n] the smallest j with below == 0 (-1: none)
        std::vector<int32_t> counts;            // [n] samples of the window
    };
    TrajDelaySweep delaySweepSE2TrajBatch(const std::vector<int>& traj_a, const std::vector<int>& traj_b, const std::vector<double>& t0_a, const std::vector<double>& t0_b,
                                          const std::vector<double>& t_from, const std::vector<double>& t_to, const std::vector<double>& radius, double delay0,
                                          double delay_step, int D, double dt = 0.01, const ALMTrajOpt* other = nullptr) {
        const size_t m = traj_a.size();
        pairCheck("delaySweepSE2TrajBatch", m, {traj_b.size(), t0_a.size(), t0_b.size(), t_from.size(), t_to.size(), radius.size()}, other);
        TrajDelaySweep out;
        out.D = (int32_t)D;
        if (m == 0) return out;
        const size_t rows = m * (size_t)std::max(D, 1);
        std::vector<int32_t> ta(traj_a.begin(), traj_a.end()), tb(traj_b.begin(), traj_b.end());
        out.min_d2.assign(rows, 0.0); out.min_t.assign(rows, 0.0); out.below.assign(rows, 0); out.first_clear.assign(m, -1); out.counts.assign(m, 0);
        if (uph_delay_sweep_batch(ctx_, other ? other->ctx_ : nullptr, (int32_t)m, ta.data(), tb.data(), t0_a.data(), t0_b.data(), t_from.data(), t_to.data(), dt,
                                  radius.data(), delay0, delay_step, (int32_t)D, out.min_d2.data(), out.min_t.data(), out.below.data(), out.first_clear.data(),
                                  out.counts.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_delay_sweep_batch: ") + uph_last_error());
        return out;
    }
    // the box that holds a vehicle under every delay of the table (uph_delay_extent_batch): the broad phase on these boxes holds whatever delays are chosen
    TrajExtent delayExtentSE2TrajBatch(const std::vector<int>& traj, const std::vector<double>& t0, const std::vector<double>& t_from, const std::vector<double>& t_to,
                                       double delay0, double delay_step, int D, double dt = 0.01) {
        if (t0.size() != traj.size() || t_from.size() != traj.size() || t_to.size() != traj.size())
            throw std::runtime_error("delayExtentSE2TrajBatch: traj, t0, t_from and t_to differ in number");
        if (last_multi_) throw std::runtime_error("delayExtentSE2TrajBatch: the last batch was split over several devices");
        const int32_t n = (int32_t)traj.size();
        TrajExtent out;
        if (n == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end());
        out.box.assign((size_t)4 * n, 0.0); out.counts.assign((size_t)2 * n, 0);
        if (uph_delay_extent_batch(ctx_, n, tr.data(), t0.data(), t_from.data(), t_to.data(), dt, delay0, delay_step, (int32_t)D, out.box.data(), out.counts.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_delay_extent_batch: ") + uph_last_error());
        return out;
    }
    // the fleet in priority order (the smaller index goes first): every vehicle gets the smallest delay -- among its first n_delays[i], empty: all D -- that
    // clears it against all vehicles ahead of it at their chosen starts (uph_delays_batch).  After conflictsSE2TrajBatch has reported pairs; the vehicles left
    // with choice == -1 go to replanSE2TrajBatch / refineSE2TrajBatch.
    struct TrajDelays {
        std::vector<int32_t> choice;            // [n] index into the table; -1: no delay clears the vehicle (it stays at delay 0)
        std::vector<double> start;              // [n] the effective start on the common clock
        std::vector<int32_t> blocker;           // [n] the first vehicle in the way of an unresolved one, else -1
        int64_t n_candidates = 0;
        int32_t n_rounds = 0, n_unresolved = 0;
    };
    TrajDelays delaysSE2TrajBatch(const std::vector<int>& traj, const std::vector<double>& t0, const std::vector<double>& radius, double t_from, double t_to,
                                  double delay0, double delay_step, int D, const std::vector<int>& n_delays = std::vector<int>(), double dt = 0.05) {
        if (t0.size() != traj.size() || radius.size() != traj.size() || (!n_delays.empty() && n_delays.size() != traj.size()))
            throw std::runtime_error("delaysSE2TrajBatch: traj, t0, radius and n_delays differ in number");
        if (last_multi_) throw std::runtime_error("delaysSE2TrajBatch: the last batch was split over several devices");
        const int32_t n = (int32_t)traj.size();
        TrajDelays out;
        if (n == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end()), nd(n_delays.begin(), n_delays.end());
        out.choice.assign((size_t)n, 0); out.start.assign((size_t)n, 0.0); out.blocker.assign((size_t)n, -1);
        if (uph_delays_batch(ctx_, n, tr.data(), t0.data(), radius.data(), nd.empty() ? nullptr : nd.data(), t_from, t_to, dt, delay0, delay_step, (int32_t)D,
                             out.choice.data(), out.start.data(), out.blocker.data(), &out.n_candidates, &out.n_rounds, &out.n_unresolved) != UPH_OK)
            throw std::runtime_error(std::string("uph_delays_batch: ") + uph_last_error());
        return out;
    }
    // ---- clearing the conflicts of footprintConflictsSE2TrajBatch by starting later, with the same rectangles: no vehicle waits for a pass side by side or
    // nose to tail that the rectangles allow (delaysSE2TrajBatch on the circumscribed discs would make it wait).  footprintSeparationSE2TrajBatch of a against
    // b started at t0_b[q] + delta_j, for every j, in one call and bit for bit (uph_footprint_delay_sweep_batch).
    struct TrajFootprintDelaySweep {
        int32_t D = 0;
        std::vector<double> min_c2, min_t;      // [n][D]
        std::vector<int32_t> below;             // [n][D] samples below
        std::vector<int32_t> overlapping;       // [n][D] samples that overlap
        std::vector<int32_t> first_clear;       // [n] the smallest j with below == 0 (-1: none)
        std::vector<int32_t> counts;            // [n] samples of the window
    };
    TrajFootprintDelaySweep footprintDelaySweepSE2TrajBatch(const std::vector<int>& traj_a, const std::vector<int>& traj_b, const std::vector<double>& t0_a,
                                                            const std::vector<double>& t0_b, const std::vector<double>& t_from, const std::vector<double>& t_to,
                                                            const std::vector<std::array<double, 3>>& shape_a, const std::vector<std::array<double, 3>>& shape_b,
                                                            const std::vector<double>& margin, double delay0, double delay_step, int D, double dt = 0.01,
                                                            const ALMTrajOpt* other = nullptr) {
        const size_t m = traj_a.size();
        pairCheck("footprintDelaySweepSE2TrajBatch", m, {traj_b.size(), t0_a.size(), t0_b.size(), t_from.size(), t_to.size(), shape_a.size(), shape_b.size(), margin.size()},
                  other);
        TrajFootprintDelaySweep out;
        out.D = (int32_t)D;
        if (m == 0) return out;
        const size_t rows = m * (size_t)std::max(D, 1);
        std::vector<int32_t> ta(traj_a.begin(), traj_a.end()), tb(traj_b.begin(), traj_b.end());
        out.min_c2.assign(rows, 0.0); out.min_t.assign(rows, 0.0); out.below.assign(rows, 0); out.overlapping.assign(rows, 0); out.first_clear.assign(m, -1);
        out.counts.assign(m, 0);
        if (uph_footprint_delay_sweep_batch(ctx_, other ? other->ctx_ : nullptr, (int32_t)m, ta.data(), tb.data(), t0_a.data(), t0_b.data(), t_from.data(), t_to.data(), dt,
                                            shape_a[0].data(), shape_b[0].data(), margin.data(), delay0, delay_step, (int32_t)D, out.min_c2.data(), out.min_t.data(),
                                            out.below.data(), out.overlapping.data(), out.first_clear.data(), out.counts.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_footprint_delay_sweep_batch: ") + uph_last_error());
        return out;
    }
    // the fleet in priority order with rectangles: delaysSE2TrajBatch with shape[i] and margin[i] for radius[i] (uph_footprint_delays_batch).  After
    // footprintConflictsSE2TrajBatch has reported pairs; with the returned starts it reports none whose later vehicle was placed.
    TrajDelays footprintDelaysSE2TrajBatch(const std::vector<int>& traj, const std::vector<double>& t0, const std::vector<std::array<double, 3>>& shape,
                                           const std::vector<double>& margin, double t_from, double t_to, double delay0, double delay_step, int D,
                                           const std::vector<int>& n_delays = std::vector<int>(), double dt = 0.05) {
        if (t0.size() != traj.size() || shape.size() != traj.size() || margin.size() != traj.size() || (!n_delays.empty() && n_delays.size() != traj.size()))
            throw std::runtime_error("footprintDelaysSE2TrajBatch: traj, t0, shape, margin and n_delays differ in number");
        if (last_multi_) throw std::runtime_error("footprintDelaysSE2TrajBatch: the last batch was split over several devices");
        const int32_t n = (int32_t)traj.size();
        TrajDelays out;
        if (n == 0) return out;
        std::vector<int32_t> tr(traj.begin(), traj.end()), nd(n_delays.begin(), n_delays.end());
        out.choice.assign((size_t)n, 0); out.start.assign((size_t)n, 0.0); out.blocker.assign((size_t)n, -1);
        if (uph_footprint_delays_batch(ctx_, n, tr.data(), t0.data(), shape[0].data(), margin.data(), nd.empty() ? nullptr : nd.data(), t_from, t_to, dt, delay0,
                                       delay_step, (int32_t)D, out.choice.data(), out.start.data(), out.blocker.data(), &out.n_candidates, &out.n_rounds,
                                       &out.n_unresolved) != UPH_OK)
            throw std::runtime_error(std::string("uph_footprint_delays_batch: ") + uph_last_error());
        return out;
    }
    double getTrajJerkCost() const { return last_.jerk_cost; }   // minco_se2.getTrajJerkCost() (alm_traj_opt.cpp:273)

    // getMaxVxAxAyCurAttSig (alm_traj_opt.h:170-229): max vx, ax, ay, curvature, attitude (-cos xi), sigma sampled every 0.01 s -- evaluated
    // on the device for the trajectory of the last optimizeSE2Traj (the argument is what getTraj() returned for it)
    std::vector<double> getMaxVxAxAyCurAttSig(const SE2Trajectory&) {
        const std::vector<double> all = getMaxVxAxAyCurAttSigBatch();     // (after optimizeSE2TrajBatch the context holds B trajectories: row 0)
        return std::vector<double>(all.begin(), all.begin() + 6);
    }
    // the same report for every trajectory of the last call: [B][7] = max vx, ax, ay, cur, att, sigma, non-holonomic error (rows of
    // UPH_RET_UNSUPPORTED problems describe a placeholder, not a path)
    // After a call with `peers` the rows were collected from every device's share at the end of that call (cached here).
    std::vector<double> getMaxVxAxAyCurAttSigBatch() {
        if (last_multi_) return last_report_;
        const int B = uph_batch_count(ctx_);
        if (B <= 0) throw std::runtime_error("getMaxVxAxAyCurAttSig: no trajectory has been optimised on this object");
        std::vector<double> o((size_t)7 * B, 0.0);
        if (uph_report_batch(ctx_, o.data()) != UPH_OK) throw std::runtime_error(std::string("uph_report_batch: ") + uph_last_error());
        return o;
    }
    // members PlanManager calls that have no device side: the A* handle, RViz output
    template <class FrontendPtr> void setFrontend(const FrontendPtr&) {}
    void visSE2Traj(const SE2Trajectory&) {}
    void visSE3Traj(const SE2Trajectory&) {}

    // visSE3Traj's path (alm_traj_opt.cpp:1102-1135) without the publishing: the trajectory of the last optimizeSE2Traj sampled at
    // t = 0, dt, 2 dt ... (the running sum t += dt) below its duration, plus the end point, each as UnevenMap::getTerrainPos of
    // getNormSE2Pos(t) -- rolled out on the device (uph_rollout_batch)
    std::vector<SE3Pose> getSE3Path(double dt = 0.03) {
        if (last_multi_) return getSE3PathBatch(dt).at(0);
        return rolloutPoses(ctx_, dt, 0, 1).at(0);
    }
    // the same for every trajectory of the last call, in the caller's order (an UPH_RET_UNSUPPORTED problem has an empty path).  After a call with
    // `peers` the rows come from every device's share: the peers must still hold that batch (not destroyed, no other batch uploaded since)
    std::vector<std::vector<SE3Pose>> getSE3PathBatch(double dt = 0.03) {
        if (!last_multi_) return rolloutPoses(ctx_, dt, 0, -1);
        std::vector<std::vector<SE3Pose>> out((size_t)last_B_);
        int32_t seen = 0;
        for (uph_ctx* c : last_ctxs_) {
            const int n = uph_batch_count(c);
            if (n <= 0) continue;
            std::vector<int32_t> idx(n);
            if (uph_batch_origin(c, idx.data()) != UPH_OK) throw std::runtime_error(std::string("uph_batch_origin: ") + uph_last_error());
            std::vector<std::vector<SE3Pose>> part = rolloutPoses(c, dt, 0, n);
            for (int k = 0; k < n; k++) {
                if (idx[k] < 0 || idx[k] >= last_B_) throw std::runtime_error("getSE3PathBatch: a device no longer holds the last batch");
                out[(size_t)idx[k]] = std::move(part[(size_t)k]);
                seen++;
            }
        }
        if (seen != last_B_) throw std::runtime_error("getSE3PathBatch: the devices no longer hold the last batch");
        return out;
    }

protected:      // (TrajFleet below is the same object over a context made by uph_fleet_create)
    // what the calls on pairs of vehicles check first: every query array has traj_a's length m, neither side's last batch was split
    void pairCheck(const char* who, size_t m, std::initializer_list<size_t> sizes, const ALMTrajOpt* other) const {
        for (const size_t s : sizes) if (s != m) throw std::runtime_error(std::string(who) + ": the query arrays differ in number");
        if (last_multi_ || (other && other->last_multi_)) throw std::runtime_error(std::string(who) + ": the last batch was split over several devices");
    }
    // the conflict list of a fleet call -- call(room, pairs, rows, below): the C call `who` with room for `room` conflicts, which also sets out.n_conflicts; cap < 0:
    // every conflict (repeated once with room for all of them) -- unpacked into out.pairs, min (out.min_d2 / out.min_c2), out.min_t, first_t, last_t and below
    template <class Out, class Call>
    static void conflictList(Out& out, std::vector<double>& min, int32_t n, int64_t cap, const char* who, Call call) {
        int64_t room = cap >= 0 ? cap : std::max<int64_t>(1024, 4 * (int64_t)n);
        std::vector<int32_t> pairs, below;
        std::vector<double> rows;
        for (;;) {
            pairs.assign((size_t)2 * room + 2, 0); rows.assign((size_t)4 * room + 4, 0.0); below.assign((size_t)room + 1, 0);
            if (call(room, pairs.data(), rows.data(), below.data()) != UPH_OK) throw std::runtime_error(std::string(who) + ": " + uph_last_error());
            if (cap >= 0 || out.n_conflicts <= room) break;
            room = out.n_conflicts;
        }
        const size_t m = (size_t)std::min<int64_t>(room, out.n_conflicts);
        for (size_t k = 0; k < m; k++) {
            out.pairs.push_back({pairs[2 * k], pairs[2 * k + 1]});
            min.push_back(rows[4 * k]); out.min_t.push_back(rows[4 * k + 1]); out.first_t.push_back(rows[4 * k + 2]); out.last_t.push_back(rows[4 * k + 3]);
            out.below.push_back(below[k]);
        }
    }
    GoalPlan finishGoalPlan(int rc, int32_t B, GoalPlan& out, const std::vector<int32_t>& nxy, const std::vector<int32_t>& nyw, const char* who, const char* caller);
    // coefficient blocks of the C-ABI (lowest order first, xy interleaved per row) -> pieces with the highest order first (se2traj.hpp:682-695)
    static SE2Trajectory makeTraj(const double* cxy, int Nxy, double Txy, const double* cyaw, int Nyaw, double Tyaw) {
        SE2Trajectory t;
        for (int i = 0; i < Nxy; i++) {
            Piece<2> p; p.duration = Txy;
            for (int d = 0; d < 2; d++) for (int k = 0; k < 6; k++) p.coeff[d][5 - k] = cxy[(size_t)(6 * i + k) * 2 + d];
            t.pos_traj.emplace_back(p);
        }
        for (int i = 0; i < Nyaw; i++) {
            Piece<1> p; p.duration = Tyaw;
            for (int k = 0; k < 6; k++) p.coeff[0][5 - k] = cyaw[(size_t)6 * i + k];
            t.yaw_traj.emplace_back(p);
        }
        return t;
    }

    // trajectories [b0, b1) (b1 < 0: all) of context c as visSE3Traj's poses: the POSE channel at dt with the end point
    static std::vector<std::vector<SE3Pose>> rolloutPoses(uph_ctx* c, double dt, int32_t b0, int32_t b1) {
        const int B = uph_batch_count(c);
        if (B <= 0) throw std::runtime_error("getSE3Path: no trajectory has been optimised on this object");
        if (b1 < 0) b1 = B;
        std::vector<int64_t> off((size_t)B + 1, 0);
        if (uph_rollout_plan(c, dt, 1, off.data()) != UPH_OK) throw std::runtime_error(std::string("uph_rollout_plan: ") + uph_last_error());
        std::vector<double> rows((size_t)12 * (size_t)(off[b1] - off[b0]) + 1);
        if (uph_rollout_batch(c, dt, 1, UPH_ROLLOUT_POSE, b0, b1, rows.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_rollout_batch: ") + uph_last_error());
        std::vector<std::vector<SE3Pose>> out((size_t)(b1 - b0));
        for (int32_t b = b0; b < b1; b++) {
            std::vector<SE3Pose>& path = out[(size_t)(b - b0)];
            path.resize((size_t)(off[b + 1] - off[b]));
            for (size_t i = 0; i < path.size(); i++) {
                const double* r = rows.data() + (size_t)12 * ((size_t)(off[b] - off[b0]) + i);
                for (int k = 0; k < 9; k++) path[i].R[k] = r[k];
                for (int k = 0; k < 3; k++) path[i].p[k] = r[9 + k];
            }
        }
        return out;
    }

    UnevenMapHandle* env_ = nullptr;
    uph_ctx* ctx_ = nullptr;
    uph_result last_{};
    std::vector<double> cxy_, cyaw_, x_;
    std::vector<double> last_report_;       // [B][7] of the last optimizeSE2TrajBatch over several devices, in the caller's order
    bool last_multi_ = false;
    std::vector<uph_ctx*> last_ctxs_;       // the contexts of the last optimizeSE2TrajBatch (getSE3PathBatch after a call with peers)
    int32_t last_B_ = 0;
};

// A fleet of resident trajectories (include/uneven_hip.h uph_fleet_*): `slots` slots on one map that the trajectories ALMTrajOpt objects solved are adopted
// into on the device, one slot per vehicle.  It IS an ALMTrajOpt as far as the queries on resident trajectories go -- checkSE2TrajBatch, locateSE2TrajBatch,
// withinSE2TrajBatch, extentSE2TrajBatch, separationSE2TrajBatch, conflictsSE2TrajBatch, their footprint and delay forms, getSE3PathBatch -- with `traj` meaning
// slots, and is accepted as `other`; what uploads, solves or reports (optimizeSE2Traj, optimizeSE2TrajBatch, getMaxVxAxAyCurAttSig, ...) throws: the C-ABI
// refuses it on a fleet.  The parameter members are those uph_check_limits reads.
class TrajFleet : public ALMTrajOpt {
public:
    // slots empty slots of at most cap_xy / cap_yaw pieces each on env's device (uph_fleet_bytes of device memory)
    void setEnvironment(UnevenMapHandle* env, int slots, int cap_xy = UPH_MAX_PIECE_XY, int cap_yaw = UPH_MAX_PIECE_YAW) {
        env_ = env;
        if (ctx_) { uph_ctx_destroy(ctx_); ctx_ = nullptr; }
        const uph_opt_params p = optParams();
        if (uph_fleet_create(env->get(), &p, slots, cap_xy, cap_yaw, &ctx_) != UPH_OK) throw std::runtime_error(std::string("uph_fleet_create: ") + uph_last_error());
        cap_xy_ = cap_xy; cap_yaw_ = cap_yaw;
    }
    int slots() const { return uph_batch_count(ctx_); }
    // trajectory traj[q] of src's last batch (or of another fleet's slots) into slot[q], started at t0[q] on the common clock (empty: 0).  All or nothing.
    void adoptSE2TrajBatch(const ALMTrajOpt& src, const std::vector<int>& traj, const std::vector<int>& slot, const std::vector<double>& t0 = std::vector<double>()) {
        if (slot.size() != traj.size() || (!t0.empty() && t0.size() != traj.size())) throw std::runtime_error("adoptSE2TrajBatch: traj, slot and t0 differ in number");
        if (src.get() == nullptr) throw std::runtime_error("adoptSE2TrajBatch: the source has no device context");
        std::vector<int32_t> tr(traj.begin(), traj.end()), sl(slot.begin(), slot.end());
        if (uph_fleet_adopt(ctx_, src.get(),(int32_t)tr.size(), tr.data(), sl.data(), t0.empty() ? nullptr : t0.data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_fleet_adopt: ") + uph_last_error());
    }
    void releaseSlots(const std::vector<int>& slot) {
        std::vector<int32_t> sl(slot.begin(), slot.end());
        if (uph_fleet_release(ctx_, (int32_t)sl.size(), sl.data()) != UPH_OK) throw std::runtime_error(std::string("uph_fleet_release: ") + uph_last_error());
    }
    std::vector<int32_t> occupied() const {
        std::vector<int32_t> o((size_t)std::max(0, slots()), 0);
        if (uph_fleet_info(ctx_, nullptr, nullptr, nullptr, o.data(), nullptr) != UPH_OK) throw std::runtime_error(std::string("uph_fleet_info: ") + uph_last_error());
        return o;
    }
    std::vector<double> startTimes() const {      // the starts stored at adoption: the t0 to pass to the fleet-wide queries
        std::vector<double> t((size_t)std::max(0, slots()), 0.0);
        if (uph_fleet_info(ctx_, nullptr, nullptr, nullptr, nullptr, t.data()) != UPH_OK) throw std::runtime_error(std::string("uph_fleet_info: ") + uph_last_error());
        return t;
    }
    // the trajectory of a slot as the reference's SE2Trajectory (what getTraj() gave for it on the object that solved it, bit for bit)
    SE2Trajectory getTraj(int slot) const {
        const int32_t s = slot;
        int32_t nx = 0, ny = 0, ret = 0;
        double tx = 0.0, ty = 0.0;
        std::vector<double> cx((size_t)12 * cap_xy_), cy((size_t)6 * cap_yaw_);
        if (uph_fleet_get(ctx_, 1, &s, &nx, &ny, &tx, &ty, &ret, cx.data(), cy.data()) != UPH_OK) throw std::runtime_error(std::string("uph_fleet_get: ") + uph_last_error());
        if (nx == 0) throw std::runtime_error("getTraj: the slot is empty");
        return makeTraj(cx.data(), nx, tx, cy.data(), ny, ty);
    }
    // uph_traj_states' rows [n][10] of slot[q] at t[q]
    std::vector<double> trajStates(const std::vector<int>& slot, const std::vector<double>& t) {
        if (t.size() != slot.size()) throw std::runtime_error("trajStates: slot and t differ in number");
        std::vector<int32_t> sl(slot.begin(), slot.end());
        std::vector<double> out((size_t)10 * sl.size(), 0.0);
        if (!sl.empty() && uph_traj_states(ctx_, (int32_t)sl.size(), sl.data(), t.data(), out.data()) != UPH_OK) throw std::runtime_error(std::string("uph_traj_states: ") + uph_last_error());
        return out;
    }
    double adoptKernelMs() const {
        double ms = 0.0;
        if (uph_fleet_kernel_ms(ctx_, &ms) != UPH_OK) throw std::runtime_error(std::string("uph_fleet_kernel_ms: ") + uph_last_error());
        return ms;
    }

private:
    int cap_xy_ = 0, cap_yaw_ = 0;
};


// The body layer (include/uneven_hip.h uph_body_*, no counterpart in the reference beyond the commented-out per-yaw read of kino_astar.cpp:178): the map's
// occupancy dilated by the vehicle's rectangle (front, rear, half_width) inflated by `margin`, one slice per yaw bin, on the map's device.  Owns a
// uph_body_layer; the map must outlive it, and it must outlive every KinoAstar::setBodyLayer that names it (the destructor cannot refuse: it reports to stderr
// what uph_body_layer_destroy refused).  The layer does not follow the map: after UnevenMapHandle::updateMap call updateChanged(info), after anything else
// that writes the map call build().
class BodyLayer {
public:
    struct Info {
        std::array<double, 3> shape{};
        double margin = 0.0;
        int32_t layers = 0, R = 0;
        std::array<int32_t, 3> dims{};
        int32_t behind = 0;             // occupancy writes of the map since the layer was made (0: fresh)
        bool fresh() const { return behind == 0; }
    };
    // the margin with which a 0 of the layer holds for every pose inside the cell (uph_body_layer_margin)
    static double conservativeMargin(const uph_map_params& mp, const std::array<double, 3>& shape) {
        double m = 0.0;
        if (uph_body_layer_margin(&mp, shape.data(), &m) != UPH_OK) throw std::runtime_error(std::string("uph_body_layer_margin: ") + uph_last_error());
        return m;
    }
    BodyLayer(UnevenMapHandle& map, const std::array<double, 3>& shape, double margin, int32_t layers = UPH_FOOT_OCC_XY | UPH_FOOT_OUTSIDE) {
        if (uph_body_layer_create(map.get(), shape.data(), margin, layers, &l_) != UPH_OK) throw std::runtime_error(std::string("uph_body_layer_create: ") + uph_last_error());
    }
    ~BodyLayer() {
        if (l_ && uph_body_layer_destroy(l_) != UPH_OK) std::fprintf(stderr, "uneven_hip::BodyLayer: %s\n", uph_last_error());
    }
    BodyLayer(const BodyLayer&) = delete;
    BodyLayer& operator=(const BodyLayer&) = delete;
    void build() { if (uph_body_layer_build(l_) != UPH_OK) throw std::runtime_error(std::string("uph_body_layer_build: ") + uph_last_error()); }
    // rect = {x0, x1, y0, y1}, half-open: the columns whose occupancy changed (uph_map_update_info::changed)
    void update(const std::array<int32_t, 4>& rect) {
        if (uph_body_layer_update(l_, rect.data()) != UPH_OK) throw std::runtime_error(std::string("uph_body_layer_update: ") + uph_last_error());
    }
    void updateChanged(const uph_map_update_info& info) { update(std::array<int32_t, 4>{info.changed[0], info.changed[1], info.changed[2], info.changed[3]}); }
    Info info() const {
        Info i;
        if (uph_body_layer_info(l_, i.shape.data(), &i.margin, &i.layers, &i.R, i.dims.data(), &i.behind) != UPH_OK)
            throw std::runtime_error(std::string("uph_body_layer_info: ") + uph_last_error());
        return i;
    }
    std::vector<char> get() const {                 // [nx][ny][nyaw], laid out as the map's occ
        const Info i = info();
        std::vector<char> b((size_t)i.dims[0] * (size_t)i.dims[1] * (size_t)i.dims[2]);
        if (uph_body_layer_get(l_, b.data()) != UPH_OK) throw std::runtime_error(std::string("uph_body_layer_get: ") + uph_last_error());
        return b;
    }
    void set(const std::vector<char>& bytes) {
        const Info i = info();
        if (bytes.size() != (size_t)i.dims[0] * (size_t)i.dims[1] * (size_t)i.dims[2]) throw std::runtime_error("BodyLayer::set: a layer has nx * ny * nyaw bytes");
        if (uph_body_layer_set(l_, bytes.data()) != UPH_OK) throw std::runtime_error(std::string("uph_body_layer_set: ") + uph_last_error());
    }
    double kernelMs() const {
        double ms = 0.0;
        if (uph_body_layer_kernel_ms(l_, &ms) != UPH_OK) throw std::runtime_error(std::string("uph_body_layer_kernel_ms: ") + uph_last_error());
        return ms;
    }
    uint64_t writes() const {                       // build, update and set count one each: what a ClearanceLayer is stamped with
        uint64_t w = 0;
        if (uph_body_layer_writes(l_, &w) != UPH_OK) throw std::runtime_error(std::string("uph_body_layer_writes: ") + uph_last_error());
        return w;
    }
    uph_body_layer* handle() const { return l_; }

private:
    uph_body_layer* l_ = nullptr;
};

// The clearance layer (include/uneven_hip.h uph_clearance_*, no counterpart in the reference): the exact squared Euclidean distance transform of a BodyLayer,
// truncated at rmax cells, one field per yaw slice, on the body layer's device.  Owns a uph_clearance; the body layer must outlive it (declare it first:
// uph_body_layer_destroy is refused while a clearance layer names it).  The layer does not follow the body layer: after BodyLayer::update(rect) call
// update(growRect(dims, rect, R)), after BodyLayer::build or set call build().
class ClearanceLayer {
public:
    struct Info {
        int32_t rmax = 0, polarity = 0;
        std::array<int32_t, 3> dims{};
        int32_t behind = 0;             // writes of the body layer since the clearance layer was made (0: fresh)
        bool fresh() const { return behind == 0; }
    };
    // rect = {x0, x1, y0, y1} grown by r and clipped to the grid (uph_clearance_grow_rect): the map's changed rect grown by BodyLayer::Info::R is what
    // BodyLayer::update rewrote, and that rect is what update() below takes
    static std::array<int32_t, 4> growRect(const std::array<int32_t, 3>& dims, const std::array<int32_t, 4>& rect, int32_t r) {
        std::array<int32_t, 4> out{};
        if (uph_clearance_grow_rect(dims.data(), rect.data(), r, out.data()) != UPH_OK) throw std::runtime_error(std::string("uph_clearance_grow_rect: ") + uph_last_error());
        return out;
    }
    // a distance in metres as the query's threshold in squared cells: ceil((below / res)^2)
    static int32_t below2(double below, double res) { const double q = below / res; return (int32_t)std::min(std::ceil(q * q), 2147483647.0); }
    ClearanceLayer(BodyLayer& body, int32_t rmax, int32_t polarity = UPH_CLEAR_TO_OCCUPIED) {
        if (uph_clearance_create(body.handle(), rmax, polarity, &l_) != UPH_OK) throw std::runtime_error(std::string("uph_clearance_create: ") + uph_last_error());
    }
    ~ClearanceLayer() { uph_clearance_destroy(l_); }
    ClearanceLayer(const ClearanceLayer&) = delete;
    ClearanceLayer& operator=(const ClearanceLayer&) = delete;
    void build() { if (uph_clearance_build(l_) != UPH_OK) throw std::runtime_error(std::string("uph_clearance_build: ") + uph_last_error()); }
    // rect = {x0, x1, y0, y1}, half-open: the columns whose body bytes changed
    void update(const std::array<int32_t, 4>& rect) {
        if (uph_clearance_update(l_, rect.data()) != UPH_OK) throw std::runtime_error(std::string("uph_clearance_update: ") + uph_last_error());
    }
    Info info() const {
        Info i;
        if (uph_clearance_info(l_, &i.rmax, &i.polarity, i.dims.data(), &i.behind) != UPH_OK) throw std::runtime_error(std::string("uph_clearance_info: ") + uph_last_error());
        return i;
    }
    std::vector<uint16_t> get() const {             // [nx][ny][nyaw], laid out as the body layer
        const Info i = info();
        std::vector<uint16_t> d((size_t)i.dims[0] * (size_t)i.dims[1] * (size_t)i.dims[2]);
        if (uph_clearance_get(l_, d.data()) != UPH_OK) throw std::runtime_error(std::string("uph_clearance_get: ") + uph_last_error());
        return d;
    }
    double kernelMs() const {
        double ms = 0.0;
        if (uph_clearance_kernel_ms(l_, &ms) != UPH_OK) throw std::runtime_error(std::string("uph_clearance_kernel_ms: ") + uph_last_error());
        return ms;
    }
    // the continuous field the clearance term reads (uph_clearance_field): value [n] in metres and gradient [n] = {dc/dx, dc/dy} at poses {x, y, yaw}
    struct Field {
        std::vector<double> value;
        std::vector<std::array<double, 2>> grad;
    };
    Field field(const std::vector<std::array<double, 3>>& pos) const {
        Field f;
        f.value.assign(pos.size(), 0.0); f.grad.assign(pos.size(), std::array<double, 2>{0.0, 0.0});
        if (!pos.empty() && uph_clearance_field(l_, (int32_t)pos.size(), pos[0].data(), f.value.data(), f.grad[0].data()) != UPH_OK)
            throw std::runtime_error(std::string("uph_clearance_field: ") + uph_last_error());
        return f;
    }
    uph_clearance* handle() const { return l_; }

private:
    uph_clearance* l_ = nullptr;
};

inline void ALMTrajOpt::setClearanceTerm(const ClearanceLayer* layer, double d_safe, double weight) {
    if (uph_ctx_set_clearance_term(ctx_, layer ? layer->handle() : nullptr, d_safe, weight) != UPH_OK)
        throw std::runtime_error(std::string("uph_ctx_set_clearance_term: ") + uph_last_error());
}

inline ALMTrajOpt::TrajClearance ALMTrajOpt::clearanceSE2TrajBatch(const ClearanceLayer& layer, const std::vector<int>& traj, const std::vector<double>& t_from,
                                                                   const std::vector<double>& t_to, const std::vector<int32_t>& below2, double dt, bool with_end) {
    if (t_from.size() != traj.size() || (!t_to.empty() && t_to.size() != traj.size()) || below2.size() != traj.size())
        throw std::runtime_error("clearanceSE2TrajBatch: traj, t_from, t_to and below2 differ in number");
    if (last_multi_) throw std::runtime_error("clearanceSE2TrajBatch: the last batch was split over several devices");
    const int32_t n = (int32_t)traj.size();
    TrajClearance out;
    if (n == 0) return out;
    std::vector<int32_t> tr(traj.begin(), traj.end());
    out.min_d2.assign((size_t)n, -1); out.min_t.assign((size_t)n, 0.0); out.min_cell.assign((size_t)n, std::array<int32_t, 3>{-1, -1, -1});
    out.first_t.assign((size_t)n, 0.0); out.last_t.assign((size_t)n, 0.0); out.counts.assign((size_t)4 * n, 0);
    if (uph_clearance_check_batch(ctx_, layer.handle(), n, tr.data(), t_from.data(), t_to.empty() ? nullptr : t_to.data(), dt, with_end ? 1 : 0, below2.data(),
                                  out.min_d2.data(), out.min_t.data(), out.min_cell[0].data(), out.first_t.data(), out.last_t.data(), out.counts.data()) != UPH_OK)
        throw std::runtime_error(std::string("uph_clearance_check_batch: ") + uph_last_error());
    return out;
}

// KinoAstar (front_end/include/front_end/kino_astar.h:99-168): the front-end PlanManager calls right before the back-end
// (`kino_astar->plan(start_state, end_state)`, plan_manager.cpp:59-60).  Same public parameter members as the reference reads from rosparam
// (kino_astar.cpp:7-20; defaults = run_hill.yaml:16-30), same plan() signature; the search runs on the device, one wave64 per query.
class KinoAstar {
public:
    double yaw_resolution = 3.15, lambda_heu = 1.0, weight_r2 = 1.0, weight_so2 = 0.5, weight_v_change = 0.0, weight_delta_change = 0.0, weight_sigma = 10.0;
    double time_interval = 0.3, collision_interval = 0.06, oneshot_range = 1.0, wheel_base = 0.26, max_steer = 0.5, max_vel = 0.5;
    bool in_test = false;

    KinoAstar() = default;
    ~KinoAstar() { if (k_) uph_kino_destroy(k_); }
    KinoAstar(const KinoAstar&) = delete;
    KinoAstar& operator=(const KinoAstar&) = delete;

    // void KinoAstar::init(ros::NodeHandle& nh)  (front_end/src/kino_astar.cpp:5-20): nh.param with the REFERENCE's defaults -- a key the
    // parameter server does not hold sets the member to that default (weight_so2 1.0, weight_sigma 0.0, time_interval 1.0, ...: not the YAML
    // values the members start with).  The publishers / subscribers of :22-30 and the RViz model of :36-43 stay with the host; the Dubins
    // radius wheel_base / tan(max_steer) (:34) is formed by uph_kino_create from the parameters setEnvironment hands over.
    template <class NodeHandle>
    void init(NodeHandle& nh) {
        nh.param("kino_astar/yaw_resolution", yaw_resolution, 3.15);
        nh.param("kino_astar/lambda_heu", lambda_heu, 1.0);
        nh.param("kino_astar/weight_r2", weight_r2, 1.0);
        nh.param("kino_astar/weight_so2", weight_so2, 1.0);
        nh.param("kino_astar/weight_v_change", weight_v_change, 0.0);
        nh.param("kino_astar/weight_delta_change", weight_delta_change, 0.0);
        nh.param("kino_astar/weight_sigma", weight_sigma, 0.0);
        nh.param("kino_astar/time_interval", time_interval, 1.0);
        nh.param("kino_astar/collision_interval", collision_interval, 1.0);
        nh.param("kino_astar/oneshot_range", oneshot_range, 1.0);
        nh.param("kino_astar/wheel_base", wheel_base, 1.0);
        nh.param("kino_astar/max_steer", max_steer, 1.0);
        nh.param("kino_astar/max_vel", max_vel, 1.0);
        nh.param("kino_astar/in_test", in_test, false);
    }
    uph_kino_params kinoParams() const {
        return uph_kino_params{yaw_resolution, lambda_heu, weight_r2, weight_so2, weight_v_change, weight_delta_change, weight_sigma,
                               time_interval, collision_interval, oneshot_range, wheel_base, max_steer, max_vel};
    }
    void setEnvironment(UnevenMapHandle* env, int slots = 0) {        // kino_astar.h:170-178: binds the map, allocates the node pools
        if (k_) { uph_kino_destroy(k_); k_ = nullptr; }
        const uph_kino_params kp = kinoParams();
        if (uph_kino_create(env->get(), &kp, slots, &k_) != UPH_OK) throw std::runtime_error(std::string("uph_kino_create: ") + uph_last_error());
    }
    // std::vector<Eigen::Vector3d> plan(const Eigen::Vector3d& start_state, const Eigen::Vector3d& end_state)   (kino_astar.cpp:67-236)
    template <class V3>
    std::vector<VecN<3>> plan(const V3& start_state, const V3& end_state) {
        std::vector<std::vector<VecN<3>>> r = planBatch(std::vector<V3>(1, start_state), std::vector<V3>(1, end_state));
        front_end_path = r[0];
        return front_end_path;
    }
    // many goals at once: paths[b] is empty where the reference would return an empty vector (start / goal occupied, no path, pool exhausted);
    // status[b] says which (UPH_KINO_*)
    template <class V3>
    std::vector<std::vector<VecN<3>>> planBatch(const std::vector<V3>& starts, const std::vector<V3>& goals, int path_cap = 2048) {
        if (!k_) throw std::runtime_error("KinoAstar: setEnvironment has not been called");
        const int32_t B = (int32_t)starts.size();
        std::vector<std::vector<VecN<3>>> out((size_t)B);
        status.assign((size_t)B, 0); iter_num.assign((size_t)B, 0);
        if (B == 0 || goals.size() != starts.size()) return out;
        std::vector<double> s((size_t)3 * B), g((size_t)3 * B), paths((size_t)3 * B * path_cap);
        std::vector<int32_t> np(B), use(B);
        for (int32_t b = 0; b < B; b++) for (int k = 0; k < 3; k++) { s[(size_t)3 * b + k] = starts[b][k]; g[(size_t)3 * b + k] = goals[b][k]; }
        if (uph_kino_plan_batch(k_, B, s.data(), g.data(), path_cap, paths.data(), np.data(), status.data(), iter_num.data(), use.data(), 0, 0, nullptr) != UPH_OK)
            throw std::runtime_error(std::string("uph_kino_plan_batch: ") + uph_last_error());
        std::vector<int32_t> longer;                    // queries whose front_end_path has more poses than path_cap: searched again with room for all of them
        int32_t need = 0;                               // (the reference returns the whole path; a clipped one would end short of the goal)
        for (int32_t b = 0; b < B; b++) {
            if (status[b] != UPH_KINO_OK) continue;
            if (np[b] > path_cap) { longer.push_back(b); if (np[b] > need) need = np[b]; continue; }
            out[b].resize((size_t)np[b]);
            for (int i = 0; i < np[b]; i++) for (int k = 0; k < 3; k++) out[b][i][k] = paths[((size_t)b * path_cap + i) * 3 + k];
        }
        if (!longer.empty()) {
            const int32_t L = (int32_t)longer.size();
            std::vector<double> s2((size_t)3 * L), g2((size_t)3 * L), p2((size_t)3 * L * need);
            std::vector<int32_t> np2(L), st2(L), it2(L), us2(L);
            for (int32_t j = 0; j < L; j++) for (int k = 0; k < 3; k++) { s2[(size_t)3 * j + k] = s[(size_t)3 * longer[j] + k]; g2[(size_t)3 * j + k] = g[(size_t)3 * longer[j] + k]; }
            if (uph_kino_plan_batch(k_, L, s2.data(), g2.data(), need, p2.data(), np2.data(), st2.data(), it2.data(), us2.data(), 0, 0, nullptr) != UPH_OK)
                throw std::runtime_error(std::string("uph_kino_plan_batch: ") + uph_last_error());
            for (int32_t j = 0; j < L; j++) {
                const int32_t b = longer[j];
                if (st2[j] != UPH_KINO_OK || np2[j] > need) { status[b] = UPH_KINO_INTERNAL; continue; }      // (the search is deterministic: not expected)
                out[b].resize((size_t)np2[j]);
                for (int i = 0; i < np2[j]; i++) for (int k = 0; k < 3; k++) out[b][i][k] = p2[((size_t)j * need + i) * 3 + k];
            }
        }
        return out;
    }
    std::vector<VecN<3>> front_end_path;
    std::vector<int32_t> status, iter_num;      // of the last plan / planBatch
    void visFrontEnd() {}                        // RViz output stays with the host (no device side)
    void visExpanded() {}
    // the search reads `layer` (of the same map) where it reads occ_r2 by default -- goal test, one-shot samples, collision samples --; nullptr: back to occ_r2.
    // plan / planBatch and ALMTrajOpt::planSE2TrajBatch / replanSE2TrajBatch through this object follow it; a stale layer makes them throw.
    void setBodyLayer(BodyLayer* layer) {
        if (!k_) throw std::runtime_error("KinoAstar: setEnvironment has not been called");
        if (uph_kino_set_body_layer(k_, layer ? layer->handle() : nullptr) != UPH_OK) throw std::runtime_error(std::string("uph_kino_set_body_layer: ") + uph_last_error());
    }
    uph_kino* handle() const { return k_; }      // the search context (ALMTrajOpt::planSE2TrajBatch)

private:
    uph_kino* k_ = nullptr;
};

template <class V3>
ALMTrajOpt::GoalPlan ALMTrajOpt::planSE2TrajBatch(KinoAstar& kino, const std::vector<V3>& starts, const std::vector<V3>& goals, const uph_manager_params& mgr,
                                                  int32_t path_cap) {
    if (!kino.handle()) throw std::runtime_error("planSE2TrajBatch: KinoAstar::setEnvironment has not been called");
    if (goals.size() != starts.size()) throw std::runtime_error("planSE2TrajBatch: starts and goals differ in number");
    const int32_t B = (int32_t)starts.size();
    GoalPlan out;
    if (B == 0) return out;
    std::vector<double> s((size_t)3 * B), g((size_t)3 * B);
    for (int32_t b = 0; b < B; b++) for (int k = 0; k < 3; k++) { s[(size_t)3 * b + k] = starts[b][k]; g[(size_t)3 * b + k] = goals[b][k]; }
    std::vector<int32_t> nxy(B), nyw(B);
    out.status.assign((size_t)B, -1); out.traj_of.assign((size_t)B, -1);      // (-1: no UPH_KINO_* code -- tells whether the call wrote the outputs)
    in_opt = true;
    last_report_.clear(); last_multi_ = false; last_ctxs_.assign(1, ctx_); last_B_ = 0;
    const int rc = uph_plan_upload(kino.handle(), ctx_, &mgr, B, s.data(), g.data(), path_cap, out.status.data(), out.traj_of.data(), nxy.data(), nyw.data());
    return finishGoalPlan(rc, B, out, nxy, nyw, "uph_plan_upload", "planSE2TrajBatch");
}

template <class V3>
ALMTrajOpt::GoalPlan ALMTrajOpt::replanSE2TrajBatch(KinoAstar& kino, const std::vector<int>& traj, const std::vector<double>& t_switch, const std::vector<V3>* goals,
                                                    const uph_manager_params& mgr, int32_t path_cap) {
    if (!kino.handle()) throw std::runtime_error("replanSE2TrajBatch: KinoAstar::setEnvironment has not been called");
    if (t_switch.size() != traj.size() || (goals && goals->size() != traj.size())) throw std::runtime_error("replanSE2TrajBatch: traj, t_switch and goals differ in number");
    if (last_multi_) throw std::runtime_error("replanSE2TrajBatch: the last batch was split over several devices");
    const int32_t B = (int32_t)traj.size();
    GoalPlan out;
    if (B == 0) return out;
    std::vector<int32_t> tr(traj.begin(), traj.end()), nxy(B), nyw(B);
    std::vector<double> g;
    if (goals) {
        g.resize((size_t)3 * B);
        for (int32_t b = 0; b < B; b++) for (int k = 0; k < 3; k++) g[(size_t)3 * b + k] = (*goals)[b][k];
    }
    out.status.assign((size_t)B, -1); out.traj_of.assign((size_t)B, -1);
    in_opt = true;
    const int rc = uph_replan_upload(kino.handle(), ctx_, ctx_, &mgr, B, tr.data(), t_switch.data(), goals ? g.data() : nullptr, path_cap, nullptr, out.status.data(),
                                     out.traj_of.data(), nxy.data(), nyw.data());
    if (rc == UPH_ERR_INVALID && out.status[0] < 0) {            // refused: the last batch is still resident, nothing of it changes
        in_opt = false;
        throw std::runtime_error(std::string("uph_replan_upload: ") + uph_last_error());
    }
    last_report_.clear(); last_multi_ = false; last_ctxs_.assign(1, ctx_); last_B_ = 0;
    return finishGoalPlan(rc, B, out, nxy, nyw, "uph_replan_upload", "replanSE2TrajBatch");
}

// after uph_plan_upload / uph_replan_upload / uph_refine_upload into ctx_: solve and download the found goals, one GoalPlan entry per goal
inline ALMTrajOpt::GoalPlan ALMTrajOpt::finishGoalPlan(int rc, int32_t B, GoalPlan& out, const std::vector<int32_t>& nxy, const std::vector<int32_t>& nyw, const char* who,
                                                     const char* caller) {
    const int F = uph_batch_count(ctx_);
    // "no goal produced a path" is the one UPH_ERR_INVALID returned with the outputs written and no UPH_KINO_OK among them: every entry empty, no
    // throw.  Every other failure (a HIP error in the search included) leaves the outputs untouched and throws.
    bool written = true, any_ok = false;
    for (int32_t b = 0; b < B; b++) { written = written && out.status[b] >= 0; any_ok = any_ok || out.status[b] == UPH_KINO_OK; }
    if (rc != UPH_OK && !(rc == UPH_ERR_INVALID && written && !any_ok)) {
        in_opt = false;
        throw std::runtime_error(std::string(who) + ": " + uph_last_error());
    }
    std::vector<size_t> ox(B, 0), oc(B, 0), oy(B, 0);
    size_t sx = 0, sc = 0, sy = 0;
    for (int32_t b = 0; b < B; b++) {
        if (out.traj_of[b] < 0) continue;
        ox[b] = sx; oc[b] = sc; oy[b] = sy;
        sx += (size_t)2 * nxy[b] + nyw[b] + 1; sc += (size_t)12 * (nxy[b] + 1); sy += (size_t)6 * (nyw[b] + 1);
    }
    std::vector<double> xs(sx + 1, 0.0), cx(sc + 1, 0.0), cy(sy + 1, 0.0);
    std::vector<uph_result> rs((size_t)std::max(F, 0));
    for (int32_t b = 0; b < B; b++) {
        const int32_t j = out.traj_of[b];
        if (j < 0) continue;
        rs[j] = uph_result{};
        rs[j].x_final = xs.data() + ox[b]; rs[j].c_xy = cx.data() + oc[b]; rs[j].c_yaw = cy.data() + oy[b];
    }
    if (F > 0) {
        if (uph_batch_solve(ctx_) != UPH_OK || uph_batch_download(ctx_, rs.data()) != UPH_OK) {
            in_opt = false;
            throw std::runtime_error(std::string(caller) + ": " + uph_last_error());
        }
        last_B_ = F;
    }
    in_opt = false;
    for (int32_t b = 0; b < B; b++) {
        const int32_t j = out.traj_of[b];
        if (j < 0) {
            out.ret.push_back(-1); out.jerk_cost.push_back(0.0); out.total_time.push_back(0.0); out.traj.push_back(SE2Trajectory());
            continue;
        }
        out.ret.push_back(rs[j].ret_code);
        out.jerk_cost.push_back(rs[j].jerk_cost);
        out.total_time.push_back(rs[j].ret_code == UPH_RET_UNSUPPORTED ? 0.0 : (nxy[b] + 1) * rs[j].piece_T_xy);
        out.traj.push_back(rs[j].ret_code == UPH_RET_UNSUPPORTED ? SE2Trajectory()
                               : makeTraj(cx.data() + oc[b], nxy[b] + 1, rs[j].piece_T_xy, cy.data() + oy[b], nyw[b] + 1, rs[j].piece_T_yaw));
    }
    return std::move(out);
}

}  // namespace uneven_hip
